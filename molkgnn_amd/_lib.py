"""ctypes binding of libmolkgnn_hip.so (the C ABI declared in include/molkgnn_hip.h).

The library is built in-tree by ``make -C molkgnn_amd/csrc`` (or
``__graft_entry__.build()``).  There is no CPU or PyTorch fallback: if the
library is missing or a call fails, an exception is raised.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional, Sequence

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# MKGNN_LIB: a diagnostic build of the same library (make VARIANT=... in csrc/), e.g. with cycle stamps compiled in
LIB_PATH = os.environ.get("MKGNN_LIB") or os.path.join(_HERE, "libmolkgnn_hip.so")
MAX_DEGREE = 4
ABI_VERSION = 8
# MKGNN_LOSS_*: the loss kinds of the single-task head (mkgnn_tail_args.loss_kind, mkgnn_head_loss_*)
LOSS_BCE_MEAN, LOSS_SQERR_MEAN, LOSS_SQERR_SUM = 0, 1, 2
TASK_HEAD_MAX_TASKS, TASK_HEAD_MAX_H = 32, 64   # MKGNN_TASK_HEAD_MAX_TASKS, the task-indexed head's widest embedding
EMBED_COSINE_MAX_QUERIES, EMBED_COSINE_MAX_H = 32, 64   # MKGNN_EMBED_COSINE_MAX_QUERIES, mkgnn_embed_cosine's widest embedding
MAX_COSINE_MAX_REFS, MAX_COSINE_MAX_H = 1 << 20, 64     # MKGNN_MAX_COSINE_MAX_REFS, mkgnn_embed_max_cosine's widest embedding
# kgnn_max_cosine.hip's tiling (MC_ROWS, MC_TILE, MC_MAX_PARTS, MC_TARGET_BLOCKS; SEL_THREADS): rows per block, references per LDS
# tile, the most parts a launch splits the references into, the blocks it aims at; the slots of one pass of mkgnn_select_rows
MAX_COSINE_ROWS, MAX_COSINE_TILE, MAX_COSINE_MAX_PARTS, MAX_COSINE_TARGET_BLOCKS = 128, 32, 256, 2048
SELECT_ROWS_PASS = 1024
DIVERSE_MAX_ROWS, DIVERSE_MAX_H = 1 << 20, 64           # MKGNN_DIVERSE_MAX_ROWS, mkgnn_diverse_pick's widest embedding
# kgnn_diverse.hip's tiling (DV_COVER_ROWS, DV_COVER_TILE): rows per block and picks per LDS tile of the cover launch
DIVERSE_COVER_ROWS, DIVERSE_COVER_TILE = 128, 32
# MKGNN_MAXMIN_MAX_ROWS, MKGNN_MAXMIN_MAX_PICKS, mkgnn_maxmin_pick's widest embedding
MAXMIN_MAX_ROWS, MAXMIN_MAX_PICKS, MAXMIN_MAX_H = 1 << 20, 4096, 64
# kgnn_maxmin.hip's tiling (MM_TILE, MM_ROWS): the rows ONE workgroup walks in one launch; rows per block of the grid-wide launches
MAXMIN_TILE, MAXMIN_ROWS = 1024, 256
EXEMPLARS_MAX_K, EXEMPLARS_MAX_COLUMNS = 64, 256        # MKGNN_EXEMPLARS_MAX_K, MKGNN_EXEMPLARS_MAX_COLUMNS
# kgnn_exemplars.hip's tiling (EX_TILE, EX_CHUNK): degree-bucket slots per tile and columns per workgroup of the runs launch
EXEMPLARS_TILE, EXEMPLARS_CHUNK = 128, 64
KNN_MAX_K, KNN_MAX_QUERIES, KNN_MAX_ROWS, KNN_MAX_H = 64, 1 << 20, 1 << 20, 64   # MKGNN_KNN_MAX_*, mkgnn_embed_knn_update's widest embedding
# kgnn_knn.hip's tiling (KNN_WAVES, KNN_TILE, KNN_MIN_PART_TILES, KNN_MAX_PARTS, KNN_TARGET_BLOCKS): queries (= waves) per block,
# candidate rows per LDS tile, the fewest tiles of a part, the most parts a launch splits the candidates into, the blocks it aims at
KNN_WAVES, KNN_TILE, KNN_MIN_PART_TILES, KNN_MAX_PARTS, KNN_TARGET_BLOCKS = 4, 64, 2, 32, 1024
# MKGNN_BOOTSTRAP_MAX_ROWS, MKGNN_BOOTSTRAP_MAX_REPLICATES, MKGNN_BOOTSTRAP_WORKSPACE_CAP (bytes the wrapper keeps the scratch under)
BOOTSTRAP_MAX_ROWS, BOOTSTRAP_MAX_REPLICATES, BOOTSTRAP_WORKSPACE_CAP = 1 << 22, 4096, 1 << 30
# MKGNN_BOOTSTRAP_MAX_CUTS, MKGNN_BOOTSTRAP_MAX_ALPHAS: the enrichment cuts and BEDROC alphas one mkgnn_bootstrap_early takes
BOOTSTRAP_MAX_CUTS, BOOTSTRAP_MAX_ALPHAS = 8, 4
# kgnn_bootstrap.hip's tiling (BS_TILE, BS_DRAW_ROWS, BS_LDS_MAX_N): ranks per tile of the walk, rows per block of the draw launch,
# the most rows whose multiplicities one workgroup keeps in LDS (beyond: the workspace and three launches per pass)
BOOTSTRAP_TILE, BOOTSTRAP_DRAW_ROWS, BOOTSTRAP_LDS_MAX_N = 1024, 1024, 8192
# MKGNN_BOOTSTRAP_REG_MAX_ROWS: the rows of one mkgnn_bootstrap_regression (the int64 rank sums, at most n (n - 1)^2, stay exact)
BOOTSTRAP_REG_MAX_ROWS = 1 << 20


def diverse_tile(H: int) -> int:
    """``DV_TILE`` of ``mkgnn_diverse_pick`` for an embedding of width ``H`` (``DvTile``, kgnn_diverse.hip): the rows one workgroup
    decides per launch.  It is chosen per padded width (32 or 64 columns) from the compiler's resource report; both widths take
    1 024.  The result of a call does not depend on it; the tests place their shapes around it."""
    if not 1 <= int(H) <= DIVERSE_MAX_H:
        raise ValueError(f"H = {H} outside [1, {DIVERSE_MAX_H}]")
    return {32: 1024, 64: 1024}[32 if int(H) <= 32 else 64]


def max_cosine_split(n_rows: int, R: int):
    """``(references per part, parts)`` of one ``mkgnn_embed_max_cosine`` launch (``mc_split``, kgnn_max_cosine.hip): whole tiles per
    part, at most ``MAX_COSINE_MAX_PARTS`` parts and no more than bring the grid to ``MAX_COSINE_TARGET_BLOCKS`` blocks.  The result
    of a call does not depend on it; the tests place their shapes around it."""
    row_blocks = -(-int(n_rows) // MAX_COSINE_ROWS)
    tiles = -(-int(R) // MAX_COSINE_TILE)
    want = min(-(-MAX_COSINE_TARGET_BLOCKS // row_blocks), tiles, MAX_COSINE_MAX_PARTS)
    per_part = -(-tiles // want)
    return per_part * MAX_COSINE_TILE, -(-tiles // per_part)


def count_within_split(n_rows: int, R: int):
    """``(references per part, parts)`` of one ``mkgnn_embed_count_within`` launch: the count is a second reduction over
    ``mkgnn_embed_max_cosine``'s walk (one kernel text, one ``mc_split``), so it is ``max_cosine_split`` with ``MAX_COSINE_ROWS``,
    ``MAX_COSINE_TILE`` and ``MAX_COSINE_MAX_PARTS`` as its tiling; a split launch keeps ``parts x n_rows`` int32 partial counts
    in the workspace.  The result of a call does not depend on it; the tests place their shapes around it."""
    return max_cosine_split(n_rows, R)


COMPONENTS_MAX_VERTICES = 1 << 27               # MKGNN_COMPONENTS_MAX_VERTICES


def components_rounds(n: int) -> int:
    """The rounds one ``mkgnn_graph_components`` enqueues for ``n`` vertices (``cc_rounds``, kgnn_components.hip):
    ``2 * ceil(log2(max(n, 2))) + 1``."""
    return 2 * (max(int(n), 2) - 1).bit_length() + 1


def knn_split(n_rows: int, Q: int):
    """``(rows per part, parts)`` of one ``mkgnn_embed_knn_update`` launch (``knn_split``, kgnn_knn.hip): whole tiles per part, at
    least ``KNN_MIN_PART_TILES`` of them, at most ``KNN_MAX_PARTS`` parts and no more than bring the grid to ``KNN_TARGET_BLOCKS``
    blocks of ``KNN_WAVES`` queries.  The result of a call does not depend on it; the tests place their shapes around it."""
    query_blocks = -(-int(Q) // KNN_WAVES)
    tiles = -(-int(n_rows) // KNN_TILE)
    want = min(-(-KNN_TARGET_BLOCKS // query_blocks), KNN_MAX_PARTS)
    per_part = max(-(-tiles // want), KNN_MIN_PART_TILES)
    return per_part * KNN_TILE, max(-(-tiles // per_part), 1)


class KernelBank(C.Structure):
    _fields_ = [("num_kernels", C.c_int32), ("reserved", C.c_int32),
                ("x_center", C.c_void_p), ("x_support", C.c_void_p),
                ("edge_attr_support", C.c_void_p), ("p_support", C.c_void_p),
                ("support_attr_sc_weight", C.c_void_p), ("center_attr_sc_weight", C.c_void_p),
                ("edge_attr_support_sc_weight", C.c_void_p)]


class KernelBankGrad(C.Structure):
    _fields_ = [("x_center", C.c_void_p), ("x_support", C.c_void_p), ("edge_attr_support", C.c_void_p),
                ("support_attr_sc_weight", C.c_void_p), ("center_attr_sc_weight", C.c_void_p),
                ("edge_attr_support_sc_weight", C.c_void_p)]


class DegreeBucket(C.Structure):
    _fields_ = [("count", C.c_int64), ("selected_index", C.c_void_p), ("nei_index", C.c_void_p),
                ("nei_edge_attr", C.c_void_p), ("p_focal", C.c_void_p), ("nei_p", C.c_void_p), ("nei_edge_unit", C.c_void_p)]


class Saved(C.Structure):
    _fields_ = [("pair_state", C.c_void_p), ("chirality", C.c_void_p)]


class ReadoutParams(C.Structure):
    _fields_ = [("lin1_weight", C.c_void_p), ("lin1_bias", C.c_void_p), ("lin2_weight", C.c_void_p),
                ("lin2_bias", C.c_void_p), ("F", C.c_int32), ("H", C.c_int32), ("G", C.c_int32)]


class TailArgs(C.Structure):
    """``mkgnn_tail_args`` (include/molkgnn_hip.h): the fused tail of a training step (and, forward only, ``mkgnn_tail_score``)."""
    _fields_ = [("sim", C.c_void_p), ("sim_stride", C.c_int64), ("num_kernels", C.c_int32 * 4), ("buckets", C.c_void_p),
                ("in_rowptr", C.c_void_p), ("in_col", C.c_void_p), ("out_rowptr", C.c_void_p), ("out_col", C.c_void_p),
                ("mol_ptr", C.c_void_p), ("atom_mol", C.c_void_p), ("n_atoms", C.c_int64), ("n_mols", C.c_int64),
                ("n_loss_mols", C.c_int64), ("readout", ReadoutParams), ("head_weight", C.c_void_p), ("head_bias", C.c_void_p),
                ("target", C.c_void_p), ("dropout_p", C.c_float), ("rng_state", C.c_void_p), ("rng_used", C.c_void_p),
                ("emb", C.c_void_p), ("emb_stride", C.c_int64), ("pred", C.c_void_p), ("loss", C.c_void_p),
                ("grad_sim", C.c_void_p), ("grad_sim_stride", C.c_int64), ("grad_lin1_weight", C.c_void_p),
                ("grad_lin1_bias", C.c_void_p), ("grad_lin2_weight", C.c_void_p), ("grad_lin2_bias", C.c_void_p),
                ("grad_head_weight", C.c_void_p), ("grad_head_bias", C.c_void_p), ("defer_reduce", C.c_int32),
                ("loss_kind", C.c_int32)]


TAIL_MAX_ATOMS, TAIL_MAX_EDGES = 128, 512      # MKGNN_TAIL_MAX_ATOMS / _EDGES
TAIL_MC_MAX_SAMPLES = 64                       # MKGNN_TAIL_MC_MAX_SAMPLES


class TailMcOut(C.Structure):
    """``mkgnn_tail_mc_out`` (include/molkgnn_hip.h): where ``mkgnn_tail_score_mc`` writes; every pointer may be NULL."""
    _fields_ = [("samples", C.c_void_p), ("samples_stride", C.c_int64), ("mean", C.c_void_p), ("std", C.c_void_p),
                ("acq", C.c_void_p), ("alpha", C.c_float), ("beta", C.c_float)]

ATOM_CONTRIB_MAX_TASKS = 32                    # MKGNN_ATOM_CONTRIB_MAX_TASKS


class AtomContribArgs(C.Structure):
    """``mkgnn_atom_contrib_args`` (include/molkgnn_hip.h): every atom's share of every logit (``mkgnn_atom_contributions``)."""
    _fields_ = [("sim", C.c_void_p), ("sim_stride", C.c_int64), ("num_kernels", C.c_int32 * 4), ("buckets", C.c_void_p),
                ("in_rowptr", C.c_void_p), ("in_col", C.c_void_p), ("n_atoms", C.c_int64), ("readout", ReadoutParams),
                ("head_weight", C.c_void_p), ("head_stride", C.c_int64), ("T", C.c_int32), ("contrib", C.c_void_p),
                ("contrib_stride", C.c_int64)]


class CopyItem(C.Structure):
    """``mkgnn_copy_item``."""
    _fields_ = [("dst", C.c_void_p), ("src", C.c_void_p), ("numel", C.c_int64)]


class AdamWTensor(C.Structure):
    _fields_ = [("param", C.c_void_p), ("grad", C.c_void_p), ("state", C.c_void_p), ("numel", C.c_int64),
                ("group", C.c_int32), ("reserved", C.c_int32), ("active", C.c_void_p)]


class AdamWGroup(C.Structure):
    _fields_ = [("lr_device", C.c_void_p), ("lr", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float),
                ("eps", C.c_float), ("weight_decay", C.c_float), ("maximize", C.c_int32), ("grad_scale", C.c_float)]


class AdamWAverage(C.Structure):
    """``mkgnn_adamw_average``; ``mode``: ``ADAMW_AVERAGE_EMA`` or ``ADAMW_AVERAGE_MEAN``."""
    _fields_ = [("mode", C.c_int32), ("decay", C.c_float), ("warmup", C.c_int32), ("start", C.c_int32)]


ADAMW_AVERAGE_EMA, ADAMW_AVERAGE_MEAN = 0, 1


class SwapItem(C.Structure):
    """``mkgnn_swap_item``."""
    _fields_ = [("a", C.c_void_p), ("b", C.c_void_p), ("numel", C.c_int64)]


class ShardView(C.Structure):
    _fields_ = [("x", C.c_void_p), ("p", C.c_void_p), ("edge_src", C.c_void_p), ("edge_dst", C.c_void_p),
                ("edge_attr", C.c_void_p), ("y", C.c_void_p), ("mol_atom_ptr", C.c_void_p), ("mol_edge_ptr", C.c_void_p),
                ("mol_deg_ptr", C.c_void_p), ("n_molecules", C.c_int64), ("x_dim", C.c_int32), ("p_dim", C.c_int32),
                ("e_dim", C.c_int32), ("reserved", C.c_int32)]


class ResidentShardView(C.Structure):
    """``mkgnn_resident_shard``: DEVICE pointers of a shard that lives in GPU memory (``shards.ResidentShard``)."""
    _fields_ = [("x", C.c_void_p), ("p", C.c_void_p), ("bond_ij", C.c_void_p), ("bond_attr", C.c_void_p), ("y", C.c_void_p),
                ("mol_atom_ptr", C.c_void_p), ("mol_bond_ptr", C.c_void_p), ("mol_deg", C.c_void_p), ("n_molecules", C.c_int64),
                ("x_dim", C.c_int32), ("p_dim", C.c_int32), ("e_dim", C.c_int32), ("reserved", C.c_int32)]


class ResidentShardPackedView(C.Structure):
    """``mkgnn_resident_shard_packed``: ``x_rec`` and the other arrays are DEVICE pointers, ``x_col`` is a HOST pointer
    (``shards.ResidentShard(..., packed=True)`` keeps the table alive)."""
    _fields_ = [("x_rec", C.c_void_p), ("x_col", C.c_void_p), ("p", C.c_void_p), ("bond_ij", C.c_void_p), ("bond_attr", C.c_void_p),
                ("y", C.c_void_p), ("mol_atom_ptr", C.c_void_p), ("mol_bond_ptr", C.c_void_p), ("mol_deg", C.c_void_p),
                ("n_molecules", C.c_int64), ("x_dim", C.c_int32), ("p_dim", C.c_int32), ("e_dim", C.c_int32), ("rec_bytes", C.c_int32)]


PACKED_MAX_X_DIM = 160                          # MKGNN_PACKED_MAX_X_DIM
TOPK_MAX_K = 1024                               # MKGNN_TOPK_MAX_K
GATHER_BAD_ID, GATHER_MISFIT = 1, 2             # MKGNN_GATHER_*: bits of the gather's status word
Int64x6 = C.c_int64 * 6
Banks4 = KernelBank * MAX_DEGREE
BankGrads4 = KernelBankGrad * MAX_DEGREE
Buckets4 = DegreeBucket * MAX_DEGREE
Saved4 = Saved * MAX_DEGREE
Int32x4 = C.c_int32 * MAX_DEGREE
Int64x4 = C.c_int64 * MAX_DEGREE

MOLECULE_MAX_LAYERS = 4
MOLECULE_MAX_ATOMS = 64
MOLECULE_MAX_MOLS = 16
MOLECULE_HEAD, MOLECULE_BACKWARD, MOLECULE_GRAD_EMB, MOLECULE_SQERR, MOLECULE_SUM = 1, 2, 4, 8, 16
MOLECULE_READOUT_DROPOUT = 32


class MoleculeLayer(C.Structure):
    _fields_ = [("bank", Banks4), ("grad", BankGrads4), ("saved", Saved4), ("F", C.c_int32), ("reserved", C.c_int32),
                ("sim_out", C.c_void_p), ("sim_stride", C.c_int64)]


class BnStats(C.Structure):
    """``mkgnn_bn_stats``: the statistics-only companion of a batch norm (reference MolKGNNNet.py:116)."""
    _fields_ = [("x", C.c_void_p), ("x_stride", C.c_int64), ("n_rows", C.c_int64), ("C", C.c_int32),
                ("running_mean", C.c_void_p), ("running_var", C.c_void_p), ("momentum", C.c_float),
                ("num_batches_tracked", C.c_void_p), ("row_key", C.c_void_p), ("key_limit", C.c_void_p)]


class MoleculeNet(C.Structure):
    _fields_ = [("num_layers", C.c_int32), ("E", C.c_int32), ("layer", MoleculeLayer * MOLECULE_MAX_LAYERS),
                ("bn_weight", C.c_void_p), ("bn_bias", C.c_void_p), ("bn_running_mean", C.c_void_p),
                ("bn_running_var", C.c_void_p), ("bn_num_batches_tracked", C.c_void_p),
                ("bn_eps", C.c_float), ("bn_momentum", C.c_float), ("bn_training", C.c_int32), ("reserved", C.c_int32),
                ("grad_bn_weight", C.c_void_p), ("grad_bn_bias", C.c_void_p),
                ("readout", ReadoutParams),
                ("grad_lin1_weight", C.c_void_p), ("grad_lin1_bias", C.c_void_p), ("grad_lin2_weight", C.c_void_p),
                ("grad_lin2_bias", C.c_void_p),
                ("ffn_weight", C.c_void_p), ("ffn_bias", C.c_void_p), ("grad_ffn_weight", C.c_void_p),
                ("grad_ffn_bias", C.c_void_p), ("head_dropout", C.c_float), ("readout_dropout", C.c_float),
                ("rng_state", C.c_void_p), ("rng_used", C.c_void_p), ("edge_stats", C.POINTER(BnStats))]


class MoleculeBatch(C.Structure):
    _fields_ = [("n_atoms", C.c_int64), ("n_mols", C.c_int64), ("n_chunks", C.c_int64), ("max_chunk_atoms", C.c_int64),
                ("chunk_mol_ptr", C.c_void_p), ("mol_atom_ptr", C.c_void_p), ("atom_degree", C.c_void_p),
                ("atom_rank", C.c_void_p), ("buckets", Buckets4), ("x", C.c_void_p), ("x_stride", C.c_int64)]


class LossWeights(C.Structure):
    """``mkgnn_loss_weights``: the optional sample weights (direct, or a table read through ids) and per-task positive weights."""
    _fields_ = [("sample_weight", C.c_void_p), ("weight_ids", C.c_void_p), ("n_sample_weight", C.c_int64),
                ("pos_weight", C.c_void_p)]


class TailLabels(C.Structure):
    """``mkgnn_tail_labels``: the T-output head of ``mkgnn_tail_fused_labels`` -- a label matrix with holes or a task per molecule
    (exactly one), optionally read through row ids, and where ``pred [n_loss_mols, T]`` goes."""
    _fields_ = [("n_tasks", C.c_int32), ("labels", C.c_void_p), ("label_stride", C.c_int64), ("n_label_rows", C.c_int64),
                ("task", C.c_void_p), ("n_task", C.c_int64), ("row_ids", C.c_void_p), ("pred", C.c_void_p),
                ("pred_stride", C.c_int64)]


EXPORTS = ("mkgnn_abi_version", "mkgnn_last_error", "mkgnn_row_inv_norm", "mkgnn_unit_rows8", "mkgnn_workspace_bytes",
           "mkgnn_kernelsetconv_forward", "mkgnn_kernelsetconv_backward", "mkgnn_segment_sum_rows",
           "mkgnn_readout_hidden_stride", "mkgnn_readout_workspace_bytes", "mkgnn_readout_forward",
           "mkgnn_readout_backward", "mkgnn_batchnorm_workspace_bytes", "mkgnn_batchnorm_forward",
           "mkgnn_batchnorm_backward", "mkgnn_bce_head_workspace_bytes", "mkgnn_bce_head_forward",
           "mkgnn_bce_head_backward", "mkgnn_rf_workspace_bytes", "mkgnn_rf_count", "mkgnn_rf_fill", "mkgnn_adamw_step", "mkgnn_adamw_state_floats",
           "mkgnn_adamw_clip_workspace_bytes", "mkgnn_adamw_step_clipped",
           "mkgnn_adamw_average_floats", "mkgnn_adamw_step_averaged", "mkgnn_flat_swap",
           "mkgnn_bce_head_dropout_forward", "mkgnn_bce_head_dropout_backward", "mkgnn_segment_sum_block_rows",
           "mkgnn_plan_workspace_bytes", "mkgnn_plan_build", "mkgnn_plan_present_blocks", "mkgnn_backward_grad_blocks",
           "mkgnn_debug_grad_blocks_launches", "mkgnn_debug_poison_backward", "mkgnn_backward_join", "mkgnn_backward_streams", "mkgnn_bank_prepare", "mkgnn_bank_prepare_deferred", "mkgnn_bank_prepare_flush", "mkgnn_bank_prepare_withdraw", "mkgnn_touch_hint", "mkgnn_expand_batch", "mkgnn_bce_head_fused", "mkgnn_collate_compact", "mkgnn_collate_compact_bytes",
           "mkgnn_readout_blocks_supported", "mkgnn_readout_blocks_forward", "mkgnn_readout_blocks_backward",
           "mkgnn_readout_blocks_workspace_bytes", "mkgnn_molecule_supported", "mkgnn_molecule_workspace_bytes",
           "mkgnn_molecule_step", "mkgnn_batchnorm_stats_workspace_bytes", "mkgnn_batchnorm_update_stats",
           "mkgnn_batchnorm_forward_with_stats", "mkgnn_index_workspace_bytes", "mkgnn_index_build",
           "mkgnn_rows_split_supported", "mkgnn_rows_presplit", "mkgnn_tail_supported", "mkgnn_tail_workspace_bytes", "mkgnn_tail_fused", "mkgnn_tail_flush", "mkgnn_flat_copy",
           "mkgnn_tail_fused_readout_dropout", "mkgnn_readout_dropout_mask", "mkgnn_tail_score", "mkgnn_tail_score_workspace_bytes",
           "mkgnn_head_loss_forward", "mkgnn_head_loss_backward", "mkgnn_head_loss_dropout_forward",
           "mkgnn_head_loss_dropout_backward", "mkgnn_head_loss_fused", "mkgnn_gather_compact",
           "mkgnn_gather_compact_workspace_bytes", "mkgnn_gather_compact_packed", "mkgnn_topk_update", "mkgnn_topk_workspace_bytes",
           "mkgnn_task_head_workspace_bytes", "mkgnn_task_head_forward", "mkgnn_task_head_backward", "mkgnn_task_head_fused",
           "mkgnn_task_head_weighted_forward", "mkgnn_task_head_weighted_backward", "mkgnn_task_head_weighted_fused",
           "mkgnn_tail_fused_weighted", "mkgnn_tail_labels_workspace_bytes", "mkgnn_tail_fused_labels",
           "mkgnn_label_head_workspace_bytes", "mkgnn_label_head_forward", "mkgnn_label_head_backward", "mkgnn_label_head_fused",
           "mkgnn_task_scores", "mkgnn_topk_tasks_workspace_bytes", "mkgnn_topk_update_tasks", "mkgnn_embed_cosine",
           "mkgnn_atom_contributions", "mkgnn_atom_contributions_workspace_bytes", "mkgnn_embed_max_cosine",
           "mkgnn_embed_max_cosine_workspace_bytes", "mkgnn_select_rows", "mkgnn_tail_defer_projection",
           "mkgnn_debug_tail_projection_launches", "mkgnn_diverse_pick", "mkgnn_diverse_pick_workspace_bytes",
           "mkgnn_kernel_exemplars_update", "mkgnn_kernel_exemplars_workspace_bytes", "mkgnn_embed_knn_update",
           "mkgnn_embed_knn_workspace_bytes", "mkgnn_embed_count_within", "mkgnn_embed_count_within_workspace_bytes",
           "mkgnn_embed_neighbours_within", "mkgnn_embed_neighbours_within_workspace_bytes", "mkgnn_graph_components",
           "mkgnn_graph_components_workspace_bytes", "mkgnn_maxmin_pick", "mkgnn_maxmin_pick_workspace_bytes",
           "mkgnn_tail_score_mc", "mkgnn_tail_score_mc_workspace_bytes", "mkgnn_debug_set_bn_merge", "mkgnn_debug_conv_dispatch",
           "mkgnn_bootstrap_roc", "mkgnn_bootstrap_roc_workspace_bytes", "mkgnn_bootstrap_early",
           "mkgnn_bootstrap_regression", "mkgnn_bootstrap_regression_workspace_bytes")

_lib: Optional[C.CDLL] = None
TORCH_LIB_PATH = os.path.join(os.path.dirname(LIB_PATH), "libmolkgnn_torch.so")
_torch_ops_loaded = False


def load_torch_ops():
    """Register ``torch.ops.molkgnn.*`` (csrc/torch_ops.cpp: TORCH_LIBRARY over the C ABI); raises if it is not built."""
    global _torch_ops_loaded
    import torch
    if not _torch_ops_loaded:
        load()                                   # (the shim links against the C-ABI library: same directory, $ORIGIN)
        if not os.path.exists(TORCH_LIB_PATH):
            raise MolKGNNLibraryError(f"{TORCH_LIB_PATH} is missing: build it with `make -C molkgnn_amd/csrc torch`")
        torch.ops.load_library(TORCH_LIB_PATH)
        if int(torch.ops.molkgnn.abi_version()) != ABI_VERSION:
            raise MolKGNNLibraryError("libmolkgnn_torch.so was built against another ABI version")
        _torch_ops_loaded = True
    return torch.ops.molkgnn


class MolKGNNLibraryError(RuntimeError):
    pass


def load() -> C.CDLL:
    """Load (once) and type the shared library; raise if it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise MolKGNNLibraryError(
            f"{LIB_PATH} is missing: build it with `make -C molkgnn_amd/csrc` "
            "(python -c 'import __graft_entry__ as g; g.build()'). There is no fallback path.")
    lib = C.CDLL(LIB_PATH)
    for name in EXPORTS:
        if not hasattr(lib, name):
            raise MolKGNNLibraryError(f"{LIB_PATH} does not export {name}")
    lib.mkgnn_abi_version.restype = C.c_int
    lib.mkgnn_last_error.restype = C.c_char_p
    lib.mkgnn_row_inv_norm.restype = C.c_int
    lib.mkgnn_row_inv_norm.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p]
    lib.mkgnn_unit_rows8.restype = C.c_int
    lib.mkgnn_unit_rows8.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p]
    lib.mkgnn_workspace_bytes.restype = C.c_size_t
    lib.mkgnn_workspace_bytes.argtypes = [Int32x4, C.c_int32, C.c_int32, C.c_int64, C.c_int64]
    lib.mkgnn_kernelsetconv_forward.restype = C.c_int
    lib.mkgnn_kernelsetconv_forward.argtypes = [
        Banks4, Buckets4, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32,
        C.c_void_p, C.c_int64, Saved4, C.c_void_p, C.c_size_t, C.c_int32, C.c_void_p]
    lib.mkgnn_kernelsetconv_backward.restype = C.c_int
    lib.mkgnn_kernelsetconv_backward.argtypes = [
        Banks4, Buckets4, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32,
        C.c_void_p, C.c_int64, Saved4, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, BankGrads4,
        C.c_void_p, C.c_size_t, C.c_int32, C.c_int32, C.c_void_p]
    lib.mkgnn_backward_streams.restype = C.c_int
    lib.mkgnn_backward_streams.argtypes = [Banks4, Buckets4, C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_int32]
    # diagnostics: (banks, buckets, x, x stride, out stride, atoms, F, E, forward variant, backward variant, grad x wanted, grad x,
    # its stride, int32[11]) -> the kernel family of every degree, forward and backward; launches nothing
    lib.mkgnn_debug_conv_dispatch.restype = C.c_int
    lib.mkgnn_debug_conv_dispatch.argtypes = [Banks4, Buckets4, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_int32, C.c_int32,
                                              C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.POINTER(C.c_int32 * 11)]
    lib.mkgnn_tail_supported.restype = C.c_int
    lib.mkgnn_tail_supported.argtypes = [C.c_int32, C.c_int32, C.c_int32, Int32x4]
    lib.mkgnn_tail_workspace_bytes.restype = C.c_size_t
    lib.mkgnn_tail_workspace_bytes.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int64]
    lib.mkgnn_tail_fused.restype = C.c_int
    lib.mkgnn_tail_fused.argtypes = [C.POINTER(TailArgs), C.c_void_p, C.c_size_t, C.c_void_p]
    lib.mkgnn_tail_score_workspace_bytes.restype = C.c_size_t
    lib.mkgnn_tail_score_workspace_bytes.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int64]
    lib.mkgnn_tail_score.restype = C.c_int
    lib.mkgnn_tail_score.argtypes = [C.POINTER(TailArgs), C.c_void_p, C.c_size_t, C.c_void_p]
    # Monte Carlo dropout samples: (args, readout dropout p, samples, {seed, offset} on the device, outputs, workspace, bytes, stream)
    lib.mkgnn_tail_score_mc_workspace_bytes.restype = C.c_size_t
    lib.mkgnn_tail_score_mc_workspace_bytes.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int64]
    lib.mkgnn_tail_score_mc.restype = C.c_int
    lib.mkgnn_tail_score_mc.argtypes = [C.POINTER(TailArgs), C.c_float, C.c_int32, C.c_void_p, C.POINTER(TailMcOut), C.c_void_p,
                                        C.c_size_t, C.c_void_p]
    # every atom's share of every logit: (args, workspace, workspace bytes, stream)
    lib.mkgnn_atom_contributions_workspace_bytes.restype = C.c_size_t
    lib.mkgnn_atom_contributions_workspace_bytes.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int64]
    lib.mkgnn_atom_contributions.restype = C.c_int
    lib.mkgnn_atom_contributions.argtypes = [C.POINTER(AtomContribArgs), C.c_void_p, C.c_size_t, C.c_void_p]
    lib.mkgnn_tail_fused_readout_dropout.restype = C.c_int
    lib.mkgnn_tail_fused_readout_dropout.argtypes = [C.POINTER(TailArgs), C.c_float, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.mkgnn_tail_fused_weighted.restype = C.c_int
    lib.mkgnn_tail_fused_weighted.argtypes = [C.POINTER(TailArgs), C.c_float, C.POINTER(LossWeights), C.c_void_p, C.c_size_t,
                                              C.c_void_p]
    lib.mkgnn_tail_labels_workspace_bytes.restype = C.c_size_t
    lib.mkgnn_tail_labels_workspace_bytes.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int64, C.c_int32]
    lib.mkgnn_tail_fused_labels.restype = C.c_int
    lib.mkgnn_tail_fused_labels.argtypes = [C.POINTER(TailArgs), C.c_float, C.POINTER(TailLabels), C.POINTER(LossWeights), C.c_void_p,
                                            C.c_size_t, C.c_void_p]
    lib.mkgnn_readout_dropout_mask.restype = C.c_int
    lib.mkgnn_readout_dropout_mask.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_float, C.c_void_p, C.c_int64, C.c_void_p]
    lib.mkgnn_flat_copy.restype = C.c_int
    lib.mkgnn_flat_copy.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
    lib.mkgnn_tail_flush.restype = C.c_int
    lib.mkgnn_tail_flush.argtypes = [C.c_void_p]
    lib.mkgnn_tail_defer_projection.restype = C.c_int
    lib.mkgnn_tail_defer_projection.argtypes = [C.c_int32]
    lib.mkgnn_debug_tail_projection_launches.restype = C.c_int
    lib.mkgnn_debug_tail_projection_launches.argtypes = [C.POINTER(C.c_int64 * 3)]
    lib.mkgnn_rows_presplit.restype = C.c_int
    lib.mkgnn_rows_presplit.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    lib.mkgnn_rows_split_supported.restype = C.c_int
    lib.mkgnn_rows_split_supported.argtypes = [Banks4, Buckets4, C.c_int64, C.c_int64, C.c_int64, C.c_int32, C.c_int32]
    lib.mkgnn_bank_prepare.restype = C.c_int
    lib.mkgnn_bank_prepare.argtypes = [C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.mkgnn_bank_prepare_deferred.restype = C.c_int
    lib.mkgnn_bank_prepare_deferred.argtypes = [C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    lib.mkgnn_bank_prepare_flush.restype = C.c_int
    lib.mkgnn_bank_prepare_flush.argtypes = [C.c_void_p]
    lib.mkgnn_bank_prepare_withdraw.restype = C.c_int
    lib.mkgnn_bank_prepare_withdraw.argtypes = []
    lib.mkgnn_touch_hint.restype = C.c_int
    lib.mkgnn_touch_hint.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
    lib.mkgnn_collate_compact_bytes.restype = C.c_size_t
    lib.mkgnn_collate_compact_bytes.argtypes = [Int64x6, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32]
    lib.mkgnn_collate_compact.restype = C.c_int
    lib.mkgnn_collate_compact.argtypes = [C.POINTER(ShardView), C.c_int64, C.c_int64, Int64x6, C.c_int32, C.c_void_p, C.c_size_t]
    lib.mkgnn_gather_compact_workspace_bytes.restype = C.c_size_t
    lib.mkgnn_gather_compact_workspace_bytes.argtypes = [C.c_int64]
    lib.mkgnn_gather_compact.restype = C.c_int
    lib.mkgnn_gather_compact.argtypes = [C.POINTER(ResidentShardView), C.c_void_p, C.c_int64, Int64x6, C.c_int32, C.c_void_p,
                                         C.c_size_t, C.c_void_p, C.c_void_p]
    lib.mkgnn_gather_compact_packed.restype = C.c_int
    lib.mkgnn_gather_compact_packed.argtypes = [C.POINTER(ResidentShardPackedView), C.c_void_p, C.c_int64, Int64x6, C.c_int32,
                                                C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
    lib.mkgnn_topk_workspace_bytes.restype = C.c_size_t
    lib.mkgnn_topk_workspace_bytes.argtypes = [C.c_int32, C.c_int32]
    lib.mkgnn_topk_update.restype = C.c_int
    lib.mkgnn_topk_update.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    # T lists in one update: (scores, row stride, task stride, ids, B, T, n_valid, shard_tag, K, the [T, K] lists, workspace, stream)
    lib.mkgnn_topk_tasks_workspace_bytes.restype = C.c_size_t
    lib.mkgnn_topk_tasks_workspace_bytes.argtypes = [C.c_int32, C.c_int32, C.c_int32]
    lib.mkgnn_topk_update_tasks.restype = C.c_int
    lib.mkgnn_topk_update_tasks.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                            C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.mkgnn_expand_batch.restype = C.c_int
    lib.mkgnn_expand_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_int64, C.c_int64,
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.mkgnn_backward_join.restype = C.c_int
    lib.mkgnn_backward_join.argtypes = [C.c_void_p]
    lib.mkgnn_segment_sum_rows.restype = C.c_int
    lib.mkgnn_segment_sum_rows.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32,
                                           C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    P, I64, I32, F32 = C.c_void_p, C.c_int64, C.c_int32, C.c_float
    lib.mkgnn_readout_hidden_stride.restype = I32
    lib.mkgnn_readout_hidden_stride.argtypes = [I32]
    lib.mkgnn_readout_workspace_bytes.restype = C.c_size_t
    lib.mkgnn_readout_workspace_bytes.argtypes = [I32, I32, I32, I64, I64]
    lib.mkgnn_readout_forward.restype = C.c_int
    lib.mkgnn_readout_forward.argtypes = [C.POINTER(ReadoutParams), P, I64, I64, P, I64, P, P, P, P, I64, P]
    lib.mkgnn_readout_backward.restype = C.c_int
    lib.mkgnn_readout_backward.argtypes = [C.POINTER(ReadoutParams), P, I64, I64, P, P, I64, P, P, P, P, I64, P, I64,
                                           P, P, P, P, P, C.c_size_t, P]
    lib.mkgnn_readout_blocks_workspace_bytes.restype = C.c_size_t
    lib.mkgnn_readout_blocks_workspace_bytes.argtypes = [I32, I32, I32, I64]
    lib.mkgnn_readout_blocks_supported.restype = C.c_int
    lib.mkgnn_readout_blocks_supported.argtypes = [I32, I32, I32, Int32x4]
    lib.mkgnn_readout_blocks_forward.restype = C.c_int
    lib.mkgnn_readout_blocks_forward.argtypes = [C.POINTER(ReadoutParams), P, I64, Int32x4, Buckets4, I64, P, P, P, I64, P, P, P, P, P, P, I64, P]
    lib.mkgnn_readout_blocks_backward.restype = C.c_int
    lib.mkgnn_readout_blocks_backward.argtypes = [C.POINTER(ReadoutParams), P, I64, Int32x4, Buckets4, I64, P, P, P, P, I64, P, P, P,
                                                  P, I64, P, P, I64, P, P, P, P, P, C.c_size_t, P]
    lib.mkgnn_batchnorm_workspace_bytes.restype = C.c_size_t
    lib.mkgnn_batchnorm_workspace_bytes.argtypes = [I32]
    lib.mkgnn_batchnorm_forward.restype = C.c_int
    lib.mkgnn_batchnorm_forward.argtypes = [P, I64, I64, I32, P, P, P, P, F32, F32, I32, P, I64, P, P, P, P, P, P, C.c_size_t, P]
    lib.mkgnn_batchnorm_stats_workspace_bytes.restype = C.c_size_t
    lib.mkgnn_batchnorm_stats_workspace_bytes.argtypes = [I32]
    lib.mkgnn_batchnorm_update_stats.restype = C.c_int
    lib.mkgnn_batchnorm_update_stats.argtypes = [C.POINTER(BnStats), P, C.c_size_t, P]
    lib.mkgnn_batchnorm_forward_with_stats.restype = C.c_int
    lib.mkgnn_batchnorm_forward_with_stats.argtypes = [P, I64, I64, I32, P, P, P, P, F32, F32, I32, P, I64, P, P, P, P, P, P, C.c_size_t,
                                                       C.POINTER(BnStats), P, C.c_size_t, P]
    lib.mkgnn_batchnorm_backward.restype = C.c_int
    lib.mkgnn_batchnorm_backward.argtypes = [P, I64, P, I64, I64, I32, P, P, P, I32, P, I64, P, P, P, P, C.c_size_t, P]
    # tests: 0 = the loop form of the batch norm's merges at every width, 1 = the register forms, < 0 = the default
    lib.mkgnn_debug_set_bn_merge.restype = C.c_int
    lib.mkgnn_debug_set_bn_merge.argtypes = [I32]
    lib.mkgnn_bce_head_forward.restype = C.c_int
    lib.mkgnn_bce_head_forward.argtypes = [P, I64, I64, I32, P, P, P, P, P, P, C.c_size_t, P]
    lib.mkgnn_bce_head_backward.restype = C.c_int
    lib.mkgnn_bce_head_backward.argtypes = [P, I64, I64, I32, P, P, P, P, P, I64, P, P, P, C.c_size_t, P]
    lib.mkgnn_bce_head_dropout_forward.restype = C.c_int
    lib.mkgnn_bce_head_dropout_forward.argtypes = [P, I64, I64, I32, P, P, P, C.c_float, P, P, P, P, P, C.c_size_t, P]
    lib.mkgnn_bce_head_dropout_backward.restype = C.c_int
    lib.mkgnn_bce_head_dropout_backward.argtypes = [P, I64, I64, I32, P, P, P, P, C.c_float, P, P, I64, P, P, P, C.c_size_t, P]
    lib.mkgnn_bce_head_fused.restype = C.c_int
    lib.mkgnn_bce_head_fused.argtypes = [P, I64, I64, I32, P, P, P, C.c_float, P, P, P, P, P, I64, P, P, P, C.c_size_t, P]
    for name, args in (("mkgnn_head_loss_forward", lib.mkgnn_bce_head_forward.argtypes),
                       ("mkgnn_head_loss_backward", lib.mkgnn_bce_head_backward.argtypes),
                       ("mkgnn_head_loss_dropout_forward", lib.mkgnn_bce_head_dropout_forward.argtypes),
                       ("mkgnn_head_loss_dropout_backward", lib.mkgnn_bce_head_dropout_backward.argtypes),
                       ("mkgnn_head_loss_fused", lib.mkgnn_bce_head_fused.argtypes)):
        getattr(lib, name).restype = C.c_int
        getattr(lib, name).argtypes = [I32] + list(args)          # (loss_kind, then the mkgnn_bce_head_* arguments)
    lib.mkgnn_bce_head_workspace_bytes.restype = C.c_size_t
    lib.mkgnn_bce_head_workspace_bytes.argtypes = [I64, I32]
    # the task-indexed head: (loss_kind, emb, stride, n_rows, H, T, weight, [bias,] target, task, row_ids, n_task, ...)
    lib.mkgnn_task_head_workspace_bytes.restype = C.c_size_t
    lib.mkgnn_task_head_workspace_bytes.argtypes = [I64, I32, I32]
    lib.mkgnn_task_head_forward.restype = C.c_int
    lib.mkgnn_task_head_forward.argtypes = [I32, P, I64, I64, I32, I32, P, P, P, P, P, I64, C.c_float, P, P, P, P, P, C.c_size_t, P]
    lib.mkgnn_task_head_backward.restype = C.c_int
    lib.mkgnn_task_head_backward.argtypes = [I32, P, I64, I64, I32, I32, P, P, P, P, I64, P, P, C.c_float, P, P, I64, P, P, P,
                                             C.c_size_t, P]
    lib.mkgnn_task_head_fused.restype = C.c_int
    lib.mkgnn_task_head_fused.argtypes = [I32, P, I64, I64, I32, I32, P, P, P, P, P, I64, C.c_float, P, P, P, P, P, I64, P, P, P,
                                          C.c_size_t, P]
    # the weighted forms: the same arguments with a `const mkgnn_loss_weights*` in front of the workspace
    for name in ("forward", "backward", "fused"):
        args = list(getattr(lib, "mkgnn_task_head_" + name).argtypes)
        getattr(lib, "mkgnn_task_head_weighted_" + name).restype = C.c_int
        getattr(lib, "mkgnn_task_head_weighted_" + name).argtypes = args[:-3] + [C.POINTER(LossWeights)] + args[-3:]
    # the label-matrix head: (loss_kind, emb, stride, n_rows, H, T, weight, [bias,] labels, label stride, row_ids, n_label_rows, ...,
    # pred, pred stride, ..., weights, workspace, bytes, stream)
    LW = C.POINTER(LossWeights)
    lib.mkgnn_label_head_workspace_bytes.restype = C.c_size_t
    lib.mkgnn_label_head_workspace_bytes.argtypes = [I64, I32, I32]
    lib.mkgnn_label_head_forward.restype = C.c_int
    lib.mkgnn_label_head_forward.argtypes = [I32, P, I64, I64, I32, I32, P, P, P, I64, P, I64, C.c_float, P, P, P, I64, P, LW, P,
                                             C.c_size_t, P]
    lib.mkgnn_label_head_backward.restype = C.c_int
    lib.mkgnn_label_head_backward.argtypes = [I32, P, I64, I64, I32, I32, P, P, I64, P, I64, P, I64, P, C.c_float, P, P, I64, P, P,
                                              LW, P, C.c_size_t, P]
    lib.mkgnn_label_head_fused.restype = C.c_int
    lib.mkgnn_label_head_fused.argtypes = [I32, P, I64, I64, I32, I32, P, P, P, I64, P, I64, C.c_float, P, P, P, I64, P, P, I64, P,
                                           P, LW, P, C.c_size_t, P]
    # every task's logit of every row: (emb, stride, n_rows, H, T, weight, bias, pred, row stride, task stride, stream)
    lib.mkgnn_task_scores.restype = C.c_int
    lib.mkgnn_task_scores.argtypes = [P, I64, I64, I32, I32, P, P, P, I64, I64, P]
    # cosine of every row with every query: (emb, stride, n_rows, H, queries, stride, Q, sim, row stride, query stride, stream)
    lib.mkgnn_embed_cosine.restype = C.c_int
    lib.mkgnn_embed_cosine.argtypes = [P, I64, I64, I32, P, I64, I32, P, I64, I64, P]
    # the nearest reference of every row: (emb, stride, n_rows, H, refs, stride, R, max_sim, arg_ref, workspace, bytes, stream)
    lib.mkgnn_embed_max_cosine_workspace_bytes.restype = C.c_size_t
    lib.mkgnn_embed_max_cosine_workspace_bytes.argtypes = [I64, I32]
    lib.mkgnn_embed_max_cosine.restype = C.c_int
    lib.mkgnn_embed_max_cosine.argtypes = [P, I64, I64, I32, P, I64, I32, P, P, P, C.c_size_t, P]
    # the references above a threshold of every row: (emb, stride, n_rows, H, refs, stride, R, min_sim, counts, workspace, bytes, stream)
    lib.mkgnn_embed_count_within_workspace_bytes.restype = C.c_size_t
    lib.mkgnn_embed_count_within_workspace_bytes.argtypes = [I64, I32]
    lib.mkgnn_embed_count_within.restype = C.c_int
    lib.mkgnn_embed_count_within.argtypes = [P, I64, I64, I32, P, I64, I32, F32, P, P, C.c_size_t, P]
    # those references themselves, into a CSR: (emb, stride, n_rows, H, refs, stride, R, min_sim, row_ptr, capacity, nbr_ref, nbr_sim,
    # found, workspace, bytes, stream)
    lib.mkgnn_embed_neighbours_within_workspace_bytes.restype = C.c_size_t
    lib.mkgnn_embed_neighbours_within_workspace_bytes.argtypes = [I64, I32]
    lib.mkgnn_embed_neighbours_within.restype = C.c_int
    lib.mkgnn_embed_neighbours_within.argtypes = [P, I64, I64, I32, P, I64, I32, F32, P, I64, P, P, P, P, C.c_size_t, P]
    # connected components of CSR lists: (row_ptr, col, n, labels, state, resume, workspace, bytes, stream)
    lib.mkgnn_graph_components_workspace_bytes.restype = C.c_size_t
    lib.mkgnn_graph_components_workspace_bytes.argtypes = [I32]
    lib.mkgnn_graph_components.restype = C.c_int
    lib.mkgnn_graph_components.argtypes = [P, P, I32, P, P, I32, P, C.c_size_t, P]
    # stable compaction by a key: (scores, ids, key, B, n_valid, bounds, out_scores, out_ids, n_kept, stream)
    lib.mkgnn_select_rows.restype = C.c_int
    lib.mkgnn_select_rows.argtypes = [P, P, P, I32, P, P, P, P, P, P]
    lib.mkgnn_diverse_pick_workspace_bytes.restype = C.c_size_t
    lib.mkgnn_diverse_pick_workspace_bytes.argtypes = [I64]
    lib.mkgnn_diverse_pick.restype = C.c_int
    lib.mkgnn_diverse_pick.argtypes = [P, I64, I64, I32, C.c_float, I32, P, P, P, P, P, C.c_size_t, P]
    # (emb, stride, n_rows, H, start_sim or null, stop_sim, k_max, picks, pick_sim, n_picks, leader, leader_sim, workspace, bytes, stream)
    lib.mkgnn_maxmin_pick_workspace_bytes.restype = C.c_size_t
    lib.mkgnn_maxmin_pick_workspace_bytes.argtypes = [I64]
    lib.mkgnn_maxmin_pick.restype = C.c_int
    lib.mkgnn_maxmin_pick.argtypes = [P, I64, I64, I32, P, C.c_float, I32, P, P, P, P, P, P, C.c_size_t, P]
    # bootstrap replicates of AUC and logAUC: (rank, y_sorted, group_last, n, split, B, seed, offset, lower, upper, auc, logauc, two_u,
    # n_pos, workspace, bytes, stream); the sizing takes (n, replicates per pass)
    lib.mkgnn_bootstrap_roc_workspace_bytes.restype = C.c_size_t
    lib.mkgnn_bootstrap_roc_workspace_bytes.argtypes = [I64, I32]
    lib.mkgnn_bootstrap_roc.restype = C.c_int
    lib.mkgnn_bootstrap_roc.argtypes = [P, P, P, I64, I64, I32, C.c_uint64, C.c_uint64, C.c_double, C.c_double, P, P, P, P, P,
                                        C.c_size_t, P]
    # the same with the early-recognition sums: (.., lower, upper, cuts, J, alphas, A, auc, logauc, two_u, n_pos, ap, hits, rie,
    # workspace, bytes, stream)
    lib.mkgnn_bootstrap_early.restype = C.c_int
    lib.mkgnn_bootstrap_early.argtypes = [P, P, P, I64, I64, I32, C.c_uint64, C.c_uint64, C.c_double, C.c_double, P, I32, P, I32,
                                          P, P, P, P, P, P, P, P, C.c_size_t, P]
    # bootstrap replicates of the regression metrics: (rank_p, first_p, last_p, cross, first_t, last_t, p_sorted, t_by_prank, centre,
    # cuts, J, n, B, seed, offset, mom, rank_sums, hits, n_drawn, workspace, bytes, stream); the sizing takes (n, replicates per pass)
    lib.mkgnn_bootstrap_regression_workspace_bytes.restype = C.c_size_t
    lib.mkgnn_bootstrap_regression_workspace_bytes.argtypes = [I64, I32]
    lib.mkgnn_bootstrap_regression.restype = C.c_int
    lib.mkgnn_bootstrap_regression.argtypes = [P, P, P, P, P, P, P, P, P, P, I32, I64, I32, C.c_uint64, C.c_uint64, P, P, P, P, P,
                                               C.c_size_t, P]
    lib.mkgnn_kernel_exemplars_workspace_bytes.restype = C.c_size_t
    lib.mkgnn_kernel_exemplars_workspace_bytes.argtypes = [C.POINTER(Int64x4), C.POINTER(Int32x4), I32, I32]
    lib.mkgnn_kernel_exemplars_update.restype = C.c_int
    lib.mkgnn_kernel_exemplars_update.argtypes = [P, I64, I64, C.POINTER(Buckets4), C.POINTER(Int32x4), C.POINTER(Int32x4), P, P, P,
                                                  I32, P, P, P, I32, I32, P, P, P, P, P, C.c_size_t, P]
    # fused cosine and top-k: (emb, stride, n_rows, H, ids, n_valid, shard_tag, queries, stride, Q, K, the [Q, K] lists, workspace, bytes, stream)
    lib.mkgnn_embed_knn_workspace_bytes.restype = C.c_size_t
    lib.mkgnn_embed_knn_workspace_bytes.argtypes = [I64, I32, I32]
    lib.mkgnn_embed_knn_update.restype = C.c_int
    lib.mkgnn_embed_knn_update.argtypes = [P, I64, I64, I32, P, P, P, P, I64, I32, I32, P, P, P, P, C.c_size_t, P]
    lib.mkgnn_rf_workspace_bytes.restype = C.c_size_t
    lib.mkgnn_rf_workspace_bytes.argtypes = [I64]
    lib.mkgnn_rf_count.restype = C.c_int
    lib.mkgnn_rf_count.argtypes = [P, I64, I64, P, C.c_size_t, P, P]
    lib.mkgnn_rf_fill.restype = C.c_int
    lib.mkgnn_rf_fill.argtypes = [P, P, P, I64, I64, I32, P, Buckets4, P]
    lib.mkgnn_segment_sum_block_rows.restype = C.c_int
    lib.mkgnn_segment_sum_block_rows.argtypes = [P, I64, P, P, P, I64, Int32x4, I32, P, I64, P, P]
    lib.mkgnn_plan_workspace_bytes.restype = C.c_size_t
    lib.mkgnn_plan_workspace_bytes.argtypes = [I64, I64, I64]
    lib.mkgnn_plan_build.restype = C.c_int
    lib.mkgnn_plan_build.argtypes = [Buckets4, I64, P, I64, P, P, P, P, P, P, P, P, P, C.c_size_t, P]
    lib.mkgnn_plan_present_blocks.restype = C.c_int
    lib.mkgnn_plan_present_blocks.argtypes = [Buckets4, I64, P, P, P, P, P]
    lib.mkgnn_backward_grad_blocks.restype = C.c_int
    lib.mkgnn_backward_grad_blocks.argtypes = [P, P]
    lib.mkgnn_debug_grad_blocks_launches.restype = C.c_int64
    lib.mkgnn_debug_grad_blocks_launches.argtypes = []
    lib.mkgnn_debug_poison_backward.restype = C.c_int
    lib.mkgnn_debug_poison_backward.argtypes = [I32]
    lib.mkgnn_index_workspace_bytes.restype = C.c_size_t
    lib.mkgnn_index_workspace_bytes.argtypes = [I64, I64, I64]
    lib.mkgnn_index_build.restype = C.c_int
    lib.mkgnn_index_build.argtypes = [P, P, P, I64, I64, I32, Buckets4, P, P, P, P, P, P, P, P, P, P, C.c_size_t, P, P]
    lib.mkgnn_adamw_step.restype = C.c_int
    lib.mkgnn_adamw_state_floats.restype = C.c_int64
    lib.mkgnn_adamw_state_floats.argtypes = [I64]
    lib.mkgnn_adamw_step.argtypes = [P, I32, P, I32, P]
    lib.mkgnn_adamw_clip_workspace_bytes.restype = C.c_size_t
    lib.mkgnn_adamw_clip_workspace_bytes.argtypes = [P, I32]
    lib.mkgnn_adamw_step_clipped.restype = C.c_int
    lib.mkgnn_adamw_step_clipped.argtypes = [P, I32, P, I32, C.c_float, I32, P, C.c_size_t, P, P]
    lib.mkgnn_adamw_average_floats.restype = C.c_int64
    lib.mkgnn_adamw_average_floats.argtypes = [I64]
    lib.mkgnn_adamw_step_averaged.restype = C.c_int
    lib.mkgnn_adamw_step_averaged.argtypes = [P, I32, P, I32, C.POINTER(AdamWAverage), C.c_float, I32, P, C.c_size_t, P, P]
    lib.mkgnn_flat_swap.restype = C.c_int
    lib.mkgnn_flat_swap.argtypes = [P, I32, P]
    lib.mkgnn_molecule_supported.restype = C.c_int
    lib.mkgnn_molecule_supported.argtypes = [C.POINTER(MoleculeNet), I32]
    lib.mkgnn_molecule_workspace_bytes.restype = C.c_size_t
    lib.mkgnn_molecule_workspace_bytes.argtypes = [C.POINTER(MoleculeNet), I32, I64, I64]
    lib.mkgnn_molecule_step.restype = C.c_int
    lib.mkgnn_molecule_step.argtypes = [C.POINTER(MoleculeNet), C.POINTER(MoleculeBatch), I32, P, P, P, P, P, P, C.c_size_t, P]
    if lib.mkgnn_abi_version() != ABI_VERSION:
        raise MolKGNNLibraryError(f"ABI version {lib.mkgnn_abi_version()} != {ABI_VERSION}: rebuild the library")
    _lib = lib
    return lib


def check(rc: int, what: str) -> None:
    if rc != 0:
        msg = load().mkgnn_last_error()
        raise MolKGNNLibraryError(f"{what}: {msg.decode() if msg else 'error'}")


def ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None or t.numel() == 0 else t.data_ptr()


def stream_ptr(device: torch.device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def require_gpu_tensor(t: torch.Tensor, name: str) -> None:
    if not t.is_cuda:
        raise MolKGNNLibraryError(
            f"{name} is on {t.device}: the kernel convolution runs on an MI355X only (no CPU fallback)")
