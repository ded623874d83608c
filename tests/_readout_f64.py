"""References and the case table of the float64 leg of the separate readout and head operators -- what a training step runs
when the fused tail declines a batch (``readout._tail_limits_ok``): ``readout()`` (``mkgnn_readout_*``), ``readout_blocks()``
(``mkgnn_readout_blocks_*``) and ``head_loss()`` (``mkgnn_head_loss_*`` / ``mkgnn_bce_head_*``).  No GPU in this file.

The references are plain torch on the CPU, evaluated in the dtype they are given; ``both(fn, ...)`` calls one twice, in
float64 (the truth) and in float32 (the yardstick of ``tests/_f64.check``), on inputs drawn in float32 and cast up, so both
legs see identical numbers.

Every case is a named row of a table; a row names the edge of the kernels it is there for and carries a predicate on its own
shapes that proves it gets there (``tests/test_readout_reference_cpu.py`` evaluates every predicate).  The constants the
predicates use are copied from ``csrc/kgnn_readout.hip`` and ``csrc/kgnn_head.hip``; each names what it mirrors.
"""
from __future__ import annotations

import zlib
from dataclasses import dataclass
from functools import lru_cache
from typing import Callable, Dict, List, Tuple

import torch

from tests import _philox
from tests import _topologies as T

# ---------------------------------------------------------------- constants mirrored from the kernels --
TILE = 16                 # kgnn_readout.hip readout_pre_kernel / readout_bwd_atoms_kernel: `ntiles = (a.n + 15) / 16`
PRE_GRID_CAP = 1024       # mkgnn_readout_forward: `(ntiles + 3) / 4 < 1024 ? (ntiles + 3) / 4 : 1024`
PRE_TILES = 4             # readout_pre_kernel: `tile += (int64_t)gridDim.x * 4` (one tile per wave, four waves)
POOL_GRID_CAP = 2048      # mkgnn_readout_forward / _blocks_forward: `(n_mols + 3) / 4 < 2048 ? ... : 2048`
POOL_MOLS = 4             # readout_pool_kernel: `mol += (int64_t)gridDim.x * 4`
RO_ATOM_BLOCKS = 256      # `constexpr int RO_ATOM_BLOCKS = 256`
RO_MOL_BLOCKS = 256       # `constexpr int RO_MOL_BLOCKS = 256`
MOL_CHUNK = 16            # readout_bwd_mol_kernel: `constexpr int MC = 16`; nblk_mol = min((n_mols + 15) / 16, RO_MOL_BLOCKS)
SLAB_PARTS = 8            # slab_reduce_kernel: `per = (g.count + 7) / 8`, inner step 8
DZ_BLOCKS = 2048          # `constexpr int DZ_BLOCKS = 2048`
BWD_BLOCKS_MAX = 4 * (2 * RO_ATOM_BLOCKS - 4)   # mkgnn_readout_blocks_backward: tpw = ceil(tiles_all / (4 * (2 * RO_ATOM_BLOCKS - 4)))
HEAD_ROWS = 16            # kgnn_head.hip: `constexpr int HEAD_ROWS = 16`
HEAD_FINAL_THREADS = 256  # head_forward_final_kernel: `for (int bk = t; bk < nblk; bk += 256)`
HEAD_FINAL_STEP = 32      # head_backward_final_kernel / head_fused_final_kernel: `bk += 32`, loads `bk + 4 * u`, u < 8
HEAD_FINAL_COLS = 64      # the same two kernels: `for (int c0 = 0; c0 < PW; c0 += 64)`, PW = H + 1 (backward) / H + 2 (fused)


def ceil_div(a: int, b: int) -> int:
    return -(-a // b)


def atom_waves(H: int) -> int:
    """readout_bwd_atoms_kernel: `constexpr int NW = NT == 4 ? 4 : 8` (NT = 4: H > 32)."""
    return 8 if H <= 32 else 4


def hidden_stride(H: int) -> int:
    """mkgnn_readout_hidden_stride: `H <= 32 ? 32 : 64`."""
    return 32 if H <= 32 else 64


# ------------------------------------------------------------------------------------------ references --
def swish(x):
    return x * torch.sigmoid(x)


def torch_readout(h, w1, b1, w2, b2, keep, batch, size):
    """``pool(lin2(dropout(swish(lin1(h)))))`` in PyTorch operators on ``h``'s device (reference MolKGNNNet.py:144-146): the fp32
    comparison of ``tests/test_hip_parity.py``."""
    z = torch.nn.functional.linear(h, w1, b1)
    z = z * torch.sigmoid(z)
    if keep is not None:
        z = z * keep
    z = torch.nn.functional.linear(z, w2, b2)
    return torch.zeros(size, w2.shape[0], device=h.device).index_add_(0, batch, z)


def _leaf(t):
    return None if t is None else t.detach().clone().requires_grad_(True)


def _pre_of(h, w1, b1):
    pre = h @ w1.t()
    return pre if b1 is None else pre + b1


def _readout_from_pre(pre, w2, b2, keep, batch, size):
    act = swish(pre)
    if keep is not None:
        act = act * keep
    z = act @ w2.t()
    if b2 is not None:
        z = z + b2
    return torch.zeros(size, w2.shape[0], dtype=pre.dtype).index_add(0, batch, z)


def _readout_of(h, w1, b1, w2, b2, keep, batch, size):
    return _readout_from_pre(_pre_of(h, w1, b1), w2, b2, keep, batch, size)


def dense(h, w1, b1, w2, b2, keep, batch, size, cot) -> Dict[str, torch.Tensor]:
    """``index_add(lin2(keep * swish(lin1(h))))`` in the dtype of ``h`` -> ``out`` and, for the cotangent ``cot`` of it, the
    gradients ``h``, ``w1``, ``b1``, ``w2``, ``b2`` (absent biases: absent keys)."""
    h, w1, b1, w2, b2 = (_leaf(t) for t in (h, w1, b1, w2, b2))
    out = _readout_of(h, w1, b1, w2, b2, keep, batch, size)
    (out * cot).sum().backward()
    res = {"out": out.detach(), "h": h.grad, "w1": w1.grad, "w2": w2.grad}
    if b1 is not None:
        res["b1"] = b1.grad
    if b2 is not None:
        res["b2"] = b2.grad
    return res


def propagate(sim, edge_index):
    """``h[dst] += sim[src]`` over the directed edges (reference KernelLayer.py:119-123)."""
    return torch.zeros_like(sim).index_add(0, edge_index[1], sim[edge_index[0]])


def block_rows(sim_dense, edge_index, w1, b1, w2, b2, keep, batch, size, cot) -> Dict[str, torch.Tensor]:
    """``dense`` behind ``h = propagate(sim_dense)``; ``sim_dense`` is zero outside every atom's own degree block.  Also returns
    the gradient ``sim`` (dense: only an atom's own block of it means anything to the build), the value ``h_value`` and ``dz`` = propagate^T(d pre)."""
    sim, w1, b1, w2, b2 = (_leaf(t) for t in (sim_dense, w1, b1, w2, b2))
    h = propagate(sim, edge_index)
    pre = _pre_of(h, w1, b1)
    pre.retain_grad()
    out = _readout_from_pre(pre, w2, b2, keep, batch, size)
    (out * cot).sum().backward()
    # d z of the kernels' association (z[n] = W1[:, block] sim[n, block], pre = propagate(z)): propagate^T(d pre), [n, H]
    dz = torch.zeros_like(pre).index_add(0, edge_index[0], pre.grad[edge_index[1]])
    res = {"out": out.detach(), "h_value": h.detach(), "sim": sim.grad, "dz": dz, "w1": w1.grad, "w2": w2.grad}
    if b1 is not None:
        res["b1"] = b1.grad
    if b2 is not None:
        res["b2"] = b2.grad
    return res


HEAD_KINDS = ("bce", "mse", "mse_sum")


def head(emb, w, b, y, kind, keep, scale=1.0) -> Dict[str, torch.Tensor]:
    """``pred = (keep * emb) w + b`` and ``loss`` = BCE-with-logits (mean), squared error (mean) or squared error (sum) against
    ``y`` in the dtype of ``emb``, and the gradients ``emb``, ``w``, ``b`` of ``scale * loss``."""
    if kind not in HEAD_KINDS:
        raise ValueError(kind)
    emb, w, b = (_leaf(t) for t in (emb, w, b))
    e = emb if keep is None else emb * keep
    pred = e @ w.reshape(-1)
    if b is not None:
        pred = pred + b.reshape(())
    if kind == "bce":
        # log(1 + e^x) - x y.  (Not max(x, 0) - x y + log1p(e^-|x|) through autograd: the same value, but at x = 0 exactly its two
        # kinks hand autograd 1 - y where the derivative is sigmoid(0) - y.)
        terms = torch.logaddexp(pred, torch.zeros_like(pred)) - pred * y
    else:
        terms = (pred - y) ** 2
    loss = terms.sum() if kind == "mse_sum" else terms.sum() / pred.numel()
    (loss * scale).backward()
    res = {"pred": pred.detach(), "loss": loss.detach(), "emb": emb.grad, "w": w.grad}
    if b is not None:
        res["b"] = b.grad
    return res


def cast(v, dtype):
    return v.to(dtype) if torch.is_tensor(v) and v.is_floating_point() else v


def both(fn: Callable, *args) -> Tuple[Dict[str, torch.Tensor], Dict[str, torch.Tensor]]:
    """``(fn in float32, fn in float64)`` on the same float32-drawn arguments."""
    return fn(*[cast(a, torch.float32) for a in args]), fn(*[cast(a, torch.float64) for a in args])


# --------------------------------------------------------------------------------------------- batches --
_SMALL_CYCLE = (4, 5, 6, 7, 8, 8, 8, 8)          # molecule sizes of the many-molecule batches: 54 atoms per 8 molecules


def _small(times: int) -> List[T.Spec]:
    return T.repeat([T.tree(n) for n in _SMALL_CYCLE], times)


BATCHES: Dict[str, Callable[[], List[T.Spec]]] = {
    "n1": lambda: [T.single()],
    "n15": lambda: [T.chain(15)],
    "n16": lambda: [T.chain(16)],
    "n17": lambda: [T.chain(17)],
    "n63": lambda: [T.tree(63)],
    "n65": lambda: [T.tree(65)],
    # empty molecules first, in the middle and last; one-atom molecules; 7 | 8 | 9 and 15 | 16 | 17 around the pool kernel's
    # 4 * groups pass; 300 atoms: the size that sends a step to these kernels
    "edges": lambda: [T.empty(), T.single(), T.tree(7), T.tree(8), T.chain(9), T.empty(), T.tree(15), T.chain(16), T.tree(17),
                      T.tree(300), T.single(), T.empty()],
    "mixed": lambda: [T.tree(5), T.single(), T.empty(), T.tree(17), T.tree(40), T.pair(), T.chain(3)],
    "many_small": lambda: _small(1250),           # 10 000 molecules, 67 500 atoms
    "half_small": lambda: _small(625),            # 5 000 molecules, 33 750 atoms
    "mols112": lambda: T.repeat([T.tree(8)], 112),    # 896 atoms: 56 tiles
    "mols128": lambda: T.repeat([T.tree(8)], 128),    # 1 024 atoms: 64 tiles
    "mols129": lambda: T.repeat([T.tree(8)], 129),    # 1 032 atoms: 65 tiles
    "mols56": lambda: T.repeat([T.tree(8)], 56),      # 448 atoms: 28 tiles
    "mols64": lambda: T.repeat([T.tree(8)], 64),      # 512 atoms: 32 tiles
    "mols65": lambda: T.repeat([T.tree(8)], 65),      # 520 atoms: 33 tiles
    "pairs": lambda: T.repeat([T.pair()], 40),
    # atoms in no bucket: degree 0 (single), 5 and 9 (the hubs: more than four neighbours in the d z gather)
    "hubs": lambda: [T.single(), T.star(5), T.tree(9), T.star(9), T.single(), T.pair(), T.tree(20), T.empty()],
    "bucketed": lambda: [T.tree(7), T.pair(), T.chain(9), T.tree(16), T.tree(33), T.pair()],
}


@lru_cache(maxsize=None)
def batch(name: str):
    """The CPU ``GraphBatch`` of a named molecule list (node and bond features are not used by the readout: width 4 and 1)."""
    return T.batch_of(BATCHES[name](), F=4, E=1, seed=zlib.crc32(name.encode()) % 1000)


@lru_cache(maxsize=None)
def bucket_of_atom(name: str) -> torch.Tensor:
    """[n] the degree bucket 1 .. 4 every atom is in, 0 for atoms in none."""
    b = batch(name)
    deg = torch.zeros(b.x.shape[0], dtype=torch.long)
    for d in range(1, 5):
        deg[getattr(b, f"selected_index_deg{d}")] = d
    return deg


def bucket_counts(name: str) -> Tuple[int, ...]:
    b = batch(name)
    return tuple(int(getattr(b, f"selected_index_deg{d}").numel()) for d in range(1, 5))


def _seed(*parts) -> int:
    return zlib.crc32(repr(parts).encode()) & 0x7FFFFFFF


# ----------------------------------------------------------------------------------------- dense readout --
@dataclass(frozen=True)
class DenseCase:
    name: str
    edge: str                                     # the edge of the kernels this row is there for
    mols: str                                     # key of BATCHES
    F: int
    H: int
    G: int
    reaches: Callable[[Dict[str, int]], bool]     # on dense_launch(...) of this row: proves the row gets to its edge

    def launch(self) -> Dict[str, int]:
        b = batch(self.mols)
        return dense_launch(int(b.x.shape[0]), int(b.num_graphs), self.F, self.H, T.molecule_sizes(b))


def dense_launch(n: int, n_mols: int, F: int, H: int, sizes=()) -> Dict[str, int]:
    """What ``mkgnn_readout_forward`` / ``_backward`` launch for this shape (the arithmetic of the two functions)."""
    ntiles = ceil_div(n, TILE)
    pre_blocks = min(ceil_div(ntiles, PRE_TILES), PRE_GRID_CAP)
    pool_blocks = min(ceil_div(n_mols, POOL_MOLS), POOL_GRID_CAP)
    nw = atom_waves(H)
    nblk_atoms = min(ceil_div(ntiles, nw), RO_ATOM_BLOCKS)
    nblk_mol = min(ceil_div(n_mols, MOL_CHUNK), RO_MOL_BLOCKS)
    return dict(n=n, n_mols=n_mols, ntiles=ntiles, last_tile_rows=n - TILE * (ntiles - 1),
                pre_rounds=ceil_div(ntiles, PRE_TILES * pre_blocks), pool_rounds=ceil_div(n_mols, POOL_MOLS * pool_blocks),
                nblk_atoms=nblk_atoms, tiles_per_wave=ceil_div(ntiles, nw * nblk_atoms),
                nblk_mol=nblk_mol, mols_per_block=ceil_div(n_mols, nblk_mol),
                NU=1 if F <= 64 else 2, HP=hidden_stride(H), groups=64 // hidden_stride(H), F4=F + (-F) % 4,
                sizes=tuple(sizes))


DENSE_F = (1, 4, 27, 63, 64, 65, 127, 128)
DENSE_H = (1, 5, 31, 32, 33, 64)
DENSE_G = (1, 7, 32, 33, 64)

# (F, H, G) drawn so that every value above occurs at least twice and neighbours across a boundary meet different partners
_WIDTHS = [(1, 1, 1), (4, 5, 7), (27, 31, 32), (63, 32, 33), (64, 33, 64), (65, 64, 1), (127, 1, 7), (128, 5, 32),
           (1, 31, 33), (4, 32, 64), (27, 33, 1), (63, 64, 7), (64, 1, 32), (65, 5, 33), (127, 32, 64), (128, 33, 1),
           (128, 64, 64), (65, 31, 7)]

DENSE_WIDTHS: List[DenseCase] = [
    DenseCase(f"w{F}x{H}x{G}", "F at 64 | 65 (NU), 128, F % 4 != 0 under a padded stride; H at 32 | 33 (HP, groups); G = 1, 64",
              "mixed", F, H, G,
              (lambda F, H: lambda s: s["NU"] == (1 if F <= 64 else 2) and s["HP"] == (32 if H <= 32 else 64)
               and s["groups"] == (2 if H <= 32 else 1) and s["F4"] % 4 == 0 and s["F4"] - F == (-F) % 4 and s["ntiles"] > 1
               and 0 in s["sizes"] and 1 in s["sizes"])(F, H))
    for F, H, G in _WIDTHS]

_SIZE_SHAPES = {"h20": (6, 20, 9), "h40": (6, 40, 9)}            # small F in the size cases, on both sides of H = 32


def _size_rows() -> List[DenseCase]:
    rows = []
    for hw, (F, H, G) in _SIZE_SHAPES.items():
        for n in (1, 15, 16, 17, 63, 65):
            rows.append(DenseCase(f"n{n}_{hw}", "n_atoms around the 16-atom tile: one atom, a partial / whole / whole + 1 tile",
                                  f"n{n}", F, H, G,
                                  (lambda n: lambda s: s["n"] == n and s["ntiles"] == ceil_div(n, 16)
                                   and s["last_tile_rows"] == (n - 1) % 16 + 1)(n)))
        rows.append(DenseCase(f"edges_{hw}", "empty molecule first / middle / last, one-atom molecules, 7 8 9 and 15 16 17 atoms "
                              "around the pool kernel's 4 * groups pass, a 300-atom molecule", "edges", F, H, G,
                              lambda s: s["sizes"] == (0, 1, 7, 8, 9, 0, 15, 16, 17, 300, 1, 0)))
        rows.append(DenseCase(f"many_small_{hw}", "pre cap 1024 x 4 tiles, pool cap 2048 x 4, RO_ATOM_BLOCKS, RO_MOL_BLOCKS, the MC "
                              "chunk loop, a 256-slab reduction", "many_small", F, H, G,
                              lambda s: s["n"] > 65536 and s["n_mols"] >= 8300 and min(s["sizes"]) >= 4 and max(s["sizes"]) <= 8
                              and s["ntiles"] > PRE_TILES * PRE_GRID_CAP and s["pre_rounds"] > 1
                              and s["n_mols"] > POOL_MOLS * POOL_GRID_CAP and s["pool_rounds"] > 1
                              and s["nblk_atoms"] == RO_ATOM_BLOCKS and s["tiles_per_wave"] > 1
                              and s["n_mols"] > MOL_CHUNK * RO_MOL_BLOCKS and s["nblk_mol"] == RO_MOL_BLOCKS
                              and s["mols_per_block"] > MOL_CHUNK))
    # slab counts: nblk_atoms = ceil(ntiles / NW), NW = 8 (H <= 32) or 4 (H > 32); 112 / 128 / 129 molecules also give 7 / 8 / 9 molecule slabs
    for hw, table in (("h20", ((7, "mols112"), (8, "mols128"), (9, "mols129"))), ("h40", ((7, "mols56"), (8, "mols64"), (9, "mols65")))):
        F, H, G = _SIZE_SHAPES[hw]
        for count, mols in table:
            rows.append(DenseCase(f"slabs{count}_{hw}", f"slab_reduce_kernel with count = {count} (per = ceil(count / 8), inner step 8)",
                                  mols, F, H, G,
                                  (lambda count: lambda s: s["nblk_atoms"] == count
                                   and ceil_div(count, SLAB_PARTS) == (1 if count <= SLAB_PARTS else 2))(count)))
    return rows


DENSE_SIZES: List[DenseCase] = _size_rows()
DENSE_CASES: Dict[str, DenseCase] = {c.name: c for c in DENSE_WIDTHS + DENSE_SIZES}


@lru_cache(maxsize=None)
def dense_inputs(name: str, bias: bool, keep: bool) -> Dict[str, object]:
    """float32 CPU inputs of a dense row: weights ``randn * fan_in ** -0.5`` as the fp32 tests draw them."""
    c = DENSE_CASES[name]
    b = batch(c.mols)
    n, size = int(b.x.shape[0]), int(b.num_graphs)
    g = torch.Generator().manual_seed(_seed("dense", name))
    rnd = lambda *s: torch.randn(*s, generator=g)
    return dict(h=rnd(n, c.F), w1=rnd(c.H, c.F) * c.F ** -0.5, b1=rnd(c.H) if bias else None,
                w2=rnd(c.G, c.H) * c.H ** -0.5, b2=rnd(c.G) if bias else None,
                keep=((torch.rand(n, c.H, generator=g) > 0.25).float() / 0.75) if keep else None,
                batch=b.batch, size=size, cot=rnd(size, c.G))


@lru_cache(maxsize=None)
def dense_reference(name: str, bias: bool, keep: bool):
    """(float32 leg, float64 leg) of a dense row: computed once, shared, never written to."""
    i = dense_inputs(name, bias, keep)
    return both(dense, i["h"], i["w1"], i["b1"], i["w2"], i["b2"], i["keep"], i["batch"], i["size"], i["cot"])


# -------------------------------------------------------------------------------------- block-row readout --
@dataclass(frozen=True)
class BlockCase:
    name: str
    edge: str
    mols: str
    counts: Tuple[int, int, int, int]
    reaches: Callable[[Dict[str, object]], bool]
    hidden: Tuple[int, ...] = (5, 32, 33, 64)     # the H this row runs at (G follows: BLOCK_G)

    def launch(self, H: int = 32) -> Dict[str, object]:
        return block_launch(self.mols, self.counts, H)


BLOCK_G = {5: 7, 20: 9, 32: 32, 33: 1, 40: 9, 64: 64}


def block_launch(mols: str, counts, H: int) -> Dict[str, object]:
    """What ``mkgnn_readout_blocks_forward`` / ``_backward`` launch for this batch and these kernel counts."""
    b = batch(mols)
    n, cnt = int(b.x.shape[0]), bucket_counts(mols)
    offs = [sum(counts[:d]) for d in range(4)]
    tiles = [ceil_div(cnt[d], TILE) if counts[d] > 0 else 0 for d in range(4)]
    tiles_all = sum(tiles)
    tpw = max(1, ceil_div(tiles_all, BWD_BLOCKS_MAX))
    rpb = 256 // (hidden_stride(H) // 4)                              # readout_dz_gather_kernel: `RPB = 256 / CPR`
    dz_blocks = min(ceil_div(n, rpb), DZ_BLOCKS)
    return dict(n=n, n_mols=int(b.num_graphs), K=sum(counts), cnt=cnt, off=tuple(offs), align=tuple(o % 4 for o in offs),
                n_focal=sum(c for c, L in zip(cnt, counts) if L > 0), n_bucketed=sum(cnt),
                nj=tuple(ceil_div(L, 16) for L in counts), tiles_all=tiles_all, tiles_per_wave=tpw,
                absent=tuple(L > 0 and c == 0 for c, L in zip(cnt, counts)),
                dz_rounds=ceil_div(n, rpb * dz_blocks), max_degree=int(T.degrees(b).max()) if n else 0,
                mols_per_block=ceil_div(int(b.num_graphs), min(ceil_div(int(b.num_graphs), MOL_CHUNK), RO_MOL_BLOCKS)),
                sizes=tuple(T.molecule_sizes(b)))


def _partial_chunk(L: int) -> bool:
    """block_project_mfma_kernel: a lane's four columns `col .. col + 3` with `col + 3 < T.L` false and `col < T.L` true."""
    return L % 4 != 0


BLOCK_CASES_LIST: List[BlockCase] = [
    BlockCase("c1111", "L = 1: every chunk is the partial one; offsets 0 1 2 3 (all four alignments of load4_at's caller)", "edges",
              (1, 1, 1, 1), lambda s: s["align"] == (0, 1, 2, 3) and s["nj"] == (1, 1, 1, 1) and all(c > 0 for c in s["cnt"])),
    BlockCase("c3251", "load4_at at alignments 0, 3, 1, 2 (offsets 0, 3, 5, 10); L < 4; the whole chunk of L = 5 unaligned", "edges",
              (3, 2, 5, 1), lambda s: s["off"] == (0, 3, 5, 10) and s["align"] == (0, 3, 1, 2) and all(c > 0 for c in s["cnt"])),
    BlockCase("c16_17_48_49", "L at 16 | 17 and 48 | 49 (nj 1 | 2 and 3 | 4), a one-column last chunk", "edges",
              (16, 17, 48, 49), lambda s: s["nj"] == (1, 2, 3, 4) and all(c > 0 for c in s["cnt"])),
    BlockCase("c64x3_63", "K = 255, L = 64 (nj = 4, no partial chunk) beside L = 63", "edges",
              (64, 64, 64, 63), lambda s: s["K"] == 255 and s["nj"] == (4, 4, 4, 4) and all(c > 0 for c in s["cnt"])),
    BlockCase("c10_20_30_50", "the reference's counts on a batch with empty, one-atom and 300-atom molecules", "edges",
              (10, 20, 30, 50), lambda s: s["sizes"] == (0, 1, 7, 8, 9, 0, 15, 16, 17, 300, 1, 0) and s["n_focal"] < s["n"]),
    BlockCase("c4_0_9_0", "buckets with atoms but L_d = 0: their z rows come from the memset, grad W1 has no columns for them",
              "edges", (4, 0, 9, 0), lambda s: s["cnt"][1] > 0 and s["cnt"][3] > 0 and s["n_focal"] < s["n_bucketed"]),
    BlockCase("pairs_only", "degrees 2 .. 4 have kernels but no atoms: the `absent` memset of grad W1 ahead of the slab reduction",
              "pairs", (10, 20, 30, 50), lambda s: s["absent"] == (False, True, True, True) and s["cnt"][0] == s["n"]),
    BlockCase("hubs", "atoms in no bucket (degree 0, 5, 9): memset of z; more than four neighbours in readout_dz_gather_kernel's "
              "serial tail", "hubs", (3, 2, 5, 1), lambda s: s["n_focal"] < s["n"] and s["max_degree"] > 4),
    BlockCase("all_bucketed", "every atom is in a bucket: no memset of z, every z row must be written by a tile", "bucketed",
              (3, 2, 5, 1), lambda s: s["n_focal"] == s["n"] and all(c > 0 for c in s["cnt"])),
    BlockCase("many_small", "tiles_per_wave > 1 (more than 4 x 508 tiles), DZ_BLOCKS x 32 rows, pool and molecule caps", "many_small",
              (3, 2, 5, 1), lambda s: s["n"] > 65536 and s["tiles_all"] > BWD_BLOCKS_MAX and s["tiles_per_wave"] > 1
              and s["dz_rounds"] > 1 and s["n_mols"] > POOL_MOLS * POOL_GRID_CAP and s["mols_per_block"] > MOL_CHUNK, hidden=(20,)),
    BlockCase("half_small_wide", "DZ_BLOCKS x 16 rows at H > 32, tiles_per_wave > 1", "half_small",
              (3, 2, 5, 1), lambda s: s["n"] > 32768 and s["dz_rounds"] > 1 and s["tiles_per_wave"] > 1, hidden=(40,)),
]
BLOCK_CASES: Dict[str, BlockCase] = {c.name: c for c in BLOCK_CASES_LIST}


@lru_cache(maxsize=None)
def block_inputs(name: str, H: int, full: bool) -> Dict[str, object]:
    """float32 CPU inputs of a block-row row at hidden width ``H``; ``full``: biases and dropout multipliers present.
    ``sim`` is zero outside every atom's own degree block (``mask``)."""
    c = BLOCK_CASES[name]
    b = batch(c.mols)
    n, size, K, G = int(b.x.shape[0]), int(b.num_graphs), sum(c.counts), BLOCK_G[H]
    g = torch.Generator().manual_seed(_seed("blocks", name, H))
    rnd = lambda *s: torch.randn(*s, generator=g)
    deg = bucket_of_atom(c.mols)
    mask = torch.zeros(n, K, dtype=torch.bool)
    off = 0
    for d in range(1, 5):
        mask[deg == d, off:off + c.counts[d - 1]] = True
        off += c.counts[d - 1]
    return dict(sim=torch.where(mask, rnd(n, K), torch.zeros(())), mask=mask, edge_index=b.edge_index,
                w1=rnd(H, K) * K ** -0.5, b1=rnd(H) if full else None, w2=rnd(G, H) * H ** -0.5, b2=rnd(G) if full else None,
                keep=((torch.rand(n, H, generator=g) > 0.25).float() / 0.75) if full else None,
                batch=b.batch, size=size, cot=rnd(size, G), G=G)


@lru_cache(maxsize=None)
def block_reference(name: str, H: int, full: bool):
    i = block_inputs(name, H, full)
    return both(block_rows, i["sim"], i["edge_index"], i["w1"], i["b1"], i["w2"], i["b2"], i["keep"], i["batch"], i["size"], i["cot"])


# -------------------------------------------------------------------------------------------------- head --
@dataclass(frozen=True)
class HeadCase:
    name: str
    edge: str
    B: int
    H: int
    bias: bool
    emb_grad: bool
    p: float
    n_pad: int
    reaches: Callable[[Dict[str, int]], bool]

    def launch(self) -> Dict[str, int]:
        nb = ceil_div(self.B, HEAD_ROWS)
        return dict(B=self.B, H=self.H, nb=nb, last_rows=self.B - HEAD_ROWS * (nb - 1), PW_bwd=self.H + 1, PW_fused=self.H + 2,
                    final_rounds_fwd=ceil_div(nb, HEAD_FINAL_THREADS), final_rounds=ceil_div(nb, HEAD_FINAL_STEP),
                    wide=self.H > 32, wide_lanes=self.H - 32 if self.H > 32 else 0)


HEAD_B = (1, 15, 16, 17, 496, 512, 528, 577, 592, 4097)
HEAD_H = (1, 31, 32, 33, 62, 63, 64)
HEAD_SEED = 1234          # the generator seed of the dropout rows (offset 0): the mask is _philox.head_mask(HEAD_SEED, 0, B, H, p)
HEAD_SCALE = 1.7          # the split entry points' grad_loss


def _head_rows() -> List[HeadCase]:
    # (B, H, bias, emb_grad, p, n_pad)
    table = [(1, 1, True, True, 0.0, 0), (15, 31, False, True, 0.25, 3), (16, 32, True, False, 0.0, 0), (17, 33, True, True, 0.25, 0),
             (496, 62, True, True, 0.0, 5), (512, 63, False, False, 0.25, 0), (528, 64, True, True, 0.25, 0), (576, 1, True, True, 0.25, 0),
             (577, 31, True, False, 0.0, 2), (592, 32, False, True, 0.0, 0), (4097, 33, True, True, 0.0, 0), (4097, 64, True, True, 0.25, 1),
             (1, 64, False, True, 0.25, 0), (15, 62, True, False, 0.0, 0), (16, 63, True, True, 0.0, 4), (17, 1, False, True, 0.0, 0),
             (496, 33, False, True, 0.25, 0), (512, 64, True, True, 0.0, 0), (528, 62, True, False, 0.25, 0), (577, 63, True, True, 0.25, 0),
             (592, 31, True, True, 0.25, 0), (1, 32, True, True, 0.0, 2)]
    edge_of_B = {1: "one row: 15 clamped rows in the only block", 15: "B = HEAD_ROWS - 1", 16: "B = HEAD_ROWS", 17: "B = HEAD_ROWS + 1",
                 496: "nb = 31: below one `bk += 32` round", 512: "nb = 32: exactly one round", 528: "nb = 33: a second round of one block",
                 576: "nb = 36: the second round's `bk + 4 u` ends on a whole u", 577: "nb = 37: one block past it",
                 592: "nb = 37 with a whole last block", 4097: "nblk = 257: head_forward_final_kernel's strided sum takes a second term"}
    pred_of_B = {1: lambda s: s["nb"] == 1 and s["last_rows"] == 1, 15: lambda s: s["nb"] == 1 and s["last_rows"] == 15,
                 16: lambda s: s["nb"] == 1 and s["last_rows"] == 16, 17: lambda s: s["nb"] == 2 and s["last_rows"] == 1,
                 496: lambda s: s["nb"] == HEAD_FINAL_STEP - 1 and s["final_rounds"] == 1,
                 512: lambda s: s["nb"] == HEAD_FINAL_STEP and s["final_rounds"] == 1,
                 528: lambda s: s["nb"] == HEAD_FINAL_STEP + 1 and s["final_rounds"] == 2, 576: lambda s: s["nb"] == 36,
                 577: lambda s: s["nb"] == 37 and s["last_rows"] == 1, 592: lambda s: s["nb"] == 37 and s["last_rows"] == 16,
                 4097: lambda s: s["nb"] > HEAD_FINAL_THREADS and s["final_rounds_fwd"] == 2}
    edge_of_H = {1: "H = 1", 31: "H = 31", 32: "H = 32: no wide path", 33: "H = 33: the `h0 >= 32` wide path with one lane",
                 62: "PW = 63 / 64: one `c0` round in both finals", 63: "PW = 64 / 65: the fused final takes a second `c0` round",
                 64: "PW = 65 / 66: both finals take a second `c0` round"}
    pred_of_H = {1: lambda s: s["H"] == 1, 31: lambda s: not s["wide"], 32: lambda s: not s["wide"] and s["H"] == 32,
                 33: lambda s: s["wide"] and s["wide_lanes"] == 1,
                 62: lambda s: s["PW_bwd"] <= HEAD_FINAL_COLS and s["PW_fused"] <= HEAD_FINAL_COLS,
                 63: lambda s: s["PW_bwd"] <= HEAD_FINAL_COLS < s["PW_fused"],
                 64: lambda s: s["PW_bwd"] > HEAD_FINAL_COLS and s["PW_fused"] > HEAD_FINAL_COLS}
    rows = []
    for B, H, bias, emb_grad, p, n_pad in table:
        rows.append(HeadCase(f"B{B}xH{H}", edge_of_B[B] + "; " + edge_of_H[H], B, H, bias, emb_grad, p, n_pad,
                             (lambda fb, fh: lambda s: fb(s) and fh(s))(pred_of_B[B], pred_of_H[H])))
    return rows


HEAD_CASES_LIST: List[HeadCase] = _head_rows()
HEAD_CASES: Dict[str, HeadCase] = {c.name: c for c in HEAD_CASES_LIST}

# BCE at saturated logits: rows 0 .. 5 of the embedding are +-e_0 or 0 and w[0] = 90 with no bias, so their logits are exactly
# +90, -90 and 0 (each with target 0 and target 1); expf(-x) overflows at x = -90 and 1 / (1 + inf) must come out 0
SATURATED = HeadCase("bce_pm90", "BCE at logits of +-90 and exactly 0: expf(-x) overflows, 1 / (1 + inf) = 0", 21, 5, False, True, 0.0, 0,
                     lambda s: s["nb"] == 2)
SATURATED_LOGITS = (90.0, 90.0, -90.0, -90.0, 0.0, 0.0)
SATURATED_TARGETS = (0.0, 1.0, 0.0, 1.0, 0.0, 1.0)


@lru_cache(maxsize=None)
def head_inputs(name: str, kind: str) -> Dict[str, object]:
    """float32 CPU inputs of a head row: ``emb`` holds ``B + n_pad`` rows, the leading ``B`` enter the loss."""
    c = SATURATED if name == SATURATED.name else HEAD_CASES[name]
    g = torch.Generator().manual_seed(_seed("head", name, kind))
    emb = torch.randn(c.B + c.n_pad, c.H, generator=g) * 2
    w = torch.randn(c.H, generator=g) * c.H ** -0.5
    b = torch.randn(1, generator=g) if c.bias else None
    if kind == "bce":
        y = (torch.rand(c.B, generator=g) < 0.3).float()
    else:
        y = torch.randn(c.B, generator=g) * 1.5 - 8.0
    if name == SATURATED.name:
        w[0] = 90.0
        for r, x in enumerate(SATURATED_LOGITS):
            emb[r] = 0.0
            emb[r, 0] = x / 90.0
            y[r] = SATURATED_TARGETS[r]
    keep = torch.from_numpy(_philox.head_mask(HEAD_SEED, 0, c.B, c.H, c.p)) if c.p > 0.0 else None
    return dict(emb=emb, w=w, b=b, y=y, keep=keep)


@lru_cache(maxsize=None)
def head_reference(name: str, kind: str, scale: float):
    c = SATURATED if name == SATURATED.name else HEAD_CASES[name]
    i = head_inputs(name, kind)
    return both(lambda emb, w, b, y, keep: head(emb, w, b, y, kind, keep, scale), i["emb"][:c.B], i["w"], i["b"], i["y"], i["keep"])
