"""Screening a compound library that lives in device memory: score every molecule of a ``shards.ResidentShard`` (the short tail
included) from ONE captured graph per shard, and keep the best ``k`` of all shards in a running list on the device.

``topk_update_reference``  the order of the ranking, in numpy: the specification ``mkgnn_topk_update`` is tested against
``TopK``                   the running list on the device (``mkgnn_topk_update``: sorted, updated in place, capturable)
``score_resident``         ``scores[n_molecules]`` of one resident shard, optionally feeding a ``TopK``
``screen``                 a sequence (or a generator) of resident shards -> the top ``k`` of all of them

Every assay of a multi-task model (``GNNModel(task_dim=T)``, ``1 <= T <= 32``) from ONE pass over the library -- the network runs
once per molecule, ``GNNModel.predict_tasks`` gives all ``T`` outputs, ``T`` running lists are updated in one launch:

``topk_update_tasks_reference``  ``topk_update_reference`` list by list: the specification of ``mkgnn_topk_update_tasks``
``TopKTasks``                    ``T`` running lists on the device (``[T, k]`` tensors)
``score_resident_tasks``         ``scores[n_molecules, T]`` of one resident shard, optionally feeding a ``TopKTasks``
``screen_tasks``                 shards -> the top ``k`` per task

Analogue search -- the library molecules whose graph embeddings lie closest, by cosine similarity, to a few query embeddings
(``GNNModel.embed``, ``mkgnn_embed_cosine``; one list per query, a ``TopKTasks`` of ``Q <= 32`` lists):

``cosine_reference`` / ``cosine_bound``  the similarity in float64 numpy, and the error bound of a float32 evaluation
``embed_resident``                       ``emb[n_molecules, G]`` of one resident shard
``nearest_resident``                     ``sim[n_molecules, Q]`` of one resident shard, optionally feeding the ``Q`` lists
``nearest``                              shards -> the ``k`` nearest molecules per query
``rank_embeddings``                      the same ranking from a stored embedding matrix

The analogues of ANY number of queries -- every confirmed active of an assay -- in one pass: fused cosine and top-k
(``mkgnn_embed_knn_update``: raw embeddings and raw queries in, one sorted list per query updated in place, no similarity matrix;
the similarities and the order are those above, bit for bit; lists of at most 64 entries):

``NearestLists``                         ``Q`` running lists on the device (``[Q, k]`` tensors), ``k <= 64``, ``Q`` up to 2^20
``nearest_many_resident``                one captured pass over a resident shard feeding the ``Q`` lists; returns its embeddings
``nearest_many``                         shards -> the ``k`` nearest molecules per query, ``nearest``'s keys without ``sims``
``nearest_embeddings``                   the same ranking from a stored embedding matrix

Why a hit scores what it scores -- every atom's exact share of every output (``GNNModel.atom_contributions``,
``mkgnn_atom_contributions``):

``explain_resident``                     ``contrib[atoms of the listed molecules, T]`` for a list of ids of one resident shard

Novel hits -- how close every library molecule lies to a set of known ones (``mkgnn_embed_max_cosine``), and a ranking that keeps
only the molecules inside a band of that similarity (``mkgnn_select_rows`` in front of the running list):

``max_cosine_reference`` / ``select_rows_reference``  the two definitions in numpy
``reference_similarity_resident``        ``(max_sim[n_molecules], arg_ref[n_molecules])`` of one resident shard
``screen_novel``                         shards -> the top ``k`` of the molecules whose nearest reference passes the bounds

Diverse hits -- the best molecule of every chemical series among the top of a ranking, and the series every other hit belongs to
(leader clustering of the ranked list by the cosine similarity of the graph embeddings, ``mkgnn_diverse_pick``):

``diverse_pick_reference``               the walk in numpy over a given similarity matrix: the definition
``pick_diverse_embeddings``              the stored-embedding route: embeddings and scores -> picks, leaders, cluster sizes
``screen_diverse``                       shards -> a pool of the best ``pool`` molecules, and the ``k`` diverse picks among them

Neighbour counts and Butina clusters -- how many molecules lie above a similarity threshold of each (``mkgnn_embed_count_within``),
and the clustering that ranks by that count and then does the leader walk (``mkgnn_diverse_pick``) in count order:

``count_within_reference`` / ``butina_reference``  the two definitions in numpy over a given similarity matrix
``neighbour_counts``                     stored embeddings against any number of references: analogue counts
``cluster_butina_embeddings``            stored embeddings -> centroids, every row's cluster, the best-scoring member of each

Neighbour lists and linked components -- which molecules lie above the threshold (``mkgnn_embed_neighbours_within``), and the
connected components of that graph (``mkgnn_graph_components``), the one partition with no pair above it across its parts:

``neighbours_reference`` / ``components_reference``  the two definitions on the host
``neighbour_lists``                      stored embeddings against up to 2^20 references: the analogues of every row, as CSR lists
``cluster_components_embeddings``        stored embeddings -> every row's component, their sizes, the lists, the best member of each
``split_leakage``                        stored pairs by (fold of the row, fold of the reference): what a split lets through

MaxMin picking -- ``k`` molecules that are as different from each other as possible (the farthest-first traversal,
``mkgnn_maxmin_pick``), and the similarity at which each was taken: the selection by budget instead of by threshold:

``maxmin_pick_reference``                the rounds in numpy over a given similarity matrix: the definition
``pick_maxmin_embeddings``               stored embeddings (a deck one owns, rows to leave out) -> picks, ``pick_sim``, nearest picks
``select_maxmin``                        shards -> every molecule embedded, one selection over all of them

What each kernel learned -- for every kernel column of a convolution layer the ``k`` atoms of the library it matches best
(``GNNModel.kernel_scores``, ``mkgnn_kernel_exemplars_update``; one running list per column, a candidate is an atom):

``kernel_exemplars_reference``           the definition in numpy
``KernelExemplars``                      the running lists on the device (``[n_columns, k]`` tensors)
``kernel_exemplars``                     shards -> ``top_score`` / ``top_shard`` / ``top_mol`` / ``top_atom`` per kernel column
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

EMPTY = (np.float32(-np.inf), np.int32(-1), np.int32(-1))     # an empty slot of a list


def empty_top(k: int):
    """A list of ``k`` empty slots: ``(top_score float32[k], top_shard int32[k], top_mol int32[k])``."""
    return (np.full(k, EMPTY[0], dtype=np.float32), np.full(k, EMPTY[1], dtype=np.int32), np.full(k, EMPTY[2], dtype=np.int32))


def topk_update_reference(top, scores, ids, n_valid, shard_tag):
    """The definition of ``mkgnn_topk_update`` (include/molkgnn_hip.h), on the host: ``top = (score, shard, mol)`` arrays of
    length K -> the best K entries of ``top`` and ``{(scores[i], shard_tag, ids[i]) : i < min(n_valid, len(scores))}``, sorted:

    * occupied slots before empty ones (``(-inf, -1, -1)``; a real entry whose score is ``-inf`` ranks before them),
    * non-NaN scores before NaN scores, then score descending with ``-0.0 == +0.0``,
    * then shard ascending, then molecule id ascending,
    * entries alike in all of that in their order of arrival: the old list first, then the batch by slot (``np.lexsort`` is
      stable).

    Repeated ``(shard, mol)`` pairs are kept.  Score BITS are carried over (a NaN's payload, a zero's sign)."""
    ts, th, tm = (np.asarray(a) for a in top)
    K = ts.shape[0]
    scores = np.asarray(scores, dtype=np.float32).reshape(-1)
    n = int(min(max(int(n_valid), 0), scores.shape[0]))
    s = np.concatenate([ts.astype(np.float32, copy=False), scores[:n]])
    h = np.concatenate([th.astype(np.int32, copy=False), np.full(n, int(shard_tag), dtype=np.int32)])
    m = np.concatenate([tm.astype(np.int32, copy=False), np.asarray(ids, dtype=np.int32).reshape(-1)[:n]])
    empty = (s.view(np.int32) == np.float32(-np.inf).view(np.int32)) & (h == -1) & (m == -1)
    nan = np.isnan(s)
    with np.errstate(invalid="ignore"):
        falling = np.where(nan, np.float32(0), -(s + np.float32(0)))            # (-0.0 + 0.0 = +0.0; descending by negation)
    order = np.lexsort((m, h, falling, nan, empty))[:K]                          # (the LAST key is the primary one)
    return s[order].copy(), h[order].copy(), m[order].copy()


def topk_update_tasks_reference(top, scores, ids, n_valid, shard_tag):
    """The definition of ``mkgnn_topk_update_tasks``, on the host: ``top = (score, shard, mol)`` arrays ``[T, K]``, ``scores``
    ``[T, n]`` -> list ``t`` becomes ``topk_update_reference`` of list ``t`` and ``scores[t]``; ``ids``, ``n_valid`` and ``shard_tag``
    are the same for every task."""
    ts, th, tm = (np.asarray(a) for a in top)
    scores = np.asarray(scores, dtype=np.float32)
    if ts.ndim != 2 or scores.ndim != 2 or scores.shape[0] != ts.shape[0]:
        raise ValueError("top arrays [T, K] and scores [T, n]")
    rows = [topk_update_reference((ts[t], th[t], tm[t]), scores[t], ids, n_valid, shard_tag) for t in range(ts.shape[0])]
    return tuple(np.stack([r[j] for r in rows]) for j in range(3))


class TopK:
    """The running top ``k`` of a screen on ``device``: three tensors ``top_score`` float32, ``top_shard`` int32, ``top_mol``
    int32 of length ``k``, always sorted by the order of ``topk_update_reference``; the kernels' workspace; and the two device
    int32 scalars every update reads ON THE DEVICE -- ``n_valid`` (how many leading slots of the batch count) and
    ``shard_tag`` (the shard the batch's molecule ids belong to) -- so that one captured ``update`` serves every batch of every
    shard: refill the scalars (and the inputs) between replays."""

    def __init__(self, k: int, device):
        self._allocate(k, device, (int(k),))

    def _allocate(self, k: int, device, shape) -> None:
        from . import _lib
        self.k, self.device = int(k), torch.device(device)
        if not 1 <= self.k <= _lib.TOPK_MAX_K:
            raise ValueError(f"k = {k} outside [1, {_lib.TOPK_MAX_K}] (MKGNN_TOPK_MAX_K)")
        if self.device.type != "cuda":
            raise ValueError("a running list lives on the GPU (topk_update_reference is the host form)")
        _lib.load()
        dev = self.device
        self.top_score = torch.empty(shape, dtype=torch.float32, device=dev)
        self.top_shard = torch.empty(shape, dtype=torch.int32, device=dev)
        self.top_mol = torch.empty(shape, dtype=torch.int32, device=dev)
        self.n_valid = torch.zeros(1, dtype=torch.int32, device=dev)
        self.shard_tag = torch.zeros(1, dtype=torch.int32, device=dev)
        self.workspace = None
        self.reset()

    def reset(self) -> None:
        """All slots empty."""
        self.top_score.fill_(float("-inf"))
        self.top_shard.fill_(-1)
        self.top_mol.fill_(-1)

    def _workspace_bytes(self, batch: int) -> int:
        from . import _lib
        return int(_lib.load().mkgnn_topk_workspace_bytes(int(batch), self.k))

    def reserve(self, batch: int) -> None:
        """Make the workspace large enough for updates of ``batch`` slots (before a capture: a captured update must not allocate)."""
        need = self._workspace_bytes(batch)
        if need == 0:
            raise ValueError(f"a batch of {batch} slots cannot be ranked")
        if self.workspace is None or self.workspace.numel() < need:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError(f"{type(self).__name__}.update would allocate its workspace inside a capture: call reserve(batch) first")
            self.workspace = torch.empty(need, dtype=torch.uint8, device=self.device)

    def _scalar(self, own: torch.Tensor, value) -> torch.Tensor:
        if value is None:
            return own
        if torch.is_tensor(value):
            if value.dtype != torch.int32 or value.numel() != 1 or value.device != self.device:
                raise ValueError("a device scalar of an update is one int32 on the list's device")
            return value                                 # (read where it lies: nothing is copied)
        own.fill_(int(value))
        return own

    _WHOSE = "list's"

    def _check_batch(self, scores: torch.Tensor, ids: torch.Tensor) -> None:
        dev = self.device
        if scores.dtype != torch.float32 or ids.dtype != torch.int32 or scores.device != dev or ids.device != dev:
            raise ValueError(f"scores float32 and ids int32 on the {self._WHOSE} device")

    def _launch_args(self, B: int, n_valid, shard_tag):
        """What every update hands its kernel behind the batch: the two device scalars (filled first when given as ints), then the
        workspace for ``B`` slots -- ``(n_valid, shard_tag, workspace, workspace bytes)`` as addresses and a size."""
        nv, tag = self._scalar(self.n_valid, n_valid), self._scalar(self.shard_tag, shard_tag)
        self.reserve(B)
        ws = self.workspace
        return nv.data_ptr(), tag.data_ptr(), ws.data_ptr(), ws.numel() * ws.element_size()

    def update(self, scores: torch.Tensor, ids: torch.Tensor, n_valid=None, shard_tag=None) -> None:
        """One ``mkgnn_topk_update`` on the current stream: the list becomes the best ``k`` of itself and the first ``n_valid``
        entries ``(scores[i], shard_tag, ids[i])``.  ``n_valid`` / ``shard_tag``: None -- what ``self.n_valid`` /
        ``self.shard_tag`` hold when the launch RUNS; an int -- written into them first; a one-element device int32 tensor --
        read in their place (by address: a captured update follows its contents)."""
        from . import _lib
        self._check_batch(scores, ids)
        if not scores.is_contiguous() or not ids.is_contiguous() or scores.numel() != ids.numel():
            raise ValueError("scores and ids: contiguous, one id per score")
        B = scores.numel()
        if B < 1:
            raise ValueError("an update needs at least one slot")
        nv, tag, ws, ws_bytes = self._launch_args(B, n_valid, shard_tag)
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().mkgnn_topk_update(scores.data_ptr(), ids.data_ptr(), B, nv, tag, self.k, self.top_score.data_ptr(),
                                                     self.top_shard.data_ptr(), self.top_mol.data_ptr(), ws, ws_bytes,
                                                     _lib.stream_ptr(self.device)), "mkgnn_topk_update")

    def result(self):
        """``(top_score, top_shard, top_mol, n_occupied)``: the three tensors (not copies) and the number of occupied slots -- they
        come first -- as a host int (this synchronises)."""
        empty = (self.top_score == float("-inf")) & (self.top_shard == -1) & (self.top_mol == -1)
        return self.top_score, self.top_shard, self.top_mol, self.k - int(empty.sum())


class TopKTasks(TopK):
    """``n_tasks`` running lists of ``k`` slots each on ``device`` -- ``top_score`` float32, ``top_shard`` int32, ``top_mol`` int32 of
    shape ``[n_tasks, k]``, list ``t`` always sorted by the order of ``topk_update_reference`` -- updated together by ONE
    ``mkgnn_topk_update_tasks`` (the task on the grid's second dimension).  ``TopK``'s contract otherwise: ``n_valid`` and
    ``shard_tag`` are device scalars read when the launch runs, the same for every task (every molecule enters every list);
    ``reserve`` before a capture, nothing is allocated inside one."""

    def __init__(self, k: int, n_tasks: int, device):
        from . import _lib
        self.n_tasks = int(n_tasks)
        if not 1 <= self.n_tasks <= _lib.TASK_HEAD_MAX_TASKS:
            raise ValueError(f"n_tasks = {n_tasks} outside [1, {_lib.TASK_HEAD_MAX_TASKS}] (MKGNN_TASK_HEAD_MAX_TASKS)")
        self._allocate(k, device, (self.n_tasks, int(k)))

    _WHOSE = "lists'"

    def _workspace_bytes(self, batch: int) -> int:
        from . import _lib
        return int(_lib.load().mkgnn_topk_tasks_workspace_bytes(int(batch), self.k, self.n_tasks))

    def update(self, scores: torch.Tensor, ids: torch.Tensor, n_valid=None, shard_tag=None) -> None:
        """One ``mkgnn_topk_update_tasks`` on the current stream: list ``t`` becomes the best ``k`` of itself and the first
        ``n_valid`` entries ``(scores[i, t], shard_tag, ids[i])``.  ``scores``: float32 ``[B, T]`` or ``[T, B]`` with ``B =
        ids.numel()`` (``B == T``: read as ``[B, T]``), contiguous or the transposed view of a contiguous tensor -- its strides are
        passed on, nothing is copied; any other layout (a row stride that is neither 1 nor ``T``) raises ``ValueError``.
        ``n_valid`` / ``shard_tag``: as in ``TopK.update``."""
        from . import _lib
        T = self.n_tasks
        self._check_batch(scores, ids)
        B = ids.numel()
        if B < 1 or not ids.is_contiguous():
            raise ValueError("an update needs at least one slot and contiguous ids")
        if scores.dim() == 2 and tuple(scores.shape) == (B, T):
            rs, ts = scores.stride()
        elif scores.dim() == 2 and tuple(scores.shape) == (T, B):
            ts, rs = scores.stride()
        else:
            raise ValueError(f"scores: [{B}, {T}] or [{T}, {B}], one row of {T} scores per id")
        rs, ts = (0 if B == 1 else rs), (0 if T == 1 else ts)       # (the stride of a one-element dimension means nothing)
        row_major = (B == 1 or rs == T) and (T == 1 or ts == 1)
        task_major = (B == 1 or rs == 1) and (T == 1 or ts >= B)
        if not (row_major or task_major):
            raise ValueError(f"scores: strides {tuple(scores.stride())} are neither [B, T] rows (row stride T) nor [T, B] rows (row stride 1)")
        nv, tag, ws, ws_bytes = self._launch_args(B, n_valid, shard_tag)
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().mkgnn_topk_update_tasks(
                scores.data_ptr(), rs, ts, ids.data_ptr(), B, T, nv, tag, self.k, self.top_score.data_ptr(), self.top_shard.data_ptr(),
                self.top_mol.data_ptr(), ws, ws_bytes, _lib.stream_ptr(self.device)), "mkgnn_topk_update_tasks")

    def result(self):
        """``(top_score, top_shard, top_mol, n_occupied)``: the three ``[n_tasks, k]`` tensors (not copies) and the number of occupied
        slots of every list -- they come first -- as a host int64 tensor ``[n_tasks]`` (this synchronises)."""
        empty = (self.top_score == float("-inf")) & (self.top_shard == -1) & (self.top_mol == -1)
        return self.top_score, self.top_shard, self.top_mol, (self.k - empty.sum(dim=1)).cpu()


def _check_model(model, resident, tasks: bool = False) -> torch.device:
    T = getattr(getattr(model, "ffn", None), "out_features", None)
    if tasks:
        from . import _lib
        if not isinstance(T, int) or not 1 <= T <= _lib.TASK_HEAD_MAX_TASKS:
            raise ValueError(f"per-task screening takes a model with 1 to {_lib.TASK_HEAD_MAX_TASKS} outputs (task_dim), not {T}")
    elif T != 1:
        raise ValueError("screening ranks ONE score per molecule: a one-task model (task_dim = 1) is needed")
    return _check_device(model, resident)


def _check_device(model, resident) -> torch.device:
    """The device-only part of ``_check_model``: what the embedding routes need of a model with any number of outputs."""
    dev = next(model.parameters()).device
    if dev.type != "cuda":
        raise ValueError("screening runs on the GPU: move the model there (there is no CPU path)")
    if resident.view is None or resident.device != dev:
        raise ValueError(f"the shard is resident on {resident.device}, the model is on {dev}")
    return dev


def static_batch_for(loader, resident):
    """The ``padding.CompactStaticBatch`` of a ``ResidentLoader``'s plan (its shape and its molecule-size bounds, which let a step
    on it run the fused tail)."""
    from .padding import CompactStaticBatch
    return CompactStaticBatch(loader.shape, loader.batch_size, resident.x_dim, resident.p_dim, resident.e_dim, loader.device,
                              max_mol_atoms=loader.max_mol_atoms, max_mol_edges=loader.max_mol_edges)


class _ScoringStep:
    """The captured step of a shard pass (``_run_shard``): static buffers, the per-batch feed rows and ONE graph over ``gather`` ->
    ``expand`` -> ``attach_receptive_fields`` -> ``predict`` -> scatter of the live slots -> ``rank``.  ``predict(data)`` gives the
    batch's result -- one row per slot -- and ``shape`` is the shape of one molecule's: ``()`` for a score vector ``ext [n + 1]``
    (``score_resident``: ``model.predict`` as a vector), ``(T,)`` for ``ext [n + 1, T]`` (``score_resident_tasks``:
    ``model.predict_tasks``).  ``rank(pred, ids, n_live)``, when given, is called inside the capture with the batch's result, its id
    view and its live count (a one-element device int32 view); ``_run_shard`` passes the running list's ``update``,
    tools/screen_timing.py other formulations.  The model is in evaluation mode already.

    ``extras``: further per-molecule results of one value each, as ``(dtype, filler)`` pairs -- ``predict`` then returns ``(pred,
    *extras)``, one ``[batch]`` tensor per pair; each is scattered like ``pred`` into its own vector of ``more`` (``[n + 1]``, filled
    with the filler first) and ``rank`` is called with them behind the live count.  Without them nothing is captured that was not."""

    def __init__(self, model, resident, batch_size: int, predict, shape, rank=None, extras=()):
        from .receptive_field import attach_receptive_fields
        from .shards import ResidentLoader
        dev = resident.device
        bs, n = int(batch_size), int(resident.n_molecules)
        self.loader = loader = ResidentLoader(resident, bs, np.arange(n, dtype=np.int64), dev, drop_last=False)
        plan, n_live = loader.plan(), loader.n_live
        # one int32 row per batch: ids [bs] | live count [1] | (gap to an 8-byte boundary) | scatter index as int64 [bs]: the id for
        # a live slot, n -- a spare slot behind the score vector -- for a filler
        off = (bs + 2) // 2 * 2
        rows = np.zeros((plan.shape[0], off + 2 * bs), dtype=np.int32)
        rows[:, :bs] = plan
        rows[:, bs] = n_live
        rows[:, off:].view(np.int64)[:] = np.where(np.arange(bs)[None, :] < n_live[:, None], plan, n)
        self.rows = torch.from_numpy(rows).pin_memory().to(dev, non_blocking=True)
        self.feed = feed = torch.zeros(rows.shape[1], dtype=torch.int32, device=dev)
        f_ids, f_live, f_index = feed[:bs], feed[bs:bs + 1], feed[off:].view(torch.int64)
        self.csb = csb = static_batch_for(loader, resident)
        self.ext = ext = torch.full((n + 1, *shape), float("nan"), dtype=torch.float32, device=dev)
        self.more = more = [torch.full((n + 1,), filler, dtype=dtype, device=dev) for dtype, filler in extras]
        self.n = n

        def step(rank):
            csb.gather(resident, f_ids)
            csb.expand()
            attach_receptive_fields(csb.data, sizes=csb.data.bucket_sizes, overlap=True)
            pred = predict(csb.data)
            if more:
                pred, *rest = pred
                for vector, values in zip(more, rest):
                    vector.index_copy_(0, f_index, values)
            ext.index_copy_(0, f_index, pred)
            if rank is not None:
                rank(pred, f_ids, f_live, *rest) if more else rank(pred, f_ids, f_live)

        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            feed.copy_(self.rows[0], non_blocking=True)
            step(None)                                   # (eager once: lazily made buffers exist before the capture; no ranking)
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph, stream=side):
                step(rank)
        torch.cuda.current_stream(dev).wait_stream(side)

    def __len__(self):
        return int(self.rows.shape[0])

    def run(self, b: int) -> None:
        """Batch ``b`` on the current stream: one small copy and the replay."""
        self.feed.copy_(self.rows[b], non_blocking=True)
        self.graph.replay()


def _check_out(out, shape, dev) -> None:
    if out is not None and (out.dtype != torch.float32 or out.device != dev or tuple(out.shape) != shape or not out.is_contiguous()):
        raise ValueError(f"out: a contiguous float32 tensor of shape {shape} on {dev}")


def _run_shard(who: str, doing: str, model, resident, dev, batch_size: int, predict, shape, topk=None, list_class=TopK,
               n_lists: Optional[int] = None, per_query: bool = False, shard_tag: int = 0, out=None, extras=(), rank=None):
    """The one pass over a resident shard, behind the callers' own checks of model and shard (``dev``: their device): one captured
    ``_ScoringStep`` with ``predict`` (``shape``: the shape of one molecule's result) replayed over every batch; the ``[n, *shape]``
    result (copied into ``out`` when given, and ``out`` returned); the gather's status word read once, at the end.  ``topk``, when
    given, must be a ``list_class`` (a ``TopKTasks``: of ``n_lists`` lists, one per task, or ``per_query``) on ``dev``: every
    batch's live rows enter it under ``shard_tag``.  ``who`` names the entry point in a refusal, ``doing`` what a status interrupted.
    The model runs in evaluation mode and is handed back in the mode it came in.

    ``extras`` (``_ScoringStep``'s): ``predict`` gives further one-value results; the pass then returns ``(out, *vectors)``, the
    vectors ``[n]`` each.  ``rank``: the caller's own ranking inside the capture, in the place of a running list's ``update``
    (``topk``, when also given, is only checked, reserved and tagged)."""
    from .train import evaluation_mode
    bs, n = int(batch_size), int(resident.n_molecules)
    if bs < 1:
        raise ValueError("batch_size >= 1")
    if topk is not None:
        noun, verb, unit = ("lists", "are", "lists, one per query") if per_query else ("list", "is", "tasks")
        many = list_class is TopKTasks
        if isinstance(topk, TopKTasks) != many or (many and topk.n_tasks != n_lists):
            raise ValueError(f"{who}: the running {noun} must be a " + (f"TopKTasks of {n_lists} {unit}" if many else "TopK"))
        if topk.device != dev:
            raise ValueError(f"the running {noun} {verb} on {topk.device}, the model on {dev}")
    _check_out(out, (n, *shape), dev)
    if topk is not None:
        topk.reserve(bs)
        topk.shard_tag.fill_(int(shard_tag))
        if rank is None:
            rank = lambda pred, ids, n_live: topk.update(pred, ids, n_valid=n_live)     # noqa: E731
    with evaluation_mode(model):
        scoring = _ScoringStep(model, resident, bs, predict, shape, rank, extras)
        for b in range(len(scoring)):
            scoring.run(b)
        if out is None:
            out = scoring.ext[:n]
        else:
            out.copy_(scoring.ext[:n])
        status = scoring.csb.gather_status()             # (the one host read)
        if status:
            raise RuntimeError(f"mkgnn_gather_compact reported status {status} while {doing} the shard")
        return (out, *(vector[:n] for vector in scoring.more)) if extras else out


def score_resident(model, resident, batch_size: int, *, topk: Optional[TopK] = None, shard_tag: int = 0,
                   out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``scores[n_molecules]`` (float32, on the device): ``model.predict`` of every molecule of the ``ResidentShard``, in id
    order, the short tail included (``ResidentLoader(drop_last=False)``: the last batch is filled up with its last real
    molecule, whose extra scores are dropped).  ``out`` is filled with NaN first (allocated when not given), so a slot that
    was not scored shows.  With ``topk`` every batch's live scores also enter that running list under ``shard_tag``.

    One graph is captured per call and replayed per batch: ``CompactStaticBatch.gather``, ``expand``,
    ``attach_receptive_fields``, the model's scoring of all ``batch_size`` slots, the scatter of the live slots into the score
    vector, ``topk.update``.  Per batch the host enqueues one small copy (ids, live count, scatter index) and the replay; nothing
    synchronises with the host between batches.  The gather's status word is read once, at the end: non-zero raises.

    The model is put in evaluation mode and handed back in the mode it came in.  It must be a one-task model on the shard's
    GPU: anything else raises ``ValueError`` before a launch."""
    dev = _check_model(model, resident)
    return _run_shard("score_resident", "scoring", model, resident, dev, batch_size, lambda data: model.predict(data)[0].reshape(-1), (),
                      topk, TopK, shard_tag=shard_tag, out=out)


def score_resident_tasks(model, resident, batch_size: int, *, topk: Optional[TopKTasks] = None, shard_tag: int = 0,
                         out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``scores[n_molecules, T]`` (float32, on the device): ``model.predict_tasks`` of every molecule of the ``ResidentShard`` -- all
    ``T`` outputs of a multi-task model from ONE run of the network per molecule -- in id order, the short tail included, as
    ``score_resident`` does it: one captured graph per call, replayed per batch, in which the model's scoring is ``predict_tasks``
    (the forward-only tail for the embedding, ``mkgnn_task_scores`` for the ``T`` logits) and ``topk.update`` is ONE
    ``mkgnn_topk_update_tasks`` that feeds every batch's live rows to all ``T`` lists of a ``TopKTasks`` under ``shard_tag``.  ``out``
    (``[n_molecules, T]``, contiguous) is filled with NaN first.  The model needs ``1 <= T <= 32`` outputs and must be on the
    shard's GPU: anything else raises ``ValueError`` before a launch.  It comes back in the mode it came in."""
    dev = _check_model(model, resident, tasks=True)
    T = int(model.ffn.out_features)
    return _run_shard("score_resident_tasks", "scoring", model, resident, dev, batch_size, lambda data: model.predict_tasks(data)[0], (T,),
                      topk, TopKTasks, T, shard_tag=shard_tag, out=out)


def _check_mc(who: str, model, n_samples, seed) -> None:
    """What a Monte Carlo pass refuses before a launch, beyond ``_check_model``: ``GNNModel.predict_mc``'s own refusals (asked here,
    before a shard is touched) and a seed that is no integer."""
    from .readout import _check_mc_samples
    _check_mc_samples(n_samples)
    if float(model.dropout.p) == 0.0 and float(model.gnn_model.dropout.p) == 0.0:
        raise ValueError(f"{who}: both dropouts of this model are 0 -- it has no dropout uncertainty (score_resident scores it)")
    if seed is not None and int(seed) != seed:
        raise ValueError(f"{who}: seed must be an integer or None")


def _mc_pass(who: str, model, resident, dev, batch_size: int, n_samples: int, alpha: float, beta: float, topk=None, shard_tag: int = 0):
    """One shard pass whose scoring is ``model.predict_mc``: ``(pred, mean, std, acq)``, ``[n_molecules]`` each; with ``topk`` the
    batches' live rows enter that list ranked by ``acq``."""
    def predict(data):
        r = model.predict_mc(data, n_samples, alpha, beta)
        return tuple(r[k].reshape(-1) for k in ("pred", "mean", "std", "acq"))

    rank = None
    if topk is not None:
        rank = lambda pred, ids, n_live, mean, std, acq: topk.update(acq, ids, n_valid=n_live)     # noqa: E731
    nan = float("nan")
    return _run_shard(who, "scoring", model, resident, dev, batch_size, predict, (), topk, TopK, shard_tag=shard_tag,
                      extras=((torch.float32, nan),) * 3, rank=rank)


def score_resident_mc(model, resident, batch_size: int, n_samples: int, alpha: float = 1.0, beta: float = 0.0, seed=None):
    """``(pred[n], mean[n], std[n], acq[n])`` (float32, on the device): ``model.predict_mc`` of every molecule of the
    ``ResidentShard`` -- the point score, and mean, spread and acquisition value ``alpha * mean + beta * std`` of ``n_samples`` Monte
    Carlo dropout samples -- in id order, the short tail included, as ``score_resident`` makes its pass: one graph captured per
    call and replayed per batch, in which the model's scoring is ``predict_mc`` (on its kernel route two launches behind the last
    convolution, ``readout.tail_score_mc``).  ``pred`` is ``score_resident``'s, bit for bit.  Every replay draws fresh masks: the
    generator's offset advances on the device by ``n_samples`` per batch.  ``seed``: the head generator is reset to ``{seed, 0}``
    (``readout.reset_head_rng``) before the pass.  A molecule's masks depend on its slot in its batch and on its atoms' rows
    there, so the result is reproducible for a given ``(seed, batch_size)`` -- not across batch sizes.  (On ``predict_mc``'s
    PyTorch route the masks come from PyTorch's generator, which a captured graph advances too; ``seed`` does not reach it.)
    A one-task model on the shard's GPU with at least one dropout above 0, ``1 <= n_samples <= 64``: anything else raises
    ``ValueError`` before a launch.  The model comes back in the mode it came in."""
    who = "score_resident_mc"
    dev = _check_model(model, resident)
    _check_mc(who, model, n_samples, seed)
    if seed is not None:
        from .readout import reset_head_rng
        reset_head_rng(dev, int(seed))
    return _mc_pass(who, model, resident, dev, batch_size, int(n_samples), float(alpha), float(beta))


def screen_acquisition(model, residents, k: int, batch_size: int, n_samples: int, alpha: float = 1.0, beta: float = 1.0,
                       seed=None) -> dict:
    """``screen`` ranked by an acquisition value instead of the point score: the ``k`` molecules of a library with the largest
    ``acq = alpha * mean + beta * std`` of ``n_samples`` Monte Carlo dropout samples (``GNNModel.predict_mc``) -- the next batch of
    an active-learning campaign: exploit with ``beta = 0``, explore with ``beta > 0``; ``alpha = -1`` serves a task where lower is
    better, such as docking scores.  ``residents`` as in ``screen``; shard ``j`` carries tag ``j``; one ``TopK`` is carried across the
    shards, fed by the running list's own ``update`` with ``acq`` as the key inside every batch's captured graph.

    Returns ``top_score`` (the acquisition value), ``top_shard``, ``top_mol`` (trimmed to the occupied slots, best first);
    ``top_pred``, ``top_mean``, ``top_std`` of the hits, gathered at the end from the per-shard vectors (which stay on the device at
    12 bytes per molecule); and ``n_scored``.  ``seed``: the head generator is reset once, before the first shard; reproducible for
    a given ``(seed, batch_size)`` and shard order, as ``score_resident_mc``.  Refusals as ``score_resident_mc``."""
    who = "screen_acquisition"
    if getattr(getattr(model, "ffn", None), "out_features", None) != 1:
        raise ValueError("screening ranks ONE score per molecule: a one-task model (task_dim = 1) is needed")
    _check_mc(who, model, n_samples, seed)
    S, alpha, beta = int(n_samples), float(alpha), float(beta)
    if seed is not None:
        from .readout import reset_head_rng
        dev = next(model.parameters()).device
        if dev.type == "cuda":
            reset_head_rng(dev, int(seed))

    def per_shard(resident, topk, tag):
        pred, mean, std, _ = _mc_pass(who, model, resident, topk.device, batch_size, S, alpha, beta, topk, tag)
        return pred.clone(), mean.clone(), std.clone()   # (clones: without the spare slot's storage)

    top_score, top_shard, top_mol, occupied, n_scored, shards = _over_shards(
        who, residents, lambda r: _check_model(model, r), lambda dev: TopK(k, dev), per_shard, True)
    top_shard, top_mol = top_shard[:occupied], top_mol[:occupied]
    dev = top_score.device
    sizes = [int(pred.numel()) for pred, _, _ in shards]
    first = torch.tensor(np.concatenate([[0], np.cumsum(sizes)[:-1]]), dtype=torch.int64, device=dev)
    at = first[top_shard.long()] + top_mol.long()
    return {"top_score": top_score[:occupied], "top_shard": top_shard, "top_mol": top_mol,
            "top_pred": torch.cat([v for v, _, _ in shards])[at], "top_mean": torch.cat([v for _, v, _ in shards])[at],
            "top_std": torch.cat([v for _, _, v in shards])[at], "n_scored": n_scored}


def explain_resident(model, resident, ids, batch_size: int = 256) -> dict:
    """Why the molecules ``ids`` of one ``ResidentShard`` score what they score (the ``top_mol`` of a screen where ``top_shard`` is
    this shard, say; repeats allowed, order kept): ``GNNModel.atom_contributions`` of every one of them, as a dict --

    ``atom_ptr``  int64 numpy ``[len(ids) + 1]``, from the host's ``resident.mol_atoms``: molecule ``ids[i]`` owns the rows
                  ``atom_ptr[i] .. atom_ptr[i + 1]``
    ``contrib``   float32 ``[atom_ptr[-1], T]`` on the device: row ``atom_ptr[i] + a`` is atom ``a`` of molecule ``ids[i]`` in the
                  shard's atom order, column ``t`` its exact share of output ``t``
    ``bias``      ``[T]``: the head's bias (zeros for a head without one) -- a molecule's rows plus it sum to its ``predict_tasks``

    Every molecule is explained IN THE BATCH THE SHARD PASS SCORES IT IN: the batches of ``score_resident`` / ``score_resident_tasks``
    at this ``batch_size`` (ids ``k * batch_size ..``, the short tail filled up with its last id, the whole shard's shape) that hold
    a listed molecule are gathered, expanded and given their receptive fields as there, ``atom_contributions`` runs on each, and
    the listed molecules' rows are copied out.  So with the screen's ``batch_size`` a molecule's rows plus ``bias`` sum to the score
    the screen reported, to float32 rounding.  That needs the same layout: the network's logit of a molecule is defined up to
    the choice among mathematically tied neighbour permutations ("Ties"), which last-bit differences between batch
    layouts decide -- in another batch a few molecules' logits differ in the third digit, and the contributions
    with them.  At most ``len(set(ids))`` batches run, launched eagerly -- a hit list is a few thousand molecules at most.  A batch's
    live slots come first, so their real atoms are one run at its head; one indexed copy per batch moves the listed molecules'
    rows.  The gather's status word is read once, at the end: non-zero raises.  The model is put in evaluation mode and handed back
    in the mode it came in.  Empty ``ids``, ids outside the shard, a model or a shard that is not on the GPU: ``ValueError`` before
    a launch."""
    from .receptive_field import attach_receptive_fields
    from .shards import ResidentLoader
    from .train import evaluation_mode
    ids = np.asarray(ids.tolist() if torch.is_tensor(ids) else list(ids), dtype=np.int64).reshape(-1)
    n, bs = int(resident.n_molecules), int(batch_size)
    if ids.size == 0:
        raise ValueError("explain_resident needs at least one molecule id")
    if int(ids.min()) < 0 or int(ids.max()) >= n:
        raise ValueError(f"molecule ids outside [0, {n})")
    if bs < 1:
        raise ValueError("batch_size >= 1")
    dev = _check_device(model, resident)
    T = int(model.ffn.out_features)
    atom_ptr = np.zeros(ids.size + 1, dtype=np.int64)
    np.cumsum(resident.mol_atoms[ids], out=atom_ptr[1:])
    contrib = torch.empty((int(atom_ptr[-1]), T), dtype=torch.float32, device=dev)
    bias = model.ffn.bias.detach().float().clone() if model.ffn.bias is not None else torch.zeros(T, dtype=torch.float32, device=dev)
    # the shard pass's plan (host only: nothing is uploaded), and those of its batches that hold a listed molecule -- in order, so
    # the short tail, if listed, is the last piece and is filled up as the pass fills it
    whole = ResidentLoader(resident, bs, np.arange(n, dtype=np.int64), "cpu", drop_last=False)
    pieces = np.unique(ids // bs)
    loader = ResidentLoader(resident, bs, np.concatenate([np.arange(k * bs, min((k + 1) * bs, n), dtype=np.int64) for k in pieces]),
                            dev, shape=whole.shape, drop_last=False)
    # per batch: the rows of its head run to copy (src) and where they go (dst), for every listed molecule it holds
    src, dst, cut = [], [], [0]
    listed = np.argsort(ids // bs, kind="stable")
    piece_of = (ids // bs)[listed]
    for k in pieces:
        start = np.zeros(bs + 1, dtype=np.int64)
        members = np.arange(k * bs, min((k + 1) * bs, n))
        np.cumsum(resident.mol_atoms[members], out=start[1:members.size + 1])
        mine = listed[np.searchsorted(piece_of, k, "left"):np.searchsorted(piece_of, k, "right")]
        for i in mine:
            a = int(resident.mol_atoms[ids[i]])
            src.append(start[ids[i] - k * bs] + np.arange(a, dtype=np.int64))
            dst.append(atom_ptr[i] + np.arange(a, dtype=np.int64))
        cut.append(cut[-1] + int(resident.mol_atoms[ids[mine]].sum()))
    rows = torch.from_numpy(np.stack([np.concatenate(src), np.concatenate(dst)])).to(dev, non_blocking=True)
    with evaluation_mode(model):
        csb = static_batch_for(loader, resident)
        for b, f_ids in enumerate(loader):
            csb.gather(resident, f_ids)
            csb.expand()
            attach_receptive_fields(csb.data, sizes=csb.data.bucket_sizes, overlap=True)
            lo, hi = cut[b], cut[b + 1]
            contrib.index_copy_(0, rows[1, lo:hi], model.atom_contributions(csb.data).index_select(0, rows[0, lo:hi]))
        status = csb.gather_status()                     # (the one host read)
        if status:
            raise RuntimeError(f"mkgnn_gather_compact reported status {status} while explaining the shard's molecules")
    return {"atom_ptr": atom_ptr, "contrib": contrib, "bias": bias}


def _over_shards(who: str, residents, check, make_lists, per_shard, keep: bool):
    """The loop of ``screen``, ``screen_tasks`` and ``nearest``: shard ``j`` of ``residents`` (a sequence, or a generator, consumed one
    shard at a time) carries tag ``j``; it is checked (``check(resident)`` -> its device), the running lists are made on the first
    shard's device (``make_lists(dev)``), and ``per_shard(resident, lists, tag)`` runs it.  Returns ``lists.result()``, the number of
    molecules and the per-shard results (kept only with ``keep``); no shard at all raises."""
    lists, n_molecules, kept = None, 0, []
    for tag, resident in enumerate(residents):
        dev = check(resident)
        if lists is None:
            lists = make_lists(dev)
        result = per_shard(resident, lists, tag)
        n_molecules += int(resident.n_molecules)
        if keep:
            kept.append(result)
    if lists is None:
        raise ValueError(f"{who} needs at least one shard")
    return (*lists.result(), n_molecules, kept)


def screen(model, residents, k: int, batch_size: int, return_scores: bool = False) -> dict:
    """Rank a library: ``residents`` is a sequence of ``ResidentShard``s, or a generator that uploads them one at a time (a
    library larger than device memory); shard ``j`` carries tag ``j``.  One ``TopK`` of ``k`` slots is carried across the
    shards on the device.  Returns ``top_score``, ``top_shard``, ``top_mol`` (trimmed to the occupied slots, best first) and
    ``n_scored``; with ``return_scores`` also ``scores``, the per-shard score vectors."""
    top_score, top_shard, top_mol, occupied, n_scored, kept = _over_shards(
        "screen", residents, lambda r: _check_model(model, r), lambda dev: TopK(k, dev),
        lambda r, topk, tag: score_resident(model, r, batch_size, topk=topk, shard_tag=tag), return_scores)
    result = {"top_score": top_score[:occupied], "top_shard": top_shard[:occupied], "top_mol": top_mol[:occupied],
              "n_scored": n_scored}
    if return_scores:
        result["scores"] = kept
    return result


def screen_tasks(model, residents, k: int, batch_size: int, return_scores: bool = False) -> dict:
    """Rank a library in every assay of a multi-task model: ``screen`` with one ``TopKTasks`` of ``T x k`` slots carried across the
    shards (shard ``j`` carries tag ``j``; every molecule enters every task's list).  Returns ``top_score``, ``top_shard``,
    ``top_mol`` as ``[T, k]`` tensors, list ``t`` best first with its empty slots -- ``(-inf, -1, -1)`` -- at the end (not trimmed:
    the lists fill alike, but a tensor has one width), ``n_occupied`` (int64 ``[T]``, on the host), ``n_scored`` and, with
    ``return_scores``, ``scores``: the per-shard ``[n_molecules, T]`` tensors."""
    top_score, top_shard, top_mol, occupied, n_scored, kept = _over_shards(
        "screen_tasks", residents, lambda r: _check_model(model, r, tasks=True),
        lambda dev: TopKTasks(k, int(model.ffn.out_features), dev),
        lambda r, topk, tag: score_resident_tasks(model, r, batch_size, topk=topk, shard_tag=tag), return_scores)
    result = {"top_score": top_score, "top_shard": top_shard, "top_mol": top_mol, "n_occupied": occupied, "n_scored": n_scored}
    if return_scores:
        result["scores"] = kept
    return result


# ------------------------------------------------------------------------------------------ analogue search --
# Nearest embeddings: rank the molecules of a resident library by the cosine similarity of their graph embeddings
# (``GNNModel.embed``) with a few query embeddings -- the reference's own comparison of molecules (its graph-embedding analysis
# uses ``CosineSimilarity(dim=-1)``).  One running list per query: a ``TopKTasks(k, Q, dev)`` IS the ``Q`` lists.
#
# ``cosine_reference`` / ``cosine_bound``  the definition of ``mkgnn_embed_cosine`` in float64 numpy, and its error bound
# ``embed_resident``                       ``emb[n_molecules, G]`` of one resident shard, for a model of any ``task_dim``
# ``nearest_resident``                     ``sim[n_molecules, Q]`` of one resident shard, optionally feeding the ``Q`` lists
# ``nearest``                              shards -> the ``k`` nearest molecules of every query
# ``rank_embeddings``                      the same ranking from a stored embedding matrix, without running the network
#
# Three things hold for all of them.  ``cos(e, e)`` is 1 only to within ``cosine_bound`` (three float32 roundings of one vector do
# not cancel exactly).  A query that is itself in the library is not excluded: it is found, at the head of its list or tied with
# its duplicates.  Ties -- equal similarities, ``-0.0 == +0.0``, NaN last -- follow ``topk_update_reference``: shard ascending, then
# molecule id ascending.
COSINE_EPS = np.float32(1e-8)                   # MKGNN_EPS: each norm is clamped from below by it, on its own
MAX_QUERIES = 32                                # MKGNN_EMBED_COSINE_MAX_QUERIES = the lists of one TopKTasks


def _f64(a) -> np.ndarray:
    if torch.is_tensor(a):
        a = a.detach().cpu().numpy()
    a = np.asarray(a)
    if a.ndim != 2:
        raise ValueError("a matrix of row vectors is needed")
    return a.astype(np.float64)


def _inverse_norms(a: np.ndarray) -> np.ndarray:
    return 1.0 / np.maximum(np.sqrt((a * a).sum(axis=1)), float(COSINE_EPS))


def cosine_reference(emb, queries) -> np.ndarray:
    """The definition of ``mkgnn_embed_cosine`` (include/molkgnn_hip.h), on the host, in float64 on the values as given:
    ``sim[i, q] = (emb_i . queries_q) / (max(||emb_i||, eps) * max(||queries_q||, eps))`` with ``eps = float32(1e-8)`` -- each vector
    clamped on its own, as ``torch.nn.functional.cosine_similarity`` does; float64 ``[n, Q]``.  A zero vector gives 0, a NaN its row
    or column of NaN."""
    e, q = _f64(emb), _f64(queries)
    if e.shape[1] != q.shape[1]:
        raise ValueError(f"emb [n, {e.shape[1]}] and queries [Q, {q.shape[1]}] differ in width")
    with np.errstate(invalid="ignore"):
        return (e @ q.T) * _inverse_norms(e)[:, None] * _inverse_norms(q)[None, :]


def cosine_bound(emb, queries) -> np.ndarray:
    """How far a float32 evaluation of ``cosine_reference`` may lie from it, element by element (float64 ``[n, Q]``):

        ``(2 H + 10) 2^-24 M ie iq  +  H 2^-149 ie iq  +  2^-149``,   ``M = sum_h |e_h| |q_h|``, ``ie`` / ``iq`` the inverse clamped norms.

    First term, the standard rounding model (Higham 3.1, first order): ``H + 1`` roundings for the dot product, ``(H + 1) / 2 + 2``
    for each inverse norm (its sum of squares, halved by the square root; the root; the division), two multiplies -- ``2 H + 8`` units
    of ``2^-24``, taken as ``2 H + 10`` for the second-order terms and for an order that scales the query first.  Second term: a
    product that underflows carries up to half a denormal spacing, ``2^-150``, ``H`` of them, scaled like the dot product; the factor
    two is margin.  Third term: the rounding of a result that is itself denormal.  It holds for EVERY element."""
    e, q = _f64(emb), _f64(queries)
    if e.shape[1] != q.shape[1]:
        raise ValueError(f"emb [n, {e.shape[1]}] and queries [Q, {q.shape[1]}] differ in width")
    H = e.shape[1]
    scale = _inverse_norms(e)[:, None] * _inverse_norms(q)[None, :]
    return (2 * H + 10) * 2.0 ** -24 * (np.abs(e) @ np.abs(q).T) * scale + H * 2.0 ** -149 * scale + 2.0 ** -149


def _check_vectors(who: str, t, G: int, dev, noun: str, cap, cap_hint: str) -> int:
    """The number of rows of a matrix of ``noun`` ("queries", "references"): float32 ``[n, G]``, ``1 <= n <= cap`` (``cap`` None: any
    ``n >= 1``), on ``dev`` (a CUDA device) -- the value checks first, the device last; ``ValueError`` otherwise, before anything is
    loaded or launched."""
    if not torch.is_tensor(t) or t.dim() != 2:
        raise ValueError(f"{who}: the {noun} are a [{noun[0].upper()}, {G}] tensor of embeddings")
    if t.dtype != torch.float32:
        raise ValueError(f"{who}: the {noun} are float32, not {t.dtype}")
    n = int(t.shape[0])
    if cap is None and n < 1:
        raise ValueError(f"{who}: at least one {noun[:-1]} is needed")
    if cap is not None and not 1 <= n <= cap:
        raise ValueError(f"{who}: {n} {noun} outside [1, {cap}] ({cap_hint})")
    if int(t.shape[1]) != int(G):
        raise ValueError(f"{who}: the {noun} are {int(t.shape[1])} wide, the embedding is {int(G)} wide")
    if t.device.type != "cuda" or (dev is not None and t.device != dev):
        raise ValueError(f"{who}: the {noun} are on {t.device}; they belong on the GPU of the library" +
                         ("" if dev is None else f" ({dev})"))
    return n


def _check_queries(who: str, query_emb, G: int, dev=None) -> int:
    """``Q`` of a query matrix: float32 ``[Q, G]``, ``1 <= Q <= 32``, on ``dev`` (``_check_vectors``)."""
    return _check_vectors(who, query_emb, G, dev, "queries", MAX_QUERIES,
                          "MKGNN_EMBED_COSINE_MAX_QUERIES: one list per query; rank more queries group by group, "
                          "screening.rank_embeddings")


def _embedding_width(model) -> int:
    G = getattr(getattr(model, "ffn", None), "in_features", None)
    if not isinstance(G, int) or G < 1:
        raise ValueError("a model whose head (ffn) reads the graph embedding is needed")
    return G


def embed_resident(model, resident, batch_size: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``emb[n_molecules, G]`` (float32, on the device): ``model.embed`` of every molecule of the ``ResidentShard``, in id order, the
    short tail included, as ``score_resident`` does it -- one captured graph per call, replayed per batch, with the embedding in the
    place of the score and no ranking.  ``out`` (``[n_molecules, G]``, contiguous) is filled with NaN first, so a slot that was not
    written shows.  The model may have any ``task_dim``; it must be on the shard's GPU (``ValueError`` before a launch otherwise);
    it is put in evaluation mode and handed back in the mode it came in.  The gather's status word is read once, at the end.
    The matrix can be kept and ranked again and again (``rank_embeddings``) without running the network."""
    G = _embedding_width(model)
    dev = _check_device(model, resident)
    return _run_shard("embed_resident", "embedding", model, resident, dev, batch_size, model.embed, (G,), out=out)


def nearest_resident(model, resident, query_emb: torch.Tensor, batch_size: int, *, topk: Optional[TopKTasks] = None,
                     shard_tag: int = 0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``sim[n_molecules, Q]`` (float32, on the device): the cosine similarity (``cosine_reference``) of every molecule's graph
    embedding with each of the ``Q`` rows of ``query_emb`` (float32 ``[Q, G]`` on the shard's GPU, ``1 <= Q <= 32``), in id order, the
    short tail included.  One graph is captured per call and replayed per batch, as in ``score_resident``; the step's scoring is
    ``readout.embedding_cosine(model.embed(data), query_emb)`` -- one ``mkgnn_embed_cosine`` behind the network, which reads the
    queries raw -- and, with ``topk`` (a ``TopKTasks`` of ``Q`` lists), ``topk.update(sim, ids, n_valid=n_live)``: ONE
    ``mkgnn_topk_update_tasks`` that feeds the batch's live rows to all ``Q`` lists under ``shard_tag``; fillers never enter a list.
    ``out`` (``[n_molecules, Q]``, contiguous) is filled with NaN first.

    ``cos(e, e)`` is 1 only to within ``cosine_bound``; a query that is itself in the library is not excluded; ties follow
    ``topk_update_reference``.  A wrong ``Q``, ``G``, dtype or device, or a ``topk`` that is not a ``TopKTasks`` of ``Q`` lists, raises
    ``ValueError`` before a launch.  The model may have any ``task_dim`` and comes back in the mode it came in."""
    Q = _check_queries("nearest_resident", query_emb, _embedding_width(model))
    dev = _check_device(model, resident)
    _check_queries("nearest_resident", query_emb, query_emb.shape[1], dev)
    from .readout import embedding_cosine
    queries = query_emb.detach()
    return _run_shard("nearest_resident", "embedding", model, resident, dev, batch_size,
                      lambda data: embedding_cosine(model.embed(data), queries), (Q,), topk, TopKTasks, Q, True, shard_tag, out)


def nearest(model, queries, residents, k: int, batch_size: int, return_sims: bool = False) -> dict:
    """Analogue search: the ``k`` molecules of a library whose graph embeddings lie closest, by cosine similarity, to each query.
    ``queries``: a float32 ``[Q, G]`` tensor of embeddings on the model's GPU, or a ``ResidentShard`` of 1 to 32 query molecules
    (known actives), which is embedded with ``embed_resident`` first.  ``residents``: a sequence of ``ResidentShard``s, or a
    generator that uploads them one at a time; shard ``j`` carries tag ``j``.  One ``TopKTasks`` of ``Q x k`` slots is carried across
    the shards on the device.  Returns, as ``screen_tasks`` does, ``top_sim``, ``top_shard``, ``top_mol`` as ``[Q, k]`` tensors, list
    ``q`` nearest first with its empty slots -- ``(-inf, -1, -1)`` -- at the end; ``n_occupied`` (int64 ``[Q]``, on the host);
    ``n_searched``; ``query_emb`` (the ``[Q, G]`` matrix that was searched for); and, with ``return_sims``, ``sims``: the per-shard
    ``[n_molecules, Q]`` tensors.

    ``cos(e, e)`` is 1 only to within ``cosine_bound``; a query that is itself in the library is not excluded (it heads its list, or
    ties with its duplicates); ties follow ``topk_update_reference``.  More than 32 queries: ``nearest_many`` (lists of at most 64
    entries, one pass over the library); for longer lists embed the library once (``embed_resident``) and call ``rank_embeddings``
    per group of 32."""
    from .shards import ResidentShard
    G = _embedding_width(model)
    if isinstance(queries, ResidentShard):
        if not 1 <= int(queries.n_molecules) <= MAX_QUERIES:
            raise ValueError(f"nearest: a query shard holds 1 to {MAX_QUERIES} molecules, not {int(queries.n_molecules)}")
        query_emb = embed_resident(model, queries, batch_size)
    else:
        query_emb = queries
    dev = next(model.parameters()).device
    Q = _check_queries("nearest", query_emb, G, dev if dev.type == "cuda" else None)
    if dev.type != "cuda":
        raise ValueError("nearest runs on the GPU: move the model there (there is no CPU path)")
    top_sim, top_shard, top_mol, occupied, n_searched, kept = _over_shards(
        "nearest", residents, lambda r: _check_device(model, r), lambda dev: TopKTasks(k, Q, dev),
        lambda r, topk, tag: nearest_resident(model, r, query_emb, batch_size, topk=topk, shard_tag=tag), return_sims)
    result = {"top_sim": top_sim, "top_shard": top_shard, "top_mol": top_mol, "n_occupied": occupied, "n_searched": n_searched,
              "query_emb": query_emb}
    if return_sims:
        result["sims"] = kept
    return result


def rank_embeddings(emb: torch.Tensor, query_emb: torch.Tensor, topk: TopKTasks, ids: Optional[torch.Tensor] = None,
                    shard_tag: int = 0, chunk: int = 4096) -> None:
    """The stored-embedding route: rank the rows of ``emb`` (float32 ``[n, G]`` on the GPU, e.g. kept from ``embed_resident``) against
    ``query_emb`` (float32 ``[Q, G]``, ``1 <= Q <= 32``) into ``topk`` (a ``TopKTasks`` of ``Q`` lists) WITHOUT running the network: per
    chunk of ``chunk`` rows one ``mkgnn_embed_cosine`` and one ``mkgnn_topk_update_tasks``, launched eagerly.  Row ``i`` enters as
    ``(sim[i, q], shard_tag, ids[i])``; ``ids`` (int32 ``[n]`` on the GPU) defaults to ``arange(n)``.  It makes re-querying a library
    cheap -- the similarities are bit for bit those of ``nearest_resident`` on the same embeddings, so the lists are too.  A user with
    more than 32 queries calls it per group of 32, with a ``TopKTasks`` per group.

    ``chunk`` bounds the top-k's serial merge: an update ranks its batch in tiles in parallel and then merges the tiles' runs into
    the list one after another (``DESIGN.md`` 4.5c), so one update over a whole library would serialise on that merge, and its
    workspace grows with the batch; chunks of a few thousand rows keep both at a scoring step's size.

    ``cos(e, e)`` is 1 only to within ``cosine_bound``; a query that is itself in the library is not excluded; ties follow
    ``topk_update_reference``."""
    if not torch.is_tensor(emb) or emb.dim() != 2 or emb.dtype != torch.float32 or emb.shape[1] < 1:
        raise ValueError("rank_embeddings: emb is a float32 [n, G] tensor")
    n, G = int(emb.shape[0]), int(emb.shape[1])
    Q = _check_queries("rank_embeddings", query_emb, G)
    if not emb.is_cuda:
        raise ValueError(f"rank_embeddings: emb is on {emb.device}; the ranking runs on the GPU (there is no CPU path)")
    dev = emb.device
    _check_queries("rank_embeddings", query_emb, G, dev)
    if not isinstance(topk, TopKTasks) or topk.n_tasks != Q or topk.device != dev:
        raise ValueError(f"rank_embeddings: the running lists must be a TopKTasks of {Q} lists on {dev}")
    chunk = int(chunk)
    if chunk < 1:
        raise ValueError("chunk >= 1")
    if ids is None:
        ids = torch.arange(n, dtype=torch.int32, device=dev)
    elif not torch.is_tensor(ids) or ids.dtype != torch.int32 or ids.device != dev or ids.dim() != 1 or ids.numel() != n \
            or not ids.is_contiguous():
        raise ValueError(f"rank_embeddings: ids is a contiguous int32 [{n}] tensor on {dev}")
    if n == 0:
        return
    from .readout import embedding_cosine
    emb, query_emb = emb.detach(), query_emb.detach()
    topk.reserve(min(chunk, n))
    for a in range(0, n, chunk):
        b = min(a + chunk, n)
        topk.update(embedding_cosine(emb[a:b], query_emb), ids[a:b], n_valid=b - a, shard_tag=int(shard_tag))


# ------------------------------------------------------------------------------- analogues of many queries --
# "Show me the analogues of every confirmed active": a few hundred queries, not 32.  ``mkgnn_embed_knn_update`` takes raw
# candidate embeddings and raw queries in and updates one sorted running list per query in place -- any number of queries, no
# similarity matrix -- so the whole search is ONE pass over the library, inside the captured scoring step.  The similarities are
# ``mkgnn_embed_cosine``'s bit for bit and the order is ``topk_update_reference``'s, so for ``Q <= 32`` the lists are those of
# ``nearest`` / ``rank_embeddings``.  Lists hold at most 64 entries each (one slot per lane of a wave); longer ones stay with
# ``rank_embeddings``.
class NearestLists(TopK):
    """``n_queries`` running lists of ``k`` slots each on ``device`` -- ``top_score`` (the similarity) float32, ``top_shard`` int32,
    ``top_mol`` int32 of shape ``[n_queries, k]``, list ``q`` always sorted by the order of ``topk_update_reference`` -- fed by
    ``mkgnn_embed_knn_update`` with candidate EMBEDDINGS and the queries themselves: ``TopKTasks`` without its cap of 32 lists
    (``1 <= n_queries <= 2^20``) and with ``1 <= k <= 64``.  ``TopK``'s contract otherwise: ``n_valid`` and ``shard_tag`` are device
    scalars read when the launch runs, so one captured ``update`` serves every batch of every shard; ``reserve`` before a capture,
    nothing is allocated inside one."""

    _WHOSE = "lists'"

    def __init__(self, k: int, n_queries: int, device):
        from . import _lib
        self.n_queries = int(n_queries)
        if not 1 <= int(k) <= _lib.KNN_MAX_K:
            raise ValueError(f"k = {k} outside [1, {_lib.KNN_MAX_K}] (MKGNN_KNN_MAX_K: one slot per lane of a wave; longer lists are "
                             "rank_embeddings's, per group of 32 queries)")
        if not 1 <= self.n_queries <= _lib.KNN_MAX_QUERIES:
            raise ValueError(f"n_queries = {n_queries} outside [1, {_lib.KNN_MAX_QUERIES}] (MKGNN_KNN_MAX_QUERIES)")
        self._allocate(k, device, (self.n_queries, int(k)))

    def _workspace_bytes(self, batch: int) -> int:
        from . import _lib
        return int(_lib.load().mkgnn_embed_knn_workspace_bytes(int(batch), self.n_queries, self.k))

    def reserve(self, n_rows: int) -> None:
        """Make the workspace large enough for updates of ``n_rows`` candidate rows (before a capture: a captured update must not
        allocate)."""
        super().reserve(n_rows)

    def update(self, emb: torch.Tensor, queries: torch.Tensor, ids: Optional[torch.Tensor] = None, n_valid=None,
               shard_tag=None) -> None:
        """One ``readout.embedding_knn_update`` on the current stream: list ``q`` becomes the best ``k`` of itself and the first
        ``n_valid`` entries ``(cosine(emb[i], queries[q]), shard_tag, ids[i])``.  ``emb`` float32 ``[n, G]`` and ``queries`` float32
        ``[n_queries, G]`` on the lists' device, both read raw; ``ids`` contiguous int32 ``[n]`` (None: the row index).  ``n_valid`` /
        ``shard_tag``: as in ``TopK.update``."""
        from .readout import embedding_knn_update
        if not torch.is_tensor(queries) or queries.dim() != 2 or int(queries.shape[0]) != self.n_queries:
            raise ValueError(f"queries: a [{self.n_queries}, G] tensor, one row per list")
        if not torch.is_tensor(emb) or emb.dim() != 2 or emb.device != self.device:
            raise ValueError(f"emb: a float32 [n, G] tensor on the {self._WHOSE} device")
        nv, tag = self._scalar(self.n_valid, n_valid), self._scalar(self.shard_tag, shard_tag)
        from . import _lib
        if 1 <= int(emb.shape[0]) <= _lib.KNN_MAX_ROWS:      # (anything else: embedding_knn_update says what is wrong)
            self.reserve(int(emb.shape[0]))
        embedding_knn_update(emb, queries, self.top_score, self.top_shard, self.top_mol, ids=ids, n_valid=nv, shard_tag=tag,
                             workspace=self.workspace)

    def result(self):
        """``(top_sim, top_shard, top_mol, n_occupied)``: the three ``[n_queries, k]`` tensors (not copies) and the number of occupied
        slots of every list -- they come first -- as a host int64 tensor ``[n_queries]`` (this synchronises)."""
        return TopKTasks.result(self)


def _check_many_queries(who: str, query_emb, G: int, dev=None) -> int:
    """``_check_queries`` without the cap of 32: float32 ``[Q, G]``, ``1 <= Q <= 2^20``, on ``dev`` (``_check_vectors``)."""
    from . import _lib
    return _check_vectors(who, query_emb, G, dev, "queries", _lib.KNN_MAX_QUERIES, "MKGNN_KNN_MAX_QUERIES: one list per query")


def _check_lists(who: str, lists, Q: int, dev) -> None:
    if not isinstance(lists, NearestLists) or lists.n_queries != Q:
        raise ValueError(f"{who}: the running lists must be a NearestLists of {Q} lists, one per query")
    if lists.device != dev:
        raise ValueError(f"the running lists are on {lists.device}, the " + ("model" if who != "nearest_embeddings" else "embeddings") +
                         f" on {dev}")


def nearest_many_resident(model, resident, query_emb: torch.Tensor, batch_size: int, *, lists: NearestLists,
                          shard_tag: int = 0) -> torch.Tensor:
    """One pass over a ``ResidentShard`` that feeds every molecule's graph embedding to the ``Q`` running lists of ``lists`` (a
    ``NearestLists`` of ``Q = query_emb.shape[0]`` lists) under ``shard_tag``; returns the shard's ``[n_molecules, G]`` embeddings
    (float32, on the device), as ``embed_resident`` does.  One graph is captured per call and replayed per batch, as in
    ``score_resident``: the step's result is ``model.embed(data)`` and its ranking, inside the capture, is
    ``lists.update(emb, query_emb, ids, n_valid=n_live)`` -- ONE ``mkgnn_embed_knn_update`` behind the network, for any number of
    queries, with no similarity matrix; fillers never enter a list.  ``query_emb``: float32 ``[Q, G]`` on the shard's GPU, read raw by
    every replay.  A wrong ``Q``, ``G``, dtype or device, or ``lists`` that are not a ``NearestLists`` of ``Q`` lists on the model's
    GPU, raises ``ValueError`` before a launch.  The model may have any ``task_dim`` and comes back in the mode it came in."""
    G = _embedding_width(model)
    Q = _check_many_queries("nearest_many_resident", query_emb, G)
    dev = _check_device(model, resident)
    _check_many_queries("nearest_many_resident", query_emb, G, dev)
    _check_lists("nearest_many_resident", lists, Q, dev)
    bs = int(batch_size)
    if bs < 1:
        raise ValueError("batch_size >= 1")
    queries = query_emb.detach()
    lists.reserve(bs)
    lists.shard_tag.fill_(int(shard_tag))
    return _run_shard("nearest_many_resident", "embedding", model, resident, dev, bs, model.embed, (G,),
                      rank=lambda emb, ids, n_live: lists.update(emb, queries, ids, n_valid=n_live))


def nearest_many(model, queries, residents, k: int, batch_size: int) -> dict:
    """Analogue search for ANY number of queries: the ``k <= 64`` molecules of a library whose graph embeddings lie closest, by cosine
    similarity, to each query -- ``nearest`` without its cap of 32 queries, in one pass over the library (the network runs once
    per molecule, whatever ``Q`` is).  ``queries``: a float32 ``[Q, G]`` tensor of embeddings on the model's GPU, or a
    ``ResidentShard`` of any number of query molecules (the confirmed actives of an assay), which is embedded with ``embed_resident``
    first.  ``residents``: as in ``nearest``; shard ``j`` carries tag ``j``.  One ``NearestLists`` of ``Q x k`` slots is carried across
    the shards on the device.  Returns ``nearest``'s keys: ``top_sim``, ``top_shard``, ``top_mol`` as ``[Q, k]`` tensors, list ``q``
    nearest first with its empty slots -- ``(-inf, -1, -1)`` -- at the end; ``n_occupied`` (int64 ``[Q]``, on the host);
    ``n_searched``; ``query_emb``.  There is no ``sims``: no such matrix exists.

    The similarities are ``nearest``'s bit for bit and so are the lists.  ``cos(e, e)`` is 1 only to within ``cosine_bound``; a query
    that is itself in the library is not excluded; ties follow ``topk_update_reference``."""
    from . import _lib
    from .shards import ResidentShard
    G = _embedding_width(model)
    if not 1 <= int(k) <= _lib.KNN_MAX_K:
        raise ValueError(f"nearest_many: k = {k} outside [1, {_lib.KNN_MAX_K}] (MKGNN_KNN_MAX_K; longer lists are rank_embeddings's, per "
                         "group of 32 queries)")
    if isinstance(queries, ResidentShard):
        if not 1 <= int(queries.n_molecules) <= _lib.KNN_MAX_QUERIES:
            raise ValueError(f"nearest_many: a query shard holds 1 to {_lib.KNN_MAX_QUERIES} molecules, not {int(queries.n_molecules)}")
        query_emb = embed_resident(model, queries, batch_size)
    else:
        query_emb = queries
    dev = next(model.parameters()).device
    Q = _check_many_queries("nearest_many", query_emb, G, dev if dev.type == "cuda" else None)
    if dev.type != "cuda":
        raise ValueError("nearest_many runs on the GPU: move the model there (there is no CPU path)")
    top_sim, top_shard, top_mol, occupied, n_searched, _ = _over_shards(
        "nearest_many", residents, lambda r: _check_device(model, r), lambda dev: NearestLists(k, Q, dev),
        lambda r, lists, tag: nearest_many_resident(model, r, query_emb, batch_size, lists=lists, shard_tag=tag), False)
    return {"top_sim": top_sim, "top_shard": top_shard, "top_mol": top_mol, "n_occupied": occupied, "n_searched": n_searched,
            "query_emb": query_emb}


def nearest_embeddings(emb: torch.Tensor, query_emb: torch.Tensor, lists: NearestLists, ids: Optional[torch.Tensor] = None,
                       shard_tag: int = 0) -> None:
    """The stored-embedding route for any number of queries: rank the rows of ``emb`` (float32 ``[n, G]`` on the GPU, e.g. kept from
    ``embed_resident``) against ``query_emb`` (float32 ``[Q, G]``) into ``lists`` (a ``NearestLists`` of ``Q`` lists) WITHOUT running the
    network: one ``lists.update`` -- one ``mkgnn_embed_knn_update`` -- per ``MKGNN_KNN_MAX_ROWS`` (2^20) rows, launched eagerly.  Row
    ``i`` enters as ``(sim[i, q], shard_tag, ids[i])``; ``ids`` (int32 ``[n]`` on the GPU) defaults to ``arange(n)``.  For ``Q <= 32``
    the lists are ``rank_embeddings``'s bit for bit.  ``cos(e, e)`` is 1 only to within ``cosine_bound``; a query that is itself in
    the library is not excluded; ties follow ``topk_update_reference``."""
    from . import _lib
    if not torch.is_tensor(emb) or emb.dim() != 2 or emb.dtype != torch.float32 or emb.shape[1] < 1:
        raise ValueError("nearest_embeddings: emb is a float32 [n, G] tensor")
    n, G = int(emb.shape[0]), int(emb.shape[1])
    Q = _check_many_queries("nearest_embeddings", query_emb, G)
    if not emb.is_cuda:
        raise ValueError(f"nearest_embeddings: emb is on {emb.device}; the ranking runs on the GPU (there is no CPU path)")
    dev = emb.device
    _check_many_queries("nearest_embeddings", query_emb, G, dev)
    _check_lists("nearest_embeddings", lists, Q, dev)
    if ids is not None and (not torch.is_tensor(ids) or ids.dtype != torch.int32 or ids.device != dev or ids.dim() != 1
                            or ids.numel() != n or not ids.is_contiguous()):
        raise ValueError(f"nearest_embeddings: ids is a contiguous int32 [{n}] tensor on {dev}")
    emb, query_emb = emb.detach(), query_emb.detach()
    step = _lib.KNN_MAX_ROWS
    for a in range(0, n, step):
        b = min(a + step, n)
        piece = ids[a:b] if ids is not None else None if a == 0 else torch.arange(a, b, dtype=torch.int32, device=dev)
        lists.update(emb[a:b], query_emb, piece, n_valid=b - a, shard_tag=int(shard_tag))


# ---------------------------------------------------------------------------------------------- novel hits --
# The opposite question to ``nearest``: for EVERY library molecule, how close is it to what is already known -- the known actives,
# the training set, a patent set of thousands of molecules?  ``mkgnn_embed_max_cosine`` answers it inside the captured scoring
# step without an ``[n, R]`` matrix; ``mkgnn_select_rows`` compacts the batch to the molecules inside the bounds before the running
# list sees it, so a filtered-out molecule never pushes another off the list.  ``max_sim`` alone is the novelty filter ("not a
# near-copy of a known active"), ``min_sim`` alone the applicability domain ("only where the model can be trusted").
def max_cosine_reference(emb, refs):
    """The definition of ``mkgnn_embed_max_cosine`` (include/molkgnn_hip.h), on the host: ``(max float64 [n], arg int64 [n])`` -- per
    row of ``cosine_reference(emb, refs)`` the first reference in the order of ``topk_update_reference``: non-NaN similarities before
    NaN ones, larger first (``-0.0 == +0.0``), then the lower index.  A row without a non-NaN similarity gives ``(NaN, 0)``."""
    sim = cosine_reference(emb, refs)
    if sim.shape[1] < 1:
        raise ValueError("at least one reference is needed")
    nan = np.isnan(sim)
    clean = np.where(nan, -np.inf, sim)
    first = ((clean == clean.max(axis=1, keepdims=True)) & ~nan).argmax(axis=1)     # (argmax of booleans: the first True, else 0)
    some = ~nan.all(axis=1)
    arg = np.where(some, first, 0).astype(np.int64)
    return np.where(some, sim[np.arange(sim.shape[0]), arg], np.nan), arg


def select_rows_reference(scores, ids, key, n_valid, lo, hi):
    """The definition of ``mkgnn_select_rows``, on the host: ``(scores, ids, n_kept)`` of the slots ``i < min(max(n_valid, 0), B)`` with
    ``lo <= key[i] <= hi``, in slot order -- float32 scores with their bits, int32 ids.  A NaN key fails both comparisons; a key
    equal to a bound is kept; infinite bounds are allowed."""
    scores = np.asarray(scores, dtype=np.float32).reshape(-1)
    ids, key = np.asarray(ids, dtype=np.int32).reshape(-1), np.asarray(key, dtype=np.float32).reshape(-1)
    if not scores.shape == ids.shape == key.shape:
        raise ValueError("one id and one key per score")
    n = int(min(max(int(n_valid), 0), scores.shape[0]))
    with np.errstate(invalid="ignore"):
        keep = (np.float32(lo) <= key[:n]) & (key[:n] <= np.float32(hi))
    return scores[:n][keep].copy(), ids[:n][keep].copy(), int(keep.sum())


def _check_refs(who: str, ref_emb, G: int, dev=None) -> int:
    """``R`` of a reference matrix: float32 ``[R, G]``, ``R >= 1``, on ``dev`` (``_check_vectors``)."""
    return _check_vectors(who, ref_emb, G, dev, "references", None, "")


def _embedding_f32(emb: torch.Tensor) -> torch.Tensor:
    return emb if emb.dtype == torch.float32 else emb.float()


def reference_similarity_resident(model, resident, ref_emb: torch.Tensor, batch_size: int, out=None):
    """``(max_sim float32 [n_molecules], arg_ref int32 [n_molecules])`` on the device: for every molecule of the ``ResidentShard`` the
    cosine similarity of its graph embedding with its NEAREST row of ``ref_emb`` (float32 ``[R, G]`` on the shard's GPU) and that
    row's index (``max_cosine_reference``; ties to the lower index), in id order, the short tail included.  One pass as
    ``embed_resident`` makes it -- one graph captured per call, replayed per batch -- whose scoring is
    ``readout.embedding_max_cosine(model.embed(data), ref_emb)``: the references are read raw inside the captured call.  ``out``: a
    pair of contiguous tensors ``(float32 [n_molecules], int32 [n_molecules])`` to fill; slots that were not written would show as
    ``(NaN, -1)``.  The model may have any ``task_dim`` and comes back in the mode it came in; a wrong shape, dtype or device raises
    ``ValueError`` before a launch."""
    who = "reference_similarity_resident"
    _check_refs(who, ref_emb, _embedding_width(model))
    dev = _check_device(model, resident)
    _check_refs(who, ref_emb, ref_emb.shape[1], dev)
    n = int(resident.n_molecules)
    if out is not None:
        if not isinstance(out, (tuple, list)) or len(out) != 2 or not torch.is_tensor(out[1]) or out[1].dtype != torch.int32 \
                or out[1].device != dev or tuple(out[1].shape) != (n,) or not out[1].is_contiguous():
            raise ValueError(f"out: a pair of contiguous tensors (float32 [{n}], int32 [{n}]) on {dev}")
    from .readout import embedding_max_cosine
    refs = ref_emb.detach()
    sim, arg = _run_shard(who, "embedding", model, resident, dev, batch_size,
                          lambda data: embedding_max_cosine(_embedding_f32(model.embed(data)), refs), (),
                          out=None if out is None else out[0], extras=((torch.int32, -1),))
    if out is not None:
        out[1].copy_(arg)
        arg = out[1]
    return sim, arg


def screen_novel(model, residents, k: int, batch_size: int, ref_emb, max_sim: Optional[float] = None,
                 min_sim: Optional[float] = None, return_scores: bool = False) -> dict:
    """``screen`` with a filter in front of the running list: rank the molecules of a library whose NEAREST reference -- by cosine
    similarity of the graph embeddings, ``max_cosine_reference`` -- lies inside ``[min_sim, max_sim]`` (a bound that is not given is
    infinite; at least one must be).  ``max_sim=c`` is the novelty filter: the best ``k`` molecules that are not near-copies of a known
    active.  ``min_sim=c`` is the applicability domain: only molecules close enough to the training set.  A molecule whose reference
    similarity is NaN is never kept.  ``ref_emb``: a float32 ``[R, G]`` tensor on the model's GPU, or a ``ResidentShard`` of known
    molecules, which is embedded with ``embed_resident`` first.  ``residents`` as in ``screen``; shard ``j`` carries tag ``j``.

    Per batch ONE captured graph runs: ``model.predict`` (score and embedding from one run of the network, the forward-only tail),
    ``readout.embedding_max_cosine``, ``readout.select_rows`` with the bounds and the batch's live count, ``TopK.update`` of the kept
    rows with the kept count (both read on the device), and the running total of kept molecules.  A molecule outside the bounds
    never enters the list, so it cannot push another one off it.

    Returns ``top_score``, ``top_shard``, ``top_mol`` (trimmed to the occupied slots, best first); ``top_ref_sim`` and ``top_ref``, the
    nearest reference of every hit (gathered at the end from the per-shard vectors, which stay on the device at 8 bytes per
    molecule); ``n_scored`` and ``n_kept``; ``ref_emb`` (the ``[R, G]`` matrix that was compared with); and, with ``return_scores``,
    ``scores``, ``ref_sims`` and ``refs`` per shard.  The gather's status word is read once per shard; the model comes back in the mode
    it came in.  No bound, ``min_sim > max_sim``, a NaN bound, a multi-task model, a model, shard or references that are not on the
    GPU: ``ValueError`` before a launch."""
    from .shards import ResidentShard
    who = "screen_novel"
    if max_sim is None and min_sim is None:
        raise ValueError(f"{who}: give max_sim (novelty filter), min_sim (applicability domain) or both; screen ranks without a filter")
    lo = float("-inf") if min_sim is None else float(min_sim)
    hi = float("inf") if max_sim is None else float(max_sim)
    if lo != lo or hi != hi or lo > hi:
        raise ValueError(f"{who}: min_sim = {min_sim} and max_sim = {max_sim} leave no similarity to keep")
    G = _embedding_width(model)
    if model.ffn.out_features != 1:
        raise ValueError("screening ranks ONE score per molecule: a one-task model (task_dim = 1) is needed")
    if isinstance(ref_emb, ResidentShard):
        if int(ref_emb.n_molecules) < 1:
            raise ValueError(f"{who}: a reference shard holds at least one molecule")
        ref_emb = embed_resident(model, ref_emb, batch_size)
    dev = next(model.parameters()).device
    _check_refs(who, ref_emb, G, dev if dev.type == "cuda" else None)
    if dev.type != "cuda":
        raise ValueError(f"{who} runs on the GPU: move the model there (there is no CPU path)")
    from .readout import embedding_max_cosine, select_rows
    refs, bs = ref_emb.detach(), int(batch_size)
    if bs < 1:
        raise ValueError("batch_size >= 1")
    bounds = torch.tensor([lo, hi], dtype=torch.float32, device=dev)
    kept = (torch.empty(bs, dtype=torch.float32, device=dev), torch.empty(bs, dtype=torch.int32, device=dev),
            torch.empty(1, dtype=torch.int32, device=dev))
    total = torch.zeros(1, dtype=torch.int64, device=dev)

    def predict(data):
        pred, emb = model.predict(data)
        return (pred.reshape(-1), *embedding_max_cosine(_embedding_f32(emb), refs))

    def per_shard(resident, topk, tag):
        def rank(pred, ids, n_live, sim, arg):
            select_rows(pred, ids, sim, n_live, bounds, out=kept)
            topk.update(kept[0], kept[1], n_valid=kept[2])
            total.add_(kept[2])

        scores, sims, args = _run_shard(who, "scoring", model, resident, dev, bs, predict, (), topk, TopK, shard_tag=tag,
                                        extras=((torch.float32, float("nan")), (torch.int32, -1)), rank=rank)
        return (scores if return_scores else None), sims.clone(), args.clone()     # (clones: without the spare slot's storage)

    top_score, top_shard, top_mol, occupied, n_scored, shards = _over_shards(
        who, residents, lambda r: _check_model(model, r), lambda dev: TopK(k, dev), per_shard, True)
    top_shard, top_mol = top_shard[:occupied], top_mol[:occupied]
    sizes = [int(sims.numel()) for _, sims, _ in shards]
    first = torch.tensor(np.concatenate([[0], np.cumsum(sizes)[:-1]]), dtype=torch.int64, device=dev)
    at = first[top_shard.long()] + top_mol.long()
    result = {"top_score": top_score[:occupied], "top_shard": top_shard, "top_mol": top_mol,
              "top_ref_sim": torch.cat([sims for _, sims, _ in shards])[at], "top_ref": torch.cat([args for _, _, args in shards])[at],
              "n_scored": n_scored, "n_kept": int(total.item()), "ref_emb": ref_emb}
    if return_scores:
        result["scores"] = [scores for scores, _, _ in shards]
        result["ref_sims"] = [sims for _, sims, _ in shards]
        result["refs"] = [args for _, _, args in shards]
    return result


# -------------------------------------------------------------------------------------------- diverse hits --
# The step between "top k" and "which ones do we buy": the best thousand molecules of a library are mostly a few dozen chemical
# series repeated.  Leader clustering of the ranked list keeps the best molecule of each series and says which series every other
# hit belongs to.  The selection is sequential by definition; ``mkgnn_diverse_pick`` runs it on the device in rank-order tiles.
def diverse_pick_reference(sim, max_sim, k_max):
    """The definition of ``mkgnn_diverse_pick`` (include/molkgnn_hip.h), on the host, over a GIVEN square similarity matrix ``sim``
    (float32 or float64; only ``sim[i, p]``, ``p <= i``, is read: ``sim[i, p]`` is the similarity of row ``i`` as the row with row
    ``p`` as the query), rows in rank order: ``(picks int32 [k_max], n_picks, leader int32 [n], leader_sim [n]`` in ``sim``'s
    dtype ``)``.  Walk ``i = 0, 1, ...``: a row with a NaN ``sim[i, i]`` is never picked, never covered and covers nothing (``-1``,
    NaN); otherwise the FIRST pick ``p`` so far, in pick order, with ``sim[i, p] > max_sim`` (strict; a NaN never covers) is its
    leader (``leader[i] = p``, ``leader_sim[i] = sim[i, p]``); without one it becomes a pick (``leader[i] = i``, ``leader_sim[i] =
    sim[i, i]``) while fewer than ``k_max`` exist, and keeps ``(-1, NaN)`` once the list is full.  Unused slots of ``picks`` are
    ``-1``.  The comparison is made in ``sim``'s own dtype: ``max_sim`` is rounded to it first."""
    if torch.is_tensor(sim):
        sim = sim.detach().cpu().numpy()
    sim = np.asarray(sim)
    if sim.ndim != 2 or sim.shape[0] != sim.shape[1] or sim.dtype not in (np.float32, np.float64):
        raise ValueError("a square float32 or float64 similarity matrix is needed")
    n, k_max = sim.shape[0], int(k_max)
    if not 1 <= k_max <= max(n, 1):
        raise ValueError(f"k_max = {k_max} outside [1, {n}]")
    bound = sim.dtype.type(max_sim)
    if np.isnan(bound):
        raise ValueError("max_sim is NaN")
    picks = np.full(k_max, -1, dtype=np.int32)
    leader = np.full(n, -1, dtype=np.int32)
    leader_sim = np.full(n, np.nan, dtype=sim.dtype)
    chosen = []
    for i in range(n):
        if np.isnan(sim[i, i]):
            continue
        row = sim[i, chosen] if chosen else np.empty(0, dtype=sim.dtype)
        with np.errstate(invalid="ignore"):
            over = np.flatnonzero(row > bound)
        if over.size:
            p = chosen[int(over[0])]
            leader[i], leader_sim[i] = p, sim[i, p]
        elif len(chosen) < k_max:
            picks[len(chosen)] = i
            chosen.append(i)
            leader[i], leader_sim[i] = i, sim[i, i]
    return picks, len(chosen), leader, leader_sim


def _check_max_sim(who: str, max_sim) -> float:
    max_sim = float(max_sim)
    if max_sim != max_sim or max_sim in (float("inf"), float("-inf")):
        raise ValueError(f"{who}: max_sim = {max_sim} is not a finite similarity threshold")
    return max_sim


def rank_order(scores: torch.Tensor) -> torch.Tensor:
    """The rows of a float32 score vector in the order of ``topk_update_reference``, as int64 indices on the scores' device: non-NaN
    before NaN, descending with ``-0.0 == +0.0``, then the lower index.  (A descending torch sort alone puts NaN FIRST -- it ranks
    NaN above every number -- so the NaN rows are ranked as ``-inf`` in a stable sort and then moved behind the rest by a second
    stable sort, which keeps a true ``-inf`` score in front of them.)"""
    nan = torch.isnan(scores)
    key = torch.where(nan, torch.full_like(scores, float("-inf")), scores + 0.0)
    order = torch.sort(key, descending=True, stable=True).indices
    return order[torch.sort(nan[order].to(torch.int8), stable=True).indices]


def _cluster_sizes(leader: torch.Tensor, picks: torch.Tensor, n: int) -> torch.Tensor:
    """How many rows every pick leads, itself included: ``leader`` int ``[n]`` of row indices (``-1``: none), ``picks`` row indices."""
    led = leader.long()
    counts = torch.bincount(led[led >= 0], minlength=max(n, 1))
    return counts[picks.long()]


def pick_diverse_embeddings(emb: torch.Tensor, scores: torch.Tensor, max_sim: float, k: int,
                            ids: Optional[torch.Tensor] = None) -> dict:
    """The stored-embedding route: diverse hits among ANY scored set of molecules whose embeddings are kept -- the output of
    ``embed_resident`` and ``score_resident`` of a shard, say, up to 2^20 rows -- WITHOUT running the network.  ``emb`` float32
    ``[n, G]`` and ``scores`` float32 ``[n]`` on the GPU.  The rows are ranked by the order of ``topk_update_reference`` (non-NaN
    before NaN, descending, ``-0.0 == +0.0``, then the lower row), gathered in that order, and ``readout.diverse_pick`` walks them
    (``diverse_pick_reference`` is the definition): the best row of every cluster of cosine similarity above ``max_sim`` is a pick,
    at most ``k`` of them.  Returns a dict in terms of the caller's rows -- ``ids[row]`` when ``ids`` (an integer ``[n]`` tensor on
    the GPU) is given, the row numbers otherwise:

    ``picks``         ``[n_picks]`` int64: the picks, best first
    ``pick_score``    ``[n_picks]``: their scores
    ``leader``        ``[n]`` int64, by the caller's row: the pick that covers the row (itself for a pick), ``-1`` for none
    ``leader_sim``    ``[n]`` float32, by the caller's row: the similarity to that pick, NaN for none
    ``cluster_size``  ``[n_picks]`` int64: the rows every pick leads, itself included
    ``order``         ``[n]`` int64: the caller's rows in rank order (``order[0]`` is the best row)

    One host read at the end (the number of picks).  A wrong shape, dtype or device, a NaN or infinite ``max_sim``, ``k`` outside
    ``[1, n]``: ``ValueError`` before a launch."""
    who = "pick_diverse_embeddings"
    if not torch.is_tensor(emb) or emb.dim() != 2 or emb.dtype != torch.float32 or emb.shape[1] < 1:
        raise ValueError(f"{who}: emb is a float32 [n, G] tensor")
    n = int(emb.shape[0])
    if not torch.is_tensor(scores) or scores.dtype != torch.float32 or tuple(scores.shape) != (n,):
        raise ValueError(f"{who}: scores is a float32 [{n}] tensor, one score per row of emb")
    max_sim = _check_max_sim(who, max_sim)
    k = int(k)
    if not 1 <= k <= n:
        raise ValueError(f"{who}: k = {k} outside [1, {n}]")
    integer = (torch.int8, torch.int16, torch.int32, torch.int64, torch.uint8)
    if ids is not None and (not torch.is_tensor(ids) or ids.dtype not in integer or tuple(ids.shape) != (n,)):
        raise ValueError(f"{who}: ids is an integer [{n}] tensor")
    dev = emb.device
    if dev.type != "cuda" or scores.device != dev or (ids is not None and ids.device != dev):
        raise ValueError(f"{who}: emb is on {dev}; the selection runs on the GPU, with scores and ids on the same device (there is "
                         "no CPU path; diverse_pick_reference is the host form)")
    emb, scores = emb.detach(), scores.detach()
    order = rank_order(scores)
    picks, name, _, by_row, sim_by_row, sizes = _walk_in_order(emb, order, max_sim, k, ids)
    return {"picks": name[picks], "pick_score": scores[order[picks]], "leader": by_row, "leader_sim": sim_by_row,
            "cluster_size": sizes, "order": order}


def _walk_in_order(emb: torch.Tensor, order: torch.Tensor, max_sim: float, k: int, ids: Optional[torch.Tensor]):
    """``readout.diverse_pick`` over the rows of ``emb`` gathered in ``order`` (int64 ``[n]``, a permutation of the rows), mapped back
    to the caller's rows: ``(picks, name, leader_row, leader, leader_sim, cluster_size)`` -- ``picks`` int64 POSITIONS in ``order`` in
    pick order, ``name [n]`` what the caller calls the row at every position (``ids[order]``, or ``order`` itself), ``leader_row [n]``
    by the caller's row the ROW of the pick that covers it (``-1``: none), ``leader`` the same as ``name``s, ``leader_sim [n]`` by the
    caller's row, ``cluster_size`` the rows every pick leads.  One host read: the number of picks."""
    from .readout import diverse_pick
    picks, n_picks, leader, leader_sim = diverse_pick(emb.index_select(0, order), max_sim, k)
    picks = picks[:int(n_picks.item())].long()                   # (the one host read)
    name = order if ids is None else ids.long().index_select(0, order)          # rank position -> what the caller calls the row
    led = leader.long()
    row_by_row = torch.empty_like(led)
    row_by_row[order] = torch.where(led >= 0, order[led.clamp_min(0)], led)
    if ids is None:
        by_row = row_by_row
    else:
        by_row = torch.empty_like(led)
        by_row[order] = torch.where(led >= 0, name[led.clamp_min(0)], led)
    sim_by_row = torch.empty_like(leader_sim)
    sim_by_row[order] = leader_sim
    return picks, name, row_by_row, by_row, sim_by_row, _cluster_sizes(leader, picks, int(emb.shape[0]))


DIVERSE_MAX_POOL = 1024                         # the pool of screen_diverse is a TopK: MKGNN_TOPK_MAX_K


def screen_diverse(model, residents, k: int, batch_size: int, max_sim: float, pool: int = 1024,
                   return_embeddings: bool = False) -> dict:
    """``screen``, then the diverse hits among its best: the library is ranked into a pool of the best ``pool`` molecules (a
    ``TopK(pool)``, ``pool <= 1024``), and ``readout.diverse_pick`` walks the pool best first -- a molecule whose graph embedding has
    a cosine similarity above ``max_sim`` to an earlier pick belongs to that pick's cluster, one without becomes a pick, at most ``k
    <= pool`` of them (``diverse_pick_reference`` is the definition).  ``residents`` as in ``screen``; shard ``j`` carries tag ``j``.

    Per batch ONE captured graph runs ``model.predict`` once (score and embedding from one run of the network, the forward-only
    tail): the embedding is the pass's main result and is scattered into the shard's ``[n_molecules, G]`` matrix, the score is
    scattered into its vector and fed to the running list.  The per-shard embedding matrices stay on the device until the end --
    ``4 G`` bytes per molecule of the library (128 bytes at ``G = 32``; a library too large for that is screened with ``screen`` and
    its hits embedded again) -- because which molecules end up in the pool is known only then; the pool's rows are gathered from them
    by ``(top_shard, top_mol)``.

    Returns ``pool_score``, ``pool_shard``, ``pool_mol`` (the pool, trimmed to its occupied slots, best first: ``screen(..., k=pool)``'s
    lists bit for bit) and ``pool_emb`` (``[pool, G]``); ``pool_leader`` (int64: the POSITION IN THE POOL of the pick that covers the
    molecule, its own position for a pick, ``-1`` for none) and ``pool_leader_sim``; ``picks`` (int64 positions in the pool, best
    first); ``top_score``, ``top_shard``, ``top_mol`` of the picks; ``cluster_size`` (per pick, itself included); ``n_scored``; and,
    with ``return_embeddings``, ``embeddings``: the per-shard matrices.  The gather's status word is read once per shard; the model
    comes back in the mode it came in.  A NaN or infinite ``max_sim``, ``pool`` outside ``[1, 1024]``, ``k`` outside ``[1, pool]``, a
    multi-task model, a model or a shard that is not on the GPU: ``ValueError`` before a launch."""
    who = "screen_diverse"
    max_sim = _check_max_sim(who, max_sim)
    k, pool, bs = int(k), int(pool), int(batch_size)
    if not 1 <= pool <= DIVERSE_MAX_POOL:
        raise ValueError(f"{who}: pool = {pool} outside [1, {DIVERSE_MAX_POOL}] (the pool is a running list: MKGNN_TOPK_MAX_K)")
    if not 1 <= k <= pool:
        raise ValueError(f"{who}: k = {k} outside [1, pool = {pool}]: the picks are chosen among the pool")
    if bs < 1:
        raise ValueError("batch_size >= 1")
    G = _embedding_width(model)
    if model.ffn.out_features != 1:
        raise ValueError("screening ranks ONE score per molecule: a one-task model (task_dim = 1) is needed")
    if next(model.parameters()).device.type != "cuda":
        raise ValueError(f"{who} runs on the GPU: move the model there (there is no CPU path)")
    from .readout import diverse_pick

    def predict(data):
        pred, emb = model.predict(data)
        return _embedding_f32(emb), pred.reshape(-1)

    def per_shard(resident, topk, tag):
        dev = next(model.parameters()).device
        emb, _ = _run_shard(who, "scoring", model, resident, dev, bs, predict, (G,), topk, TopK, shard_tag=tag,
                            extras=((torch.float32, float("nan")),),
                            rank=lambda emb, ids, n_live, score: topk.update(score, ids, n_valid=n_live))
        return emb

    top_score, top_shard, top_mol, occupied, n_scored, embs = _over_shards(
        who, residents, lambda r: _check_model(model, r), lambda dev: TopK(pool, dev), per_shard, True)
    top_score, top_shard, top_mol = top_score[:occupied], top_shard[:occupied], top_mol[:occupied]
    dev = top_score.device
    pool_emb = torch.zeros((occupied, G), dtype=torch.float32, device=dev)
    for j, emb in enumerate(embs):                               # (no host read: a select per shard over at most 1 024 rows)
        here = top_shard == j
        if emb.shape[0] > 0:
            pool_emb = torch.where(here[:, None], emb.index_select(0, torch.where(here, top_mol, 0).long()), pool_emb)
    if occupied > 0:
        picks, n_picks, leader, leader_sim = diverse_pick(pool_emb, max_sim, min(k, occupied))
        picks = picks[:int(n_picks.item())].long()               # (the one host read of the selection)
    else:
        picks = torch.zeros(0, dtype=torch.int64, device=dev)
        leader = torch.zeros(0, dtype=torch.int32, device=dev)
        leader_sim = torch.zeros(0, dtype=torch.float32, device=dev)
    result = {"pool_score": top_score, "pool_shard": top_shard, "pool_mol": top_mol, "pool_emb": pool_emb,
              "pool_leader": leader.long(), "pool_leader_sim": leader_sim, "picks": picks, "top_score": top_score[picks],
              "top_shard": top_shard[picks], "top_mol": top_mol[picks], "cluster_size": _cluster_sizes(leader, picks, occupied),
              "n_scored": n_scored}
    if return_embeddings:
        result["embeddings"] = embs
    return result


# ------------------------------------------------------------------------------------------ MaxMin picking --
# Every selection above needs a similarity threshold chosen in advance and returns however many picks that threshold gives.  The
# farthest-first traversal (MaxMin, RDKit's MaxMinPicker) takes the budget k instead -- buy k compounds of a hit pool, subsample an
# over-represented class, extend a deck one owns with what it lacks most -- and returns the threshold as a by-product: pick_sim[t]
# is how close pick t was to everything chosen before it, which is also the max_sim to give screen_diverse for t picks.
#
# ``maxmin_pick_reference``    the definition in numpy, over a given similarity matrix
# ``pick_maxmin_embeddings``   stored embeddings (and a deck one owns, rows to leave out) -> the picks, every row's nearest pick
# ``select_maxmin``            shards of a library -> embed every molecule, one selection over all of them
MAXMIN_MAX_ROWS = 1 << 20                      # MKGNN_MAXMIN_MAX_ROWS
MAXMIN_MAX_PICKS = 4096                        # MKGNN_MAXMIN_MAX_PICKS
MAXMIN_DECK_SLICE = 1 << 20                    # deck rows per mkgnn_embed_max_cosine: MKGNN_MAX_COSINE_MAX_REFS


def maxmin_pick_reference(sim, k_max, stop_sim=float("inf"), start_sim=None):
    """The definition of ``mkgnn_maxmin_pick`` (include/molkgnn_hip.h), on the host, over a GIVEN square similarity matrix ``sim`` of
    any float dtype (``sim[j, i]`` is the similarity of row ``j`` as the row with row ``i`` as the query): ``(picks int32 [k_max],
    pick_sim [k_max], n_picks, leader int32 [n], leader_sim [n])``, the floats in ``sim``'s dtype.

    Row ``i`` is VALID when ``sim[i, i]`` is not NaN; any other row is never picked, takes no part and ends with ``(-1, NaN)``.
    ``cur[i]`` starts at ``start_sim[i]`` (rounded to ``sim``'s dtype), or at ``-inf`` without ``start_sim``; a valid row whose start
    value is NaN is EXCLUDED: never picked, but assigned like any other.  Round ``t = 0 .. k_max - 1``: the candidate is the valid,
    not excluded, not yet picked row with the SMALLEST ``cur`` (``-0.0 == +0.0``; among equals the lower row) -- none: stop; unless
    ``cur[i] < stop_sim`` (strict, ``stop_sim`` rounded to ``sim``'s dtype): stop.  ``picks[t] = i``, ``pick_sim[t] = cur[i]``,
    ``leader[i] = i``, ``cur[i] = sim[i, i]`` for good.  Every valid, not picked row ``j`` then meets the pick: with ``s = sim[j, i]``
    not NaN and (``cur[j]`` NaN or ``s > cur[j]``, strict: the EARLIER of equally near picks leads), ``cur[j] = s`` and ``leader[j] =
    i``.  Afterwards ``leader_sim[j] = cur[j]`` for the valid rows; unused slots of ``picks`` are ``-1``, of ``pick_sim`` NaN."""
    if torch.is_tensor(sim):
        sim = sim.detach().cpu().numpy()
    sim = np.asarray(sim)
    if sim.ndim != 2 or sim.shape[0] != sim.shape[1] or not np.issubdtype(sim.dtype, np.floating):
        raise ValueError("a square similarity matrix of a float dtype is needed")
    n, k_max = sim.shape[0], int(k_max)
    if not 1 <= k_max <= max(n, 1):
        raise ValueError(f"k_max = {k_max} outside [1, {n}]")
    stop = sim.dtype.type(stop_sim)
    if np.isnan(stop):
        raise ValueError("stop_sim is NaN")
    if start_sim is None:
        cur = np.full(n, -np.inf, dtype=sim.dtype)
    else:
        if torch.is_tensor(start_sim):
            start_sim = start_sim.detach().cpu().numpy()
        cur = np.array(start_sim, dtype=sim.dtype)               # (a copy)
        if cur.shape != (n,):
            raise ValueError(f"start_sim holds one value per row: [{n}]")
    valid = ~np.isnan(np.diagonal(sim))
    candidate = valid & ~np.isnan(cur)
    picked = np.zeros(n, dtype=bool)
    picks = np.full(k_max, -1, dtype=np.int32)
    pick_sim = np.full(k_max, np.nan, dtype=sim.dtype)
    leader = np.full(n, -1, dtype=np.int32)
    n_picks = 0
    for t in range(k_max):
        rows = np.flatnonzero(candidate)
        if rows.size == 0:
            break
        i = int(rows[np.argmin(cur[rows])])                      # (the first of the smallest: -0.0 == +0.0, the lower row)
        if not cur[i] < stop:
            break
        picks[t], pick_sim[t] = i, cur[i]
        n_picks = t + 1
        leader[i], cur[i] = i, sim[i, i]
        picked[i] = True
        candidate[i] = False
        s = sim[:, i]
        with np.errstate(invalid="ignore"):
            meet = valid & ~picked & ~np.isnan(s) & (np.isnan(cur) | (s > cur))
        cur[meet] = s[meet]
        leader[meet] = i
    return picks, pick_sim, n_picks, leader, np.where(valid, cur, sim.dtype.type(np.nan))


def _check_stop_sim(who: str, stop_sim) -> Optional[float]:
    if stop_sim is None:
        return None
    stop_sim = float(stop_sim)
    if stop_sim != stop_sim:
        raise ValueError(f"{who}: stop_sim is NaN")
    return stop_sim


def pick_maxmin_embeddings(emb: torch.Tensor, k: int, stop_sim: Optional[float] = None, deck: Optional[torch.Tensor] = None,
                           exclude: Optional[torch.Tensor] = None, ids: Optional[torch.Tensor] = None) -> dict:
    """MaxMin picking among ANY set of molecules whose embeddings are kept -- the output of ``embed_resident``, the ``pool_emb`` of
    ``screen_diverse``, up to 2^20 rows -- WITHOUT running the network: ``k`` rows of ``emb`` (float32 ``[n, G]`` on the GPU) that are
    as different from each other as possible (``readout.maxmin_pick``; ``maxmin_pick_reference`` is the definition).  Without a
    deck the first pick is the first valid row, so a list in rank order starts at its best molecule.  ``stop_sim``: stop once every
    remaining row lies within that similarity of the selection (strict; ``None``: only ``k`` ends it).  ``deck``: float32 ``[R, G]``
    embeddings one already owns -- every row starts at its similarity to its nearest deck row (``readout.embedding_max_cosine``; a
    deck beyond 2^20 rows goes in chunks combined by the maximum of what is not NaN), so the picks extend the deck with what it
    lacks most.  ``exclude``: bool ``[n]``, rows never to pick (molecules one owns that are part
    of ``emb``); they are still assigned to their nearest pick.  Returns a dict in terms of the caller's rows -- ``ids[row]`` when
    ``ids`` (an integer ``[n]`` tensor on the GPU) is given, the row numbers otherwise:

    ``picks``         ``[n_picks]`` int64: the picks, in pick order
    ``pick_sim``      ``[n_picks]`` float32: how close each was to everything chosen before it (and to the deck); non-decreasing
    ``n_picks``       their number
    ``leader``        ``[n]`` int64, by the caller's row: the pick nearest to the row (itself for a pick); ``-1`` for a row that is
                      NaN, and for one that no pick came nearer to than the deck
    ``leader_sim``    ``[n]`` float32, by the caller's row: the similarity to that pick (or to the deck); NaN for a NaN row
    ``cluster_size``  ``[n_picks]`` int64: the rows every pick leads, itself included
    ``deck_sim``      ``[n]`` float32, with a deck: every row's similarity to its nearest deck row

    One host read at the end (the number of picks).  A wrong shape, dtype or device, a NaN ``stop_sim``, ``k`` outside ``[1, min(n,
    4096)]``, more than 2^20 rows: ``ValueError`` before a launch."""
    who = "pick_maxmin_embeddings"
    if not torch.is_tensor(emb) or emb.dim() != 2 or emb.dtype != torch.float32 or emb.shape[1] < 1:
        raise ValueError(f"{who}: emb is a float32 [n, G] tensor")
    n, G = int(emb.shape[0]), int(emb.shape[1])
    if not 1 <= n <= MAXMIN_MAX_ROWS:
        raise ValueError(f"{who}: {n} rows outside [1, {MAXMIN_MAX_ROWS}]")
    k = int(k)
    if not 1 <= k <= min(n, MAXMIN_MAX_PICKS):
        raise ValueError(f"{who}: k = {k} outside [1, {min(n, MAXMIN_MAX_PICKS)}] (at most {MAXMIN_MAX_PICKS} picks per call, and no "
                         "more than there are rows)")
    stop_sim = _check_stop_sim(who, stop_sim)
    if deck is not None and (not torch.is_tensor(deck) or deck.dim() != 2 or deck.dtype != torch.float32
                             or int(deck.shape[1]) != G or int(deck.shape[0]) < 1):
        raise ValueError(f"{who}: deck is a float32 [R, {G}] tensor of at least one embedding")
    if exclude is not None and (not torch.is_tensor(exclude) or exclude.dtype != torch.bool or tuple(exclude.shape) != (n,)):
        raise ValueError(f"{who}: exclude is a bool [{n}] tensor")
    integer = (torch.int8, torch.int16, torch.int32, torch.int64, torch.uint8)
    if ids is not None and (not torch.is_tensor(ids) or ids.dtype not in integer or tuple(ids.shape) != (n,)):
        raise ValueError(f"{who}: ids is an integer [{n}] tensor")
    dev = emb.device
    if dev.type != "cuda" or any(t is not None and t.device != dev for t in (deck, exclude, ids)):
        raise ValueError(f"{who}: emb is on {dev}; the selection runs on the GPU, with deck, exclude and ids on the same device (there "
                         "is no CPU path; maxmin_pick_reference is the host form)")
    from .readout import embedding_max_cosine, maxmin_pick
    emb = emb.detach()
    deck_sim = start = None
    if deck is not None:
        deck = deck.detach()
        for a in range(0, int(deck.shape[0]), MAXMIN_DECK_SLICE):
            part = embedding_max_cosine(emb, deck[a:a + MAXMIN_DECK_SLICE])[0]
            deck_sim = part if deck_sim is None else torch.fmax(deck_sim, part)         # (the maximum of what is not NaN)
        start = deck_sim
    if exclude is not None:
        if start is None:
            start = torch.full((n,), float("-inf"), dtype=torch.float32, device=dev)
        start = torch.where(exclude, torch.full_like(start, float("nan")), start)
    picks, pick_sim, n_picks, leader, leader_sim = maxmin_pick(emb, k, stop_sim, start)
    count = int(n_picks.item())                                  # (the one host read)
    picks = picks[:count].long()
    led = leader.long()
    if ids is not None:
        name = ids.long()
        led, names = torch.where(led >= 0, name[led.clamp_min(0)], led), name[picks]
    else:
        names = picks
    result = {"picks": names, "pick_sim": pick_sim[:count], "n_picks": count, "leader": led, "leader_sim": leader_sim,
              "cluster_size": _cluster_sizes(leader, picks, n)}
    if deck_sim is not None:
        result["deck_sim"] = deck_sim
    return result


def select_maxmin(model, residents, k: int, batch_size: int, stop_sim: Optional[float] = None, deck=None) -> dict:
    """MaxMin picking over a library: every molecule of every shard of ``residents`` (as in ``screen``; shard ``j`` carries tag
    ``j``) is embedded with ``embed_resident``, and ONE ``pick_maxmin_embeddings`` runs over the concatenation -- up to 2^20 molecules
    in all (128 bytes each at ``G = 32``).  The head is not run, so the model may have any ``task_dim``.  ``deck``: what one already
    owns, a float32 ``[R, G]`` tensor of embeddings on the model's GPU or a ``ResidentShard``, which is embedded first.  Returns
    ``top_shard``, ``top_mol`` and ``pick_sim`` of the picks, in pick order; ``picks`` (int64 positions in the concatenation) and
    ``n_picks``; ``leader`` (per shard: int64 positions in the concatenation of every molecule's nearest pick, ``-1`` for none) and
    ``leader_sim`` (per shard); ``cluster_size`` (per pick, itself included); ``n_embedded``; and, with a deck, ``deck_sim`` (per shard) and
    ``deck_emb`` (the ``[R, G]`` matrix that was compared with).
    The gather's status word is read once per shard; the model comes back in the mode it came in.  A NaN ``stop_sim``, ``k`` outside
    ``[1, 4096]``, a model, shard or deck that is not on the GPU: ``ValueError`` before a launch; a library of more than 2^20
    molecules: ``ValueError`` as soon as the shards seen so far hold that many, before the selection."""
    from .shards import ResidentShard
    who = "select_maxmin"
    k, bs = int(k), int(batch_size)
    if not 1 <= k <= MAXMIN_MAX_PICKS:
        raise ValueError(f"{who}: k = {k} outside [1, {MAXMIN_MAX_PICKS}] (MKGNN_MAXMIN_MAX_PICKS)")
    if bs < 1:
        raise ValueError("batch_size >= 1")
    stop_sim = _check_stop_sim(who, stop_sim)
    G = _embedding_width(model)
    if next(model.parameters()).device.type != "cuda":
        raise ValueError(f"{who} runs on the GPU: move the model there (there is no CPU path)")
    if not isinstance(residents, (list, tuple)):
        residents = list(residents)
    if not residents:
        raise ValueError(f"{who} needs at least one shard")
    sizes = [int(r.n_molecules) for r in residents]
    if sum(sizes) > MAXMIN_MAX_ROWS:
        raise ValueError(f"{who}: the shards hold {sum(sizes)} molecules; one selection takes at most {MAXMIN_MAX_ROWS} (2^20) in all "
                         "-- select within parts of the library, then among the parts' picks")
    if sum(sizes) < k:
        raise ValueError(f"{who}: k = {k} picks among {sum(sizes)} molecules")
    for r in residents:
        _check_device(model, r)
    if isinstance(deck, ResidentShard):
        if int(deck.n_molecules) < 1:
            raise ValueError(f"{who}: a deck shard holds at least one molecule")
        deck = _embedding_f32(embed_resident(model, deck, bs))
    dev = next(model.parameters()).device
    if deck is not None:
        _check_vectors(who, deck, G, dev, "deck embeddings", None, "")
    emb = torch.cat([_embedding_f32(embed_resident(model, r, bs)) for r in residents])
    r = pick_maxmin_embeddings(emb, k, stop_sim, deck)
    first = torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.int64, device=dev)
    picks = r["picks"]
    shard = torch.bucketize(picks, first[1:], right=True)
    result = {"top_shard": shard.to(torch.int32), "top_mol": (picks - first[shard]).to(torch.int32), "pick_sim": r["pick_sim"],
              "picks": picks, "n_picks": r["n_picks"], "leader": list(torch.split(r["leader"], sizes)),
              "leader_sim": list(torch.split(r["leader_sim"], sizes)), "cluster_size": r["cluster_size"], "n_embedded": sum(sizes)}
    if deck is not None:
        result["deck_sim"] = list(torch.split(r["deck_sim"], sizes))
        result["deck_emb"] = deck
    return result


# ------------------------------------------------------------------------- neighbour counts, Butina clusters --
# Everything above asks for the nearest molecule or the first one above a threshold.  HOW MANY lie above it is what the standard
# clustering of hit lists and screening decks (Taylor-Butina) ranks by: the molecule with the most neighbours is the first
# centroid and takes its neighbours, the next unassigned molecule in count order is the next one.  With static counts that is the
# leader walk (``mkgnn_diverse_pick``) in count order; the count is ``mkgnn_embed_count_within``, over the same similarity bits.
#
# ``count_within_reference`` / ``butina_reference``  the definitions in numpy, over a given similarity matrix
# ``neighbour_counts``                               stored embeddings against any number of references: analogue counts
# ``cluster_butina_embeddings``                      stored embeddings -> centroids, every row's cluster, the best member of each
NEIGHBOUR_SLICE = 1 << 20                      # references per mkgnn_embed_count_within: MKGNN_MAX_COSINE_MAX_REFS
BUTINA_MAX_ROWS = 1 << 20                      # MKGNN_DIVERSE_MAX_ROWS = MKGNN_MAX_COSINE_MAX_REFS: the walk and the self-join


def count_within_reference(sim, min_sim) -> np.ndarray:
    """The definition of ``mkgnn_embed_count_within`` (include/molkgnn_hip.h), on the host, over a GIVEN similarity matrix ``sim [n,
    R]`` (float32 or float64; ``sim[i, r]`` is the similarity of row ``i`` as the row with reference ``r`` as the query): int64
    ``[n]``, the number of ``r`` with ``sim[i, r] > min_sim`` -- strict; a NaN never counts.  The comparison is made in ``sim``'s own
    dtype: ``min_sim`` is rounded to it first."""
    if torch.is_tensor(sim):
        sim = sim.detach().cpu().numpy()
    sim = np.asarray(sim)
    if sim.ndim != 2 or sim.dtype not in (np.float32, np.float64):
        raise ValueError("a float32 or float64 [n, R] similarity matrix is needed")
    bound = sim.dtype.type(min_sim)
    if not np.isfinite(bound):
        raise ValueError(f"min_sim = {min_sim} is not a finite similarity threshold")
    with np.errstate(invalid="ignore"):
        return (sim > bound).sum(axis=1).astype(np.int64)


def butina_reference(sim, min_sim, k_max):
    """Taylor-Butina clustering with static counts, on the host, over a GIVEN square similarity matrix (float32 or float64; ``sim[i,
    p]`` is the similarity of row ``i`` as the row with row ``p`` as the query): ``(centroids int32 [k_max], n_clusters, leader int32
    [n], leader_sim [n], counts int64 [n], order int64 [n])``.  ``counts = count_within_reference(sim, min_sim)`` (the diagonal is a
    pair like any other); ``order`` is the rows by count descending, ties to the lower row; ``diverse_pick_reference`` walks ``sim``
    permuted by ``order`` with ``min_sim`` as its threshold and at most ``k_max`` picks, and its indices are mapped back to rows.  A
    composition: NaN rows, zero rows and a full list behave as the leader walk defines them.  ``centroids`` is in cluster order,
    densest first, unused slots ``-1``; ``leader[i]`` is the centroid ROW of row ``i`` (``-1``: none), ``leader_sim[i]`` in ``sim``'s
    dtype (NaN: none)."""
    counts = count_within_reference(sim, min_sim)
    if torch.is_tensor(sim):
        sim = sim.detach().cpu().numpy()
    sim = np.asarray(sim)
    if sim.shape[0] != sim.shape[1]:
        raise ValueError("a square float32 or float64 similarity matrix is needed")
    n = sim.shape[0]
    order = np.argsort(-counts, kind="stable").astype(np.int64)
    picks, n_picks, lead, lead_sim = diverse_pick_reference(sim[np.ix_(order, order)], min_sim, k_max)
    centroids = np.where(picks >= 0, order[np.maximum(picks, 0)], -1).astype(np.int32)
    leader = np.full(n, -1, dtype=np.int32)
    leader[order] = np.where(lead >= 0, order[np.maximum(lead, 0)], -1)
    leader_sim = np.full(n, np.nan, dtype=sim.dtype)
    leader_sim[order] = lead_sim
    return centroids, n_picks, leader, leader_sim, counts, order


def _check_embeddings(who: str, emb, what: str = "emb") -> None:
    if not torch.is_tensor(emb) or emb.dim() != 2 or emb.dtype != torch.float32 or emb.shape[1] < 1:
        raise ValueError(f"{who}: {what} is a float32 [n, G] tensor")


def neighbour_counts(emb: torch.Tensor, refs: torch.Tensor, min_sim: float) -> torch.Tensor:
    """The stored-embedding route for analogue counts ("SAR by catalogue"): int64 ``[n]``, for every row of ``emb`` (float32 ``[n,
    G]`` on the GPU) the number of rows of ``refs`` (float32 ``[R, G]`` on the same device, ANY ``R >= 1``) whose cosine similarity to
    it lies above ``min_sim`` -- ``readout.embedding_count_within``'s definition and bits (``count_within_reference`` is the host
    form): strict, a NaN never counts, no "self".  The references go in slices of at most 2^20 rows, one
    ``mkgnn_embed_count_within`` each, and the int32 results are added in int64; no ``[n, R]`` matrix exists and nothing is read
    back to the host.  A wrong shape, dtype or device, a NaN or infinite ``min_sim``: ``ValueError`` before a launch."""
    who = "neighbour_counts"
    _check_embeddings(who, emb)
    _check_embeddings(who, refs, "refs")
    if refs.shape[1] != emb.shape[1] or refs.shape[0] < 1:
        raise ValueError(f"{who}: refs holds at least one row as wide as emb ({emb.shape[1]}), not {tuple(refs.shape)}")
    min_sim = _check_max_sim(who, min_sim)
    dev = emb.device
    if dev.type != "cuda" or refs.device != dev:
        raise ValueError(f"{who}: emb is on {dev}, refs on {refs.device}; the count runs on the GPU, with both on the same device "
                         "(there is no CPU path; count_within_reference is the host form)")
    from .readout import embedding_count_within
    emb, refs = emb.detach(), refs.detach()
    total = torch.zeros(emb.shape[0], dtype=torch.int64, device=dev)
    part = torch.empty(emb.shape[0], dtype=torch.int32, device=dev)
    for a in range(0, int(refs.shape[0]), NEIGHBOUR_SLICE):
        total += embedding_count_within(emb, refs[a:a + NEIGHBOUR_SLICE], min_sim, out=part)
    return total


def cluster_butina_embeddings(emb: torch.Tensor, min_sim: float, k: Optional[int] = None, scores: Optional[torch.Tensor] = None,
                              ids: Optional[torch.Tensor] = None) -> dict:
    """Taylor-Butina clustering (static counts) of ANY set of molecules whose embeddings are kept, up to 2^20 rows, WITHOUT running
    the network: ``emb`` float32 ``[n, G]`` on the GPU.  Every row's neighbours above ``min_sim`` are counted
    (``readout.embedding_count_within(emb, emb, min_sim)``: the self-join, the diagonal included), the rows are sorted by count
    descending (stable: ties to the lower row), gathered in that order, and ``readout.diverse_pick`` walks them with ``min_sim`` as
    its threshold and at most ``k`` picks (default: no cap) -- the count and the walk compare the same similarity bits, so a
    neighbour in the count is a neighbour in the walk; ``butina_reference`` is the definition.  The densest row becomes the first
    centroid and takes its neighbours, the next unassigned row in count order the next: a series is represented by its centre,
    where ``pick_diverse_embeddings`` starts its clusters at whatever scores best.  Returns a dict in terms of the caller's rows --
    ``ids[row]`` when ``ids`` (an integer ``[n]`` tensor on the GPU) is given, the row numbers otherwise:

    ``centroids``        ``[n_clusters]`` int64: the centroids in cluster order, densest first
    ``neighbour_count``  ``[n]`` int64, by the caller's row: the rows above ``min_sim`` of it, itself included
    ``leader``           ``[n]`` int64, by the caller's row: the centroid of its cluster (itself for a centroid), ``-1`` for none
    ``leader_sim``       ``[n]`` float32, by the caller's row: the similarity to that centroid, NaN for none
    ``cluster_size``     ``[n_clusters]`` int64: the rows of every cluster, the centroid included
    ``order``            ``[n]`` int64: the caller's rows in count order (``order[0]`` is the densest row)

    and, when ``scores`` (float32 ``[n]`` on the GPU) is given, the molecule one buys from every series:

    ``cluster_best``        ``[n_clusters]`` int64: the member of every cluster that comes first in ``rank_order(scores)``
    ``cluster_best_score``  ``[n_clusters]`` float32: its score

    The hit-list use needs no new pass over a library: ``r = screen_diverse(...)``, then ``cluster_butina_embeddings(r["pool_emb"],
    min_sim, scores=r["pool_score"])``; the whole-shard use is ``embed_resident`` plus ``score_resident``, then this function.  One
    host read (the number of clusters).  A wrong shape, dtype or device, a NaN or infinite ``min_sim``, ``n`` outside ``[1, 2^20]``,
    ``k`` outside ``[1, n]``: ``ValueError`` before a launch."""
    who = "cluster_butina_embeddings"
    _check_embeddings(who, emb)
    n = int(emb.shape[0])
    if not 1 <= n <= BUTINA_MAX_ROWS:
        raise ValueError(f"{who}: {n} rows outside [1, {BUTINA_MAX_ROWS}]")
    min_sim = _check_max_sim(who, min_sim)
    k = n if k is None else int(k)
    if not 1 <= k <= n:
        raise ValueError(f"{who}: k = {k} outside [1, {n}]")
    if scores is not None and (not torch.is_tensor(scores) or scores.dtype != torch.float32 or tuple(scores.shape) != (n,)):
        raise ValueError(f"{who}: scores is a float32 [{n}] tensor, one score per row of emb")
    integer = (torch.int8, torch.int16, torch.int32, torch.int64, torch.uint8)
    if ids is not None and (not torch.is_tensor(ids) or ids.dtype not in integer or tuple(ids.shape) != (n,)):
        raise ValueError(f"{who}: ids is an integer [{n}] tensor")
    dev = emb.device
    if dev.type != "cuda" or (scores is not None and scores.device != dev) or (ids is not None and ids.device != dev):
        raise ValueError(f"{who}: emb is on {dev}; the clustering runs on the GPU, with scores and ids on the same device (there is "
                         "no CPU path; butina_reference is the host form)")
    from .readout import embedding_count_within
    emb = emb.detach()
    counts = embedding_count_within(emb, emb, min_sim)
    order = torch.sort(counts, descending=True, stable=True).indices
    picks, name, leader_row, leader, leader_sim, sizes = _walk_in_order(emb, order, min_sim, k, ids)
    result = {"centroids": name[picks], "neighbour_count": counts.long(), "leader": leader, "leader_sim": leader_sim,
              "cluster_size": sizes, "order": order}
    if scores is not None:
        scores = scores.detach()
        ranked = rank_order(scores)
        place = torch.empty_like(ranked)
        place[ranked] = torch.arange(n, device=dev)               # row -> its place in the ranking
        first = torch.full((n + 1,), n, dtype=torch.int64, device=dev)             # (slot n: the rows without a cluster)
        first.scatter_reduce_(0, torch.where(leader_row >= 0, leader_row, n), place, reduce="amin")   # centroid row -> its members' best place
        best = ranked[first[order[picks]]]                         # (every centroid leads itself: its slot is set)
        result["cluster_best"] = best if ids is None else ids.long()[best]
        result["cluster_best_score"] = scores[best]
    return result


# ------------------------------------------------------------------- neighbour lists, linked components, leakage --
# WHICH molecules lie above the threshold (``mkgnn_embed_neighbours_within``: the analogues themselves, and the threshold graph),
# and that graph's connected components (``mkgnn_graph_components``): the single-linkage clusters, the ONLY partition -- and the
# finest -- with no pair above the threshold across its parts.  A Butina row joins the first centroid above the threshold, so
# rows of different Butina clusters can be closer than it; ``split_leakage`` counts such pairs for any split.
#
# ``neighbours_reference`` / ``components_reference``  the definitions on the host
# ``neighbour_lists``                  stored embeddings against up to 2^20 references: the analogues of every row
# ``cluster_components_embeddings``    stored embeddings -> every row's component, sizes, the self-join's lists, the best of each
# ``split_leakage``                    stored pairs by (fold of the row, fold of the reference)
NEIGHBOUR_MAX_PAIRS = 1 << 28                  # the default cap on the pairs of one list: 2 GiB of (reference, similarity)


def neighbours_reference(sim, min_sim):
    """The definition of ``mkgnn_embed_neighbours_within`` (include/molkgnn_hip.h), on the host, over a GIVEN similarity matrix ``sim
    [n, R]`` (float32 or float64): ``(row_ptr int64 [n + 1], nbr int32 [nnz], nbr_sim [nnz])`` -- row ``i`` owns the slots ``row_ptr[i]
    .. row_ptr[i + 1]``, which hold the ``r`` with ``sim[i, r] > min_sim`` in ascending ``r`` and those elements of ``sim``.  Strict; a
    NaN never qualifies; the comparison is made in ``sim``'s own dtype (``min_sim`` is rounded to it first), as in
    ``count_within_reference``, whose counts are ``diff(row_ptr)``."""
    if torch.is_tensor(sim):
        sim = sim.detach().cpu().numpy()
    sim = np.asarray(sim)
    if sim.ndim != 2 or sim.dtype not in (np.float32, np.float64):
        raise ValueError("a float32 or float64 [n, R] similarity matrix is needed")
    bound = sim.dtype.type(min_sim)
    if not np.isfinite(bound):
        raise ValueError(f"min_sim = {min_sim} is not a finite similarity threshold")
    with np.errstate(invalid="ignore"):
        above = sim > bound
    row_ptr = np.zeros(sim.shape[0] + 1, dtype=np.int64)
    np.cumsum(above.sum(axis=1), out=row_ptr[1:])
    rows, cols = np.nonzero(above)                               # (row-major: by row, then by ascending reference)
    return row_ptr, cols.astype(np.int32), sim[rows, cols]


def components_reference(row_ptr, col, n) -> np.ndarray:
    """The definition of ``mkgnn_graph_components``, on the host: int32 ``[n]``, for every vertex the smallest vertex of its component
    in the graph where ``u`` and ``v`` are linked if ``col`` holds ``v`` in ``u``'s segment ``row_ptr[u] .. row_ptr[u + 1]`` or ``u`` in
    ``v``'s.  A plain union-find, the smaller root kept.  A column outside ``[0, n)`` or a segment outside ``0 <= row_ptr[v] <=
    row_ptr[v + 1] <= len(col)``: ``ValueError``."""
    n = int(n)
    row_ptr, col = _host(row_ptr, np.int64).reshape(-1), _host(col, np.int64).reshape(-1)
    if n < 0 or row_ptr.shape[0] != n + 1:
        raise ValueError(f"row_ptr holds n + 1 = {n + 1} entries")
    parent = list(range(n))

    def root(v):
        while parent[v] != v:
            parent[v] = parent[parent[v]]
            v = parent[v]
        return v

    for u in range(n):
        a, b = int(row_ptr[u]), int(row_ptr[u + 1])
        if not 0 <= a <= b <= col.shape[0]:
            raise ValueError(f"the segment of vertex {u}, [{a}, {b}), is not one of col [{col.shape[0]}]")
        for v in col[a:b].tolist():
            if not 0 <= v < n:
                raise ValueError(f"col holds {v}, outside [0, {n})")
            ru, rv = root(u), root(v)
            if ru != rv:
                parent[max(ru, rv)] = min(ru, rv)
    return np.array([root(v) for v in range(n)], dtype=np.int32)


def _check_max_pairs(who: str, max_pairs) -> int:
    if isinstance(max_pairs, bool) or not isinstance(max_pairs, int) or max_pairs < 0:
        raise ValueError(f"{who}: max_pairs = {max_pairs!r} is not a count of pairs (an int >= 0)")
    return max_pairs


def neighbour_lists(emb: torch.Tensor, refs: torch.Tensor, min_sim: float, max_pairs: int = NEIGHBOUR_MAX_PAIRS):
    """The stored-embedding route to the analogues themselves ("SAR by catalogue" ends with them): ``(row_ptr int64 [n + 1], nbr int32
    [nnz], nbr_sim float32 [nnz])`` -- for every row of ``emb`` (float32 ``[n, G]`` on the GPU) the rows of ``refs`` (float32 ``[R, G]``
    on the same device, ``1 <= R <= 2^20``) whose cosine similarity to it lies above ``min_sim``, in ascending ``r``, with those
    similarities: the pairs ``neighbour_counts`` counts, by ``readout.embedding_neighbours_within``'s definition and bits
    (``neighbours_reference`` is the host form).  Strict, a NaN never qualifies, no "self".  No ``[n, R]`` matrix exists; one host read
    (``nnz``, to allocate the lists); more than ``max_pairs`` pairs raise ``ValueError`` naming the number, before the lists are
    allocated.  A wrong shape, dtype or device, a NaN or infinite ``min_sim``, a bad ``max_pairs``: ``ValueError`` before a launch."""
    who = "neighbour_lists"
    _check_embeddings(who, emb)
    _check_embeddings(who, refs, "refs")
    if refs.shape[1] != emb.shape[1] or not 1 <= refs.shape[0] <= NEIGHBOUR_SLICE:
        raise ValueError(f"{who}: refs holds 1 to {NEIGHBOUR_SLICE} rows as wide as emb ({emb.shape[1]}), not {tuple(refs.shape)}")
    min_sim = _check_max_sim(who, min_sim)
    max_pairs = _check_max_pairs(who, max_pairs)
    dev = emb.device
    if dev.type != "cuda" or refs.device != dev:
        raise ValueError(f"{who}: emb is on {dev}, refs on {refs.device}; the lists are made on the GPU, with both on the same device "
                         "(there is no CPU path; neighbours_reference is the host form)")
    from .readout import embedding_neighbours_within
    return embedding_neighbours_within(emb.detach(), refs.detach(), min_sim, max_pairs=max_pairs)


def cluster_components_embeddings(emb: torch.Tensor, min_sim: float, scores: Optional[torch.Tensor] = None,
                                  ids: Optional[torch.Tensor] = None, max_pairs: int = NEIGHBOUR_MAX_PAIRS) -> dict:
    """The connected components of the threshold graph -- single-linkage clusters at ``min_sim`` -- of ANY set of molecules whose
    embeddings are kept, up to 2^20 rows, WITHOUT running the network: ``emb`` float32 ``[n, G]`` on the GPU.  The self-join's lists
    (``readout.embedding_neighbours_within(emb, emb, min_sim)``, the diagonal included, as the count defines it) are the graph, and
    ``readout.graph_components`` labels it; rows ``i`` and ``j`` are linked if ``S[i, j] > min_sim`` OR ``S[j, i] > min_sim`` (the two
    differ in their last bit at most).  This is the one partition that guarantees NO PAIR ABOVE ``min_sim`` ACROSS ITS PARTS, and the
    finest: what ``sampling.cluster_split`` needs for a leakage-free split, which Butina clusters do not give (``split_leakage``
    measures it).  A chain of neighbours is one component however long it is.  A NaN row has no neighbours, not even itself, and is a
    component of its own.  Returns a dict in terms of the caller's rows -- ``ids[row]`` when ``ids`` (an integer ``[n]`` tensor on the
    GPU) is given, the row numbers otherwise:

    ``component``        ``[n]`` int64, by the caller's row: the name of its component -- its smallest row
    ``components``       ``[n_components]`` int64: those names, in the order of ascending smallest row
    ``n_components``     their number
    ``component_size``   ``[n_components]`` int64: the rows of every component, in that order
    ``neighbour_count``  ``[n]`` int64: the rows above ``min_sim`` of every row, itself included
    ``row_ptr``, ``neighbour``, ``neighbour_sim``   the self-join's lists (int64 ``[n + 1]``, int32 ``[nnz]`` of ROW numbers, float32 ``[nnz]``)

    and, when ``scores`` (float32 ``[n]`` on the GPU) is given, under ``cluster_butina_embeddings``' ``cluster_best`` rule:

    ``component_best``        ``[n_components]`` int64: the member of every component that comes first in ``rank_order(scores)``
    ``component_best_score``  ``[n_components]`` float32: its score

    Host reads: the size of the lists, the components' state, their number.  More than ``max_pairs`` pairs: ``ValueError`` naming the
    number.  A wrong shape, dtype or device, a NaN or infinite ``min_sim``, ``n`` outside ``[1, 2^20]``: ``ValueError`` before a
    launch."""
    who = "cluster_components_embeddings"
    _check_embeddings(who, emb)
    n = int(emb.shape[0])
    if not 1 <= n <= BUTINA_MAX_ROWS:
        raise ValueError(f"{who}: {n} rows outside [1, {BUTINA_MAX_ROWS}]")
    min_sim = _check_max_sim(who, min_sim)
    max_pairs = _check_max_pairs(who, max_pairs)
    if scores is not None and (not torch.is_tensor(scores) or scores.dtype != torch.float32 or tuple(scores.shape) != (n,)):
        raise ValueError(f"{who}: scores is a float32 [{n}] tensor, one score per row of emb")
    integer = (torch.int8, torch.int16, torch.int32, torch.int64, torch.uint8)
    if ids is not None and (not torch.is_tensor(ids) or ids.dtype not in integer or tuple(ids.shape) != (n,)):
        raise ValueError(f"{who}: ids is an integer [{n}] tensor")
    dev = emb.device
    if dev.type != "cuda" or (scores is not None and scores.device != dev) or (ids is not None and ids.device != dev):
        raise ValueError(f"{who}: emb is on {dev}; the components are found on the GPU, with scores and ids on the same device "
                         "(there is no CPU path; neighbours_reference and components_reference are the host forms)")
    from .readout import embedding_neighbours_within, graph_components
    emb = emb.detach()
    row_ptr, nbr, nbr_sim = embedding_neighbours_within(emb, emb, min_sim, max_pairs=max_pairs)
    label = graph_components(row_ptr, nbr, n).long()             # every row's component: its smallest row
    sizes_by_row = torch.bincount(label, minlength=n)
    roots = torch.nonzero(sizes_by_row, as_tuple=True)[0]        # ascending (a host read: their number)
    name = torch.arange(n, device=dev) if ids is None else ids.long()
    result = {"component": name[label], "components": name[roots], "n_components": int(roots.numel()),
              "component_size": sizes_by_row[roots], "neighbour_count": row_ptr[1:] - row_ptr[:-1], "row_ptr": row_ptr,
              "neighbour": nbr, "neighbour_sim": nbr_sim}
    if scores is not None:
        scores = scores.detach()
        ranked = rank_order(scores)
        place = torch.empty_like(ranked)
        place[ranked] = torch.arange(n, device=dev)              # row -> its place in the ranking
        first = torch.full((n,), n, dtype=torch.int64, device=dev)
        first.scatter_reduce_(0, label, place, reduce="amin")    # smallest row of a component -> its members' best place
        best = ranked[first[roots]]
        result["component_best"] = name[best]
        result["component_best_score"] = scores[best]
    return result


def split_leakage(row_ptr: torch.Tensor, neighbour: torch.Tensor, folds: torch.Tensor,
                  ref_folds: Optional[torch.Tensor] = None) -> torch.Tensor:
    """How many stored pairs cross a split: int64 ``[F, F]`` on the lists' device, entry ``[a, b]`` the number of pairs ``(i, r)`` of the
    CSR lists ``(row_ptr [n + 1], neighbour [nnz])`` -- ``neighbour_lists`` or ``cluster_components_embeddings`` made them -- with
    ``folds[i] == a`` and ``ref_folds[r] == b``; ``F`` is one more than the largest fold named.  ``folds`` is an integer ``[n]`` tensor
    of values ``>= 0`` (``sampling.cluster_split`` returns one), ``ref_folds`` one per reference, or ``None`` for a self-join, where the
    references are the rows.  The matrix's total is ``nnz``; its OFF-DIAGONAL sum is the leakage, the ordered pairs above the
    threshold whose two ends lie in different folds: 0 for a split over ``cluster_components_embeddings``' components, not for one
    over Butina clusters.  With ``refs`` a test set and ``folds`` all zero but for the rows of interest it answers "how many training
    molecules have a test neighbour" the same way.  Torch operators only, on whatever device the tensors share; the checks of the
    lists and ``F`` are read on the host.  Lists that are not a CSR, a reference outside ``ref_folds``, a negative fold:
    ``ValueError``."""
    who = "split_leakage"
    integer = (torch.int8, torch.int16, torch.int32, torch.int64, torch.uint8)
    if not all(torch.is_tensor(t) and t.dim() == 1 and t.dtype in integer for t in (row_ptr, neighbour, folds)) \
            or row_ptr.numel() != folds.numel() + 1:
        raise ValueError(f"{who}: row_ptr [n + 1], neighbour [nnz] and folds [n] are integer tensors")
    if ref_folds is None:
        ref_folds = folds
    elif not torch.is_tensor(ref_folds) or ref_folds.dim() != 1 or ref_folds.dtype not in integer:
        raise ValueError(f"{who}: ref_folds is an integer [R] tensor")
    dev = row_ptr.device
    if any(t.device != dev for t in (neighbour, folds, ref_folds)):
        raise ValueError(f"{who}: row_ptr, neighbour, folds and ref_folds lie on one device")
    n = folds.numel()
    row_ptr, nbr, folds, ref_folds = row_ptr.long(), neighbour.long(), folds.long(), ref_folds.long()
    lengths = row_ptr[1:] - row_ptr[:-1]
    bad_lists = n and (int(row_ptr[0]) != 0 or int(lengths.min()) < 0 or int(row_ptr[n]) != nbr.numel())
    if bad_lists or (n == 0 and nbr.numel()):
        raise ValueError(f"{who}: row_ptr is not the row pointers of neighbour [{nbr.numel()}]")
    if nbr.numel() and (int(nbr.min()) < 0 or int(nbr.max()) >= ref_folds.numel()):
        raise ValueError(f"{who}: neighbour names a reference outside [0, {ref_folds.numel()})")
    if (n and int(folds.min()) < 0) or (ref_folds.numel() and int(ref_folds.min()) < 0):
        raise ValueError(f"{who}: a fold is negative")
    F = int(max(folds.max() if n else 0, ref_folds.max() if ref_folds.numel() else 0)) + 1
    row = torch.repeat_interleave(torch.arange(n, device=dev), lengths)
    return torch.bincount(folds[row] * F + ref_folds[nbr], minlength=F * F).view(F, F)


# ------------------------------------------------------------------------------------- what each kernel learned --
# Every kernel of a ``KernelSetConv`` is a small learned neighbourhood pattern, and ``sim[n, c]`` -- the output of a convolution
# layer (``GNNModel.kernel_scores``) -- is how well kernel ``c`` matches the neighbourhood of atom ``n``.  The ``k`` atoms of a whole
# library that every kernel of a layer matches best are a picture book of those patterns; the same lists show the dead kernels (no
# atom scores high) and the duplicates.  One running list per kernel column, a candidate is an ATOM, and it competes only in the
# columns of its own degree: ``mkgnn_kernel_exemplars_update``.
#
# ``kernel_exemplars_reference``  the definition in numpy
# ``KernelExemplars``             the running lists on the device (``[n_columns, k]`` tensors, updated in place, capturable)
# ``kernel_exemplars``            shards -> the ``k`` best-matching atoms of every kernel of one layer
EXEMPLARS_MAX_K, EXEMPLARS_MAX_COLUMNS = 64, 256               # MKGNN_EXEMPLARS_MAX_K, MKGNN_EXEMPLARS_MAX_COLUMNS


def empty_exemplars(n_columns: int, k: int):
    """``n_columns`` lists of ``k`` empty slots: ``(top_score float32, top_shard int32, top_mol int32, top_atom int32)``, ``[n_columns,
    k]`` each; an empty slot is ``(-inf, -1, -1, -1)``."""
    shape = (int(n_columns), int(k))
    return (np.full(shape, -np.inf, dtype=np.float32), *(np.full(shape, -1, dtype=np.int32) for _ in range(3)))


def _host(a, dtype) -> np.ndarray:
    return np.asarray(a.detach().cpu().numpy() if torch.is_tensor(a) else a, dtype=dtype)


def _column_blocks(column_begin, num_kernels, n_columns: int):
    """``(begin[4], L[4])`` as ints; without ``num_kernels`` the blocks are contiguous: every degree's block ends where the next one
    begins, the last one at ``n_columns``."""
    begin = [int(b) for b in column_begin]
    if len(begin) != 4:
        raise ValueError("column_begin: one first column per degree (4)")
    L = [b - a for a, b in zip(begin, begin[1:] + [int(n_columns)])] if num_kernels is None else [int(x) for x in num_kernels]
    if len(L) != 4:
        raise ValueError("num_kernels: one count per degree (4)")
    return begin, L


def kernel_exemplars_reference(lists, sim, buckets, col_begin, L, atom_mol, mol_ptr, ids, n_live, n_valid_atoms, shard_tag):
    """The definition of ``mkgnn_kernel_exemplars_update`` (include/molkgnn_hip.h), on the host, written for clarity.  ``lists =
    (top_score, top_shard, top_mol, top_atom)``, ``[C, K]`` each -> the updated four arrays (copies).

    ``buckets[d]`` lists the atoms of degree ``d + 1`` (``selected_index``), in slot order.  Atom ``n`` of it is a candidate of the
    columns ``col_begin[d] .. col_begin[d] + L[d]`` -- and of no other -- if ``n < n_valid_atoms`` (None: every atom) and its
    molecule ``g = atom_mol[n]`` is live, ``g < min(max(n_live, 0), len(ids))``.  Its entry in column ``c`` is ``(sim[n, c], shard_tag,
    ids[g], n - mol_ptr[g])``; nothing else of ``sim`` is read.  List ``c`` becomes the first ``K``, sorted, of itself and its
    candidates:

    * occupied slots before empty ones (``(-inf, -1, -1, -1)``; a real entry whose score is ``-inf`` ranks before them),
    * non-NaN scores before NaN scores, then score descending with ``-0.0 == +0.0``,
    * then shard, molecule and atom ascending,
    * entries alike in all of that in their order of arrival: the old list first, then the bucket's slots (``np.lexsort`` is
      stable).

    Score BITS are carried over (a NaN's payload, a zero's sign)."""
    ts, th, tm, ta = (np.array(_host(a, dt), copy=True) for a, dt in zip(lists, (np.float32, np.int32, np.int32, np.int32)))
    if ts.ndim != 2 or not (ts.shape == th.shape == tm.shape == ta.shape):
        raise ValueError("lists: four [C, K] arrays")
    C, K = ts.shape
    sim = _host(sim, np.float32)
    atom_mol, mol_ptr, ids = _host(atom_mol, np.int64), _host(mol_ptr, np.int64), _host(ids, np.int32).reshape(-1)
    N = sim.shape[0]
    n_real = N if n_valid_atoms is None else int(_host(n_valid_atoms, np.int64).reshape(-1)[0])
    live = min(max(int(_host(n_live, np.int64).reshape(-1)[0]), 0), ids.shape[0])
    tag = int(_host(shard_tag, np.int64).reshape(-1)[0])
    neg_inf = np.float32(-np.inf).view(np.int32)
    for d in range(4):
        slots = _host(buckets[d], np.int64).reshape(-1)
        keep = np.array([n < n_real and atom_mol[n] < live for n in slots], dtype=bool)
        atoms = slots[keep]                                      # the candidates of this degree, in slot order
        g = atom_mol[atoms]
        mol, atom = ids[g].astype(np.int32), (atoms - mol_ptr[g]).astype(np.int32)
        for c in range(int(col_begin[d]), int(col_begin[d]) + int(L[d])):
            s = np.concatenate([ts[c], sim[atoms, c]])
            h = np.concatenate([th[c], np.full(atoms.shape[0], tag, dtype=np.int32)])
            m = np.concatenate([tm[c], mol])
            a = np.concatenate([ta[c], atom])
            empty = (s.view(np.int32) == neg_inf) & (h == -1) & (m == -1) & (a == -1)
            nan = np.isnan(s)
            with np.errstate(invalid="ignore"):
                falling = np.where(nan, np.float32(0), -(s + np.float32(0)))    # (-0.0 + 0.0 = +0.0; descending by negation)
            order = np.lexsort((a, m, h, falling, nan, empty))[:K]               # (the LAST key is the primary one)
            ts[c], th[c], tm[c], ta[c] = s[order], h[order], m[order], a[order]
    return ts, th, tm, ta


class KernelExemplars(TopK):
    """``n_columns`` running lists of ``k`` slots on ``device``, one per kernel column of a convolution layer: ``top_score`` float32,
    ``top_shard``, ``top_mol``, ``top_atom`` int32, ``[n_columns, k]`` each, list ``c`` always sorted by the order of
    ``kernel_exemplars_reference``.  ``TopK``'s contract otherwise: the live count (``self.n_valid``) and ``shard_tag`` are device
    int32 scalars read when the launches run, so one captured ``update`` serves every batch of every shard; ``reserve`` before a
    capture, nothing is allocated inside one."""

    def __init__(self, n_columns: int, k: int, device):
        from . import _lib
        self.n_columns = int(n_columns)
        if not 1 <= int(k) <= _lib.EXEMPLARS_MAX_K:
            raise ValueError(f"k = {k} outside [1, {_lib.EXEMPLARS_MAX_K}] (MKGNN_EXEMPLARS_MAX_K)")
        if not 1 <= self.n_columns <= _lib.EXEMPLARS_MAX_COLUMNS:
            raise ValueError(f"n_columns = {n_columns} outside [1, {_lib.EXEMPLARS_MAX_COLUMNS}] (MKGNN_EXEMPLARS_MAX_COLUMNS)")
        self.top_atom = None
        self._allocate(k, device, (self.n_columns, int(k)))

    def reset(self) -> None:
        """All slots empty."""
        super().reset()
        if self.top_atom is None:
            self.top_atom = torch.empty_like(self.top_mol)
        self.top_atom.fill_(-1)

    def _workspace_bytes(self, counts, num_kernels) -> int:
        from . import _lib
        return int(_lib.load().mkgnn_kernel_exemplars_workspace_bytes(_lib.Int64x4(*[int(c) for c in counts]),
                                                                      _lib.Int32x4(*[int(x) for x in num_kernels]), self.k, self.n_columns))

    def reserve(self, counts, num_kernels) -> None:
        """Make the workspace large enough for updates with ``counts[d]`` slots and ``num_kernels[d]`` columns per degree (before
        a capture: a captured update must not allocate)."""
        need = self._workspace_bytes(counts, num_kernels)
        if need == 0:
            raise ValueError(f"buckets of {list(counts)} slots with {list(num_kernels)} columns cannot be ranked")
        if self.workspace is None or self.workspace.numel() < need:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("KernelExemplars.update would allocate its workspace inside a capture: call reserve(counts, num_kernels) first")
            self.workspace = torch.empty(need, dtype=torch.uint8, device=self.device)

    def update(self, sim: torch.Tensor, plan_or_buckets, column_begin, atom_mol: torch.Tensor, mol_ptr: torch.Tensor,
               ids: torch.Tensor, n_live=None, n_valid_atoms: Optional[torch.Tensor] = None, shard_tag=None, num_kernels=None) -> None:
        """One ``mkgnn_kernel_exemplars_update`` on the current stream.  ``sim``: float32 ``[N, >= n_columns]`` with unit column
        stride (a layer's ``kernel_scores``; its row stride is passed on, nothing is copied).  ``plan_or_buckets``: a ``BatchPlan``,
        or the four ``selected_index`` tensors (int64, contiguous) of the batch.  ``column_begin``: the first column of every
        degree's block; the blocks are contiguous (the last one ends at ``n_columns``) unless ``num_kernels`` gives their widths.
        ``atom_mol`` int32 ``[N]``, ``mol_ptr`` int32 ``[len(ids) + 1]`` or longer, ``ids`` int32.  ``n_live`` / ``shard_tag``: as
        ``n_valid`` / ``shard_tag`` of ``TopK.update``; ``n_valid_atoms``: a one-element int64 device tensor, or None for every atom."""
        from . import _lib
        dev = self.device
        sels = [b.sel for b in plan_or_buckets.buckets] if hasattr(plan_or_buckets, "buckets") else list(plan_or_buckets)
        if len(sels) != 4 or any(s.dtype != torch.int64 or s.device != dev or not s.is_contiguous() for s in sels):
            raise ValueError("buckets: the four selected_index tensors of the batch, int64 and contiguous on the lists' device")
        if sim.dtype != torch.float32 or sim.device != dev or sim.dim() != 2 or sim.shape[1] < self.n_columns or sim.shape[0] < 1 \
                or sim.stride(1) != 1:
            raise ValueError(f"sim: float32 [N, >= {self.n_columns}] on the lists' device, unit column stride")
        N, B = int(sim.shape[0]), int(ids.numel())
        for name, t, n in (("atom_mol", atom_mol, N), ("mol_ptr", mol_ptr, B + 1), ("ids", ids, max(B, 1))):
            if t.dtype != torch.int32 or t.device != dev or not t.is_contiguous() or t.numel() < n:
                raise ValueError(f"{name}: a contiguous int32 tensor of at least {n} entries on the lists' device")
        if n_valid_atoms is not None and (not torch.is_tensor(n_valid_atoms) or n_valid_atoms.dtype != torch.int64
                                          or n_valid_atoms.numel() != 1 or n_valid_atoms.device != dev):
            raise ValueError("n_valid_atoms: one int64 on the lists' device, or None")
        begin, L = _column_blocks(column_begin, num_kernels, self.n_columns)
        live, tag = self._scalar(self.n_valid, n_live), self._scalar(self.shard_tag, shard_tag)
        counts = [int(s.numel()) for s in sels]
        self.reserve(counts, L)
        bk = _lib.Buckets4()
        for d, s in enumerate(sels):
            bk[d].count = counts[d]
            bk[d].selected_index = s.data_ptr() if counts[d] else None
        ws = self.workspace
        stride = int(sim.stride(0)) if N > 1 else max(int(sim.stride(0)), self.n_columns)     # (one row: its stride means nothing)
        with torch.cuda.device(dev):
            _lib.check(_lib.load().mkgnn_kernel_exemplars_update(
                sim.data_ptr(), stride, N, bk, _lib.Int32x4(*begin),
                _lib.Int32x4(*L), atom_mol.data_ptr(), mol_ptr.data_ptr(), ids.data_ptr(), B, live.data_ptr(),
                _lib.ptr(n_valid_atoms), tag.data_ptr(), self.k, self.n_columns, self.top_score.data_ptr(), self.top_shard.data_ptr(),
                self.top_mol.data_ptr(), self.top_atom.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_ptr(dev)),
                "mkgnn_kernel_exemplars_update")

    def result(self):
        """``(top_score, top_shard, top_mol, top_atom, occupied)``: the four ``[n_columns, k]`` tensors (not copies) and the number of
        occupied slots of every list -- they come first -- as a host int64 tensor ``[n_columns]`` (this synchronises)."""
        empty = (self.top_score == float("-inf")) & (self.top_shard == -1) & (self.top_mol == -1) & (self.top_atom == -1)
        return self.top_score, self.top_shard, self.top_mol, self.top_atom, (self.k - empty.sum(dim=1)).cpu()


class _ExemplarStep:
    """The captured step of ``kernel_exemplars``, a sibling of ``_ScoringStep`` with its batches (``ResidentLoader`` over every id,
    the short tail filled up) and its front -- ``gather`` -> ``expand`` -> ``attach_receptive_fields`` -- followed by
    ``model.kernel_scores(data, layer)`` and ONE ``lists.update``.  Per batch the feed row is the ids and the live count.  The model
    is in evaluation mode already."""

    def __init__(self, model, resident, batch_size: int, layer: int, lists: KernelExemplars, Ls):
        from .receptive_field import attach_receptive_fields
        from .shards import ResidentLoader
        dev = resident.device
        bs, n = int(batch_size), int(resident.n_molecules)
        self.loader = loader = ResidentLoader(resident, bs, np.arange(n, dtype=np.int64), dev, drop_last=False)
        plan, n_live = loader.plan(), loader.n_live
        rows = np.zeros((plan.shape[0], bs + 1), dtype=np.int32)
        rows[:, :bs] = plan
        rows[:, bs] = n_live
        self.rows = torch.from_numpy(rows).pin_memory().to(dev, non_blocking=True)
        self.feed = feed = torch.zeros(bs + 1, dtype=torch.int32, device=dev)
        f_ids, f_live = feed[:bs], feed[bs:bs + 1]
        self.csb = csb = static_batch_for(loader, resident)
        begin = [sum(Ls[:d]) for d in range(4)]
        lists.reserve(csb.data.bucket_sizes, Ls)

        def step(update: bool):
            csb.gather(resident, f_ids)
            csb.expand()
            attach_receptive_fields(csb.data, sizes=csb.data.bucket_sizes, overlap=True)
            data = csb.data
            sim = model.kernel_scores(data, layer)[0]
            if update:
                lists.update(sim, [getattr(data, f"selected_index_deg{d}") for d in range(1, 5)], begin, data.atom_mol, data.mol_ptr,
                             f_ids, f_live, data.n_valid_atoms, num_kernels=Ls)

        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            feed.copy_(self.rows[0], non_blocking=True)
            step(False)                                  # (eager once: lazily made buffers exist before the capture; no update)
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph, stream=side):
                step(True)
        torch.cuda.current_stream(dev).wait_stream(side)

    def __len__(self):
        return int(self.rows.shape[0])

    def run(self, b: int) -> None:
        """Batch ``b`` on the current stream: one small copy and the replay."""
        self.feed.copy_(self.rows[b], non_blocking=True)
        self.graph.replay()


def kernel_exemplars(model, residents, layer: int, k: int, batch_size: int) -> dict:
    """What each kernel of convolution layer ``layer`` (0: the 1-hop layer) learned: for every kernel column the ``k`` atoms of the
    whole library it matches best.  ``residents`` as in ``screen`` (a sequence of ``ResidentShard``s, or a generator that uploads
    them one at a time); shard ``j`` carries tag ``j``.  Any ``task_dim``: the head is not run.

    Per shard ONE graph is captured and replayed per batch -- ``score_resident``'s batches at this ``batch_size``, the short tail
    included: ``gather``, ``expand``, ``attach_receptive_fields``, ``model.kernel_scores(data, layer)`` and one
    ``KernelExemplars.update`` (``mkgnn_kernel_exemplars_update``: only real atoms of live molecules enter, each in the columns of its
    own degree).  Per batch the host enqueues one small copy and the replay; the gather's status word is read once per shard
    (non-zero raises).  The model is put in evaluation mode and handed back in the mode it came in.

    Returns ``top_score``, ``top_shard``, ``top_mol``, ``top_atom`` (``[K_layer, k]`` on the device, list ``c`` best first by the order
    of ``kernel_exemplars_reference``, its empty slots -- ``(-inf, -1, -1, -1)`` -- at the end), ``occupied`` (int64 ``[K_layer]``, on
    the host), ``column_degree`` and ``column_kernel`` (int32 ``[K_layer]``: column ``c`` is kernel ``column_kernel[c]`` of the bank of
    degree ``column_degree[c]``) and ``n_scored``, the number of molecules.  ``top_atom`` is the atom's index inside its molecule in
    the shard's atom order -- the index the rows of ``explain_resident``'s ``atom_ptr`` use.  A score is ``kernel_scores`` of the batch
    the pass holds the molecule in: re-running that batch gives its bits.

    ``k`` outside ``[1, 64]``, a layer with more than 256 kernels, ``layer`` outside ``[0, num_layers)``, a model or a shard that is
    not on the GPU, no shard: ``ValueError`` before a launch."""
    from .train import evaluation_mode
    who = "kernel_exemplars"
    k, layer, bs = int(k), int(layer), int(batch_size)
    if not 1 <= k <= EXEMPLARS_MAX_K:
        raise ValueError(f"{who}: k = {k} outside [1, {EXEMPLARS_MAX_K}] (MKGNN_EXEMPLARS_MAX_K)")
    net = model.gnn_model
    if not 0 <= layer < net.num_layers:
        raise ValueError(f"{who}: layer = {layer} outside [0, {net.num_layers})")
    Ls = [int(x) for x in net.gnn.layers[layer].L]
    K_layer = sum(Ls)
    if not 1 <= K_layer <= EXEMPLARS_MAX_COLUMNS:
        raise ValueError(f"{who}: layer {layer} has {K_layer} kernels, outside [1, {EXEMPLARS_MAX_COLUMNS}] (MKGNN_EXEMPLARS_MAX_COLUMNS)")
    if bs < 1:
        raise ValueError("batch_size >= 1")

    def per_shard(resident, lists, tag):
        lists.shard_tag.fill_(int(tag))
        with evaluation_mode(model):
            step = _ExemplarStep(model, resident, bs, layer, lists, Ls)
            for b in range(len(step)):
                step.run(b)
            status = step.csb.gather_status()            # (the one host read)
            if status:
                raise RuntimeError(f"mkgnn_gather_compact reported status {status} while scoring the shard's atoms")

    top_score, top_shard, top_mol, top_atom, occupied, n_scored, _ = _over_shards(
        who, residents, lambda r: _check_device(model, r), lambda dev: KernelExemplars(K_layer, k, dev), per_shard, False)
    column_degree, column_kernel = net.kernel_column_layout(layer, top_score.device)
    return {"top_score": top_score, "top_shard": top_shard, "top_mol": top_mol, "top_atom": top_atom, "occupied": occupied,
            "column_degree": column_degree, "column_kernel": column_kernel, "n_scored": n_scored}
