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

    def update(self, scores: torch.Tensor, ids: torch.Tensor, n_valid=None, shard_tag=None) -> None:
        """One ``mkgnn_topk_update`` on the current stream: the list becomes the best ``k`` of itself and the first ``n_valid``
        entries ``(scores[i], shard_tag, ids[i])``.  ``n_valid`` / ``shard_tag``: None -- what ``self.n_valid`` /
        ``self.shard_tag`` hold when the launch RUNS; an int -- written into them first; a one-element device int32 tensor --
        read in their place (by address: a captured update follows its contents)."""
        from . import _lib
        dev = self.device
        if scores.dtype != torch.float32 or ids.dtype != torch.int32 or scores.device != dev or ids.device != dev:
            raise ValueError("scores float32 and ids int32 on the list's device")
        if not scores.is_contiguous() or not ids.is_contiguous() or scores.numel() != ids.numel():
            raise ValueError("scores and ids: contiguous, one id per score")
        B = scores.numel()
        if B < 1:
            raise ValueError("an update needs at least one slot")
        nv, tag = self._scalar(self.n_valid, n_valid), self._scalar(self.shard_tag, shard_tag)
        self.reserve(B)
        ws = self.workspace
        with torch.cuda.device(dev):
            _lib.check(_lib.load().mkgnn_topk_update(scores.data_ptr(), ids.data_ptr(), B, nv.data_ptr(), tag.data_ptr(), self.k,
                                                     self.top_score.data_ptr(), self.top_shard.data_ptr(), self.top_mol.data_ptr(),
                                                     ws.data_ptr(), ws.numel() * ws.element_size(), _lib.stream_ptr(dev)),
                       "mkgnn_topk_update")

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
        dev, T = self.device, self.n_tasks
        if scores.dtype != torch.float32 or ids.dtype != torch.int32 or scores.device != dev or ids.device != dev:
            raise ValueError("scores float32 and ids int32 on the lists' device")
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
        nv, tag = self._scalar(self.n_valid, n_valid), self._scalar(self.shard_tag, shard_tag)
        self.reserve(B)
        ws = self.workspace
        with torch.cuda.device(dev):
            _lib.check(_lib.load().mkgnn_topk_update_tasks(
                scores.data_ptr(), rs, ts, ids.data_ptr(), B, T, nv.data_ptr(), tag.data_ptr(), self.k, self.top_score.data_ptr(),
                self.top_shard.data_ptr(), self.top_mol.data_ptr(), ws.data_ptr(), ws.numel() * ws.element_size(),
                _lib.stream_ptr(dev)), "mkgnn_topk_update_tasks")

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
    """The captured step of ``score_resident``: static buffers, the per-batch feed rows and ONE graph over ``gather`` ->
    ``expand`` -> ``attach_receptive_fields`` -> ``model.predict`` -> scatter of the live slots -> ``rank``.  ``rank(pred, ids,
    n_live)`` is called inside the capture with the batch's scores, its id view and its live count (a one-element device int32
    view); ``score_resident`` passes ``TopK.update``, tools/screen_timing.py other formulations.  ``predict(data)`` gives the
    batch's scores -- one row per slot -- and ``width`` their number per molecule: None (``score_resident``) is ``model.predict`` as a
    vector and a score vector ``ext [n + 1]``; ``score_resident_tasks`` passes ``model.predict_tasks`` and ``T``: ``ext [n + 1, T]``.
    The model is in evaluation mode already."""

    def __init__(self, model, resident, batch_size: int, rank=None, predict=None, width: Optional[int] = None):
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
        self.ext = ext = torch.full((n + 1,) if width is None else (n + 1, int(width)), float("nan"), dtype=torch.float32, device=dev)
        self.n = n
        if predict is None:
            predict = lambda data: model.predict(data)[0].reshape(-1)     # noqa: E731

        def step(ranked: bool):
            csb.gather(resident, f_ids)
            csb.expand()
            attach_receptive_fields(csb.data, sizes=csb.data.bucket_sizes, overlap=True)
            pred = predict(csb.data)
            ext.index_copy_(0, f_index, pred)
            if ranked and rank is not None:
                rank(pred, f_ids, f_live)

        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            feed.copy_(self.rows[0], non_blocking=True)
            step(False)                                  # (eager once: lazily made buffers exist before the capture; no ranking)
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


def _score_shard(who: str, model, resident, batch_size: int, topk, shard_tag: int, out, tasks: bool) -> torch.Tensor:
    """The body of ``score_resident`` (``tasks`` False: one score per molecule) and ``score_resident_tasks`` (all ``T`` outputs)."""
    dev = _check_model(model, resident, tasks)
    bs, n = int(batch_size), int(resident.n_molecules)
    T = int(model.ffn.out_features)
    shape = (n, T) if tasks else (n,)
    if bs < 1:
        raise ValueError("batch_size >= 1")
    if topk is not None and (isinstance(topk, TopKTasks) != tasks or (tasks and topk.n_tasks != T)):
        raise ValueError(f"{who}: the running list must be a " + (f"TopKTasks of {T} tasks" if tasks else "TopK"))
    if topk is not None and topk.device != dev:
        raise ValueError(f"the running list is on {topk.device}, the model on {dev}")
    if out is not None and (out.dtype != torch.float32 or out.device != dev or tuple(out.shape) != shape or not out.is_contiguous()):
        raise ValueError(f"out: a contiguous float32 tensor of shape {shape} on {dev}")
    was_training = model.training
    model.eval()
    try:
        rank = None
        if topk is not None:
            topk.reserve(bs)
            topk.shard_tag.fill_(int(shard_tag))
            rank = lambda pred, ids, n_live: topk.update(pred, ids, n_valid=n_live)     # noqa: E731
        if tasks:
            scoring = _ScoringStep(model, resident, bs, rank, predict=lambda data: model.predict_tasks(data)[0], width=T)
        else:
            scoring = _ScoringStep(model, resident, bs, rank)
        for b in range(len(scoring)):
            scoring.run(b)
        if out is None:
            out = scoring.ext[:n]
        else:
            out.copy_(scoring.ext[:n])
        status = scoring.csb.gather_status()             # (the one host read)
        if status:
            raise RuntimeError(f"mkgnn_gather_compact reported status {status} while scoring the shard")
        return out
    finally:
        model.train(was_training)


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
    return _score_shard("score_resident", model, resident, batch_size, topk, shard_tag, out, False)


def score_resident_tasks(model, resident, batch_size: int, *, topk: Optional[TopKTasks] = None, shard_tag: int = 0,
                         out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``scores[n_molecules, T]`` (float32, on the device): ``model.predict_tasks`` of every molecule of the ``ResidentShard`` -- all
    ``T`` outputs of a multi-task model from ONE run of the network per molecule -- in id order, the short tail included, as
    ``score_resident`` does it: one captured graph per call, replayed per batch, in which the model's scoring is ``predict_tasks``
    (the forward-only tail for the embedding, ``mkgnn_task_scores`` for the ``T`` logits) and ``topk.update`` is ONE
    ``mkgnn_topk_update_tasks`` that feeds every batch's live rows to all ``T`` lists of a ``TopKTasks`` under ``shard_tag``.  ``out``
    (``[n_molecules, T]``, contiguous) is filled with NaN first.  The model needs ``1 <= T <= 32`` outputs and must be on the
    shard's GPU: anything else raises ``ValueError`` before a launch.  It comes back in the mode it came in."""
    return _score_shard("score_resident_tasks", model, resident, batch_size, topk, shard_tag, out, True)


def screen(model, residents, k: int, batch_size: int, return_scores: bool = False) -> dict:
    """Rank a library: ``residents`` is a sequence of ``ResidentShard``s, or a generator that uploads them one at a time (a
    library larger than device memory); shard ``j`` carries tag ``j``.  One ``TopK`` of ``k`` slots is carried across the
    shards on the device.  Returns ``top_score``, ``top_shard``, ``top_mol`` (trimmed to the occupied slots, best first) and
    ``n_scored``; with ``return_scores`` also ``scores``, the per-shard score vectors."""
    topk, n_scored, kept = None, 0, []
    for tag, resident in enumerate(residents):
        dev = _check_model(model, resident)
        if topk is None:
            topk = TopK(k, dev)
        scores = score_resident(model, resident, batch_size, topk=topk, shard_tag=tag)
        n_scored += int(resident.n_molecules)
        if return_scores:
            kept.append(scores)
    if topk is None:
        raise ValueError("screen needs at least one shard")
    top_score, top_shard, top_mol, occupied = topk.result()
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
    topk, n_scored, kept = None, 0, []
    for tag, resident in enumerate(residents):
        dev = _check_model(model, resident, tasks=True)
        if topk is None:
            topk = TopKTasks(k, int(model.ffn.out_features), dev)
        scores = score_resident_tasks(model, resident, batch_size, topk=topk, shard_tag=tag)
        n_scored += int(resident.n_molecules)
        if return_scores:
            kept.append(scores)
    if topk is None:
        raise ValueError("screen_tasks needs at least one shard")
    top_score, top_shard, top_mol, occupied = topk.result()
    result = {"top_score": top_score, "top_shard": top_shard, "top_mol": top_mol, "n_occupied": occupied, "n_scored": n_scored}
    if return_scores:
        result["scores"] = kept
    return result
