"""Screening a compound library that lives in device memory: score every molecule of a ``shards.ResidentShard`` (the short tail
included) from ONE captured graph per shard, and keep the best ``k`` of all shards in a running list on the device.

``topk_update_reference``  the order of the ranking, in numpy: the specification ``mkgnn_topk_update`` is tested against
``TopK``                   the running list on the device (``mkgnn_topk_update``: sorted, updated in place, capturable)
``score_resident``         ``scores[n_molecules]`` of one resident shard, optionally feeding a ``TopK``
``screen``                 a sequence (or a generator) of resident shards -> the top ``k`` of all of them
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


class TopK:
    """The running top ``k`` of a screen on ``device``: three tensors ``top_score`` float32, ``top_shard`` int32, ``top_mol``
    int32 of length ``k``, always sorted by the order of ``topk_update_reference``; the kernels' workspace; and the two device
    int32 scalars every update reads ON THE DEVICE -- ``n_valid`` (how many leading slots of the batch count) and
    ``shard_tag`` (the shard the batch's molecule ids belong to) -- so that one captured ``update`` serves every batch of every
    shard: refill the scalars (and the inputs) between replays."""

    def __init__(self, k: int, device):
        from . import _lib
        self.k, self.device = int(k), torch.device(device)
        if not 1 <= self.k <= _lib.TOPK_MAX_K:
            raise ValueError(f"k = {k} outside [1, {_lib.TOPK_MAX_K}] (MKGNN_TOPK_MAX_K)")
        if self.device.type != "cuda":
            raise ValueError("TopK lives on the GPU (topk_update_reference is the host form)")
        _lib.load()
        dev = self.device
        self.top_score = torch.empty(self.k, dtype=torch.float32, device=dev)
        self.top_shard = torch.empty(self.k, dtype=torch.int32, device=dev)
        self.top_mol = torch.empty(self.k, dtype=torch.int32, device=dev)
        self.n_valid = torch.zeros(1, dtype=torch.int32, device=dev)
        self.shard_tag = torch.zeros(1, dtype=torch.int32, device=dev)
        self.workspace = None
        self.reset()

    def reset(self) -> None:
        """All slots empty."""
        self.top_score.fill_(float("-inf"))
        self.top_shard.fill_(-1)
        self.top_mol.fill_(-1)

    def reserve(self, batch: int) -> None:
        """Make the workspace large enough for updates of ``batch`` slots (before a capture: a captured update must not allocate)."""
        from . import _lib
        need = int(_lib.load().mkgnn_topk_workspace_bytes(int(batch), self.k))
        if need == 0:
            raise ValueError(f"a batch of {batch} slots cannot be ranked")
        if self.workspace is None or self.workspace.numel() < need:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("TopK.update would allocate its workspace inside a capture: call reserve(batch) first")
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


def _check_model(model, resident) -> torch.device:
    if getattr(getattr(model, "ffn", None), "out_features", None) != 1:
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
    view); ``score_resident`` passes ``TopK.update``, tools/screen_timing.py other formulations.  The model is in evaluation
    mode already."""

    def __init__(self, model, resident, batch_size: int, rank=None):
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
        self.ext = ext = torch.full((n + 1,), float("nan"), dtype=torch.float32, device=dev)
        self.n = n

        def step(ranked: bool):
            csb.gather(resident, f_ids)
            csb.expand()
            attach_receptive_fields(csb.data, sizes=csb.data.bucket_sizes, overlap=True)
            pred, _ = model.predict(csb.data)
            pred = pred.reshape(-1)
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
    bs, n = int(batch_size), int(resident.n_molecules)
    if bs < 1:
        raise ValueError("batch_size >= 1")
    if topk is not None and topk.device != dev:
        raise ValueError(f"the running list is on {topk.device}, the model on {dev}")
    if out is not None and (out.dtype != torch.float32 or out.device != dev or out.shape != (n,) or not out.is_contiguous()):
        raise ValueError(f"out: a contiguous float32 vector of {n} entries on {dev}")
    was_training = model.training
    model.eval()
    try:
        rank = None
        if topk is not None:
            topk.reserve(bs)
            topk.shard_tag.fill_(int(shard_tag))
            rank = lambda pred, ids, n_live: topk.update(pred, ids, n_valid=n_live)     # noqa: E731
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
