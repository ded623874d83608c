"""Evaluation metrics of the reference (``evaluation.py:11-127``) on torch tensors.

Same function names and return values as the reference's numpy / scikit-learn code, computed with torch sorts and
cumulative sums in float64 on whatever device the predictions live on (the validation set's scores never have to
leave the GPU).  ``roc_curve`` is restated with scikit-learn's semantics -- one threshold per distinct score, the
``drop_intermediate`` thinning of collinear points (which matters for logAUC: the trapezoids are taken in
log10(FPR)), the leading (0, 0) point -- and ``np.interp``'s convention for repeated abscissae.
Pinned by ``tests/golden/g8_metrics.npz`` (numbers produced by the reference's own functions).
"""
from __future__ import annotations

import math
from typing import Tuple

import torch


def _as_vectors(true_y, predicted_score) -> Tuple[torch.Tensor, torch.Tensor]:
    y = torch.as_tensor(true_y).reshape(-1)
    s = torch.as_tensor(predicted_score).reshape(-1).to(torch.float64)
    y = y.to(s.device)
    if y.numel() != s.numel():
        raise ValueError("true_y and predicted_score differ in length")
    return (y == 1).to(torch.float64), s


def roc_curve(true_y, predicted_score, drop_intermediate: bool = True) -> Tuple[torch.Tensor, torch.Tensor]:
    """(fpr, tpr) as ``sklearn.metrics.roc_curve(true_y, predicted_score, pos_label=1)`` returns them."""
    y, s = _as_vectors(true_y, predicted_score)
    order = torch.sort(s, descending=True, stable=True).indices
    s, y = s[order], y[order]
    n = s.numel()
    distinct = torch.nonzero(s[1:] != s[:-1]).reshape(-1)
    idx = torch.cat([distinct, torch.tensor([n - 1], device=s.device)])
    tps = torch.cumsum(y, 0)[idx]
    fps = 1.0 + idx.to(torch.float64) - tps
    if drop_intermediate and fps.numel() > 2:
        d2f = fps[2:] - 2 * fps[1:-1] + fps[:-2]
        d2t = tps[2:] - 2 * tps[1:-1] + tps[:-2]
        keep = torch.cat([torch.tensor([True], device=s.device), (d2f != 0) | (d2t != 0), torch.tensor([True], device=s.device)])
        fps, tps = fps[keep], tps[keep]
    zero = torch.zeros(1, dtype=torch.float64, device=s.device)
    fps, tps = torch.cat([zero, fps]), torch.cat([zero, tps])
    fpr = fps / fps[-1] if float(fps[-1]) > 0 else torch.full_like(fps, float("nan"))
    tpr = tps / tps[-1] if float(tps[-1]) > 0 else torch.full_like(tps, float("nan"))
    return fpr, tpr


def _interp(xq: torch.Tensor, xp: torch.Tensor, fp: torch.Tensor) -> torch.Tensor:
    """``np.interp`` for non-decreasing ``xp`` (a query equal to repeated abscissae takes the last of them)."""
    j = torch.searchsorted(xp, xq, right=True) - 1
    j = j.clamp(0, xp.numel() - 1)
    j1 = (j + 1).clamp(max=xp.numel() - 1)
    x0, x1, y0, y1 = xp[j], xp[j1], fp[j], fp[j1]
    w = torch.where(x1 > x0, (xq - x0) / (x1 - x0), torch.zeros_like(xq))
    out = y0 + w * (y1 - y0)
    out = torch.where(xq <= xp[0], fp[0].expand_as(out), out)
    out = torch.where(xq >= xp[-1], fp[-1].expand_as(out), out)
    return out


def _trapz(y: torch.Tensor, x: torch.Tensor) -> float:
    return float(((x[1:] - x[:-1]) * (y[1:] + y[:-1]) * 0.5).sum())


def calculate_logAUC(true_y, predicted_score, FPR_range=(0.001, 0.1)) -> float:
    """Area under the ROC curve over ``log10(FPR)`` in ``FPR_range``, normalised by the range (evaluation.py:11-79)."""
    if FPR_range is None:
        raise Exception('FPR range cannot be None')
    lower, upper = FPR_range
    if lower >= upper:
        raise Exception('FPR upper_bound must be greater than lower_bound')
    fpr, tpr = roc_curve(true_y, predicted_score)
    q = torch.tensor([lower, upper], dtype=torch.float64, device=fpr.device)
    tpr = torch.sort(torch.cat([tpr, _interp(q, fpr, tpr)])).values
    fpr = torch.sort(torch.cat([fpr, q])).values
    x = torch.log10(fpr)
    lo, hi = math.log10(lower), math.log10(upper)
    lo_t = torch.log10(torch.tensor(lower, dtype=torch.float64, device=fpr.device))
    hi_t = torch.log10(torch.tensor(upper, dtype=torch.float64, device=fpr.device))
    i0 = int(torch.nonzero(x == lo_t).reshape(-1)[-1])
    i1 = int(torch.nonzero(x == hi_t).reshape(-1)[-1])
    return _trapz(tpr[i0:i1 + 1], x[i0:i1 + 1]) / (hi - lo)


def calculate_auc(true_y, predicted_score) -> float:
    """``roc_auc_score``, or ``-1`` when it is undefined (reference ``evaluation.py:81-86``: ``try: roc_auc_score(...)
    except: -1``).  With only one class present the reference's pinned scikit-learn (``requirements.txt:101``: 1.0.2) raises
    ``ValueError`` and the caller gets ``-1``; the build container's scikit-learn 1.7 warns and returns NaN instead (which
    is what the golden file, generated here, holds) -- the pinned behaviour is the contract."""
    y, _ = _as_vectors(true_y, predicted_score)
    if float(y.sum()) == 0.0 or float(y.sum()) == float(y.numel()):
        return -1
    fpr, tpr = roc_curve(true_y, predicted_score)
    return _trapz(tpr, fpr)


def _confusion(true_y, predicted_score, cutoff: float):
    y, s = _as_vectors(true_y, predicted_score)
    pred = (torch.sigmoid(s) > cutoff).to(torch.float64)
    tp = float((pred * y).sum())
    fp = float((pred * (1 - y)).sum())
    fn = float(((1 - pred) * y).sum())
    tn = float(((1 - pred) * (1 - y)).sum())
    return tn, fp, fn, tp


def calculate_ppv(true_y, predicted_score, cutoff: float = 0.5) -> float:
    tn, fp, fn, tp = _confusion(true_y, predicted_score, cutoff)
    return tp / (tp + fp) if (tp + fp) != 0 else float("nan")


def calculate_accuracy(true_y, predicted_score) -> float:
    tn, fp, fn, tp = _confusion(true_y, predicted_score, 0.5)
    tot = tp + fp + tn + fn
    return (tp + tn) / tot if tot != 0 else float("nan")


def calculate_f1_score(true_y, predicted_score) -> float:
    tn, fp, fn, tp = _confusion(true_y, predicted_score, 0.5)
    den = 2 * tp + fp + fn
    return 2 * tp / den if den != 0 else 0.0


def calculate_rmse(true_y, predicted_score) -> float:
    """Root mean squared error of the docking-score task (reference ``model.py:504-507``:
    ``mean_squared_error(true_y, predicted_score, squared=False)``), in float64 on the predictions' device."""
    s = torch.as_tensor(predicted_score).reshape(-1).to(torch.float64)
    y = torch.as_tensor(true_y).reshape(-1).to(device=s.device, dtype=torch.float64)
    if y.numel() != s.numel():
        raise ValueError("true_y and predicted_score differ in length")
    if y.numel() == 0:
        raise ValueError("calculate_rmse needs at least one sample")
    return math.sqrt(float(((y - s) ** 2).mean()))


def per_task(true_y, pred_y, task, fn, num_tasks: int) -> list:
    """``fn(true_y[rows], pred_y[rows])`` for every task ``0 .. num_tasks - 1`` over the rows labelled with it (``task`` holds one
    task index per row; -1, or anything outside the range, is no label) -- a mixed-assay panel scored assay by assay with any
    metric of this module.  A task without a row gives ``nan``."""
    y = torch.as_tensor(true_y).reshape(-1)
    s = torch.as_tensor(pred_y).reshape(-1)
    t = torch.as_tensor(task).reshape(-1).to(s.device)
    if not (y.numel() == s.numel() == t.numel()):
        raise ValueError("true_y, pred_y and task differ in length")
    y = y.to(s.device)
    out = []
    for k in range(int(num_tasks)):
        rows = t == k
        out.append(fn(y[rows], s[rows]) if bool(rows.any()) else float("nan"))
    return out


# ---- bootstrap confidence intervals for AUC and logAUC ----
# A replicate resamples the rows with replacement; it is a vector of integer multiplicities over the rows sorted ONCE, and one
# ordered walk over the weighted curve.  bootstrap_reference is the definition in numpy; CUDA scores take mkgnn_bootstrap_roc
# (readout.bootstrap_roc), whose integers and AUC agree with it exactly and whose logAUC agrees within the rounding of a float64 sum.

BOOTSTRAP_MAX_ROWS = 1 << 22                     # (every count, and 2 T F, stay exactly representable)


def _philox_words(seed: int, offset: int, n: int):
    """``philox_word(seed, offset, i)`` of csrc/kgnn_philox.h for ``i = 0 .. n - 1`` (numpy uint64 holding 32-bit words): Philox4x32-10
    keyed by ``seed``, counter ``(i / 4, offset)``, word ``i % 4``."""
    import numpy as np
    u, lo, s32 = np.uint64, np.uint64(0xFFFFFFFF), np.uint64(32)
    blocks = np.arange((n + 3) // 4, dtype=np.uint64)
    c0, c1 = blocks & lo, blocks >> s32                           # (element >> 2, element >> 34)
    c2 = np.full_like(blocks, u(offset & 0xFFFFFFFF))
    c3 = np.full_like(blocks, u((offset >> 32) & 0xFFFFFFFF))
    k0, k1 = u(seed & 0xFFFFFFFF), u((seed >> 32) & 0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = u(0xD2511F53) * c0, u(0xCD9E8D57) * c2           # (< 2^64: no wrap)
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ k0, p1 & lo, (p0 >> s32) ^ c3 ^ k1, p0 & lo
        k0, k1 = (k0 + u(0x9E3779B9)) & lo, (k1 + u(0xBB67AE85)) & lo
    return np.stack([c0, c1, c2, c3], axis=1).reshape(-1)[:n]


def _check_fpr_range(FPR_range) -> Tuple[float, float]:
    if FPR_range is None or len(FPR_range) != 2:
        raise ValueError("FPR_range: a pair (lower, upper)")
    lower, upper = float(FPR_range[0]), float(FPR_range[1])
    if not (0.0 < lower < upper <= 1.0):
        raise ValueError(f"FPR_range = ({lower}, {upper}): 0 < lower < upper <= 1 is required")
    return lower, upper


def _check_bootstrap_sizes(n: int, n_boot: int, seed: int, offset: int) -> None:
    if not 1 <= n <= BOOTSTRAP_MAX_ROWS:
        raise ValueError(f"the bootstrap takes 1 .. {BOOTSTRAP_MAX_ROWS} rows, not {n}")
    if n_boot < 1:
        raise ValueError(f"n_boot = {n_boot}: at least one replicate")
    if not (0 <= seed < 1 << 64 and 0 <= offset and offset + n_boot <= 1 << 64):
        raise ValueError("seed and offset .. offset + n_boot - 1 are unsigned 64-bit values")


def bootstrap_draw(n: int, split: int, seed: int, offset: int):
    """The rows one replicate draws (numpy int64 ``[n]``): row ``i`` draws ``lo + ((uint64) philox_word(seed, offset, i) * size >> 32)``
    with ``(lo, size) = (0, split)`` for ``i < split`` and ``(split, n - split)`` otherwise -- a function of ``(seed, offset, i, n,
    split)`` alone."""
    import numpy as np
    w = _philox_words(seed, offset, n)
    i = np.arange(n)
    lo = np.where(i < split, 0, split).astype(np.uint64)
    size = np.where(i < split, split, n - split).astype(np.uint64)
    return (lo + ((w * size) >> np.uint64(32))).astype(np.int64)


def bootstrap_order(y_active, stratified: bool):
    """``(perm, split)``: the rows in the order the draw indexes them.  Unstratified: the caller's order, ``split = n``.  Stratified:
    actives first, then inactives, each in the caller's order (a stable partition; no sort), ``split`` the number of actives."""
    import numpy as np
    y_active = np.asarray(y_active, dtype=bool)
    n = y_active.size
    if not stratified:
        return np.arange(n), n
    return np.concatenate([np.nonzero(y_active)[0], np.nonzero(~y_active)[0]]), int(y_active.sum())


def _replicate_reference(c, y, gid, n_groups: int, lower: float, upper: float):
    """One replicate from its multiplicities ``c`` over the ranks (``y``: active by rank, ``gid``: tie group by rank):
    ``(auc, logauc, two_u, T)``."""
    import numpy as np
    gt = np.bincount(gid, weights=c * y, minlength=n_groups).astype(np.int64)
    gf = np.bincount(gid, weights=c * (1 - y), minlength=n_groups).astype(np.int64)
    exists = (gt + gf) > 0
    gt, gf = gt[exists], gf[exists]
    tps, fps = np.cumsum(gt), np.cumsum(gf)
    T, F = int(tps[-1]), int(fps[-1])
    two_u = int(np.sum(gf * (2 * (tps - gt) + gt)))
    if T == 0 or F == 0:
        return float("nan"), float("nan"), two_u, T
    auc = float(np.float64(two_u) / np.float64(2 * T * F))
    m = gt.size
    keep = np.ones(m, dtype=bool)
    if m > 2:                                                     # (an interior point stays iff its step differs from the NEXT one)
        keep[1:-1] = (gf[1:-1] != gf[2:]) | (gt[1:-1] != gt[2:])
    x = np.concatenate([[0], fps[keep]]).astype(np.float64) / np.float64(F)
    v = np.concatenate([[0], tps[keep]]).astype(np.float64) / np.float64(T)
    xa, xb, ya, yb = x[:-1], x[1:], v[:-1], v[1:]
    ca, cb = np.clip(xa, lower, upper), np.clip(xb, lower, upper)
    live = cb > ca                                                # (clip first, logarithm afterwards: log10(0) is never taken)
    xa, xb, ya, yb, ca, cb = xa[live], xb[live], ya[live], yb[live], ca[live], cb[live]
    slope = (yb - ya) / (xb - xa)                                 # np.interp's formula: slope * (x - xa) + ya
    yca = np.where(ca == xa, ya, slope * (ca - xa) + ya)
    ycb = np.where(cb == xb, yb, slope * (cb - xa) + ya)
    area = float(np.sum((np.log10(cb) - np.log10(ca)) * (yca + ycb) / 2.0))
    return auc, area / (math.log10(upper) - math.log10(lower)), two_u, T


def bootstrap_reference(true_y, predicted_score, n_boot: int, FPR_range=(0.001, 0.1), seed: int = 0, offset: int = 0,
                        stratified: bool = False) -> dict:
    """The definition of the bootstrap replicates, on the host in numpy: ``{'AUC': float64 [B], 'logAUC': float64 [B], 'two_u': int64
    [B], 'n_pos': int32 [B], 'n_undefined': int}``.

    A row is active iff ``true_y == 1``; a NaN or infinite score raises ``ValueError``.  Rows are taken in ``bootstrap_order``;
    replicate ``b`` draws with ``bootstrap_draw(n, split, seed, offset + b)`` (the call consumes ``offset .. offset + B - 1``).  Rows
    are ranked by score descending (stable); tie groups are the runs of equal score (``-0.0 == +0.0``).  Per tie group ``gt`` and
    ``gf`` are the drawn actives and inactives; groups with none do not exist in the replicate; the ROC points are the running sums
    ``(fps, tps)`` at the end of each remaining group; ``T``, ``F`` the totals (``n_pos = T``).  ``two_u = sum gf * (2 * tps_before +
    gt)`` and ``AUC = float64(two_u) / float64(2 T F)``.  logAUC: the points thinned as ``sklearn.roc_curve(drop_intermediate=True)``
    thins them, ``(0, 0)`` in front, every consecutive pair clipped to ``FPR_range`` in linear FPR (the TPR at a bound by
    ``np.interp``'s formula), ``(log10(b) - log10(a)) * (ya + yb) / 2`` summed and divided by the window's width.  With ``T == 0`` or
    ``F == 0`` both metrics of the replicate are NaN (not the reference's ``-1``: a replicate is not a caller) and it counts in
    ``n_undefined``."""
    import numpy as np
    lower, upper = _check_fpr_range(FPR_range)
    y_t, s_t = _as_vectors(true_y, predicted_score)
    y = y_t.detach().cpu().numpy() == 1.0
    s = s_t.detach().cpu().numpy()
    n, B, seed, offset = s.size, int(n_boot), int(seed), int(offset)
    _check_bootstrap_sizes(n, B, seed, offset)
    if not np.isfinite(s).all():
        raise ValueError("predicted_score holds a NaN or an infinite value")
    perm, split = bootstrap_order(y, stratified)
    y, s = y[perm], s[perm]
    order = np.argsort(-s, kind="stable")
    rank = np.empty(n, dtype=np.int64)
    rank[order] = np.arange(n)
    ss = s[order]
    group_last = np.concatenate([ss[1:] != ss[:-1], [True]])
    return bootstrap_reference_sorted(rank, y[order], group_last, split, B, seed, offset, lower, upper)


def bootstrap_reference_sorted(rank, y_sorted, group_last, split: int, n_boot: int, seed: int, offset: int, lower: float,
                               upper: float) -> dict:
    """``bootstrap_reference`` behind its sort -- the host form of ``readout.bootstrap_roc`` / ``mkgnn_bootstrap_roc``, with the same
    arguments as numpy arrays: ``rank [n]`` the rank of row ``i``, ``y_sorted [n]`` non-zero where the row at a rank is active,
    ``group_last [n]`` non-zero where a rank ends its tie group, ``split`` rows in front forming one stratum and the rest another."""
    import numpy as np
    rank = np.asarray(rank).astype(np.int64)
    ys = (np.asarray(y_sorted) != 0).astype(np.int64)
    last = np.asarray(group_last) != 0
    n, split, B = rank.size, int(split), int(n_boot)
    lower, upper = _check_fpr_range((lower, upper))
    _check_bootstrap_sizes(n, B, int(seed), int(offset))
    if not 0 <= split <= n:
        raise ValueError(f"split = {split} outside [0, {n}]")
    gid = np.concatenate([[0], np.cumsum(last[:-1])]).astype(np.int64)
    n_groups = int(gid[-1]) + 1
    out = {"AUC": np.empty(B), "logAUC": np.empty(B), "two_u": np.empty(B, dtype=np.int64), "n_pos": np.empty(B, dtype=np.int32)}
    for b in range(B):
        c = np.bincount(rank[bootstrap_draw(n, split, int(seed), int(offset) + b)], minlength=n).astype(np.int64)
        out["AUC"][b], out["logAUC"][b], out["two_u"][b], out["n_pos"][b] = _replicate_reference(c, ys, gid, n_groups, lower, upper)
    out["n_undefined"] = int(np.isnan(out["AUC"]).sum())
    return out


def _bootstrap_replicates(true_y, predicted_score, n_boot: int, FPR_range, seed: int, offset: int, stratified: bool):
    """``(auc, logauc, two_u, n_pos)`` tensors ``[n_boot]`` on the scores' device: CUDA scores through one stable sort and
    ``readout.bootstrap_roc`` (at most ``BOOTSTRAP_MAX_REPLICATES`` per launch sequence), CPU scores through ``bootstrap_reference``."""
    lower, upper = _check_fpr_range(FPR_range)
    y, s = _as_vectors(true_y, predicted_score)
    y, s = y.detach(), s.detach()
    n, B, seed, offset = s.numel(), int(n_boot), int(seed), int(offset)
    _check_bootstrap_sizes(n, B, seed, offset)
    if not bool(torch.isfinite(s).all()):
        raise ValueError("predicted_score holds a NaN or an infinite value")
    if not s.is_cuda:
        ref = bootstrap_reference(y, s, B, (lower, upper), seed, offset, stratified)
        return (torch.from_numpy(ref["AUC"]), torch.from_numpy(ref["logAUC"]), torch.from_numpy(ref["two_u"]),
                torch.from_numpy(ref["n_pos"]))
    from . import _lib, readout
    rank, y_sorted, group_last, split = bootstrap_prepare(y == 1.0, s, stratified)
    parts = []
    for b0 in range(0, B, _lib.BOOTSTRAP_MAX_REPLICATES):
        nb = min(_lib.BOOTSTRAP_MAX_REPLICATES, B - b0)
        parts.append(readout.bootstrap_roc(rank, y_sorted, group_last, split, nb, seed, offset + b0, lower, upper))
    return tuple(torch.cat([p[k] for p in parts]) if len(parts) > 1 else parts[0][k] for k in range(4))


def bootstrap_prepare(y_active: torch.Tensor, score: torch.Tensor, stratified: bool = False):
    """``(rank int32 [n], y_sorted uint8 [n], group_last uint8 [n], split)`` for ``readout.bootstrap_roc`` from a boolean ``y_active``
    and finite float64 ``score`` on one device, with torch operators: the stable partition of a stratified bootstrap by two running
    counts, ONE stable sort of the scores, nothing else sorts.  ``split`` is given as a Python int only when it has to be read back
    (stratified); unstratified it is ``n``."""
    n, dev = score.numel(), score.device
    if stratified:
        split = int(y_active.sum())
        act = y_active.to(torch.int64)
        dest = torch.where(y_active, torch.cumsum(act, 0) - 1, split + torch.cumsum(1 - act, 0) - 1)
        perm = torch.empty(n, dtype=torch.int64, device=dev)
        perm[dest] = torch.arange(n, device=dev)
        y_active, score = y_active[perm], score[perm]
    else:
        split = n
    ordered = torch.sort(score, descending=True, stable=True)
    rank = torch.empty(n, dtype=torch.int32, device=dev)
    rank[ordered.indices] = torch.arange(n, dtype=torch.int32, device=dev)
    y_sorted = y_active[ordered.indices].to(torch.uint8)
    group_last = torch.ones(n, dtype=torch.uint8, device=dev)
    group_last[:-1] = (ordered.values[1:] != ordered.values[:-1]).to(torch.uint8)
    return rank, y_sorted, group_last, split


def _interval(values: torch.Tensor, confidence: float) -> dict:
    """``mean``, ``std`` (unbiased) and ``ci`` of the defined (not NaN) entries of ``values``; the interval's ends are the ``(1 -
    confidence) / 2`` and ``1 - (1 - confidence) / 2`` quantiles by ``torch.nanquantile``'s linear rule."""
    alpha = (1.0 - float(confidence)) / 2.0
    defined = values[~torch.isnan(values)]
    if defined.numel() == 0:
        nan = float("nan")
        return {"mean": nan, "std": nan, "ci": (nan, nan)}
    q = torch.nanquantile(values, torch.tensor([alpha, 1.0 - alpha], dtype=values.dtype, device=values.device))
    return {"mean": float(defined.mean()), "std": float(defined.std(unbiased=True)) if defined.numel() > 1 else float("nan"),
            "ci": (float(q[0]), float(q[1]))}


def _check_confidence(confidence: float) -> None:
    if not 0.0 < float(confidence) < 1.0:
        raise ValueError(f"confidence = {confidence} outside (0, 1)")


def _check_two_classes(true_y, predicted_score) -> None:
    y, _ = _as_vectors(true_y, predicted_score)
    if y.numel() == 0 or float(y.sum()) == 0.0 or float(y.sum()) == float(y.numel()):
        raise ValueError("the bootstrap needs both classes in true_y")


def bootstrap_metrics(true_y, predicted_score, n_boot: int = 1000, FPR_range=(0.001, 0.1), confidence: float = 0.95,
                      seed: int = 0, offset: int = 0, stratified: bool = False) -> dict:
    """Non-parametric bootstrap of AUC and ``logAUC_{FPR_range}``: ``point`` (the existing functions on the full data), ``replicates``
    (``{'AUC': [B], 'logAUC': [B]}`` on the scores' device; NaN where a resample holds one class only), per metric ``mean``, ``std``
    (unbiased) and the percentile interval ``ci`` over the defined replicates, ``n_undefined``, ``n_pos`` (the actives of each
    replicate, int32 ``[B]``) and the ``seed``, ``offset`` and ``n_boot`` used (the call consumes ``offset .. offset + n_boot - 1``).
    CUDA scores are evaluated by ``mkgnn_bootstrap_roc`` behind one sort, CPU scores by ``bootstrap_reference``; the resamples are
    the same either way.  ``stratified`` resamples actives and inactives separately.  Only one class in the full data raises
    ``ValueError``."""
    _check_confidence(confidence)
    _check_fpr_range(FPR_range)
    _check_two_classes(true_y, predicted_score)
    auc, logauc, _, n_pos = _bootstrap_replicates(true_y, predicted_score, n_boot, FPR_range, seed, offset, stratified)
    out = {"point": {"AUC": calculate_auc(true_y, predicted_score), "logAUC": calculate_logAUC(true_y, predicted_score, FPR_range)},
           "replicates": {"AUC": auc, "logAUC": logauc}, "AUC": _interval(auc, confidence), "logAUC": _interval(logauc, confidence),
           "n_undefined": int(torch.isnan(auc).sum()), "n_pos": n_pos, "seed": int(seed), "offset": int(offset),
           "n_boot": int(n_boot), "confidence": float(confidence), "FPR_range": tuple(float(v) for v in FPR_range),
           "stratified": bool(stratified)}
    return out


def bootstrap_compare(true_y, score_a, score_b, n_boot: int = 1000, FPR_range=(0.001, 0.1), confidence: float = 0.95, seed: int = 0,
                      offset: int = 0, stratified: bool = False) -> dict:
    """The paired bootstrap of two score vectors on the same labels: both see the SAME resamples (a draw depends on ``(seed, offset +
    b, i, n, split)`` alone).  Per metric: ``diff`` (the replicate differences ``a - b``, ``[B]``), their ``mean``, ``std`` and
    ``ci``, and ``p_a_better``, the share of defined replicates with a positive difference; also ``point`` (``a``, ``b`` and ``diff`` on
    the full data), ``n_undefined`` and the ``seed``, ``offset`` and ``n_boot`` used."""
    _check_confidence(confidence)
    _check_fpr_range(FPR_range)
    _check_two_classes(true_y, score_a)
    a = _bootstrap_replicates(true_y, score_a, n_boot, FPR_range, seed, offset, stratified)
    b = _bootstrap_replicates(true_y, score_b, n_boot, FPR_range, seed, offset, stratified)
    if not torch.equal(a[3].cpu(), b[3].cpu()):
        raise RuntimeError("bootstrap_compare: the two score vectors saw different resamples")
    point_a = {"AUC": calculate_auc(true_y, score_a), "logAUC": calculate_logAUC(true_y, score_a, FPR_range)}
    point_b = {"AUC": calculate_auc(true_y, score_b), "logAUC": calculate_logAUC(true_y, score_b, FPR_range)}
    out = {"point": {"a": point_a, "b": point_b, "diff": {k: point_a[k] - point_b[k] for k in point_a}},
           "n_undefined": int(torch.isnan(a[0]).sum()), "seed": int(seed), "offset": int(offset), "n_boot": int(n_boot)}
    for name, k in (("AUC", 0), ("logAUC", 1)):
        diff = a[k] - b[k].to(a[k].device)
        defined = diff[~torch.isnan(diff)]
        entry = _interval(diff, confidence)
        entry["diff"] = diff
        entry["p_a_better"] = float((defined > 0).double().mean()) if defined.numel() else float("nan")
        out[name] = entry
    return out


def bootstrap_per_task(true_y, pred_y, task, num_tasks: int, n_boot: int = 1000, FPR_range=(0.001, 0.1), confidence: float = 0.95,
                       seed: int = 0, offset: int = 0, stratified: bool = False) -> list:
    """``bootstrap_metrics`` over each task's labelled rows, as ``per_task`` selects them; task ``t`` uses the offsets ``offset + t *
    n_boot .. offset + (t + 1) * n_boot - 1``.  A task without a row, or with one class only, gives ``None``."""
    y = torch.as_tensor(true_y).reshape(-1)
    s = torch.as_tensor(pred_y).reshape(-1)
    t = torch.as_tensor(task).reshape(-1).to(s.device)
    if not (y.numel() == s.numel() == t.numel()):
        raise ValueError("true_y, pred_y and task differ in length")
    y = y.to(s.device)
    out = []
    for k in range(int(num_tasks)):
        rows = t == k
        yk = y[rows]
        active = int((yk == 1).sum())
        if yk.numel() == 0 or active == 0 or active == yk.numel():
            out.append(None)
            continue
        out.append(bootstrap_metrics(yk, s[rows], n_boot, FPR_range, confidence, seed, int(offset) + k * int(n_boot), stratified))
    return out
