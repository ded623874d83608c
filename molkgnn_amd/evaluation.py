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
    lower, upper = _check_fpr_range(FPR_range)
    rank, y_sorted, group_last, split = _reference_sorted_inputs(true_y, predicted_score, n_boot, seed, offset, stratified)
    return bootstrap_reference_sorted(rank, y_sorted, group_last, split, int(n_boot), int(seed), int(offset), lower, upper)


def _reference_sorted_inputs(true_y, predicted_score, n_boot, seed, offset, stratified: bool):
    """``(rank, y_sorted, group_last, split)`` of ``bootstrap_reference`` and ``early_reference`` in numpy: the rows in
    ``bootstrap_order``, ranked by score descending (stable), tie groups the runs of equal score; sizes and non-finite scores are
    refused here."""
    import numpy as np
    y_t, s_t = _as_vectors(true_y, predicted_score)
    y = y_t.detach().cpu().numpy() == 1.0
    s = s_t.detach().cpu().numpy()
    n = s.size
    _check_bootstrap_sizes(n, int(n_boot), int(seed), int(offset))
    if not np.isfinite(s).all():
        raise ValueError("predicted_score holds a NaN or an infinite value")
    perm, split = bootstrap_order(y, stratified)
    y, s = y[perm], s[perm]
    order = np.argsort(-s, kind="stable")
    rank = np.empty(n, dtype=np.int64)
    rank[order] = np.arange(n)
    ss = s[order]
    group_last = np.concatenate([ss[1:] != ss[:-1], [True]])
    return rank, y[order], group_last, split


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


# ---- early recognition: average precision, enrichment factor, BEDROC ----
# Three functionals of the curve the bootstrap already walks.  Per replicate the raw sums ap, hits[j] and rie[a] are formed from the
# tie groups (early_reference is the definition; mkgnn_bootstrap_early forms them in the ROC walk); early_derived turns them, the
# actives T and the rows N into the metrics on either route.

BOOTSTRAP_MAX_CUTS, BOOTSTRAP_MAX_ALPHAS = 8, 4  # (MKGNN_BOOTSTRAP_MAX_CUTS, MKGNN_BOOTSTRAP_MAX_ALPHAS)
EARLY_MAX_ALPHA = 500.0                          # (exp(alpha) and sinh(alpha / 2) stay finite in float64)


def early_cut(fraction: float, n: int) -> int:
    """The number of top-ranked rows an enrichment factor at ``fraction`` looks at: ``max(1, min(n, ceil(fraction * n)))``."""
    return max(1, min(int(n), math.ceil(_check_fraction(fraction) * int(n))))


def _check_fraction(fraction: float) -> float:
    fraction = float(fraction)
    if not 0.0 < fraction <= 1.0:
        raise ValueError(f"enrichment fraction {fraction} outside (0, 1]")
    return fraction


def _check_alpha(alpha: float) -> float:
    alpha = float(alpha)
    if not 0.0 < alpha <= EARLY_MAX_ALPHA:
        raise ValueError(f"BEDROC alpha {alpha} outside (0, {EARLY_MAX_ALPHA:g}]")
    return alpha


def _replicate_early(c, y, gid, n_groups: int, cuts, alphas):
    """One replicate from its multiplicities ``c`` over the ranks: ``(ap, hits [J], rie [A], T)``."""
    import numpy as np
    n = c.size
    gt = np.bincount(gid, weights=c * y, minlength=n_groups).astype(np.int64)
    gf = np.bincount(gid, weights=c * (1 - y), minlength=n_groups).astype(np.int64)
    exists = (gt + gf) > 0
    gt, sg = gt[exists], (gt + gf)[exists]
    end, tps = np.cumsum(sg), np.cumsum(gt)
    before = end - sg
    T, N = int(tps[-1]), int(end[-1])
    pos = gt > 0
    ap = float(np.sum((gt[pos] / np.float64(T)) * (tps[pos] / end[pos].astype(np.float64)))) if T > 0 else 0.0
    hits = np.full(len(cuts), np.nan)
    for j, k in enumerate(cuts):
        k = int(k)
        if not 1 <= k <= n:
            continue
        if k > N:
            hits[j] = np.float64(T)
            continue
        g = int(np.searchsorted(end, k, side="left"))             # (before[g] < k <= end[g])
        hits[j] = np.float64(tps[g] - gt[g]) + np.float64(gt[g]) * np.float64(k - before[g]) / np.float64(sg[g])
    rie = np.full(len(alphas), np.nan)
    for a, alpha in enumerate(alphas):
        alpha = float(alpha)
        if not 0.0 < alpha <= EARLY_MAX_ALPHA:                    # (a NaN fails both)
            continue
        den = -np.expm1(-alpha / N)
        rie[a] = float(np.sum(gt[pos] * np.exp(-(alpha * (before[pos] + 1)) / N) * (-np.expm1(-(alpha * sg[pos]) / N)) / den / sg[pos]))
    return ap, hits, rie, T


def early_reference_sorted(rank, y_sorted, group_last, split: int, n_boot: int, seed: int, offset: int, cuts, alphas) -> dict:
    """The definition of the early-recognition sums behind the sort -- the host form of ``readout.bootstrap_early`` /
    ``mkgnn_bootstrap_early``, with ``bootstrap_reference_sorted``'s arguments, draw, order and tie groups: ``{'ap': float64 [B], 'hits':
    float64 [B, J], 'rie': float64 [B, A], 'n_pos': int32 [B], 'n_undefined': int}``.

    Per replicate, ``c`` the multiplicities over the ranks and the groups the tie groups with a drawn row: group ``g`` has ``gt`` drawn
    actives, ``gf`` drawn inactives, ``sg = gt + gf`` rows, ``P_g`` drawn rows in front of it and ``tps_g`` actives up to and including
    it; ``T`` and ``F`` are the totals and ``N = T + F``.  In exactly this order of operations:

    ``ap = sum_{g: gt > 0} (gt / float64(T)) * (tps_g / float64(P_g + sg))`` -- ``sklearn.metrics.average_precision_score`` with the
    multiplicities as sample weights (a group without a drawn active adds an exact zero; without any active the sum is empty, 0).

    ``hits[j]`` for a cut ``1 <= k_j <= n``: the expected number of actives among the first ``k_j`` drawn rows when a tie group's rows
    are in random order -- ``float64(tps_g - gt) + float64(gt) * float64(k_j - P_g) / float64(sg)`` for the one group with ``P_g < k_j
    <= P_g + sg``, and ``float64(T)`` for ``k_j > N``.

    ``rie[a] = sum_{g: gt > 0} gt * exp(-(alpha * (P_g + 1)) / N) * (-expm1(-(alpha * sg) / N)) / (-expm1(-alpha / N)) / sg`` -- the
    sum over the drawn actives of ``exp(-alpha r / N)``, a tied active taking the mean over its group's positions (a geometric sum;
    the ``expm1`` form keeps the digits a difference of two ``exp`` would lose for a group of one).

    A cut outside ``[1, n]``, and an alpha outside ``(0, 500]`` or not finite, gives NaN in its column.  ``n_undefined`` counts the
    replicates with ``T == 0`` or ``F == 0``, whose derived metrics (``early_derived``) are NaN."""
    import numpy as np
    rank = np.asarray(rank).astype(np.int64)
    ys = (np.asarray(y_sorted) != 0).astype(np.int64)
    last = np.asarray(group_last) != 0
    n, split, B = rank.size, int(split), int(n_boot)
    _check_bootstrap_sizes(n, B, int(seed), int(offset))
    if not 0 <= split <= n:
        raise ValueError(f"split = {split} outside [0, {n}]")
    cuts, alphas = [int(k) for k in cuts], [float(a) for a in alphas]
    if len(cuts) > BOOTSTRAP_MAX_CUTS or len(alphas) > BOOTSTRAP_MAX_ALPHAS:
        raise ValueError(f"at most {BOOTSTRAP_MAX_CUTS} cuts and {BOOTSTRAP_MAX_ALPHAS} alphas")
    gid = np.concatenate([[0], np.cumsum(last[:-1])]).astype(np.int64)
    n_groups = int(gid[-1]) + 1
    out = {"ap": np.empty(B), "hits": np.empty((B, len(cuts))), "rie": np.empty((B, len(alphas))), "n_pos": np.empty(B, dtype=np.int32)}
    for b in range(B):
        c = np.bincount(rank[bootstrap_draw(n, split, int(seed), int(offset) + b)], minlength=n).astype(np.int64)
        out["ap"][b], out["hits"][b], out["rie"][b], out["n_pos"][b] = _replicate_early(c, ys, gid, n_groups, cuts, alphas)
    out["n_undefined"] = int(((out["n_pos"] == 0) | (out["n_pos"] == n)).sum())
    return out


def early_reference(true_y, predicted_score, n_boot: int, cuts, alphas, seed: int = 0, offset: int = 0,
                    stratified: bool = False) -> dict:
    """``early_reference_sorted`` of labels and scores, prepared as ``bootstrap_reference`` prepares them (the same resamples, order,
    tie groups and refusal of non-finite scores)."""
    rank, y_sorted, group_last, split = _reference_sorted_inputs(true_y, predicted_score, n_boot, seed, offset, stratified)
    return early_reference_sorted(rank, y_sorted, group_last, split, int(n_boot), int(seed), int(offset), cuts, alphas)


def early_derived(ap, hits, rie, n_pos, n: int, cuts, alphas) -> dict:
    """The metrics from the raw sums, on either route (float64 tensors on the sums' device): ``{'AP': [B], 'EF': [B, J], 'BEDROC': [B,
    A]}`` from ``ap [B]``, ``hits [B, J]``, ``rie [B, A]``, the actives ``n_pos [B]``, the rows ``n`` and the host values ``cuts`` and
    ``alphas``.  ``AP = ap``; ``EF = (hits / k) / (T / N)``; BEDROC by Truchon & Bayly (2007), eq. 36, as RDKit's ``CalcBEDROC``
    evaluates it: ``Ra = T / N``, ``RIE = rie / T / ((1 / N) * (1 - exp(-alpha)) / (exp(alpha / N) - 1))``, ``BEDROC = RIE * Ra * sinh(alpha
    / 2) / (cosh(alpha / 2) - cosh(alpha / 2 - alpha * Ra)) + 1 / (1 - exp(alpha * (1 - Ra)))``.  All three are NaN where ``T == 0`` or
    ``T == N``."""
    ap = torch.as_tensor(ap, dtype=torch.float64)
    dev = ap.device
    hits = torch.as_tensor(hits, dtype=torch.float64, device=dev).reshape(ap.numel(), -1)
    rie = torch.as_tensor(rie, dtype=torch.float64, device=dev).reshape(ap.numel(), -1)
    T = torch.as_tensor(n_pos, device=dev).to(torch.float64).reshape(-1, 1)
    N = torch.tensor(float(n), dtype=torch.float64, device=dev)  # (a tensor: torch divides by it; by a Python number it may multiply
    #                                                              by the reciprocal on one device and divide on the other)
    k = torch.tensor([float(v) for v in cuts], dtype=torch.float64, device=dev).reshape(1, -1)
    alpha = torch.tensor([float(v) for v in alphas], dtype=torch.float64, device=dev).reshape(1, -1)
    nan = torch.full((), float("nan"), dtype=torch.float64, device=dev)
    undefined = (T == 0) | (T == N)
    Ra = T / N
    ef = (hits / k) / Ra
    RIE = rie / T / ((1.0 / N) * (1.0 - torch.exp(-alpha)) / (torch.exp(alpha / N) - 1.0))
    bedroc = RIE * Ra * torch.sinh(alpha / 2) / (torch.cosh(alpha / 2) - torch.cosh(alpha / 2 - alpha * Ra)) \
        + 1.0 / (1.0 - torch.exp(alpha * (1.0 - Ra)))
    return {"AP": torch.where(undefined.reshape(-1), nan, ap.reshape(-1)), "EF": torch.where(undefined, nan, ef),
            "BEDROC": torch.where(undefined, nan, bedroc)}


def _early_point(true_y, predicted_score, cuts, alphas):
    """The definition with every multiplicity equal to 1, in torch operators on the scores' device: ``(ap [1], hits [1, J], rie [1, A],
    T)``."""
    y, s = _as_vectors(true_y, predicted_score)
    y, s = y.detach(), s.detach()
    n, dev = s.numel(), s.device
    order = torch.sort(s, descending=True, stable=True)
    ys, ss = y[order.indices], order.values
    last = torch.ones(n, dtype=torch.bool, device=dev)
    last[:-1] = ss[1:] != ss[:-1]
    idx = torch.nonzero(last).reshape(-1)
    end = (idx + 1).to(torch.float64)                             # rows up to and including each tie group
    tps = torch.cumsum(ys, 0)[idx]
    zero = torch.zeros(1, dtype=torch.float64, device=dev)
    before, tps_before = torch.cat([zero, end[:-1]]), torch.cat([zero, tps[:-1]])
    gt, sg = tps - tps_before, end - before
    T, N = float(tps[-1]), float(n)
    pos = gt > 0
    ap = ((gt[pos] / T) * (tps[pos] / end[pos])).sum().reshape(1) if T > 0 else zero.clone()
    k = torch.tensor([float(v) for v in cuts], dtype=torch.float64, device=dev)
    g = torch.searchsorted(end, k).clamp(max=end.numel() - 1)     # (before[g] < k <= end[g])
    hits = (tps_before[g] + gt[g] * (k - before[g]) / sg[g]).reshape(1, -1)
    rie = torch.stack([(gt[pos] * torch.exp(-(a * (before[pos] + 1)) / N) * (-torch.expm1(-(a * sg[pos]) / N))
                        / (-math.expm1(-a / N)) / sg[pos]).sum() for a in (float(v) for v in alphas)]).reshape(1, -1) \
        if len(alphas) else torch.zeros((1, 0), dtype=torch.float64, device=dev)
    return ap, hits, rie, T


def _point_or_minus_one(true_y, predicted_score, cuts, alphas, key: str):
    y, s = _as_vectors(true_y, predicted_score)
    if y.numel() == 0 or float(y.sum()) == 0.0 or float(y.sum()) == float(y.numel()):
        return -1
    ap, hits, rie, T = _early_point(true_y, predicted_score, cuts, alphas)
    return float(early_derived(ap, hits, rie, torch.tensor([T], dtype=torch.float64, device=ap.device), y.numel(), cuts,
                               alphas)[key].reshape(-1)[0])


def calculate_average_precision(true_y, predicted_score) -> float:
    """Average precision (the area under the precision-recall curve as ``sklearn.metrics.average_precision_score`` sums it: one step
    per distinct score), or ``-1`` when a class is absent."""
    return _point_or_minus_one(true_y, predicted_score, (), (), "AP")


def calculate_enrichment_factor(true_y, predicted_score, fraction: float = 0.01) -> float:
    """The enrichment factor at ``fraction``: the share of actives among the top ``k = early_cut(fraction, n)`` rows over their share
    among all rows, rows of equal score counted in random order (their expectation); ``-1`` when a class is absent."""
    y, _ = _as_vectors(true_y, predicted_score)
    return _point_or_minus_one(true_y, predicted_score, (early_cut(fraction, max(1, y.numel())),), (), "EF")


def calculate_bedroc(true_y, predicted_score, alpha: float = 20.0) -> float:
    """BEDROC (Truchon & Bayly 2007; RDKit's ``CalcBEDROC``) at ``alpha``, a tied active taking the mean over its group's positions;
    ``-1`` when a class is absent."""
    return _point_or_minus_one(true_y, predicted_score, (), (_check_alpha(alpha),), "BEDROC")


class EarlySpec:
    """The early-recognition names of a call, parsed: ``names`` in the caller's order, the distinct ``fractions`` and ``alphas`` they
    need, and per name ``('AP', None)``, ``('EF', column of fractions)`` or ``('BEDROC', column of alphas)``."""

    def __init__(self, names):
        if isinstance(names, str):
            raise ValueError("early: a tuple of names, not one string")
        self.names, self.fractions, self.alphas, self.where = tuple(names), [], [], {}
        for name in self.names:
            kind, value = parse_early_name(name)
            if kind == "AP":
                self.where[name] = ("AP", None)
                continue
            column = self.fractions if kind == "EF" else self.alphas
            if value not in column:
                column.append(value)
            self.where[name] = (kind, column.index(value))
        if len(self.fractions) > BOOTSTRAP_MAX_CUTS:
            raise ValueError(f"early: {len(self.fractions)} distinct enrichment fractions, at most {BOOTSTRAP_MAX_CUTS} per call")
        if len(self.alphas) > BOOTSTRAP_MAX_ALPHAS:
            raise ValueError(f"early: {len(self.alphas)} distinct BEDROC alphas, at most {BOOTSTRAP_MAX_ALPHAS} per call")

    def cuts(self, n: int) -> list:
        return [early_cut(x, n) for x in self.fractions]

    def pick(self, derived: dict) -> dict:
        """``{name: [B]}`` out of ``early_derived``'s result."""
        return {name: derived[kind] if col is None else derived[kind][:, col] for name, (kind, col) in self.where.items()}


def parse_early_name(name):
    """``('AP', None)``, ``('EF', fraction)`` or ``('BEDROC', alpha)`` for ``'AP'``, ``'EF_<fraction>'`` (``0 < fraction <= 1``) or
    ``'BEDROC_<alpha>'`` (``0 < alpha <= 500``); anything else raises ``ValueError``."""
    if name == "AP":
        return "AP", None
    if isinstance(name, str):
        for kind, check in (("EF", _check_fraction), ("BEDROC", _check_alpha)):
            if name.startswith(kind + "_"):
                try:
                    value = float(name[len(kind) + 1:])
                except ValueError:
                    raise ValueError(f"early-recognition metric {name!r}: '{kind}_<number>' is required") from None
                return kind, check(value)
    raise ValueError(f"unknown early-recognition metric {name!r}: 'AP', 'EF_<fraction>' or 'BEDROC_<alpha>'")


def is_early_name(name) -> bool:
    """Whether ``name`` spells an early-recognition metric (``'EF_'`` / ``'BEDROC_'`` names with a bad number raise)."""
    if name == "AP":
        return True
    return isinstance(name, str) and name.startswith(("EF_", "BEDROC_")) and parse_early_name(name) is not None


def early_points(true_y, predicted_score, spec: "EarlySpec") -> dict:
    """``{name: value}`` on the full data (every multiplicity 1), from one sort."""
    y, _ = _as_vectors(true_y, predicted_score)
    cuts = spec.cuts(y.numel())
    ap, hits, rie, T = _early_point(true_y, predicted_score, cuts, spec.alphas)
    derived = early_derived(ap, hits, rie, torch.tensor([T], dtype=torch.float64, device=ap.device), y.numel(), cuts, spec.alphas)
    return {name: float(v[0]) for name, v in spec.pick(derived).items()}


def _bootstrap_replicates(true_y, predicted_score, n_boot: int, FPR_range, seed: int, offset: int, stratified: bool, spec=None):
    """``(auc, logauc, two_u, n_pos)`` tensors ``[n_boot]`` on the scores' device: CUDA scores through one stable sort and
    ``readout.bootstrap_roc`` (at most ``BOOTSTRAP_MAX_REPLICATES`` per launch sequence), CPU scores through ``bootstrap_reference``.
    With an ``EarlySpec`` that names something, also ``(ap [n_boot], hits [n_boot, J], rie [n_boot, A])`` behind them: the launch is
    ``readout.bootstrap_early`` then, and the host route adds ``early_reference``."""
    lower, upper = _check_fpr_range(FPR_range)
    y, s = _as_vectors(true_y, predicted_score)
    y, s = y.detach(), s.detach()
    n, B, seed, offset = s.numel(), int(n_boot), int(seed), int(offset)
    _check_bootstrap_sizes(n, B, seed, offset)
    if not bool(torch.isfinite(s).all()):
        raise ValueError("predicted_score holds a NaN or an infinite value")
    early = spec is not None and bool(spec.names)
    cuts = spec.cuts(n) if early else None
    if not s.is_cuda:
        ref = bootstrap_reference(y, s, B, (lower, upper), seed, offset, stratified)
        out = (torch.from_numpy(ref["AUC"]), torch.from_numpy(ref["logAUC"]), torch.from_numpy(ref["two_u"]),
               torch.from_numpy(ref["n_pos"]))
        if early:
            e = early_reference(y, s, B, cuts, spec.alphas, seed, offset, stratified)
            out += (torch.from_numpy(e["ap"]), torch.from_numpy(e["hits"]), torch.from_numpy(e["rie"]))
        return out
    from . import _lib, readout
    rank, y_sorted, group_last, split = bootstrap_prepare(y == 1.0, s, stratified)
    if early:
        cuts_t = torch.tensor(cuts, dtype=torch.int32).to(s.device)
        alphas_t = torch.tensor(spec.alphas, dtype=torch.float64).to(s.device)
    parts = []
    for b0 in range(0, B, _lib.BOOTSTRAP_MAX_REPLICATES):
        nb = min(_lib.BOOTSTRAP_MAX_REPLICATES, B - b0)
        if early:
            parts.append(readout.bootstrap_early(rank, y_sorted, group_last, split, nb, seed, offset + b0, lower, upper, cuts_t, alphas_t))
        else:
            parts.append(readout.bootstrap_roc(rank, y_sorted, group_last, split, nb, seed, offset + b0, lower, upper))
    return tuple(torch.cat([p[k] for p in parts]) if len(parts) > 1 else parts[0][k] for k in range(len(parts[0])))


def _early_replicates(spec, reps, n: int) -> dict:
    """``{name: [B]}`` of the spec's names from ``_bootstrap_replicates``' seven tensors."""
    return spec.pick(early_derived(reps[4], reps[5], reps[6], reps[3], n, spec.cuts(n), spec.alphas))


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
                      seed: int = 0, offset: int = 0, stratified: bool = False, early=()) -> dict:
    """Non-parametric bootstrap of AUC and ``logAUC_{FPR_range}``: ``point`` (the existing functions on the full data), ``replicates``
    (``{'AUC': [B], 'logAUC': [B]}`` on the scores' device; NaN where a resample holds one class only), per metric ``mean``, ``std``
    (unbiased) and the percentile interval ``ci`` over the defined replicates, ``n_undefined``, ``n_pos`` (the actives of each
    replicate, int32 ``[B]``) and the ``seed``, ``offset`` and ``n_boot`` used (the call consumes ``offset .. offset + n_boot - 1``).
    CUDA scores are evaluated by ``mkgnn_bootstrap_roc`` behind one sort, CPU scores by ``bootstrap_reference``; the resamples are
    the same either way.  ``stratified`` resamples actives and inactives separately.  Only one class in the full data raises
    ``ValueError``.

    ``early``: a tuple of names out of ``'AP'`` (average precision), ``'EF_<fraction>'`` (enrichment factor) and ``'BEDROC_<alpha>'``, at
    most 8 distinct fractions and 4 distinct alphas; an unknown or malformed name raises ``ValueError`` before any launch.  Empty (the
    default), the result and the launch (``mkgnn_bootstrap_roc``) are exactly as described above.  Otherwise every name gets its
    ``point``, ``replicates`` and ``mean`` / ``std`` / ``ci`` as AUC has them, from the SAME resamples and one ``mkgnn_bootstrap_early``
    per chunk of replicates (CPU scores: ``early_reference``), and ``cuts`` maps every ``'EF_'`` name to the rows it looked at."""
    _check_confidence(confidence)
    _check_fpr_range(FPR_range)
    spec = EarlySpec(early)
    _check_two_classes(true_y, predicted_score)
    reps = _bootstrap_replicates(true_y, predicted_score, n_boot, FPR_range, seed, offset, stratified, spec)
    auc, logauc, n_pos = reps[0], reps[1], reps[3]
    out = {"point": {"AUC": calculate_auc(true_y, predicted_score), "logAUC": calculate_logAUC(true_y, predicted_score, FPR_range)},
           "replicates": {"AUC": auc, "logAUC": logauc}, "AUC": _interval(auc, confidence), "logAUC": _interval(logauc, confidence),
           "n_undefined": int(torch.isnan(auc).sum()), "n_pos": n_pos, "seed": int(seed), "offset": int(offset),
           "n_boot": int(n_boot), "confidence": float(confidence), "FPR_range": tuple(float(v) for v in FPR_range),
           "stratified": bool(stratified)}
    if spec.names:
        n = torch.as_tensor(predicted_score).numel()
        out["point"].update(early_points(true_y, predicted_score, spec))
        for name, values in _early_replicates(spec, reps, n).items():
            out["replicates"][name] = values
            out[name] = _interval(values, confidence)
        out["cuts"] = {name: spec.cuts(n)[col] for name, (kind, col) in spec.where.items() if kind == "EF"}
    return out


def bootstrap_compare(true_y, score_a, score_b, n_boot: int = 1000, FPR_range=(0.001, 0.1), confidence: float = 0.95, seed: int = 0,
                      offset: int = 0, stratified: bool = False, early=()) -> dict:
    """The paired bootstrap of two score vectors on the same labels: both see the SAME resamples (a draw depends on ``(seed, offset +
    b, i, n, split)`` alone).  Per metric: ``diff`` (the replicate differences ``a - b``, ``[B]``), their ``mean``, ``std`` and
    ``ci``, and ``p_a_better``, the share of defined replicates with a positive difference; also ``point`` (``a``, ``b`` and ``diff`` on
    the full data), ``n_undefined`` and the ``seed``, ``offset`` and ``n_boot`` used.  ``early``: as in ``bootstrap_metrics`` -- every
    name is compared as AUC is, and the result carries ``cuts``."""
    _check_confidence(confidence)
    _check_fpr_range(FPR_range)
    spec = EarlySpec(early)
    _check_two_classes(true_y, score_a)
    a = _bootstrap_replicates(true_y, score_a, n_boot, FPR_range, seed, offset, stratified, spec)
    b = _bootstrap_replicates(true_y, score_b, n_boot, FPR_range, seed, offset, stratified, spec)
    if not torch.equal(a[3].cpu(), b[3].cpu()):
        raise RuntimeError("bootstrap_compare: the two score vectors saw different resamples")
    point_a = {"AUC": calculate_auc(true_y, score_a), "logAUC": calculate_logAUC(true_y, score_a, FPR_range)}
    point_b = {"AUC": calculate_auc(true_y, score_b), "logAUC": calculate_logAUC(true_y, score_b, FPR_range)}
    out = {"point": {"a": point_a, "b": point_b, "diff": {k: point_a[k] - point_b[k] for k in point_a}},
           "n_undefined": int(torch.isnan(a[0]).sum()), "seed": int(seed), "offset": int(offset), "n_boot": int(n_boot)}
    pairs = {"AUC": (a[0], b[0]), "logAUC": (a[1], b[1])}
    if spec.names:
        n = torch.as_tensor(score_a).numel()
        point_a.update(early_points(true_y, score_a, spec))
        point_b.update(early_points(true_y, score_b, spec))
        out["point"]["diff"] = {k: point_a[k] - point_b[k] for k in point_a}
        early_a, early_b = _early_replicates(spec, a, n), _early_replicates(spec, b, n)
        pairs.update({name: (early_a[name], early_b[name]) for name in early_a})
        out["cuts"] = {name: spec.cuts(n)[col] for name, (kind, col) in spec.where.items() if kind == "EF"}
    for name, (va, vb) in pairs.items():
        diff = va - vb.to(va.device)
        defined = diff[~torch.isnan(diff)]
        entry = _interval(diff, confidence)
        entry["diff"] = diff
        entry["p_a_better"] = float((defined > 0).double().mean()) if defined.numel() else float("nan")
        out[name] = entry
    return out


def bootstrap_per_task(true_y, pred_y, task, num_tasks: int, n_boot: int = 1000, FPR_range=(0.001, 0.1), confidence: float = 0.95,
                       seed: int = 0, offset: int = 0, stratified: bool = False, early=()) -> list:
    """``bootstrap_metrics`` over each task's labelled rows, as ``per_task`` selects them; task ``t`` uses the offsets ``offset + t *
    n_boot .. offset + (t + 1) * n_boot - 1``.  A task without a row, or with one class only, gives ``None``.  ``early``: as in
    ``bootstrap_metrics`` (refused here, before any task is run)."""
    EarlySpec(early)
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
        out.append(bootstrap_metrics(yk, s[rows], n_boot, FPR_range, confidence, seed, int(offset) + k * int(n_boot), stratified,
                                     early))
    return out


# ---- regression: MAE, R2, Pearson, Spearman, top-fraction recall, and the bootstrap of all of them with RMSE ----
# Both vectors are sorted ONCE, best first.  A replicate is the SAME vector of multiplicities the unstratified classification
# bootstrap draws, and everything a metric needs is a sum over the rows of a function of the row, its multiplicity and the prefix
# sums of the multiplicities in the two orders: seven float64 moments, three exact integer rank sums (Spearman by midranks) and
# one exact integer per top-k cut.  regression_reference is the definition in numpy; CUDA inputs take mkgnn_bootstrap_regression
# (readout.bootstrap_regression); regression_derived turns the sums into the metrics on either route.

BOOTSTRAP_REG_MAX_ROWS = 1 << 20                 # (MKGNN_BOOTSTRAP_REG_MAX_ROWS: sum c a^2 <= n (n - 1)^2 < 2^63 up to here)
REGRESSION_METRICS = ("RMSE", "MAE", "R2", "pearson", "spearman")
REGRESSION_SMALLER_IS_BETTER = ("RMSE", "MAE")


def top_name(fraction: float) -> str:
    """The name of the top-fraction recall at ``fraction``: ``'top_' + repr(float(fraction))``, e.g. ``'top_0.01'``."""
    return "top_" + repr(_check_fraction(fraction))


def parse_top_name(name) -> float:
    """The fraction of ``'top_<fraction>'`` (``0 < fraction <= 1``); anything else raises ``ValueError``."""
    if isinstance(name, str) and name.startswith("top_"):
        try:
            value = float(name[4:])
        except ValueError:
            raise ValueError(f"top-fraction recall {name!r}: 'top_<number>' is required") from None
        return _check_fraction(value)
    raise ValueError(f"unknown top-fraction recall {name!r}: 'top_<fraction>'")


def is_top_name(name) -> bool:
    """Whether ``name`` spells a top-fraction recall (a ``'top_'`` name with a bad number raises)."""
    return isinstance(name, str) and name.startswith("top_") and parse_top_name(name) > 0.0


def _regression_vectors(true_y, pred) -> Tuple[torch.Tensor, torch.Tensor]:
    """``(t, p)`` as detached float64 vectors on the predictions' device."""
    p = torch.as_tensor(pred).detach().reshape(-1).to(torch.float64)
    t = torch.as_tensor(true_y).detach().reshape(-1).to(device=p.device, dtype=torch.float64)
    if t.numel() != p.numel():
        raise ValueError("true_y and pred differ in length")
    return t, p


def _check_regression_sizes(n: int, n_boot: int, seed: int, offset: int) -> None:
    if not 1 <= n <= BOOTSTRAP_REG_MAX_ROWS:
        raise ValueError(f"the regression bootstrap takes 1 .. {BOOTSTRAP_REG_MAX_ROWS} rows, not {n}")
    if n_boot < 1:
        raise ValueError(f"n_boot = {n_boot}: at least one replicate")
    if not (0 <= seed < 1 << 64 and 0 <= offset and offset + n_boot <= 1 << 64):
        raise ValueError("seed and offset .. offset + n_boot - 1 are unsigned 64-bit values")


def _check_cuts(cuts) -> list:
    cuts = [int(k) for k in cuts]
    if len(cuts) > BOOTSTRAP_MAX_CUTS:
        raise ValueError(f"{len(cuts)} cuts, at most {BOOTSTRAP_MAX_CUTS} per call")
    return cuts


def _top_cuts(top, n: int):
    """``(names, cuts)`` of the fractions ``top``: ``top_name`` and ``early_cut`` of each; at most ``BOOTSTRAP_MAX_CUTS`` distinct ones."""
    if isinstance(top, (str, float, int)):
        raise ValueError("top: a tuple of fractions")
    fractions = []
    for f in top:
        f = _check_fraction(f)
        if f not in fractions:
            fractions.append(f)
    if len(fractions) > BOOTSTRAP_MAX_CUTS:
        raise ValueError(f"top: {len(fractions)} distinct fractions, at most {BOOTSTRAP_MAX_CUTS} per call")
    return [top_name(f) for f in fractions], [early_cut(f, n) for f in fractions]


def _tie_ends_numpy(v):
    """``(first, last)`` by rank of a sorted numpy vector: the ends of the maximal run of equal values every rank lies in."""
    import numpy as np
    n = v.size
    change = v[1:] != v[:-1]
    idx = np.arange(n)
    first = np.maximum.accumulate(np.where(np.concatenate([[True], change]), idx, 0))
    last = np.minimum.accumulate(np.where(np.concatenate([change, [True]]), idx, n - 1)[::-1])[::-1]
    return first.astype(np.int32), last.astype(np.int32)


def regression_reference_inputs(true_y, pred, lower_is_better: bool = True):
    """The arguments of ``regression_reference_sorted`` (and of ``mkgnn_bootstrap_regression``) in numpy, by numpy's stable sorts:
    ``(rank_p, first_p, last_p, cross, first_t, last_t, p_sorted, t_by_prank, centre)``.  Best first is ascending with
    ``lower_is_better``, descending (the stable sort of the negated values) otherwise, for both vectors; ``centre`` is ``(mean p,
    mean t)``.  A NaN or an infinite value raises ``ValueError``."""
    import numpy as np
    t_t, p_t = _regression_vectors(true_y, pred)
    t, p = t_t.cpu().numpy(), p_t.cpu().numpy()
    n = p.size
    if not 1 <= n <= BOOTSTRAP_REG_MAX_ROWS:
        raise ValueError(f"the regression bootstrap takes 1 .. {BOOTSTRAP_REG_MAX_ROWS} rows, not {n}")
    if not (np.isfinite(p).all() and np.isfinite(t).all()):
        raise ValueError("true_y or pred holds a NaN or an infinite value")
    order_p = np.argsort(p if lower_is_better else -p, kind="stable")
    order_t = np.argsort(t if lower_is_better else -t, kind="stable")
    rank_p = np.empty(n, dtype=np.int32)
    rank_p[order_p] = np.arange(n, dtype=np.int32)
    first_p, last_p = _tie_ends_numpy(p[order_p])
    first_t, last_t = _tie_ends_numpy(t[order_t])
    return (rank_p, first_p, last_p, rank_p[order_t], first_t, last_t, p[order_p], t[order_p],
            np.array([p.mean(), t.mean()], dtype=np.float64))


def regression_reference_sorted(rank_p, first_p, last_p, cross, first_t, last_t, p_sorted, t_by_prank, centre, cuts, n_boot: int,
                                seed: int = 0, offset: int = 0) -> dict:
    """The definition of the regression bootstrap's raw sums behind the two sorts -- the host form of ``readout.bootstrap_regression``
    / ``mkgnn_bootstrap_regression``, with the same arguments as numpy arrays: ``{'mom': float64 [B, 7], 'rank_sums': int64 [B, 3],
    'hits': int64 [B, J], 'n_drawn': int32 [B]}`` and, for error bounds, ``'mom_abs'`` (``sum c |term|`` per column) and ``'n_terms'``
    (the ranks with ``c > 0``).

    Replicate ``b`` draws ``bootstrap_draw(n, n, seed, offset + b)`` -- the unstratified classification bootstrap's rows -- and ``c``
    counts them by prediction rank (``rank_p`` of the drawn row; one outside ``[0, n)`` is not drawn).  ``Cp`` is the inclusive prefix
    sum of ``c`` over the prediction ranks, ``N = Cp[n - 1]`` (``n_drawn``); the multiplicity at truth rank ``r`` is that of prediction
    rank ``cross[r]`` (0 where that is out of range) and ``Ct`` its inclusive prefix sum; ``Cp[-1] = Ct[-1] = 0``.

    ``mom``: over the prediction ranks with ``c > 0``, ``float64(c) * term`` summed for the terms ``dp``, ``dt``, ``dp * dp``, ``dt * dt``,
    ``dp * dt``, ``|p - t|`` and ``(p - t) * (p - t)``, with ``dp = p - centre[0]`` and ``dt = t - centre[1]``.

    ``rank_sums``: ``sum c a b``, ``sum c a a``, ``sum c b b`` over the truth ranks ``r`` with ``x = cross[r]``, ``a = Cp[first_p[x] - 1] +
    Cp[last_p[x]] - N`` (twice the row's midrank among the drawn copies in prediction order, less ``N + 1``) and ``b = Ct[first_t[r] - 1]
    + Ct[last_t[r]] - N``, in int64.

    ``hits[j]``: ``sum min(clamp(k_j - (Cp[x] - c), 0, c), clamp(k_j - (Ct[r] - c), 0, c))`` -- the drawn copies among the first ``k_j``
    copies in both orders, copies ordered by (stable rank, copy number); ``-1`` for a cut outside ``[1, n]``.

    A truth rank with ``first_*`` or ``last_*`` out of range enters neither ``rank_sums`` nor ``hits``."""
    import numpy as np
    ints = [np.asarray(a).astype(np.int64) for a in (rank_p, first_p, last_p, cross, first_t, last_t)]
    rank_p, first_p, last_p, cross, first_t, last_t = ints
    p = np.asarray(p_sorted, dtype=np.float64)
    t = np.asarray(t_by_prank, dtype=np.float64)
    centre = np.asarray(centre, dtype=np.float64).reshape(2)
    n, B = rank_p.size, int(n_boot)
    if any(a.size != n for a in ints) or p.size != n or t.size != n:
        raise ValueError("the eight arrays differ in length")
    _check_regression_sizes(n, B, int(seed), int(offset))
    cuts = _check_cuts(cuts)
    dp, dt, e = p - centre[0], t - centre[1], p - t
    terms = np.stack([dp, dt, dp * dp, dt * dt, dp * dt, np.abs(e), e * e], axis=1)
    inside = lambda a: (a >= 0) & (a < n)
    x_ok = inside(cross)
    x = np.where(x_ok, cross, 0)
    ok = x_ok & inside(first_t) & inside(last_t) & inside(first_p[x]) & inside(last_p[x])
    fp, lp = np.where(ok, first_p[x], 0), np.where(ok, last_p[x], 0)
    ft, lt = np.where(ok, first_t, 0), np.where(ok, last_t, 0)
    out = {"mom": np.empty((B, 7)), "rank_sums": np.empty((B, 3), dtype=np.int64), "hits": np.empty((B, len(cuts)), dtype=np.int64),
           "n_drawn": np.empty(B, dtype=np.int32), "mom_abs": np.empty((B, 7)), "n_terms": np.empty(B, dtype=np.int64)}
    for b in range(B):
        drawn = rank_p[bootstrap_draw(n, n, int(seed), int(offset) + b)]
        c = np.bincount(drawn[inside(drawn)], minlength=n).astype(np.int64)
        live = c > 0
        weighted = c[live].astype(np.float64)[:, None] * terms[live]
        out["mom"][b], out["mom_abs"][b], out["n_terms"][b] = weighted.sum(axis=0), np.abs(weighted).sum(axis=0), int(live.sum())
        Cp0 = np.concatenate([[0], np.cumsum(c)])                 # Cp0[i] = Cp[i - 1]
        N = int(Cp0[-1])
        ct = np.where(x_ok, c[x], 0)
        Ct0 = np.concatenate([[0], np.cumsum(ct)])
        cr = np.where(ok, ct, 0)
        a = Cp0[fp] + Cp0[lp + 1] - N
        bb = Ct0[ft] + Ct0[lt + 1] - N
        out["rank_sums"][b] = int(np.sum(cr * a * bb)), int(np.sum(cr * a * a)), int(np.sum(cr * bb * bb))
        ep, et = Cp0[x + 1] - ct, Ct0[1:] - ct
        for j, k in enumerate(cuts):
            out["hits"][b, j] = int(np.sum(np.minimum(np.clip(k - ep, 0, cr), np.clip(k - et, 0, cr)))) if 1 <= k <= n else -1
        out["n_drawn"][b] = N
    return out


def regression_reference(true_y, pred, n_boot: int, cuts=(), seed: int = 0, offset: int = 0, lower_is_better: bool = True) -> dict:
    """``regression_reference_sorted`` of truths and predictions, prepared by ``regression_reference_inputs``; the result also holds the
    ``centre`` used."""
    inputs = regression_reference_inputs(true_y, pred, lower_is_better)
    out = regression_reference_sorted(*inputs, cuts, int(n_boot), int(seed), int(offset))
    out["centre"] = inputs[8]
    return out


def regression_derived(mom, rank_sums, hits, n_drawn, cuts, centre=None) -> dict:
    """The metrics from the raw sums, on either route (float64 tensors on the sums' device): ``{'RMSE', 'MAE', 'R2', 'pearson',
    'spearman': [B], 'top': [B, J]}`` from ``mom [B, 7]``, ``rank_sums [B, 3]`` (``xy``, ``xx``, ``yy``), ``hits [B, J]``, the drawn rows
    ``n_drawn [B]`` (``N``) and the host values ``cuts``.  ``RMSE = sqrt(mom6 / N)``; ``MAE = mom5 / N``; with ``Sxx = mom2 - mom0^2 / N``,
    ``Syy = mom3 - mom1^2 / N`` and ``Sxy = mom4 - mom0 mom1 / N``, ``pearson = Sxy / sqrt(Sxx Syy)`` (kept inside ``[-1, 1]``) and ``R2 = 1 -
    mom6 / Syy``; ``spearman = xy / sqrt(float64(xx) float64(yy))``; ``top = hits / k``.  A variance that is not positive makes the metrics
    that divide by it NaN -- and a vector is constant in a replicate exactly when its integer rank sum (``xx`` or ``yy``) is 0, which is
    tested first, so rounding in the centred moments cannot turn a constant resample into a correlation.  A cut whose ``hits`` is
    ``-1`` gives NaN.  The moments are centred sums, so the metrics do not depend on ``centre``; it is accepted for symmetry with the
    operator's arguments."""
    mom = torch.as_tensor(mom, dtype=torch.float64)
    dev, B = mom.device, mom.shape[0]
    rs = torch.as_tensor(rank_sums, device=dev).to(torch.int64).reshape(B, 3)
    hits = torch.as_tensor(hits, device=dev).to(torch.int64).reshape(B, -1)
    N = torch.as_tensor(n_drawn, device=dev).to(torch.float64).reshape(B)
    k = torch.tensor([float(v) for v in cuts], dtype=torch.float64, device=dev).reshape(1, -1)
    nan = torch.full((), float("nan"), dtype=torch.float64, device=dev)
    m = [mom[:, q] for q in range(7)]
    xy, xx, yy = rs[:, 0].to(torch.float64), rs[:, 1].to(torch.float64), rs[:, 2].to(torch.float64)
    const_p, const_t = rs[:, 1] == 0, rs[:, 2] == 0
    Sxx, Syy, Sxy = m[2] - m[0] * m[0] / N, m[3] - m[1] * m[1] / N, m[4] - m[0] * m[1] / N
    bad_p, bad_t = const_p | ~(Sxx > 0), const_t | ~(Syy > 0)
    return {"RMSE": torch.sqrt(m[6] / N), "MAE": m[5] / N, "R2": torch.where(bad_t, nan, 1.0 - m[6] / Syy),
            "pearson": torch.where(bad_p | bad_t, nan, (Sxy / torch.sqrt(Sxx * Syy)).clamp(-1.0, 1.0)),
            "spearman": torch.where(const_p | const_t, nan, xy / torch.sqrt(xx * yy)),
            "top": torch.where(hits < 0, nan, hits.to(torch.float64) / k)}


def _tie_ends(v: torch.Tensor):
    """``(first, last)`` int32 by rank of a sorted vector, with two running extrema (no sort, no host read)."""
    n, dev = v.numel(), v.device
    idx = torch.arange(n, dtype=torch.int64, device=dev)
    change = v[1:] != v[:-1]
    one = torch.ones(1, dtype=torch.bool, device=dev)
    first = torch.cummax(torch.where(torch.cat([one, change]), idx, torch.zeros_like(idx)), 0).values
    ends = torch.where(torch.cat([change, one]), idx, torch.full_like(idx, n - 1))
    last = torch.flip(torch.cummin(torch.flip(ends, [0]), 0).values, [0])
    return first.to(torch.int32), last.to(torch.int32)


def regression_prepare(true_y, pred, lower_is_better: bool = True):
    """``(rank_p, first_p, last_p, cross, first_t, last_t, p_sorted, t_by_prank)`` for ``readout.bootstrap_regression`` from truths and
    finite predictions on one device, with torch operators: TWO stable sorts (best first: ascending with ``lower_is_better``,
    descending otherwise, the same for both), nothing else sorts, and nothing is read back to the host."""
    t, p = _regression_vectors(true_y, pred)
    n, dev = p.numel(), p.device
    sp = torch.sort(p, descending=not lower_is_better, stable=True)
    st = torch.sort(t, descending=not lower_is_better, stable=True)
    rank_p = torch.empty(n, dtype=torch.int32, device=dev)
    rank_p[sp.indices] = torch.arange(n, dtype=torch.int32, device=dev)
    first_p, last_p = _tie_ends(sp.values)
    first_t, last_t = _tie_ends(st.values)
    return rank_p, first_p, last_p, rank_p[st.indices].contiguous(), first_t, last_t, sp.values.contiguous(), t[sp.indices].contiguous()


def regression_points(true_y, pred, top=(), lower_is_better: bool = True) -> dict:
    """``{'RMSE', 'MAE', 'R2', 'pearson', 'spearman', 'top_<f>' ..: float}`` on the full data: the definition's sums with every
    multiplicity equal to 1, in torch operators on the predictions' device, through ``regression_derived``.  An undefined metric (a
    constant vector) is NaN."""
    t, p = _regression_vectors(true_y, pred)
    n, dev = p.numel(), p.device
    if n == 0:
        raise ValueError("the regression metrics need at least one sample")
    names, cuts = _top_cuts(top, n)
    rank_p, first_p, last_p, cross, first_t, last_t, ps, ts = regression_prepare(t, p, lower_is_better)
    dp, dt, e = ps - ps.mean(), ts - ts.mean(), ps - ts
    mom = torch.stack([dp.sum(), dt.sum(), (dp * dp).sum(), (dt * dt).sum(), (dp * dt).sum(), e.abs().sum(), (e * e).sum()]).reshape(1, 7)
    x = cross.long()
    a = (first_p.long() + last_p.long() + 1 - n)[x]               # Cp[i] = i + 1
    b = first_t.long() + last_t.long() + 1 - n
    rank_sums = torch.stack([(a * b).sum(), (a * a).sum(), (b * b).sum()]).reshape(1, 3)
    r = torch.arange(n, device=dev)
    hits = torch.stack([((x < k) & (r < k)).sum() for k in cuts]).reshape(1, -1) if cuts else torch.zeros((1, 0), dtype=torch.int64, device=dev)
    d = regression_derived(mom, rank_sums, hits, torch.tensor([n], device=dev), cuts)
    out = {name: float(d[name][0]) for name in REGRESSION_METRICS}
    out.update({name: float(d["top"][0, j]) for j, name in enumerate(names)})
    return out


def calculate_mae(true_y, pred) -> float:
    """Mean absolute error, in float64 on the predictions' device."""
    return regression_points(true_y, pred)["MAE"]


def calculate_r2(true_y, pred) -> float:
    """The coefficient of determination ``1 - sum (p - t)^2 / sum (t - mean t)^2`` (``sklearn.metrics.r2_score``); NaN for constant truths."""
    return regression_points(true_y, pred)["R2"]


def calculate_pearson(true_y, pred) -> float:
    """Pearson's correlation of predictions and truths; NaN when either is constant."""
    return regression_points(true_y, pred)["pearson"]


def calculate_spearman(true_y, pred) -> float:
    """Spearman's rank correlation with midranks for ties (``scipy.stats.spearmanr``); NaN when either vector is constant."""
    return regression_points(true_y, pred)["spearman"]


def calculate_top_recall(true_y, pred, fraction: float = 0.01, lower_is_better: bool = True) -> float:
    """The share of the truly best ``k = early_cut(fraction, n)`` rows that are among the model's best ``k``, both taken best first by
    a stable sort (ties between rows follow their order)."""
    return regression_points(true_y, pred, (fraction,), lower_is_better)[top_name(fraction)]


def _regression_sums(t: torch.Tensor, p: torch.Tensor, n_boot: int, seed: int, offset: int, cuts, lower_is_better: bool):
    """``(mom, rank_sums, hits, n_drawn)`` tensors of ``n_boot`` replicates on the predictions' device: CUDA through two stable sorts and
    ``readout.bootstrap_regression`` (at most ``BOOTSTRAP_MAX_REPLICATES`` per launch sequence), CPU through ``regression_reference``."""
    n, B = p.numel(), int(n_boot)
    _check_regression_sizes(n, B, int(seed), int(offset))
    if not (bool(torch.isfinite(p).all()) and bool(torch.isfinite(t).all())):
        raise ValueError("true_y or pred holds a NaN or an infinite value")
    if not p.is_cuda:
        ref = regression_reference(t, p, B, cuts, seed, offset, lower_is_better)
        return tuple(torch.from_numpy(ref[k]) for k in ("mom", "rank_sums", "hits", "n_drawn"))
    from . import _lib, readout
    prepared = regression_prepare(t, p, lower_is_better)
    centre = torch.stack([p.mean(), t.mean()])
    cuts_t = torch.tensor(list(cuts), dtype=torch.int32).to(p.device)
    parts = [readout.bootstrap_regression(*prepared, centre, cuts_t, min(_lib.BOOTSTRAP_MAX_REPLICATES, B - b0), seed, offset + b0)
             for b0 in range(0, B, _lib.BOOTSTRAP_MAX_REPLICATES)]
    return tuple(torch.cat([q[k] for q in parts]) if len(parts) > 1 else parts[0][k] for k in range(4))


def _regression_replicates(true_y, pred, n_boot, seed, offset, top, lower_is_better):
    """``({metric: [B]}, n_drawn [B], {top name: k})`` of one prediction vector."""
    t, p = _regression_vectors(true_y, pred)
    names, cuts = _top_cuts(top, max(1, p.numel()))
    mom, rank_sums, hits, n_drawn = _regression_sums(t, p, n_boot, int(seed), int(offset), cuts, bool(lower_is_better))
    d = regression_derived(mom, rank_sums, hits, n_drawn, cuts)
    reps = {name: d[name] for name in REGRESSION_METRICS}
    reps.update({name: d["top"][:, j] for j, name in enumerate(names)})
    return reps, n_drawn, dict(zip(names, cuts))


def bootstrap_regression(true_y, pred, n_boot: int = 1000, confidence: float = 0.95, seed: int = 0, offset: int = 0, top=(0.01,),
                         lower_is_better: bool = True) -> dict:
    """Non-parametric bootstrap of the regression metrics ``RMSE``, ``MAE``, ``R2``, ``pearson``, ``spearman`` and, per fraction in ``top``,
    ``top_<fraction>`` (``top_name``: the share of the truly best ``k = early_cut(fraction, n)`` rows among the model's best ``k``; best is
    lowest with ``lower_is_better``, highest otherwise; at most 8 distinct fractions): ``point`` (``regression_points`` on the full
    data), ``replicates`` (``{metric: [B]}`` on the predictions' device; NaN where a resample makes the metric undefined -- a constant
    vector), per metric ``mean``, ``std`` (unbiased) and the percentile interval ``ci`` over the defined replicates, ``n_undefined`` per
    metric, ``cuts`` (every ``top_`` name's ``k``), ``n_drawn`` and the ``seed``, ``offset``, ``n_boot`` and ``confidence`` used (the call
    consumes ``offset .. offset + n_boot - 1``).  The resamples are those of the unstratified ``bootstrap_metrics`` for the same
    ``(seed, offset, n)``.  CUDA inputs are evaluated by ``mkgnn_bootstrap_regression`` behind two sorts, CPU inputs by
    ``regression_reference``; the resamples are the same either way.  A NaN or infinite value, no row, or more than
    ``BOOTSTRAP_REG_MAX_ROWS`` rows raises ``ValueError`` before any launch."""
    _check_confidence(confidence)
    reps, n_drawn, cuts = _regression_replicates(true_y, pred, n_boot, seed, offset, top, lower_is_better)
    out = {"point": regression_points(true_y, pred, top, lower_is_better), "replicates": reps,
           "n_undefined": {name: int(torch.isnan(v).sum()) for name, v in reps.items()}, "cuts": cuts, "n_drawn": n_drawn,
           "seed": int(seed), "offset": int(offset), "n_boot": int(n_boot), "confidence": float(confidence),
           "lower_is_better": bool(lower_is_better)}
    for name, values in reps.items():
        out[name] = _interval(values, confidence)
    return out


def bootstrap_regression_compare(true_y, pred_a, pred_b, n_boot: int = 1000, confidence: float = 0.95, seed: int = 0, offset: int = 0,
                                 top=(0.01,), lower_is_better: bool = True) -> dict:
    """The paired bootstrap of two prediction vectors on the same truths: both see the SAME resamples.  Per metric: ``diff`` (the
    replicate differences ``a - b``, ``[B]``), their ``mean``, ``std`` and ``ci``, and ``p_a_better``, the share of defined replicates in
    which ``a`` is the better one -- the smaller for ``RMSE`` and ``MAE``, the larger for the rest; also ``point`` (``a``, ``b`` and ``diff`` on
    the full data), ``n_undefined`` per metric, ``cuts`` and the ``seed``, ``offset`` and ``n_boot`` used."""
    _check_confidence(confidence)
    a, drawn_a, cuts = _regression_replicates(true_y, pred_a, n_boot, seed, offset, top, lower_is_better)
    b, drawn_b, _ = _regression_replicates(true_y, pred_b, n_boot, seed, offset, top, lower_is_better)
    if not torch.equal(drawn_a.cpu(), drawn_b.cpu()):
        raise RuntimeError("bootstrap_regression_compare: the two prediction vectors saw different resamples")
    point_a = regression_points(true_y, pred_a, top, lower_is_better)
    point_b = regression_points(true_y, pred_b, top, lower_is_better)
    out = {"point": {"a": point_a, "b": point_b, "diff": {k: point_a[k] - point_b[k] for k in point_a}}, "n_undefined": {},
           "cuts": cuts, "seed": int(seed), "offset": int(offset), "n_boot": int(n_boot)}
    for name, va in a.items():
        diff = va - b[name].to(va.device)
        defined = diff[~torch.isnan(diff)]
        better = defined < 0 if name in REGRESSION_SMALLER_IS_BETTER else defined > 0
        entry = _interval(diff, confidence)
        entry["diff"] = diff
        entry["p_a_better"] = float(better.double().mean()) if defined.numel() else float("nan")
        out[name] = entry
        out["n_undefined"][name] = int(torch.isnan(diff).sum())
    return out
