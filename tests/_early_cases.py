"""Fixtures of the early-recognition tests (test_early_cpu.py, test_early_gpu.py) on top of ``tests/_bootstrap_cases.py`` (its cases,
its sorted inputs, its Philox mirror), and a brute force that shares nothing with ``evaluation.early_reference``'s closed forms:
the rows are resampled EXPLICITLY and sorted; the average precision is summed over the distinct thresholds; the hits at a cut are
the exact rational (``fractions.Fraction``) of a tie group in random order; the RIE sum is an explicit loop of ``exp`` over every
position of every tie group."""
import functools
import math
from fractions import Fraction

import numpy as np

from tests import _bootstrap_cases as BC

ALPHAS = (20.0, 160.9, 0.5)
# Definition against brute force on the host, n <= 300: both are float64 sums of at most 300 positive terms ((m + 16) 2^-53 < 4e-14)
# whose terms carry a few roundings and the ulp of exp / expm1 each; a factor 25 over it
HOST_TOL = 1e-12
# hits: the Fraction is exact and float() rounds it once; the definition rounds one division and one addition
HITS_TOL = 4 * 2.0 ** -53


def cuts_for(n: int, tile: int = 1024):
    """{1, 2, n - 1, n, tile, tile + 1}, clipped to the valid ones (``1 <= k <= n``), ascending."""
    return tuple(sorted({k for k in (1, 2, n - 1, n, tile, tile + 1) if 1 <= k <= n}))


def brute_force(y, s, n_boot, cuts, alphas, seed, offset, stratified):
    """``(ap [B], hits [B, J], rie [B, A], n_pos [B])`` of explicitly resampled rows (``hits`` as correctly rounded floats)."""
    y, s = np.asarray(y), np.asarray(s, dtype=np.float64)
    n = y.size
    if stratified:
        perm = np.concatenate([np.nonzero(y == 1)[0], np.nonzero(y != 1)[0]])
        split = int((y == 1).sum())
    else:
        perm, split = np.arange(n), n
    ap, hits, rie = np.zeros(n_boot), np.zeros((n_boot, len(cuts))), np.zeros((n_boot, len(alphas)))
    n_pos = np.zeros(n_boot, dtype=np.int64)
    for b in range(n_boot):
        idx = perm[BC.draws(n, split, seed, offset + b)]
        order = np.argsort(-s[idx], kind="stable")
        yb, sb = (y[idx] == 1)[order], s[idx][order]
        T = n_pos[b] = int(yb.sum())
        # average precision: one step per distinct threshold, (recall - previous recall) * precision
        prev_tp = 0
        for v in sorted(set(sb.tolist()), reverse=True):
            at_least = sb >= v
            tp, pp = int(yb[at_least].sum()), int(at_least.sum())
            if tp > prev_tp:
                ap[b] += (tp - prev_tp) / T * (tp / pp)
            prev_tp = tp
        # tie groups as (first position, rows, actives), positions counted from 1
        groups, start = [], 0
        for i in range(n):
            if i == n - 1 or sb[i + 1] != sb[i]:
                groups.append((start + 1, i + 1 - start, int(yb[start:i + 1].sum())))
                start = i + 1
        for j, k in enumerate(cuts):
            exact = Fraction(0)
            for first, rows, actives in groups:
                inside = min(max(k - (first - 1), 0), rows)       # rows of the group among the first k
                exact += Fraction(actives * inside, rows)
            hits[b, j] = float(exact)
        for a, alpha in enumerate(alphas):
            total = 0.0
            for first, rows, actives in groups:
                if actives:
                    total += actives * sum(math.exp(-alpha * r / n) for r in range(first, first + rows)) / rows
            rie[b, a] = total
    return ap, hits, rie, n_pos


@functools.lru_cache(maxsize=None)
def reference(kind: str, n: int, n_boot: int, cuts, alphas=ALPHAS, seed: int = 11, offset: int = 3, stratified: bool = False):
    """``evaluation.early_reference`` of a named case, computed once and shared (never modified by a test)."""
    from molkgnn_amd import evaluation as E
    y, s = BC.case(kind, n)
    return E.early_reference(y, s, n_boot, cuts, alphas, seed, offset, stratified)


def relative_error(got, want):
    """The largest ``|got - want| / max(|want|, tiny)`` over the entries that are not NaN in ``want`` (NaN must match NaN)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape and np.array_equal(np.isnan(got), np.isnan(want))
    live = ~np.isnan(want)
    zero = live & (want == 0.0)
    assert (got[zero] == 0.0).all()
    live &= want != 0.0
    return float((np.abs(got[live] - want[live]) / np.abs(want[live])).max(initial=0.0))
