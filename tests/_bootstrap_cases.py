"""Fixtures of the bootstrap tests (test_bootstrap_cpu.py, test_bootstrap_gpu.py) and the brute-force counterpart of
``evaluation.bootstrap_reference``: resample the rows EXPLICITLY with ``tests/_philox.py``'s words, then call the existing
``evaluation.calculate_auc`` / ``calculate_logAUC`` on the resampled arrays."""
import functools

import numpy as np

from tests import _philox

WINDOWS = ((0.001, 0.1), (0.001, 1.0))
KINDS = ("distinct", "grid1", "grid2", "grid8", "equal")
# AUC: one division against a sum of <= n exact terms divided once.  logAUC: about 16 (m + 2) 2^-53 < 1e-11 for m <= 5 000 curve
# points, with a factor 10 over it for the device's log10
AUC_TOL, LOGAUC_TOL = 4 * 2.0 ** -53, 1e-10


def scores(kind: str, n: int, seed: int) -> np.ndarray:
    """float64 ``[n]``: all distinct; rounded to a grid of 1 / 2 / 8 steps per unit (heavy ties); all equal; ``actives_last`` is
    built by ``labels_and_scores``."""
    rng = np.random.default_rng([seed, n, KINDS.index(kind)])
    s = rng.normal(size=n)
    if kind == "distinct":
        assert np.unique(s).size == n
        return s
    if kind == "equal":
        return np.full(n, 0.25)
    steps = {"grid1": 1.0, "grid2": 2.0, "grid8": 8.0}[kind]
    return np.round(s * steps) / steps + 0.0                  # (+ 0.0: no -0.0, whose tie with +0.0 one test plants itself)


def labels(n: int, seed: int, share: float = 0.25) -> np.ndarray:
    """int64 ``[n]`` in {0, 1} with both classes present where ``n >= 2``."""
    y = (np.random.default_rng([seed, n, 99]).random(n) < share).astype(np.int64)
    if n >= 2:
        y[0], y[-1] = 1, 0
    return y


def draws(n: int, split: int, seed: int, offset: int) -> np.ndarray:
    """The rows replicate ``(seed, offset)`` draws, from this directory's Philox mirror (not the package's)."""
    w = _philox.philox_word(seed, offset, np.arange(n, dtype=np.uint64)).astype(np.uint64)
    i = np.arange(n)
    lo = np.where(i < split, 0, split).astype(np.uint64)
    size = np.where(i < split, split, n - split).astype(np.uint64)
    return (lo + ((w * size) >> np.uint64(32))).astype(np.int64)


def brute_force(y, s, n_boot, window, seed, offset, stratified):
    """``(auc [B], logauc [B], n_pos [B])``: NaN where the resample holds one class only."""
    from molkgnn_amd import evaluation as E
    y, s = np.asarray(y), np.asarray(s, dtype=np.float64)
    n = y.size
    if stratified:
        perm = np.concatenate([np.nonzero(y == 1)[0], np.nonzero(y != 1)[0]])
        split = int((y == 1).sum())
    else:
        perm, split = np.arange(n), n
    auc, logauc, n_pos = np.full(n_boot, np.nan), np.full(n_boot, np.nan), np.zeros(n_boot, dtype=np.int64)
    for b in range(n_boot):
        idx = perm[draws(n, split, seed, offset + b)]
        yb, sb = y[idx], s[idx]
        n_pos[b] = int((yb == 1).sum())
        if 0 < n_pos[b] < n:
            auc[b] = E.calculate_auc(yb, sb)
            logauc[b] = E.calculate_logAUC(yb, sb, window)
    return auc, logauc, n_pos


# one active in eight rows: among 64 replicates of seed 0 some hold no active at all (checked when this was written: 21 of them)
UNDEFINED_Y = np.array([1, 0, 0, 0, 0, 0, 0, 0])
UNDEFINED_S = np.array([0.5, 0.1, 0.9, 0.3, 0.7, 0.2, 0.8, 0.4])
UNDEFINED_SEED, UNDEFINED_BOOT = 0, 64


def sorted_inputs(y, s, stratified=False):
    """``(rank int32, y_sorted uint8, group_last uint8, split)`` as numpy arrays: the raw operator's inputs for labels ``y`` and scores
    ``s``, by numpy's stable sort."""
    y, s = np.asarray(y) == 1, np.asarray(s, dtype=np.float64)
    n = s.size
    split = n
    if stratified:
        perm = np.concatenate([np.nonzero(y)[0], np.nonzero(~y)[0]])
        y, s, split = y[perm], s[perm], int(y.sum())
    order = np.argsort(-s, kind="stable")
    rank = np.empty(n, dtype=np.int32)
    rank[order] = np.arange(n, dtype=np.int32)
    ss = s[order]
    return rank, y[order].astype(np.uint8), np.concatenate([ss[1:] != ss[:-1], [True]]).astype(np.uint8), split


@functools.lru_cache(maxsize=None)
def case(kind: str, n: int, seed: int = 5):
    """``(y, s)`` of a named case, computed once.  Besides ``KINDS``: ``actives_last`` (distinct scores, every active ranked below every
    inactive), ``straddle`` (one tie group from rank ``tile - 3`` to ``tile + 2`` of the walk's tile between distinct scores; ``n`` must
    reach past it), ``one_class`` (no active)."""
    from molkgnn_amd import _lib
    if kind == "actives_last":
        y, s = labels(n, seed), scores("distinct", n, seed).copy()
        s[y == 1] -= 100.0
        return y, s
    if kind == "one_class":
        return np.zeros(n, dtype=np.int64), scores("grid8", n, seed)
    if kind == "straddle":
        t = _lib.BOOTSTRAP_TILE
        assert n >= t + 3
        y = labels(n, seed)
        s = -np.arange(n, dtype=np.float64)                   # rank r = row r
        s[t - 3:t + 3] = s[t - 3]
        y[t - 2], y[t + 1] = 1, 1
        return y, s
    return labels(n, seed), scores(kind, n, seed)


@functools.lru_cache(maxsize=None)
def reference(kind: str, n: int, n_boot: int, window=(0.001, 0.1), seed: int = 11, offset: int = 3, stratified: bool = False):
    """``evaluation.bootstrap_reference`` of a named case, computed once and shared (never modified by a test)."""
    from molkgnn_amd import evaluation as E
    y, s = case(kind, n)
    return E.bootstrap_reference(y, s, n_boot, window, seed, offset, stratified)
