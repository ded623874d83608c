"""Fixtures of the regression-bootstrap tests (test_bootstrap_regression_cpu.py, test_bootstrap_regression_gpu.py) and the brute-force
counterpart of ``evaluation.regression_reference``: resample the rows EXPLICITLY with ``tests/_philox.py``'s words, then take numpy and
scipy on the resampled vectors, and count top-k hits as the intersection of two explicit sets of copies."""
import functools

import numpy as np

from tests import _philox

# what the definition is held to against explicit resampling: Spearman (a ratio of exact integers against scipy's float midranks),
# and the metrics derived from the float64 moments (folds of at most 60 rows of values of a few units: a few 2^-53 of rounding each)
SPEARMAN_TOL, MOMENT_TOL = 1e-14, 1e-12
# a CUDA call against the same call on CPU copies: the project's tolerance for this comparison (tests/_bootstrap_cases.LOGAUC_TOL)
ROUTE_TOL = 1e-10


def draws(n: int, seed: int, offset: int) -> np.ndarray:
    """The rows replicate ``(seed, offset)`` draws, from this directory's Philox mirror (not the package's): unstratified."""
    w = _philox.philox_word(seed, offset, np.arange(n, dtype=np.uint64)).astype(np.uint64)
    return ((w * np.uint64(n)) >> np.uint64(32)).astype(np.int64)


def small_fold(case: int):
    """``(t, p, lower_is_better)``: a random fold of 2 .. 60 rows, truths of a few units and predictions that follow them, both rounded
    to 0, 1 or 2 decimals so that both orders have ties."""
    rng = np.random.default_rng([case, 77])
    n, decimals = int(rng.integers(2, 61)), int(rng.integers(0, 3))
    t = np.round(rng.normal(size=n) * 2.0, decimals) + 0.0
    p = np.round(t + rng.normal(size=n) * 0.7, decimals) + 0.0
    return t, p, bool(case % 2)


def brute_force(t, p, n_boot: int, cuts, seed: int, offset: int, lower_is_better: bool) -> dict:
    """Per replicate, from the explicitly resampled vectors: RMSE, MAE, R2, pearson, spearman (NaN where a vector is constant), and
    per cut the copies ``(row, copy number)`` among the first ``k`` in BOTH orders, copies ordered by (value best first, row, copy)."""
    from scipy import stats
    t, p = np.asarray(t, dtype=np.float64), np.asarray(p, dtype=np.float64)
    n, sign = t.size, 1.0 if lower_is_better else -1.0
    order_p = sorted(range(n), key=lambda i: (sign * p[i], i))
    order_t = sorted(range(n), key=lambda i: (sign * t[i], i))
    out = {k: np.full(n_boot, np.nan) for k in ("RMSE", "MAE", "R2", "pearson", "spearman")}
    out["hits"] = np.zeros((n_boot, len(cuts)), dtype=np.int64)
    for b in range(n_boot):
        idx = draws(n, seed, offset + b)
        pb, tb = p[idx], t[idx]
        out["RMSE"][b] = np.sqrt(np.mean((pb - tb) ** 2))
        out["MAE"][b] = np.mean(np.abs(pb - tb))
        if np.ptp(tb) > 0:
            out["R2"][b] = 1.0 - np.sum((pb - tb) ** 2) / np.sum((tb - tb.mean()) ** 2)
        if np.ptp(tb) > 0 and np.ptp(pb) > 0:
            out["pearson"][b] = stats.pearsonr(pb, tb)[0]
            out["spearman"][b] = stats.spearmanr(pb, tb)[0]
        c = np.bincount(idx, minlength=n)
        copies_p = [(i, j) for i in order_p for j in range(c[i])]
        copies_t = [(i, j) for i in order_t for j in range(c[i])]
        for j, k in enumerate(cuts):
            out["hits"][b, j] = len(set(copies_p[:k]) & set(copies_t[:k]))
    return out


def values(kind: str, n: int, seed: int = 5):
    """``(t, p)`` float64 ``[n]`` of a named case: ``distinct`` (no ties), ``grid`` (both rounded to eighths: heavy ties in both orders),
    ``equal_p`` (every prediction the same: ONE tie group), ``straddle_p`` / ``straddle_t`` / ``straddle_both`` (distinct values but for
    one tie group over the ranks ``tile - 3 .. tile + 2`` of the walk's tile, in prediction order, truth order or both; ``n`` must reach
    past it)."""
    from molkgnn_amd import _lib
    rng = np.random.default_rng([seed, n, 31])
    t = rng.normal(size=n) * 2.0
    p = t + rng.normal(size=n) * 0.7
    if kind == "distinct":
        assert np.unique(t).size == n and np.unique(p).size == n
    elif kind == "grid":
        t, p = np.round(t * 8.0) / 8.0 + 0.0, np.round(p * 8.0) / 8.0 + 0.0
    elif kind == "equal_p":
        p = np.full(n, 0.25)
    elif kind.startswith("straddle"):
        tile = _lib.BOOTSTRAP_TILE
        assert n >= tile + 3
        for v, wanted in ((p, kind in ("straddle_p", "straddle_both")), (t, kind in ("straddle_t", "straddle_both"))):
            if wanted:                                                    # (six consecutive ranks of the ASCENDING order take the
                rows = np.argsort(v, kind="stable")[tile - 3:tile + 3]    #  lowest of their values; every other value stays distinct.
                v[rows] = v[rows[0]]                                      #  case() negates both vectors for the descending order)
    else:
        raise KeyError(kind)
    return t, p


@functools.lru_cache(maxsize=None)
def case(kind: str, n: int, lower_is_better: bool = True):
    """``(t, p)`` of ``values``, computed once; a ``straddle`` case is built for the direction it is sorted in."""
    t, p = values(kind, n)
    if kind.startswith("straddle") and not lower_is_better:
        t, p = -t, -p                                                     # (descending order of these = ascending order of values())
    return t, p


@functools.lru_cache(maxsize=None)
def inputs(kind: str, n: int, lower_is_better: bool = True):
    """``evaluation.regression_reference_inputs`` of a named case (nine numpy arrays), computed once and never modified."""
    from molkgnn_amd import evaluation as E
    return E.regression_reference_inputs(*case(kind, n, lower_is_better), lower_is_better)


def cuts_for(n: int, J: int) -> tuple:
    """``J`` cuts of a fold of ``n`` rows: 1 and ``n`` first, then sizes in between."""
    return tuple([1, n, max(1, n // 100), max(1, n // 10), max(1, n // 3), max(1, n // 2), max(1, n - 1), max(1, n // 7)][:J])


@functools.lru_cache(maxsize=None)
def reference(kind: str, n: int, n_boot: int, cuts: tuple, seed: int = 11, offset: int = 3, lower_is_better: bool = True):
    """``evaluation.regression_reference_sorted`` of a named case, computed once and shared (never modified by a test)."""
    from molkgnn_amd import evaluation as E
    return E.regression_reference_sorted(*inputs(kind, n, lower_is_better), cuts, n_boot, seed, offset)


def mom_bound(ref: dict) -> np.ndarray:
    """``[B, 7]``: ``(m + 16) 2^-53 sum c |term|`` per replicate and column, for ``m`` terms with ``c > 0`` -- the rounding of a float64 sum
    of ``m`` terms in any order, each term a rounded product times a rounded multiplicity, with room for the reference's own sum."""
    return (ref["n_terms"][:, None] + 16.0) * 2.0 ** -53 * ref["mom_abs"]
