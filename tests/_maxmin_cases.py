"""Inputs the MaxMin tests share (test_maxmin_cpu.py, test_maxmin_gpu.py): the widths, the sizes around the one-workgroup form's
edge, the diverse fixtures' clustered embeddings, and the float64 walk of every shape with its margins -- computed once."""
import functools

import numpy as np

from tests import _diverse_cases as DC

WIDTHS = (1, 31, 32, 33, 64)
F64_WIDTHS = (31, 32, 33, 64)         # width 1 is left to the bit test: its cosines are all +-1 and every decision is a tie
TILE = 1024                           # _lib.MAXMIN_TILE (test_maxmin_cpu.py asserts it)
SIZES = (1, 5, TILE - 1, TILE, TILE + 1, 2 * TILE + 37)
F64_PICKS = 40
MARGIN = 4.0                          # a decision is float32-proof when its gap exceeds this many times the two error bounds
clustered = DC.clustered
seed_of = DC.seed_of


def walk_margins(emb, k):
    """The float64 walk of ``emb`` without a stop (``maxmin_pick_reference`` over ``cosine_reference``) and how safe its decisions are
    from a float32 evaluation inside ``cosine_bound``: ``(picks, leader, pick_margin, sure)``.  ``pick_margin``: over every round but
    the first (which the index alone decides), the gap between the two smallest ``cur`` values divided by the sum of their bounds
    (a start value's bound is 0).  ``sure [n]``: rows whose best and second-best similarity to the picks differ by more than
    ``MARGIN`` times the sum of their bounds (a pick, and any row when there is one pick, is sure)."""
    from molkgnn_amd.screening import cosine_bound, cosine_reference, maxmin_pick_reference
    n = emb.shape[0]
    sim, bound = cosine_reference(emb, emb), cosine_bound(emb, emb)
    picks, _, count, leader, _ = maxmin_pick_reference(sim, k)
    picks = picks[:count]
    cur, cur_bound, picked = np.full(n, -np.inf), np.zeros(n), np.zeros(n, dtype=bool)
    pick_margin = np.inf
    for t, i in enumerate(picks):
        rows = np.flatnonzero(~picked)
        if t > 0 and rows.size >= 2:
            two = rows[np.argsort(cur[rows], kind="stable")[:2]]
            assert two[0] == i
            pick_margin = min(pick_margin, float((cur[two[1]] - cur[two[0]]) / (cur_bound[two[0]] + cur_bound[two[1]])))
        picked[i] = True
        cur[i] = sim[i, i]
        meet = ~picked & (sim[:, i] > cur)
        cur[meet], cur_bound[meet] = sim[meet, i], bound[meet, i]
    sure = np.ones(n, dtype=bool)
    if count >= 2:
        s, b = sim[:, picks], bound[:, picks]
        order = np.argsort(-s, axis=1, kind="stable")[:, :2]
        at = np.arange(n)
        gap = s[at, order[:, 0]] - s[at, order[:, 1]]
        sure = (gap > MARGIN * (b[at, order[:, 0]] + b[at, order[:, 1]])) | picked
    return picks, leader, pick_margin, sure


@functools.lru_cache(maxsize=None)
def float64_case(n, H):
    """``(emb, picks, leader, pick_margin, sure, j)`` of ``clustered(n, H, seed_of(n, H) + 1000 j)`` for the first ``j = 0, 1, ...``
    whose walk of ``min(n, F64_PICKS)`` picks has ``pick_margin > MARGIN``."""
    for j in range(16):
        emb = clustered(n, H, seed_of(n, H) + 1000 * j)
        picks, leader, pick_margin, sure = walk_margins(emb, min(n, F64_PICKS))
        if pick_margin > MARGIN:
            emb.setflags(write=False)
            return emb, picks, leader, pick_margin, sure, j
    raise AssertionError(f"no seed of ({n}, {H}) keeps its pick decisions {MARGIN} bounds apart")
