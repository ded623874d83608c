"""Inputs the diverse-pick tests share (test_diverse_cpu.py, test_diverse_gpu.py): clustered embeddings with an arc whose picks
depend on the order of the walk, the shapes around the kernel's tile, and the float64 walk of every shape -- computed once."""
import functools

import numpy as np

WIDTHS = (1, 31, 32, 33, 64)
MAX_SIM = 0.9
ARC_STEP = 0.35                       # radians between neighbours on the arc: cos 0.35 = 0.939 (> 0.9), cos 0.70 = 0.765 (< 0.9)
ARC_ROWS = 8


def sizes(H):
    """The row counts the GPU tests use at width ``H``: the smallest, a handful, and the edges of the tile."""
    from molkgnn_amd import _lib
    tile = _lib.diverse_tile(H)
    return (1, 5, tile - 1, tile, tile + 1, 2 * tile + 37)


def arc(H, rng, steps=ARC_ROWS):
    """``steps`` vectors ``5 (cos 0.35 j u + sin 0.35 j v)``, ``u`` and ``v`` orthogonal unit vectors: neighbours are more similar than
    0.9, second neighbours less -- which of them become picks depends on where the walk starts."""
    u = rng.standard_normal(H)
    u /= np.linalg.norm(u)
    v = rng.standard_normal(H)
    v -= (v @ u) * u
    v /= np.linalg.norm(v)
    j = np.arange(steps)[:, None]
    return 5.0 * (np.cos(ARC_STEP * j) * u[None, :] + np.sin(ARC_STEP * j) * v[None, :])


def clustered(n, H, seed):
    """float32 ``[n, H]``: ``max(2, n // 6)`` random centres; every row is a centre plus 0.08 of noise, times its own scale ``exp(U(-3,
    3))`` (a cosine does not see it, the norms do).  For ``H >= 2`` and ``n >= 16`` eight rows at sorted random places are an arc."""
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((max(2, n // 6), H))
    rows = centres[rng.integers(0, len(centres), n)] + 0.08 * rng.standard_normal((n, H))
    rows *= np.exp(rng.uniform(-3.0, 3.0, n))[:, None]
    if H >= 2 and n >= 16:
        at = np.sort(rng.choice(n, ARC_ROWS, replace=False))
        rows[at] = arc(H, rng)
    return rows.astype(np.float32)


def seed_of(n, H):
    return 100003 * H + n


@functools.lru_cache(maxsize=None)
def float64_case(n, H):
    """``(emb, picks, n_picks, leader, margin)`` of ``clustered(n, H, seed_of(n, H))``: the walk over ``cosine_reference`` at ``MAX_SIM``,
    and how far the closest similarity of the lower triangle lies from ``MAX_SIM`` in units of its ``cosine_bound``."""
    from molkgnn_amd.screening import cosine_bound, cosine_reference, diverse_pick_reference
    emb = clustered(n, H, seed_of(n, H))
    sim = cosine_reference(emb, emb)
    picks, n_picks, leader, _ = diverse_pick_reference(sim, MAX_SIM, n)
    low = np.tril_indices(n)
    margin = float((np.abs(sim[low] - MAX_SIM) / cosine_bound(emb, emb)[low]).min())
    emb.setflags(write=False)
    return emb, picks, n_picks, leader, margin
