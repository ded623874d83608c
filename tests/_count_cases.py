"""Inputs the neighbour-count and Butina tests share (test_count_within_cpu.py, test_count_within_gpu.py, test_butina_cpu.py,
test_butina_gpu.py): ``_diverse_cases``' clustered embeddings, split into rows and references, at the shapes around the count
kernel's rows per block, tile and split -- with the float64 similarities and counts of every shape, computed once."""
import functools

import numpy as np

from tests._diverse_cases import MAX_SIM, WIDTHS, clustered, seed_of          # noqa: F401  (re-exported: one set of fixtures)


def tiling():
    """``(rows per block, references per tile, most parts)`` of ``mkgnn_embed_count_within``, from the binding's mirrors."""
    from molkgnn_amd import _lib
    return _lib.MAX_COSINE_ROWS, _lib.MAX_COSINE_TILE, _lib.MAX_COSINE_MAX_PARTS


def shapes():
    """Every ``(n, R)`` of the tests: the smallest, a handful, the edges of a row block and more than two of them, against one
    reference, the edges of a tile and three tiles (three parts at these row counts); and 17 rows against one reference more than
    ``tile * max_parts`` -- more than one tile per part, and a ragged last part."""
    rows, tile, parts = tiling()
    grid = [(n, R) for n in (1, 5, rows - 1, rows, rows + 1, 2 * rows + 37) for R in (1, tile - 1, tile, tile + 1, 3 * tile)]
    return tuple(grid) + ((17, tile * parts + 1),)


def self_sizes():
    """The row counts of the self-joins (``refs`` is ``emb``): the ``n`` of ``shapes()``."""
    return tuple(sorted({n for n, _ in shapes()}))


def cosine_matrix(e, r):
    """``S [n, R]`` on the host (GPU tests): ``mkgnn_embed_cosine`` of every row of ``e`` with the rows of ``r`` as queries, in groups
    of 32 -- the float32 similarities the count and the walk promise, bit for bit."""
    import torch
    from molkgnn_amd.readout import embedding_cosine
    out = torch.empty(e.shape[0], r.shape[0], dtype=torch.float32, device=e.device)
    for a in range(0, r.shape[0], 32):
        out[:, a:a + 32] = embedding_cosine(e, r[a:a + 32])
    return out.cpu().numpy()


def _frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def float64_case(n, R, H):
    """``(emb [n, H], refs [R, H], counts int64 [n], margin)``: the rows and the references are the two ends of ONE
    ``clustered(n + R, H, seed_of(n + R, H))``, so they share its centres and a row has references above ``MAX_SIM``; the counts are
    taken over ``cosine_reference`` at ``MAX_SIM``; ``margin`` is how far the closest element of the WHOLE ``[n, R]`` matrix lies from
    ``MAX_SIM`` in units of its ``cosine_bound``."""
    from molkgnn_amd.screening import cosine_bound, cosine_reference, count_within_reference
    pool = clustered(n + R, H, seed_of(n + R, H))
    emb, refs = _frozen(pool[:n].copy()), _frozen(pool[n:].copy())
    sim = cosine_reference(emb, refs)
    margin = float((np.abs(sim - MAX_SIM) / cosine_bound(emb, refs)).min())
    return emb, refs, _frozen(count_within_reference(sim, MAX_SIM)), margin


@functools.lru_cache(maxsize=None)
def float64_self_case(n, H):
    """``(emb [n, H], counts int64 [n], margin)`` of the self-join of ``clustered(n, H, seed_of(n, H))`` -- the rows of
    ``_diverse_cases.float64_case(n, H)`` -- over the full square matrix, the diagonal included."""
    from molkgnn_amd.screening import cosine_bound, cosine_reference, count_within_reference
    emb = _frozen(clustered(n, H, seed_of(n, H)))
    sim = cosine_reference(emb, emb)
    margin = float((np.abs(sim - MAX_SIM) / cosine_bound(emb, emb)).min())
    return emb, _frozen(count_within_reference(sim, MAX_SIM)), margin
