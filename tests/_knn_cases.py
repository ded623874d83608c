"""What the tests of ``mkgnn_embed_knn_update`` share (test_knn_gpu.py): inputs with the hazards planted, the shapes around the
launch's tiling, and the EXPECTED lists -- never from the code under test: the similarities are ``readout.embedding_cosine`` (the
existing ``mkgnn_embed_cosine``) on the queries in groups of at most 32, the order is ``screening.topk_update_tasks_reference`` on
the host."""
import numpy as np
import torch

DEV = "cuda:0"


def bits(a) -> np.ndarray:
    if torch.is_tensor(a):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.int32)


def inputs(n, H, Q, seed):
    """float32 ``emb [n, H]`` and ``queries [Q, H]`` with the hazards of ``test_max_cosine_gpu.py::_inputs``, as far as ``n`` has room:
    a zero row, a row below the norm clamp, denormals, a row at scale 1e15, a candidate equal to a query, the negative of a query,
    and a candidate duplicated at two indices -- the second row and the last: in different tiles and parts wherever there are
    several."""
    rng = np.random.default_rng(seed)
    emb = rng.standard_normal((n, H)).astype(np.float32)
    queries = rng.standard_normal((Q, H)).astype(np.float32)
    if n > 6:
        emb[0] = 0.0
        emb[2] = np.float32(3e-9) / np.sqrt(np.float32(H))
        emb[3] = (np.float32(1e-41) * np.arange(1, H + 1)).astype(np.float32)
        emb[4] *= np.float32(1e15)
        emb[5] = queries[min(1, Q - 1)]
        emb[6] = -queries[0]
    if n > 2:
        emb[n - 1] = emb[1]
    return emb, queries


def shapes():
    """``(n, Q, K, H)``, the smallest shapes at which each mechanism can go wrong: every width class; ``K`` = 1, 2, 63, 64; ``n`` = 1, on
    either side of a tile, on either side of a part's end, three parts plus one row, parts of several tiles with a short last one;
    ``Q`` = 1, 2, 33 and the waves of a block plus or minus one; ``K`` larger than ``n``.  The split is asserted, so a change of the
    tiling shows here first."""
    from molkgnn_amd import _lib
    tile, waves = _lib.KNN_TILE, _lib.KNN_WAVES
    P = _lib.KNN_MIN_PART_TILES * tile                             # the rows of a part while the candidates are few
    cases = [(1, 1, 1, 1), (tile - 1, 2, 2, 31), (tile, waves - 1, 63, 32), (tile + 1, waves + 1, 64, 33), (P - 1, 1, 64, 64),
             (P, 1, 16, 32), (P + 1, 1, 16, 32), (3 * P + 1, 1, 63, 33), (3 * P + 1, 33, 5, 64), (5, 2, 64, 7),
             (16001, 1, 64, 32), (16384, 2, 7, 64), (200, 33, 64, 1), (P + 1, waves, 1, 64)]
    assert _lib.knn_split(P - 1, 1) == (P, 1) and _lib.knn_split(P, 1) == (P, 1) and _lib.knn_split(P + 1, 1) == (P, 2)
    assert _lib.knn_split(3 * P + 1, 1) == (P, 4) and _lib.knn_split(3 * P + 1, 33) == (P, 4)
    assert _lib.knn_split(16001, 1) == (8 * tile, 32) and _lib.knn_split(16384, 2) == (8 * tile, 32)      # (the last part: 129 rows)
    return cases


def empty_lists(Q, K):
    from molkgnn_amd.screening import empty_top
    return tuple(np.stack([a] * Q) for a in empty_top(K))


def device_lists(Q, K, top=None):
    """Three ``[Q, K]`` device tensors: empty lists, or a copy of the host lists ``top``."""
    top = empty_lists(Q, K) if top is None else top
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in top)


def host_sims(emb, queries):
    """``sim [Q, n]`` on the host: ``mkgnn_embed_cosine`` on the queries in groups of at most 32 (beyond 32 ``embedding_cosine`` takes
    another route with other bits)."""
    from molkgnn_amd.readout import embedding_cosine
    e = emb if torch.is_tensor(emb) else torch.from_numpy(np.ascontiguousarray(emb)).to(DEV)
    q = queries if torch.is_tensor(queries) else torch.from_numpy(np.ascontiguousarray(queries)).to(DEV)
    out = torch.empty(q.shape[0], e.shape[0], dtype=torch.float32, device=e.device)
    for a in range(0, q.shape[0], 32):
        out[a:a + 32] = embedding_cosine(e.contiguous(), q[a:a + 32].contiguous(), query_major=True)
    return out.cpu().numpy()


def host_update(top, emb, queries, ids=None, n_valid=None, tag=0):
    """The definition: ``topk_update_tasks_reference`` of ``top`` and ``host_sims``."""
    from molkgnn_amd.screening import topk_update_tasks_reference
    n = emb.shape[0]
    ids = np.arange(n, dtype=np.int32) if ids is None else np.asarray(ids.cpu() if torch.is_tensor(ids) else ids, dtype=np.int32)
    return topk_update_tasks_reference(top, host_sims(emb, queries), ids, n if n_valid is None else n_valid, tag)


def host_of(lists):
    return tuple(t.cpu().numpy() for t in lists)


def same_lists(got, want) -> bool:
    """Bit equality of the similarities -- among NaN entries only NaN-ness is specified -- and equality of shards and ids."""
    gs, ws = np.asarray(got[0], dtype=np.float32), np.asarray(want[0], dtype=np.float32)
    nan = np.isnan(ws)
    return (gs.shape == ws.shape and np.array_equal(np.isnan(gs), nan) and np.array_equal(bits(gs)[~nan], bits(ws)[~nan])
            and np.array_equal(np.asarray(got[1], dtype=np.int32), np.asarray(want[1], dtype=np.int32))
            and np.array_equal(np.asarray(got[2], dtype=np.int32), np.asarray(want[2], dtype=np.int32)))
