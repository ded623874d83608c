"""Inputs the neighbour-list and component tests share (test_neighbours_cpu.py, test_neighbours_gpu.py, test_components_cpu.py,
test_components_gpu.py): ``_count_cases``' fixtures, re-exported; the chain fixture, on which Butina clusters leak and linked
components do not; the graphs of the component tests; and the operator's algorithm -- snapshot hook, full compress -- restated in
numpy, which counts the rounds that change a label."""
import functools

import numpy as np

from tests._count_cases import (MAX_SIM, WIDTHS, clustered, cosine_matrix, float64_case, float64_self_case, seed_of,          # noqa: F401
                                self_sizes, shapes, tiling)

CHAIN_WIDTHS = (31, 32, 33, 64)
CHAIN_MIN_SIM = 0.9
N_CHAINS, CHAIN_LENGTH = 12, 25
GRAPH_SIZES = (2, 3, 17, 257, 1025, 4097)


def chains(n_chains, length, H, step_degrees=20.0, seed=5):
    """``(emb float32 [n_chains * length, H], chain int64 [n_chains * length])``: every chain is ``length`` points at steps of
    ``step_degrees`` on a circle in a random orthonormal plane (QR of a standard-normal ``[H, 2]``), every row scaled by a factor in
    ``[0.5, 2)``, the rows of all chains permuted together; ``chain[i]`` names the chain of row ``i``.  At 20 degrees and a threshold
    of 0.9, ``cos 20 = 0.940 > 0.9 > cos 40 = 0.766``: a point is linked to the next one of its chain and to nothing beyond it."""
    rng = np.random.default_rng(seed)
    rows, chain = [], []
    angle = np.deg2rad(step_degrees) * np.arange(length)
    for c in range(n_chains):
        plane, _ = np.linalg.qr(rng.standard_normal((H, 2)))
        rows.append(np.cos(angle)[:, None] * plane[:, 0][None, :] + np.sin(angle)[:, None] * plane[:, 1][None, :])
        chain.append(np.full(length, c))
    rows, chain = np.concatenate(rows), np.concatenate(chain)
    rows = rows * rng.uniform(0.5, 2.0, size=(rows.shape[0], 1))
    perm = rng.permutation(rows.shape[0])
    return rows[perm].astype(np.float32), chain[perm].astype(np.int64)


@functools.lru_cache(maxsize=None)
def chain_case(H):
    """``(emb, chain, sim float64 [n, n], margin)`` of ``chains(12, 25, H)``: ``cosine_reference`` of the self-join and how far its
    closest element lies from ``CHAIN_MIN_SIM`` in units of its ``cosine_bound``."""
    from molkgnn_amd.screening import cosine_bound, cosine_reference
    emb, chain = chains(N_CHAINS, CHAIN_LENGTH, H)
    sim = cosine_reference(emb, emb)
    margin = float((np.abs(sim - CHAIN_MIN_SIM) / cosine_bound(emb, emb)).min())
    for a in (emb, chain, sim):
        a.setflags(write=False)
    return emb, chain, sim, margin


def csr(edges, n):
    """``(row_ptr int64 [n + 1], col int32 [len(edges)])`` holding every ``(u, v)`` of ``edges`` ONCE, as ``v`` in ``u``'s segment."""
    edges = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    order = np.argsort(edges[:, 0], kind="stable")
    row_ptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(edges[:, 0], minlength=n), out=row_ptr[1:])
    return row_ptr, edges[order, 1].astype(np.int32)


def symmetrised(above):
    """The CSR of the union graph of a boolean ``[n, n]`` matrix: ``u`` and ``v`` linked if ``above[u, v]`` or ``above[v, u]``."""
    u, v = np.nonzero(above | above.T)
    return csr(np.stack([u, v], axis=1), above.shape[0])


def _bit_reversed(n):
    bits = max(1, (n - 1).bit_length())
    rev = np.array([int(format(i, f"0{bits}b")[::-1], 2) for i in range(n)])
    return np.argsort(np.argsort(rev, kind="stable"), kind="stable")         # the rank of the reversal: a permutation of [0, n)


def numberings(n, seed=0):
    """``{name: number int64 [n]}``: the vertex number of position ``i`` of a shape."""
    return {"identity": np.arange(n), "reversed": np.arange(n)[::-1].copy(), "random": np.random.default_rng(seed + n).permutation(n),
            "bit_reversed": _bit_reversed(n)}


def shape_edges(kind, n):
    """The edges of a shape over POSITIONS ``0 .. n - 1``, each once and in one direction."""
    i = np.arange(1, n)
    if kind == "path":
        return np.stack([i - 1, i], axis=1)
    if kind == "star":
        return np.stack([np.zeros(n - 1, dtype=np.int64), i], axis=1)
    if kind == "tree":
        return np.stack([(i - 1) // 2, i], axis=1)
    raise ValueError(kind)


def graphs(n):
    """``[(name, row_ptr, col)]``: paths, stars and binary trees of ``n`` vertices under every numbering, every edge stored in ONE
    direction; and two random sparse graphs whose edges are stored in one random direction (several components, isolated
    vertices, a few self-loops and duplicates)."""
    out = []
    for kind in ("path", "star", "tree"):
        for name, number in numberings(n).items():
            out.append((f"{kind}-{name}-{n}", *csr(number[shape_edges(kind, n)], n)))
    for k, density in enumerate((0.6, 1.5)):
        rng = np.random.default_rng(100 * n + k)
        m = max(1, int(density * n))
        edges = rng.integers(0, n, size=(m, 2))
        edges = np.concatenate([edges, edges[: m // 8]])                     # duplicates
        out.append((f"random{k}-{n}", *csr(edges, n)))
    return out


def hook_compress(row_ptr, col, n, max_rounds=None):
    """``(labels int64 [n], changing rounds, converged)``: the operator's scheme in numpy.  A round HOOKS -- for every stored edge
    the parents of both ends are read from the previous round's array ``A`` (roots, after its compression; a snapshot) and the
    larger root's entry of a copy is lowered to the smaller root -- and COMPRESSES: every vertex jumps to its parent's parent
    until nothing moves.  It stops after the first round that changes nothing, or after ``max_rounds``."""
    row_ptr, col = np.asarray(row_ptr, dtype=np.int64), np.asarray(col, dtype=np.int64)
    u = np.repeat(np.arange(n), np.diff(row_ptr))
    A = np.arange(n)
    changing = 0
    while max_rounds is None or changing < max_rounds:
        ru, rv = A[u], A[col]
        T = A.copy()
        np.minimum.at(T, np.maximum(ru, rv), np.minimum(ru, rv))
        if np.array_equal(T, A):
            return A, changing, True
        changing += 1
        while True:
            jumped = T[T]
            if np.array_equal(jumped, T):
                break
            T = jumped
        A = T
    return A, changing, False


def round_bound(n):
    """``2 ceil(log2 n)``: what the changing rounds of ``hook_compress`` stay within; the operator enqueues one round more."""
    return 2 * (max(n, 2) - 1).bit_length()
