"""Batches of molecules with explicit topologies, for the tests that drive the molecule-resident step and the fused tail to
their chunk and degree limits (``synthetic.make_batch`` draws molecules of 8 to 60 atoms and never reaches them).

A molecule spec is ``(n_atoms, bonds)`` with ``bonds`` a list of undirected pairs of local atom indices.  ``batch_of``
lays the molecules out contiguously, stores every bond as two consecutive directed edges with one attribute row (the
reference's layout, ``wrapper.py:152-156``) and builds the receptive fields with ``receptive_field.build_receptive_fields``.
"""
from __future__ import annotations

from typing import List, Sequence, Tuple

import torch

Spec = Tuple[int, List[Tuple[int, int]]]


def single() -> Spec:
    return 1, []


def pair() -> Spec:
    return 2, [(0, 1)]


def empty() -> Spec:
    """A molecule without atoms (a loader's padding slot): a segment of length 0 in ``mol_ptr``."""
    return 0, []


def chain(n: int) -> Spec:
    """A path on ``n`` atoms (atom i bonds to i + 1): two ends of degree 1, everything between of degree 2."""
    return n, [(i, i + 1) for i in range(n - 1)]


def repeat(specs: Sequence[Spec], times: int) -> List[Spec]:
    """``specs`` laid end to end ``times`` times (the spec tuples are shared, not copied: ``batch_of`` only reads them)."""
    return list(specs) * times


def tree(n: int, ring: bool = True) -> Spec:
    """A ternary tree on ``n`` atoms (atom i bonds to (i - 1) // 3: inner atoms have degree 4 from n = 5 on), plus -- with
    ``ring`` -- one ring closure between the last two leaves that are not yet bonded."""
    bonds = [((i - 1) // 3, i) for i in range(1, n)]
    if ring and n >= 4:
        deg = [0] * n
        for a, c in bonds:
            deg[a] += 1
            deg[c] += 1
        leaves = [i for i in range(n) if deg[i] == 1]
        a, c = leaves[-2], leaves[-1]
        if (min(a, c), max(a, c)) not in {(min(u, v), max(u, v)) for u, v in bonds}:
            bonds.append((a, c))
    return n, bonds


def star(arms: int = 4) -> Spec:
    """A centre of degree ``arms`` and ``arms`` single-bonded leaves (``arms = 5``: the degree-5 hub no bucket takes)."""
    return arms + 1, [(0, i) for i in range(1, arms + 1)]


def circulant(n: int = 128) -> Spec:
    """The 4-regular circulant i ~ i +- 1, i +- 2 (mod n): n atoms, 2n bonds -- 4n directed edges, 2n each way per molecule
    (n = 128: exactly the fused tail's 128 atoms and 512 edges)."""
    return n, [(i, (i + k) % n) for i in range(n) for k in (1, 2)]


def batch_of(specs: Sequence[Spec], F: int = 28, E: int = 7, seed: int = 0, y_rate: float = 0.3):
    """A ``GraphBatch`` (CPU) of the molecules in ``specs``: random ``x`` [N, F], positions ``p`` [N, 3], bond attributes
    [M, E] (the same row in both directions), labels ``y``, ``num_graphs`` and every receptive-field tensor."""
    from molkgnn_amd.receptive_field import GraphBatch, build_receptive_fields
    g = torch.Generator().manual_seed(seed)
    src, dst, batch_vec = [], [], []
    off = 0
    for m, (n, bonds) in enumerate(specs):
        for a, c in bonds:
            assert 0 <= a < n and 0 <= c < n and a != c, (m, a, c)
            src += [off + a, off + c]
            dst += [off + c, off + a]
        batch_vec += [m] * n
        off += n
    N, nb = off, len(src) // 2
    edge_index = torch.tensor([src, dst], dtype=torch.long).reshape(2, -1)
    x = torch.randn(N, F, generator=g)
    p = 1.5 * torch.randn(N, 3, generator=g)
    edge_attr = torch.rand(nb, E, generator=g).repeat_interleave(2, dim=0)
    y = (torch.rand(len(specs), generator=g) < y_rate).float()
    fields = build_receptive_fields(x, p, edge_index, edge_attr)
    return GraphBatch(x=x, p=p, edge_index=edge_index, edge_attr=edge_attr, batch=torch.tensor(batch_vec, dtype=torch.long),
                      y=y, num_graphs=len(specs), **fields)


def degrees(b) -> torch.Tensor:
    return torch.bincount(b.edge_index[0], minlength=b.x.shape[0])


def molecule_sizes(b) -> List[int]:
    return torch.bincount(b.batch, minlength=b.num_graphs).tolist()
