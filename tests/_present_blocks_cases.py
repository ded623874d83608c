"""Shared by the present-block tests (tests/test_present_blocks_masks.py, tests/test_present_blocks_gpu.py): the ten-line definition of
the two mask arrays, and the batches the mask construction is checked on."""
import numpy as np
import torch

from tests import _topologies as T


def masks_by_definition(b, plan):
    """``present8[j]`` = OR of ``1 << (deg(s) - 1)`` over the edges ``s -> j`` (``deg`` = the bucket an atom is in, 0 = none);
    ``contrib_present8[row]`` = ``present8`` of the row's target: the atom itself for the focal slot, ``nei(n, a)`` for slot ``a``,
    rows numbered bucket by bucket, atom by atom, focal then neighbours."""
    n = b.x.shape[0]
    deg = np.zeros(n, dtype=np.int64)
    for bk in plan.buckets:
        deg[bk.sel.cpu().numpy()] = bk.degree
    present = np.zeros(n, dtype=np.int64)
    for s, t in b.edge_index.cpu().numpy().T:
        if deg[s]:
            present[t] |= 1 << (deg[s] - 1)
    rows = []
    for bk in plan.buckets:
        sel, nei = bk.sel.cpu().numpy(), bk.nei.cpu().numpy().reshape(bk.count, bk.degree)
        rows += [np.concatenate([sel[:, None], nei], axis=1).reshape(-1)]
    rows = np.concatenate(rows) if rows else np.zeros(0, dtype=np.int64)
    return present.astype(np.int8), present[rows].astype(np.int8)


def _hub():
    """A degree-4 hub whose neighbours have degrees 1, 2, 3 and 4 (its mask is 15); atom ids: hub 0, its neighbours 1..4."""
    edges = [(0, 1), (0, 2), (0, 3), (0, 4),       # 1: a leaf
             (2, 5),                              # 2: degree 2
             (3, 6), (3, 7),                      # 3: degree 3
             (4, 8), (4, 9), (4, 10)]             # 4: degree 4
    return (11, edges)


def batches():
    """name -> CPU batch (tests/_topologies.batch_of)."""
    out = {
        "small_molecules": T.batch_of([T.tree(9), T.tree(14), T.star(3), T.tree(6, ring=False)], seed=1),
        "atom_without_bonds": T.batch_of([T.tree(8), T.single(), T.pair(), T.single()], seed=2),
        "hub_of_all_degrees": T.batch_of([_hub(), T.tree(5)], seed=3),
        "chain": T.batch_of([T.chain(12)], seed=4),
    }
    return out


def padded_batch(dev=None):
    """Five molecules padded to the common shape of two batches (``padding.pad_batch``), receptive fields attached."""
    from molkgnn_amd import padding as P
    from molkgnn_amd.receptive_field import attach_receptive_fields
    from molkgnn_amd.synthetic import make_batch
    raw = make_batch(5, seed=21, with_receptive_fields=False)
    other = make_batch(5, seed=22, with_receptive_fields=False)
    shape = P.fixed_shape([P.degree_histogram(raw), P.degree_histogram(other)])
    pb = P.pad_batch(raw, shape, 5)
    if dev is not None:
        pb = pb.to(dev)
    return attach_receptive_fields(pb, sizes=[shape[f"n{d}"] for d in range(1, 5)])
