"""Hand-made molecules for the tests of the integer kernels that build a batch (the gather from a resident shard, the
expansion of the wire form, the receptive-field / plan / one-pass index builders).  CPU only.

The synthetic molecules of ``molkgnn_amd.synthetic`` all have about 25 atoms, so a 64-row tile of the gather never lies inside
one molecule and never spans more than three or four.  ``molecules`` is the set that does both.  Every atom has a degree in 1..4
(``ResidentShard`` refuses any other); degrees 1, 2 and 4 occur, degree 3 does not -- an absent bucket rides along:

* 40 two-atom molecules            a 64-row tile spans 32 slots
* one chain of 300 atoms           whole tiles, in more than one 256-row block, inside one molecule
* five stars of 5 atoms            the only atoms of degree 4 (their centres)
* one chain of 65 atoms            one tile and one row
* ten chains of 3 atoms

500 atoms, 443 bonds, 57 molecules.  Every molecule carries its own features, so any list of them can be collated again by hand
(``collate``) and compared with what a gather makes of the same list.  Bonds are stored as consecutive (i, j), (j, i) edges that
share byte-valued attributes: ``Shard.compact_ok`` holds.
"""
import numpy as np
import torch

from molkgnn_amd.receptive_field import GraphBatch


def _chain(n):
    return n, [(i, i + 1) for i in range(n - 1)]


def _star():
    return 5, [(0, k) for k in range(1, 5)]


def topologies():
    """``[(atoms, [(i, j), ...]), ...]`` of the molecule set, in its order."""
    return [_chain(2)] * 40 + [_chain(300)] + [_star()] * 5 + [_chain(65)] + [_chain(3)] * 10


def molecules(x_dim, p_dim, e_dim, seed=0, topo=None):
    """The molecule set with features of the given widths: a list of dicts ``x [a, x_dim]``, ``p [a, p_dim]`` (float32, normal
    draws), ``bonds [b, 2]`` (molecule-local int64), ``attr [b, e_dim]`` (float32, integers 0..255 with both ends present) and
    ``y`` (the molecule's number: a label that lands in the wrong slot shows)."""
    rng = np.random.default_rng(seed)
    out = []
    for k, (a, bonds) in enumerate(topologies() if topo is None else topo):
        attr = rng.integers(0, 256, size=(len(bonds), e_dim)).astype(np.float32)
        if attr.size:
            attr.reshape(-1)[0], attr.reshape(-1)[-1] = 255.0, 0.0
        out.append({"x": rng.standard_normal((a, x_dim)).astype(np.float32), "p": rng.standard_normal((a, p_dim)).astype(np.float32),
                    "bonds": np.asarray(bonds, dtype=np.int64).reshape(-1, 2), "attr": attr, "y": float(k)})
    return out


def collate(mols):
    """A list of molecules (``molecules``; repeats allowed) as one collated ``GraphBatch``, in the list's order."""
    a_off = np.cumsum([0] + [m["x"].shape[0] for m in mols])
    src, dst = [], []
    for k, m in enumerate(mols):
        i, j = m["bonds"][:, 0] + a_off[k], m["bonds"][:, 1] + a_off[k]
        src.append(np.stack([i, j], axis=1).reshape(-1))
        dst.append(np.stack([j, i], axis=1).reshape(-1))
    e_dim = mols[0]["attr"].shape[1]
    ea = np.concatenate([np.repeat(m["attr"], 2, axis=0) for m in mols]).reshape(-1, e_dim)
    return GraphBatch(x=torch.from_numpy(np.concatenate([m["x"] for m in mols])),
                      p=torch.from_numpy(np.concatenate([m["p"] for m in mols])),
                      edge_index=torch.from_numpy(np.stack([np.concatenate(src), np.concatenate(dst)])),
                      edge_attr=torch.from_numpy(ea),
                      batch=torch.from_numpy(np.repeat(np.arange(len(mols), dtype=np.int64), np.diff(a_off))),
                      y=torch.tensor([m["y"] for m in mols], dtype=torch.float32), num_graphs=len(mols))


def degree_counts(mols):
    """``[N_1, N_2, N_3, N_4]`` of a list of molecules."""
    h = np.zeros(6, dtype=np.int64)
    for m in mols:
        deg = np.bincount(m["bonds"].reshape(-1), minlength=m["x"].shape[0])
        h += np.bincount(np.minimum(deg, 5), minlength=6)
    assert h[0] == 0 and h[5] == 0, "every atom has degree 1..4"
    return [int(v) for v in h[1:5]]


def shape_with_padding(counts, need=(0, 0, 0, 0)):
    """The bucket shape that holds atoms of ``counts`` per degree plus ``need`` padding atoms per degree (``need`` all zero: the
    exact shape, no padding atom at all).  The padding's bond stubs must pair up: sum d * need_d even."""
    t = [int(c) + int(k) for c, k in zip(counts, need)]
    assert sum((d + 1) * int(k) for d, k in enumerate(need)) % 2 == 0, "the padding's bond stubs do not pair up"
    return {"n1": t[0], "n2": t[1], "n3": t[2], "n4": t[3], "atoms": sum(t), "edges": sum((d + 1) * t[d] for d in range(4))}


def id_lists(n, M, seed=0):
    """Three id lists of length ``n`` over ``M`` molecules: random with repeats, one molecule repeated, descending."""
    rng = np.random.default_rng(1000 * seed + n)
    repeats = rng.integers(0, M, size=n)
    repeats[n // 2:] = repeats[: n - n // 2]                # (every id of the second half is a repeat)
    return {"repeats": repeats, "one molecule": np.full(n, M // 3), "descending": (np.arange(n)[::-1] % M).copy()}
