"""Synthetic inputs of ``mkgnn_kernel_exemplars_update`` shared by test_exemplars_cpu.py and test_exemplars_gpu.py, and the brute
force both compare the numpy definition with: the candidates written out one by one and sorted with Python's ``sorted`` under the
order spelled as a tuple.  No network: ``sim`` is made up, the buckets are a random split of the atoms."""
import math

import numpy as np

NAN_PAYLOAD = np.array([0x7FC0BEEF], dtype=np.uint32).view(np.float32)[0]
SPECIAL = np.array([np.nan, NAN_PAYLOAD, np.inf, -np.inf, 0.0, -0.0, 1.0, -1.0, 3.5, 3.5, np.float32(1e-40)], dtype=np.float32)
REFERENCE_LAYOUT = (10, 20, 30, 50)                               # the reference's kernels per degree


def bits(a) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.int32)


def same_lists(got, want) -> bool:
    """Four ``[C, K]`` arrays alike: the scores as bit patterns, the rest as integers."""
    return (np.array_equal(bits(got[0]), bits(want[0]))
            and all(np.array_equal(np.asarray(g, dtype=np.int32), np.asarray(w, dtype=np.int32)) for g, w in zip(got[1:], want[1:])))


def begins(Ls):
    return [sum(Ls[:d]) for d in range(4)]


def make_case(counts, Ls, B, seed, kind="normal", outside=0.0, extra_stride=3, n_live=None, n_valid_atoms="inside", poison=False,
              id_range=1 << 20, lo=0.0, hi=1.0, structure_seed=None):
    """A batch of ``sum(counts)`` atoms in ``B`` molecules and one padding molecule (contiguous runs, some empty), split at random
    into degree buckets of ``counts`` slots (each ascending, as ``selected_index`` is).  ``sim`` is ``[N, C + extra_stride]``, filled
    with ``outside`` and, in every atom's own block, with scores of ``kind``: ``normal`` (uniform in ``[lo, hi)``), ``quantised`` (four
    levels: ties everywhere) or ``special`` (NaNs with two payloads, infinities, signed zeros, a subnormal, a repeated value).
    ``n_valid_atoms``: ``"inside"`` cuts the last two atoms of the last real molecule off as well, None means every atom.
    ``n_live`` defaults to ``B - 1``: the last real molecule is a filler.  ``poison``: every atom that is no candidate scores above
    all others in its own block.  ``ids`` are drawn from ``[0, id_range)``: a small range repeats them.  ``structure_seed``: the
    buckets and the molecules come from a generator of their own (cases that differ in scores and ids only: a static batch)."""
    rng = np.random.default_rng(seed)
    shape_rng = rng if structure_seed is None else np.random.default_rng(structure_seed)
    counts, Ls = [int(c) for c in counts], [int(x) for x in Ls]
    N, C = sum(counts), sum(Ls)
    perm = shape_rng.permutation(N)
    cuts = np.cumsum([0] + counts)
    buckets = [np.sort(perm[cuts[d]:cuts[d + 1]]).astype(np.int64) for d in range(4)]
    mol_ptr = np.zeros(B + 2, dtype=np.int32)
    mol_ptr[1:B + 1] = np.sort(shape_rng.integers(0, N + 1, size=B))
    mol_ptr[B + 1] = N
    atom_mol = (np.searchsorted(mol_ptr, np.arange(N), side="right") - 1).astype(np.int32)
    n_live = max(B - 1, 0) if n_live is None else int(n_live)
    nva = None if n_valid_atoms is None else max(int(mol_ptr[B]) - 2, 0)
    ids = rng.integers(0, id_range, size=B).astype(np.int32)
    sim = np.full((N, C + extra_stride), outside, dtype=np.float32)
    real = np.arange(N) < (N if nva is None else nva)
    candidate = real & (atom_mol < min(max(n_live, 0), B))
    for d in range(4):
        rows, L, c0 = buckets[d], Ls[d], begins(Ls)[d]
        if kind == "normal":
            block = rng.uniform(lo, hi, size=(rows.size, L)).astype(np.float32)
        elif kind == "quantised":
            block = (rng.integers(0, 4, size=(rows.size, L)) / 2).astype(np.float32)
        else:
            block = SPECIAL[rng.integers(0, SPECIAL.size, size=(rows.size, L))]
        if poison:
            block[~candidate[rows]] = np.float32(np.inf)
        sim[rows, c0:c0 + L] = block
    return {"sim": sim, "buckets": buckets, "col_begin": begins(Ls), "L": Ls, "atom_mol": atom_mol, "mol_ptr": mol_ptr, "ids": ids,
            "n_live": n_live, "n_valid_atoms": nva, "C": C, "B": B, "candidate": candidate}


def own_block_mask(case) -> np.ndarray:
    mask = np.zeros(case["sim"].shape, dtype=bool)
    for d in range(4):
        mask[case["buckets"][d], case["col_begin"][d]:case["col_begin"][d] + case["L"][d]] = True
    return mask


def _key(score, shard, mol, atom, arrival):
    empty = bits(score).item() == bits(np.float32(-np.inf)).item() and shard == -1 and mol == -1 and atom == -1
    nan = math.isnan(float(score))
    falling = 0.0 if nan else -(float(score) + 0.0)
    return (empty, nan, falling, int(shard), int(mol), int(atom), arrival)


def brute_force(lists, case, shard_tag):
    """The specification read literally: per column the old list's entries and then the candidates in degree-bucket slot order, one
    tuple each, sorted under (occupied, non-NaN, score descending with -0.0 == +0.0, shard, molecule, atom, arrival); the first K."""
    ts, th, tm, ta = (np.array(a, copy=True) for a in lists)
    C, K = ts.shape
    live = min(max(case["n_live"], 0), case["B"])
    nva = case["sim"].shape[0] if case["n_valid_atoms"] is None else case["n_valid_atoms"]
    for d in range(4):
        for c in range(case["col_begin"][d], case["col_begin"][d] + case["L"][d]):
            entries = [(ts[c, t], th[c, t], tm[c, t], ta[c, t]) for t in range(K)]
            for n in case["buckets"][d]:
                g = case["atom_mol"][n]
                if n < nva and g < live:
                    entries.append((case["sim"][n, c], shard_tag, case["ids"][g], n - case["mol_ptr"][g]))
            entries = sorted(((e, _key(*e, i)) for i, e in enumerate(entries)), key=lambda pair: pair[1])[:K]
            for t, (e, _) in enumerate(entries):
                ts[c, t], th[c, t], tm[c, t], ta[c, t] = e
    return ts, th, tm, ta


def reference(lists, case, shard_tag):
    from molkgnn_amd.screening import kernel_exemplars_reference
    return kernel_exemplars_reference(lists, case["sim"], case["buckets"], case["col_begin"], case["L"], case["atom_mol"],
                                      case["mol_ptr"], case["ids"], case["n_live"], case["n_valid_atoms"], shard_tag)
