"""Gather-collate from a resident shard, without a GPU: ``shards.gather_compact`` (the numpy definition the HIP operator
``mkgnn_gather_compact`` is tested against, and the CPU path of ``ResidentLoader``) against ``collate_compact``, and the
host-side planning of ``ResidentLoader``."""
import numpy as np
import pytest
import torch

from molkgnn_amd import padding as P
from molkgnn_amd import shards as S
from molkgnn_amd.sampling import oversampling_sampler
from molkgnn_amd.synthetic import make_batch
from tests import _batch_cases as C

DIMS = (28, 3, 7)


def _slice(b, m0, m1):
    """Molecules [m0, m1) of a collated batch, re-collated by hand (as in tests/test_shards.py)."""
    from molkgnn_amd.receptive_field import GraphBatch
    atoms = ((b.batch >= m0) & (b.batch < m1)).nonzero().view(-1)
    a0 = int(atoms[0])
    em = b.batch[b.edge_index[0]]
    edges = ((em >= m0) & (em < m1)).nonzero().view(-1)
    return GraphBatch(x=b.x[atoms], p=b.p[atoms], edge_index=b.edge_index[:, edges] - a0, edge_attr=b.edge_attr[edges],
                      batch=b.batch[atoms] - m0, y=b.y[m0:m1], assay_id=b.assay_id[m0:m1])


def _concat(parts):
    """Collated batches one after the other as one collated batch."""
    from molkgnn_amd.receptive_field import GraphBatch
    a_off = np.cumsum([0] + [int(q.x.shape[0]) for q in parts])
    return GraphBatch(x=torch.cat([q.x for q in parts]), p=torch.cat([q.p for q in parts]),
                      edge_index=torch.cat([q.edge_index + int(a_off[k]) for k, q in enumerate(parts)], dim=1),
                      edge_attr=torch.cat([q.edge_attr for q in parts]),
                      batch=torch.cat([q.batch + k for k, q in enumerate(parts)]), y=torch.cat([q.y for q in parts]),
                      assay_id=torch.cat([q.assay_id for q in parts]))


@pytest.fixture(scope="module")
def whole():
    b = make_batch(200, seed=6, assay="all9", with_receptive_fields=False)
    b.y = (torch.arange(200) % 9 == 0).to(b.y.dtype)        # (one molecule in nine active: the sampler has two classes to balance)
    return b


@pytest.fixture(scope="module")
def shard(whole, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("gather") / "a.mkgs")
    S.write_shard(path, whole)
    return S.Shard(path)


def _ids_histogram(shard, ids):
    ids = np.asarray(ids)
    d = (shard.mol_deg_ptr[ids + 1] - shard.mol_deg_ptr[ids]).sum(axis=0)
    return [int((shard.mol_atom_ptr[ids + 1] - shard.mol_atom_ptr[ids]).sum()), int(d[0]), int(d[1]), int(d[2]), int(d[3]), int(d[4])]


def _fields(host, shape, nm):
    table, total = S.compact_layout(shape, nm, *DIMS)
    return {k: host[off:off + nbytes].view(dt).reshape(shp) for k, off, shp, dt, nbytes in table}, total


def _assert_same_wire(got, want, shape, nm):
    fg, _ = _fields(got, shape, nm)
    fw, _ = _fields(want, shape, nm)
    for k in fw:
        assert fg[k].tobytes() == fw[k].tobytes(), k


def test_contiguous_range_equals_collate_compact(shard):
    for m0, m1 in ((0, 64), (17, 81), (136, 200)):
        shape = P.fixed_shape([shard.degree_histogram(m0, m1)])
        _, total = S.compact_layout(shape, m1 - m0, *DIMS)
        want = np.full(total, 0xAB, dtype=np.uint8)
        got = np.full(total, 0xCD, dtype=np.uint8)
        S.collate_compact(shard, m0, m1, shape, want)
        S.gather_compact(shard, range(m0, m1), shape, got)
        _assert_same_wire(got, want, shape, m1 - m0)


def test_arbitrary_ids_equal_the_recollated_molecules(whole, shard, tmp_path):
    ids = np.random.default_rng(0).integers(0, 200, size=64)      # (a seed whose draw repeats ids and holds both ends of the shard)
    assert len(set(ids.tolist())) < 64 and 0 in ids and 199 in ids
    path2 = str(tmp_path / "b.mkgs")
    S.write_shard(path2, _concat([_slice(whole, int(m), int(m) + 1) for m in ids]))
    shard2 = S.Shard(path2)
    assert shard2.n_molecules == 64 and shard2.compact_ok
    shape = P.fixed_shape([shard2.degree_histogram(0, 64)])
    assert shard2.degree_histogram(0, 64) == _ids_histogram(shard, ids)
    _, total = S.compact_layout(shape, 64, *DIMS)
    want = np.full(total, 0xAB, dtype=np.uint8)
    got = np.full(total, 0xCD, dtype=np.uint8)
    S.collate_compact(shard2, 0, 64, shape, want)
    S.gather_compact(shard, ids, shape, got)
    _assert_same_wire(got, want, shape, 64)
    # ... and a torch tensor or a list of ids is the same sequence
    again = np.full(total, 0xEF, dtype=np.uint8)
    S.gather_compact(shard, torch.from_numpy(ids), shape, again)
    _assert_same_wire(again, want, shape, 64)


@pytest.mark.parametrize("e_dim", [1, 5, 12])
def test_hand_made_molecules_equal_their_recollation(e_dim, tmp_path):
    """The definition itself at the widths and molecule sizes the synthetic shard does not have (tests/_batch_cases.py: two-atom
    molecules, a 300-atom chain, ``p_dim`` 4, 1 / 5 / 12 attribute bytes per bond): ``gather_compact`` of an id list equals the
    same molecules collated again by hand, written as a shard of their own and padded by ``collate_compact`` -- for the loader's
    shape, for the exact shape (no padding atom: all 64 padding molecules empty) and for shapes whose whole padding is fewer
    atoms than there are padding molecules."""
    dims = (6, 4, e_dim)
    mols = C.molecules(*dims, seed=e_dim)
    S.write_shard(str(tmp_path / "custom.mkgs"), C.collate(mols))
    shard = S.Shard(str(tmp_path / "custom.mkgs"))
    assert shard.compact_ok and shard.n_molecules == 57 and (shard.n_atoms, shard.n_edges) == (500, 886)
    assert (shard.x_dim, shard.p_dim, shard.e_dim) == dims
    res = S.ResidentShard(shard, "cpu")
    for n in (1, 57, 200):
        for name, ids in C.id_lists(n, 57).items():
            picked = [mols[int(m)] for m in ids]
            S.write_shard(str(tmp_path / "picked.mkgs"), C.collate(picked))
            shard2 = S.Shard(str(tmp_path / "picked.mkgs"))
            counts = C.degree_counts(picked)
            assert shard2.degree_histogram(0, n)[1:5] == counts == _ids_histogram(shard, ids)[1:5]
            shapes = {"loader": S.ResidentLoader(res, n, ids, "cpu").shape, "exact": C.shape_with_padding(counts),
                      "3 padding atoms": C.shape_with_padding(counts, (2, 1, 0, 0)),
                      "63 padding atoms": C.shape_with_padding(counts, (20, 20, 20, 3))}
            for what, shape in shapes.items():
                table, total = S.compact_layout(shape, n, *dims)
                want = np.full(total, 0xAB, dtype=np.uint8)
                got = np.full(total, 0xCD, dtype=np.uint8)
                S.collate_compact(shard2, 0, n, shape, want)
                S.gather_compact(shard, ids, shape, got)
                for k, off, shp, dt, nbytes in table:
                    assert got[off:off + nbytes].tobytes() == want[off:off + nbytes].tobytes(), (n, name, what, k)
                f = {k: got[off:off + nbytes].view(dt).reshape(shp) for k, off, shp, dt, nbytes in table}
                na = int(f["n_valid_atoms"][0])
                assert na == sum(m["x"].shape[0] for m in picked)
                pad = {"exact": 0, "3 padding atoms": 3, "63 padding atoms": 63}.get(what)
                assert pad is None or shape["atoms"] - na == pad
                if what == "exact":                         # no padding atom: every padding molecule is empty
                    assert na == shape["atoms"] and (f["mol_ptr"][n:] == na).all() and f["mol_ptr"].shape[0] == n + P.PAD_MOLECULES + 1


def test_errors(whole, shard, tmp_path):
    ids = list(range(10, 42))
    shape = P.fixed_shape([_ids_histogram(shard, ids)])
    _, total = S.compact_layout(shape, 32, *DIMS)
    host = np.zeros(total, dtype=np.uint8)
    S.gather_compact(shard, ids, shape, host)
    for bad in (-1, shard.n_molecules):
        with pytest.raises(ValueError, match="outside"):
            S.gather_compact(shard, ids[:-1] + [bad], shape, host)
    # one atom short in one degree
    for d in (1, 2, 3, 4):
        h = _ids_histogram(shard, ids)
        tight = dict(shape)
        tight[f"n{d}"] = h[d] - 1
        tight["atoms"] = shape["atoms"] - (shape[f"n{d}"] - tight[f"n{d}"])
        tight["edges"] = sum(k * tight[f"n{k}"] for k in range(1, 5))
        with pytest.raises(ValueError, match="do not fit"):
            S.gather_compact(shard, ids, tight, np.zeros(total, dtype=np.uint8))
    with pytest.raises(ValueError, match="too small"):
        S.gather_compact(shard, ids, shape, host[:total - 256])
    odd = make_batch(50, seed=3, with_receptive_fields=False)
    odd.edge_attr = odd.edge_attr + 0.5                  # not byte-valued: no compact form
    S.write_shard(str(tmp_path / "odd.mkgs"), odd)
    odd_shard = S.Shard(str(tmp_path / "odd.mkgs"))
    with pytest.raises(ValueError, match="compact"):
        S.gather_compact(odd_shard, [0, 1], shape, host)
    with pytest.raises(ValueError, match="compact"):
        S.ResidentShard(odd_shard, "cpu")


def test_resident_loader_plans_on_the_host(whole, shard):
    res = S.ResidentShard(shard, "cpu")
    assert res.n_molecules == 200 and torch.equal(res.y, whole.y.float())
    stream = np.random.default_rng(11).integers(0, 200, size=300)
    loader = S.ResidentLoader(res, 64, stream, "cpu")
    plan = loader.plan()
    assert len(loader) == 4 and np.array_equal(np.asarray(plan).reshape(-1), stream[:256])       # the short tail is dropped
    one = [tuple(map(int, row)) for row in S.ResidentLoader(res, 32, stream, "cpu").plan()]
    parts = [[tuple(map(int, row)) for row in S.ResidentLoader(res, 32, stream, "cpu", rank=r, world=3).plan()] for r in range(3)]
    assert sorted(sum(parts, [])) == sorted(one) and all(parts[r] == one[r::3] for r in range(3))
    with pytest.raises(ValueError):
        S.ResidentLoader(res, 32, stream, "cpu", rank=3, world=3)
    hists = [_ids_histogram(shard, row) for row in plan]
    assert loader.shape == P.fixed_shape(hists)
    # the batches are what gather_compact makes of the plan's rows, and their molecule-size bound covers pad_batch's figures
    got = list(loader)
    assert len(got) == 4
    for row, cb in zip(plan, got):
        want = np.zeros(cb.flat.numel(), dtype=np.uint8)
        S.gather_compact(shard, row, loader.shape, want)
        _assert_same_wire(cb.flat.numpy(), want, loader.shape, 64)
        assert cb.n_valid_molecules == 64 and cb.bucket_sizes == [loader.shape[f"n{d}"] for d in range(1, 5)]
        pb = P.pad_batch(_concat([_slice(whole, int(m), int(m) + 1) for m in row]), loader.shape, 64)
        assert loader.max_mol_atoms >= pb.max_mol_atoms and loader.max_mol_edges >= pb.max_mol_edges
    roomy = S.ResidentLoader(res, 64, stream, "cpu", headroom=0.5)
    base = P.fixed_shape(hists)                              # (the maxima + 1 each, before the scaling; n1 may carry a parity atom)
    for d in range(2, 5):
        assert roomy.shape[f"n{d}"] == int(np.ceil(1.5 * base[f"n{d}"]))
    assert roomy.shape["n1"] - int(np.ceil(1.5 * base["n1"])) in (0, 1)
    assert roomy.shape["edges"] % 2 == 0 and roomy.shape["atoms"] == sum(roomy.shape[f"n{d}"] for d in range(1, 5))
    for row in roomy.plan():
        pb = P.pad_batch(_concat([_slice(whole, int(m), int(m) + 1) for m in row]), roomy.shape, 64)
        assert roomy.max_mol_atoms >= pb.max_mol_atoms and roomy.max_mol_edges >= pb.max_mol_edges
    # a new draw under a kept shape: one that fits re-plans, one that does not raises and names the batch
    small = np.argsort(res.mol_atoms)[:64]
    tight = S.ResidentLoader(res, 64, small, "cpu")
    kept = dict(tight.shape)
    tight.set_epoch(small[::-1].copy())
    assert tight.shape == kept and np.array_equal(tight.plan()[0], small[::-1])
    big = np.argsort(res.mol_atoms)[-64:]
    with pytest.raises(ValueError, match="batch 1 "):
        tight.set_epoch(np.concatenate([small, big]))
    with pytest.raises(ValueError, match="outside"):
        tight.set_epoch(np.concatenate([small[:-1], [200]]))


def test_sampler_index_stream_is_the_loaders_plan(shard):
    res = S.ResidentShard(shard, "cpu")
    assert int(res.y.sum()) > 0
    loader = S.ResidentLoader(res, 32, oversampling_sampler(res.y, seed=7), "cpu")
    want = list(oversampling_sampler(res.y, seed=7))
    assert len(want) == 200 and len(set(want)) < 200         # drawn with replacement
    assert np.asarray(loader.plan()).reshape(-1).tolist() == want[:192]
    assert len(loader) == 6
