"""The kernel exemplars on the GPU.  ``mkgnn_kernel_exemplars_update`` against its numpy definition
(``screening.kernel_exemplars_reference``) on made-up scores and buckets, bit for bit; ``GNNModel.kernel_scores`` against the
composition of the public modules that defines it; ``screening.kernel_exemplars`` against the definition folded over the eager walk
of the same batches.  No tolerance anywhere: integers and float bit patterns."""
import numpy as np
import pytest
import torch

from tests import _exemplar_cases as EC
from tests._resident_library import bits as _bits, build_library, eval_model

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _tile():
    from molkgnn_amd import _lib
    return _lib.EXEMPLARS_TILE


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV).to(dtype)


def _host(lists):
    return tuple(t.cpu().numpy() for t in (lists.top_score, lists.top_shard, lists.top_mol, lists.top_atom))


def _load(lists, arrays):
    for t, a in zip((lists.top_score, lists.top_shard, lists.top_mol, lists.top_atom), arrays):
        t.copy_(torch.from_numpy(np.ascontiguousarray(a)))


def _update(lists, case, tag, sim=None):
    """One eager update from a case of tests/_exemplar_cases.py (``sim``: a device tensor to take in its place)."""
    sim = _dev(case["sim"], torch.float32) if sim is None else sim
    nva = None if case["n_valid_atoms"] is None else torch.tensor([case["n_valid_atoms"]], dtype=torch.int64, device=DEV)
    lists.update(sim, [_dev(b, torch.int64) for b in case["buckets"]], case["col_begin"], _dev(case["atom_mol"], torch.int32),
                 _dev(case["mol_ptr"], torch.int32), _dev(case["ids"], torch.int32), n_live=case["n_live"], n_valid_atoms=nva,
                 shard_tag=tag, num_kernels=case["L"])


def _run_updates(counts, Ls, K, kinds, seed, B=20, **kw):
    """A running list from empty over ``len(kinds)`` updates with changing tags, device against definition after every one."""
    from molkgnn_amd.screening import KernelExemplars, empty_exemplars
    lists = KernelExemplars(sum(Ls), K, DEV)
    want = empty_exemplars(sum(Ls), K)
    assert EC.same_lists(_host(lists), want)
    for u, kind in enumerate(kinds):
        case = EC.make_case(counts, Ls, B, seed=seed + u, kind=kind, **kw)
        tag = (3, 0, 5, 1)[u % 4]
        _update(lists, case, tag)
        want = EC.reference(want, case, tag)
        assert EC.same_lists(_host(lists), want), (counts, Ls, K, u, kind)
    return lists, want


def _edge_layouts():
    T = _tile()
    return [((1, T - 1, T, T + 1), EC.REFERENCE_LAYOUT),            # every tile edge, on the reference's layout
            ((2 * T + 1, 0, T, 5), (3, 4, 0, 2)),                     # more than two tiles; a degree without atoms; one without columns
            ((T + 2, 3, 0, 0), (1, 0, 0, 0)),                         # C = 1
            ((T + 1, 64, 2 * T + 1, 1), (64, 64, 64, 64)),            # C = 256
            ((T - 1, 2 * T + 1, 0, 7), (100, 0, 70, 65))]             # blocks wider than one chunk of columns


@pytest.mark.parametrize("layout", range(5))
def test_tile_edges_match_the_definition(layout):
    counts, Ls = _edge_layouts()[layout]
    _, want = _run_updates(counts, Ls, 8, ("normal", "quantised", "normal"), seed=100 * layout, outside=np.nan, id_range=6)
    assert (want[1] >= 0).any()


@pytest.mark.parametrize("K", [1, 5, 32, 33, 64])
def test_list_lengths_match_the_definition(K):
    T = _tile()
    _run_updates((T + 1, 40, T, 2 * T + 1), (2, 3, 1, 4), K, ("quantised", "normal", "special", "quantised"), seed=K, id_range=5)


def test_nothing_outside_the_own_block_is_read():
    """Zeros, NaN or +inf outside the own blocks of ``sim`` (and in the columns behind C: the stride is C + 3): the same lists."""
    from molkgnn_amd.screening import KernelExemplars, empty_exemplars
    T = _tile()
    counts, Ls, K = (T + 1, 30, T - 1, 9), (3, 2, 4, 1), 6
    results = []
    for outside in (0.0, np.nan, np.inf):
        lists = KernelExemplars(sum(Ls), K, DEV)
        want = empty_exemplars(sum(Ls), K)
        for u in range(2):
            case = EC.make_case(counts, Ls, 12, seed=40 + u, kind="quantised", outside=outside, id_range=50)
            assert case["sim"].shape[1] == sum(Ls) + 3
            mask = EC.own_block_mask(case)
            assert (EC.bits(case["sim"][~mask]) == EC.bits(np.float32(outside))).all()
            _update(lists, case, u)
            want = EC.reference(want, case, u)
        results.append(_host(lists))
        assert EC.same_lists(results[-1], want)
    assert EC.same_lists(results[0], results[1]) and EC.same_lists(results[0], results[2])


def test_a_running_list_over_four_updates():
    from molkgnn_amd.screening import KernelExemplars, empty_exemplars
    T = _tile()
    counts, Ls, K, B = (T + 3, 2 * T + 1, 50, T), (2, 4, 3, 3), 4, 16
    C = sum(Ls)
    lists = KernelExemplars(C, K, DEV)
    # 1. filling: scores in [1, 2), ids >= 100, tag 3
    fill = EC.make_case(counts, Ls, B, seed=1, lo=1.0, hi=2.0, n_valid_atoms=None)
    fill["ids"] = (fill["ids"] % 1000 + 100).astype(np.int32)
    _update(lists, fill, 3)
    want = EC.reference(empty_exemplars(C, K), fill, 3)
    assert EC.same_lists(_host(lists), want) and (want[1] == 3).all()
    # 2. every candidate ranks behind every list's last entry: the lists come back bit-identical
    behind = EC.make_case(counts, Ls, B, seed=2, lo=-2.0, hi=-1.0)
    before = [t.clone() for t in (lists.top_score, lists.top_shard, lists.top_mol, lists.top_atom)]
    _update(lists, behind, 0)
    after = (lists.top_score, lists.top_shard, lists.top_mol, lists.top_atom)
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(after, before))
    assert EC.same_lists(EC.reference(want, behind, 0), want)
    # 3. exactly one candidate per column -- one atom per degree -- that ties the last entry's score: in the columns of degrees 1
    # and 2 (6 of 12) its molecule id is below every id of the list (it displaces the last entry), in those of degrees 3 and 4 its
    # molecule id equals the last entry's with a higher atom, or is above it (it does not)
    N = fill["sim"].shape[0]
    atoms = [int(fill["buckets"][d][-1]) for d in range(4)]
    tie = {"sim": np.full((N, C + 3), np.nan, dtype=np.float32), "buckets": [np.array([a], dtype=np.int64) for a in atoms],
           "col_begin": fill["col_begin"], "L": Ls, "atom_mol": np.zeros(N, dtype=np.int32), "mol_ptr": np.zeros(5, dtype=np.int32),
           "ids": np.zeros(4, dtype=np.int32), "n_live": 4, "n_valid_atoms": None, "C": C, "B": 4}
    for d in range(4):                                           # molecule d holds the one atom of degree d + 1
        tie["atom_mol"][atoms[d]] = d
        tie["ids"][d] = (5, 7, 2000, 3000)[d]
        c0 = fill["col_begin"][d]
        tie["sim"][atoms[d], c0:c0 + Ls[d]] = want[0][c0:c0 + Ls[d], K - 1]
    tie["mol_ptr"][:] = 0                                        # (the atom's index inside its molecule is its row: large)
    _update(lists, tie, 3)
    got, want3 = _host(lists), EC.reference(want, tie, 3)
    assert EC.same_lists(got, want3)
    entered = np.array([(got[2][c] == tie["ids"][d]).any() for d in range(4) for c in range(fill["col_begin"][d], fill["col_begin"][d] + Ls[d])])
    assert entered.tolist() == [True] * 6 + [False] * 6
    assert np.array_equal(EC.bits(got[0]), EC.bits(want[0]))     # (the scores tie: only who holds the last slot changed)
    # the same molecule id as the last entry of a column of degree 3: the atom decides, both ways
    c = fill["col_begin"][2]
    for atom_offset, enters in ((-1, True), (1, False)):
        again = dict(tie, ids=tie["ids"].copy(), mol_ptr=tie["mol_ptr"].copy())
        again["ids"][2] = want3[2][c, K - 1]
        again["mol_ptr"][2] = atoms[2] - (int(want3[3][c, K - 1]) + atom_offset)
        probe = KernelExemplars(C, K, DEV)
        _load(probe, want3)
        _update(probe, again, 3)
        assert EC.same_lists(_host(probe), EC.reference(want3, again, 3))
        assert (int(_host(probe)[3][c, K - 1]) == int(want3[3][c, K - 1]) - 1) == enters
    # 4. the filling batch again under other shard tags (repeats are kept): equal scores, ranked by the tag -- a higher one behind
    # the entry that is there, a lower one in front of it
    _update(lists, fill, 7)
    want4 = EC.reference(want3, fill, 7)
    got = _host(lists)
    assert EC.same_lists(got, want4) and (got[1][:, 0] == 3).all() and (got[1][:, 1] == 7).all()
    _update(lists, fill, 1)
    want4 = EC.reference(want4, fill, 1)
    got = _host(lists)
    assert EC.same_lists(got, want4) and (got[1][:, :3] == np.array([1, 3, 7])).all()
    assert (EC.bits(got[0][:, :3]) == EC.bits(got[0][:, :1])).all() and (got[2][:, :3] == got[2][:, :1]).all()


def test_special_values_padding_and_dead_slots():
    from molkgnn_amd.screening import KernelExemplars, empty_exemplars
    T = _tile()
    counts, Ls, K = (T + 5, 70, T, 33), (3, 2, 2, 4), 7
    C = sum(Ls)
    # NaNs with two payloads, infinities, signed zeros; atoms that are no candidates score +inf in their own block
    lists, want = _run_updates(counts, Ls, K, ("special", "special", "quantised", "special"), seed=77, id_range=3, poison=True)
    # padding atoms and fillers with the largest scores never enter
    case = EC.make_case(counts, Ls, 20, seed=5, kind="normal", poison=True, n_live=11)
    assert (~case["candidate"]).sum() > 10 and case["candidate"].sum() > 10
    fresh = KernelExemplars(C, K, DEV)
    _update(fresh, case, 2)
    got = _host(fresh)
    assert EC.same_lists(got, EC.reference(empty_exemplars(C, K), case, 2)) and not np.isinf(got[0][got[1] == 2]).any()
    # n_live = 0 (and below): nothing enters, the lists stay what they are
    for n_live in (0, -3):
        dead = EC.make_case(counts, Ls, 20, seed=6, kind="normal", lo=5.0, hi=6.0, n_live=n_live)
        _update(lists, dead, 0)
        assert EC.same_lists(_host(lists), want) and EC.same_lists(EC.reference(want, dead, 0), want)
    # n_valid_atoms NULL: every atom of a live molecule; n_live above B is clamped
    every = EC.make_case(counts, Ls, 20, seed=8, kind="normal", lo=5.0, hi=6.0, n_valid_atoms=None, n_live=1000)
    assert every["candidate"].sum() == every["mol_ptr"][20]
    _update(lists, every, 4)
    assert EC.same_lists(_host(lists), EC.reference(want, every, 4))
    # a poisoned workspace changes nothing
    again = KernelExemplars(C, K, DEV)
    _load(again, want)
    again.reserve(counts, Ls)
    again.workspace.view(torch.int32).fill_(0x7FC0BEEF)
    _update(again, every, 4)
    assert EC.same_lists(_host(again), _host(lists))


def test_one_captured_update_serves_every_batch():
    from molkgnn_amd.screening import KernelExemplars
    T = _tile()
    counts, Ls, K, B = (T + 1, 2 * T + 1, 40, T - 1), (2, 3, 1, 4), 9, 24
    C = sum(Ls)
    # the buckets, the molecule segments and the real-atom count stay (a static batch); sim, ids, n_live and shard_tag change in place
    feeds = [(EC.make_case(counts, Ls, B, seed=60 + u, kind=("normal", "quantised", "special")[u], n_live=(B, 7, B - 1)[u], id_range=9,
                           structure_seed=60), u + 2) for u in range(3)]
    base = feeds[0][0]
    for case, _ in feeds[1:]:
        assert all(np.array_equal(a, b) for a, b in zip(case["buckets"], base["buckets"])) and case["n_valid_atoms"] == base["n_valid_atoms"]
        assert np.array_equal(case["mol_ptr"], base["mol_ptr"]) and not np.array_equal(EC.bits(case["sim"]), EC.bits(base["sim"]))
    eager = KernelExemplars(C, K, DEV)
    for case, tag in feeds:
        _update(eager, case, tag)
    replayed = KernelExemplars(C, K, DEV)
    replayed.reserve(counts, Ls)
    sim = torch.zeros(base["sim"].shape, dtype=torch.float32, device=DEV)
    ids = torch.zeros(B, dtype=torch.int32, device=DEV)
    sels = [_dev(b, torch.int64) for b in base["buckets"]]
    atom_mol, mol_ptr = _dev(base["atom_mol"], torch.int32), _dev(base["mol_ptr"], torch.int32)
    nva = torch.tensor([base["n_valid_atoms"]], dtype=torch.int64, device=DEV)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side), torch.cuda.graph(graph, stream=side):
        replayed.update(sim, sels, base["col_begin"], atom_mol, mol_ptr, ids, n_valid_atoms=nva, num_kernels=Ls)
    torch.cuda.current_stream().wait_stream(side)
    assert int((replayed.top_shard != -1).sum()) == 0            # (a capture runs nothing)
    for case, tag in feeds:
        sim.copy_(_dev(case["sim"], torch.float32))
        ids.copy_(_dev(case["ids"], torch.int32))
        replayed.n_valid.fill_(case["n_live"])
        replayed.shard_tag.fill_(tag)
        graph.replay()
    torch.cuda.synchronize()
    assert EC.same_lists(_host(replayed), _host(eager)) and np.unique(_host(eager)[1]).size >= 2      # (more than one batch shows)


def _composition(model, data, layer):
    """Section 1 of the definition, written out from the public modules."""
    from molkgnn_amd import readout
    from molkgnn_amd.receptive_field import GraphBatch
    net = model.gnn_model
    names = ("p_focal", "nei_p", "nei_edge_attr", "selected_index", "nei_index")
    fields = {f"{nm}_deg{d}": getattr(data, f"{nm}_deg{d}") for nm in names for d in range(1, 5)}
    with torch.no_grad():
        x = readout.batch_norm(data.x, net.node_batch_norm, getattr(data, "n_valid_atoms", None))
        for i in range(layer + 1):
            step = GraphBatch(x=x, p=data.p, edge_index=data.edge_index, edge_attr=data.edge_attr, **fields)
            sim = net.gnn.layers[i](i == net.num_layers - 1, data=step, save_score=False)
            if i < layer:
                x = net.gnn.propagate(edge_index=data.edge_index, sim_sc=sim)
    return sim


def _own_blocks(sim, data, Ls):
    """The own-block entries of ``sim`` as one int32 bit vector on the host: degree by degree, the bucket's rows, the block's columns."""
    out, c0 = [], 0
    for d, L in enumerate(Ls):
        rows = getattr(data, f"selected_index_deg{d + 1}")
        out.append(_bits(sim.index_select(0, rows)[:, c0:c0 + L]).reshape(-1))
        c0 += L
    return np.concatenate(out)


@pytest.mark.parametrize("kernels", [(10, 20, 30, 50), (1, 2, 3, 4)])
def test_kernel_scores_are_the_composition_bit_for_bit(kernels):
    from molkgnn_amd.synthetic import make_batch
    model = eval_model(DEV, 5, num_layers=3, kernels_1hop=kernels, kernels_Nhop=kernels, task_dim=3)
    data = make_batch(30, seed=17).to(DEV)
    N = data.x.shape[0]
    for layer in range(3):
        sim, degree, kernel = model.kernel_scores(data, layer)
        assert sim.dtype == torch.float32 and tuple(sim.shape) == (N, sum(kernels))
        assert degree.dtype == kernel.dtype == torch.int32 and degree.device == kernel.device == sim.device
        assert degree.tolist() == [d + 1 for d, L in enumerate(kernels) for _ in range(L)]
        assert kernel.tolist() == [k for L in kernels for k in range(L)]
        got, want = _own_blocks(sim, data, kernels), _own_blocks(_composition(model, data, layer), data, kernels)
        assert got.size == sum(int(getattr(data, f"selected_index_deg{d + 1}").numel()) * L for d, L in enumerate(kernels))
        assert np.array_equal(got, want), (kernels, layer)
        assert np.isfinite(got.view(np.float32)).all() and np.unique(got).size > got.size // 4
    assert not model.training
    model.train()
    with pytest.raises(ValueError, match="evaluation mode"):
        model.kernel_scores(data, 0)


@pytest.fixture(scope="module")
def library(tmp_path_factory):
    return build_library(tmp_path_factory.mktemp("exemplars"), DEV, counts=(70, 45), shard_seed=300,
                         labels=lambda n: (torch.arange(n) % 3 == 0).float(), model_seed=9, batch_size=32, num_layers=3, task_dim=2)


@pytest.mark.parametrize("layer", [0, 2])
def test_kernel_exemplars_end_to_end(library, layer):
    from molkgnn_amd.screening import empty_exemplars, kernel_exemplars, kernel_exemplars_reference
    model, residents, gathered = library
    K, bs = 8, 32
    Ls = [int(x) for x in model.gnn_model.gnn.layers[layer].L]
    C = sum(Ls)
    model.train()
    out = kernel_exemplars(model, residents, layer, K, bs)
    assert model.training                                        # (handed back in the mode it came in)
    model.eval()
    assert out["n_scored"] == 115 and tuple(out["top_score"].shape) == (C, K)
    assert out["column_degree"].tolist() == [d + 1 for d, L in enumerate(Ls) for _ in range(L)]
    assert out["column_kernel"].tolist() == [k for L in Ls for k in range(L)]
    # the definition folded over the eager walk of the same batches
    want = empty_exemplars(C, K)
    kept = {}
    for tag, resident in enumerate(residents):
        n = int(resident.n_molecules)
        for b, (data, live) in enumerate(gathered(resident)):
            sim = model.kernel_scores(data, layer)[0]
            ids = np.minimum(np.arange(b * bs, (b + 1) * bs), n - 1).astype(np.int32)
            assert live == min(bs, n - b * bs)
            want = kernel_exemplars_reference(want, sim, [getattr(data, f"selected_index_deg{d}") for d in range(1, 5)],
                                              EC.begins(Ls), Ls, data.atom_mol, data.mol_ptr, ids, live, data.n_valid_atoms, tag)
            kept[(tag, b)] = (sim.clone(), data.mol_ptr.clone())
    got = tuple(out[name].cpu().numpy() for name in ("top_score", "top_shard", "top_mol", "top_atom"))
    assert EC.same_lists(got, want)
    occupied = K - ((EC.bits(want[0]) == EC.bits(np.float32(-np.inf))) & (want[1] == -1) & (want[2] == -1) & (want[3] == -1)).sum(axis=1)
    assert out["occupied"].tolist() == occupied.tolist() and (occupied > 0).all()
    assert set(np.unique(got[1]).tolist()) == {0, 1}
    # a reported (shard, molecule, atom, column) addresses its score in the batch that holds the molecule
    for c in range(0, C, 7):
        for t in (0, K - 1):
            shard, mol, atom = int(got[1][c, t]), int(got[2][c, t]), int(got[3][c, t])
            sim, mol_ptr = kept[(shard, mol // bs)]
            row = int(mol_ptr[mol % bs]) + atom
            assert _bits(sim[row, c]).item() == EC.bits(got[0][c, t]).item(), (c, t)
            assert 0 <= atom < int(residents[shard].mol_atoms[mol])
    # a second call gives identical bits
    again = kernel_exemplars(model, residents, layer, K, bs)
    assert not model.training
    assert EC.same_lists(tuple(again[name].cpu().numpy() for name in ("top_score", "top_shard", "top_mol", "top_atom")), got)
    assert again["occupied"].tolist() == out["occupied"].tolist()
