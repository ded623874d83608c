"""``mkgnn_graph_components`` and ``cluster_components_embeddings`` on the GPU: the labels against the host's union-find on paths,
stars, trees and random graphs under every numbering, within the round bound; edges stored in one direction; resume; input that
must be skipped; capture; the chains' components; a threshold at which the graph is one-directional in its last bit; and the point
of it all -- a split over Butina clusters leaks pairs above the threshold across folds, a split over the components does not."""
import numpy as np
import pytest
import torch

from tests import _components_cases as CC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _dev(row_ptr, col):
    return torch.as_tensor(np.asarray(row_ptr), dtype=torch.int64).to(DEV), torch.as_tensor(np.asarray(col), dtype=torch.int32).to(DEV)


def _labels(row_ptr, col, n, **kw):
    from molkgnn_amd.readout import graph_components
    got = graph_components(*_dev(row_ptr, col), n, **kw)
    labels = got[0] if isinstance(got, tuple) else got
    assert labels.dtype == torch.int32 and tuple(labels.shape) == (n,)
    return (labels.cpu().numpy(), got[1]) if isinstance(got, tuple) else labels.cpu().numpy()


@pytest.mark.parametrize("n", CC.GRAPH_SIZES)
def test_labels_are_union_finds_within_the_round_bound(n):
    from molkgnn_amd.screening import components_reference
    for name, row_ptr, col in CC.graphs(n):
        labels, rounds = _labels(row_ptr, col, n, return_rounds=True)
        assert np.array_equal(labels, components_reference(row_ptr, col, n)), name
        assert rounds == CC.hook_compress(row_ptr, col, n)[1] <= CC.round_bound(n), (name, rounds)


def test_small_and_degenerate_graphs():
    from molkgnn_amd.screening import components_reference
    assert _labels([0, 0], [], 1).tolist() == [0]                                      # one vertex
    assert _labels([0, 1], [0], 1).tolist() == [0]                                     # ... with a self-loop
    assert _labels([0], [], 0).shape == (0,)
    n = 1000
    labels, rounds = _labels(np.zeros(n + 1, dtype=np.int64), [], n, return_rounds=True)           # isolated vertices, an empty col
    assert np.array_equal(labels, np.arange(n)) and rounds == 0
    # self-loops and duplicate edges are harmless; 4 -> 2 and 3 -> 4 are stored in one direction only
    row_ptr, col = CC.csr([(4, 2), (3, 4), (1, 1), (0, 5), (0, 5), (5, 0), (6, 6), (6, 6)], 7)
    assert _labels(row_ptr, col, 7).tolist() == components_reference(row_ptr, col, 7).tolist() == [0, 1, 2, 2, 2, 0, 6]
    # col may be longer than the lists
    assert _labels(row_ptr, np.concatenate([col, [99, -4]]), 7).tolist() == [0, 1, 2, 2, 2, 0, 6]


def test_a_bridge_stored_in_one_direction_joins_two_components():
    n = 600
    left = np.stack([np.arange(0, 299), np.arange(1, 300)], axis=1)                    # a path over 0 .. 299
    right = np.stack([np.arange(301, 600), np.arange(300, 599)], axis=1)               # a path over 300 .. 599, stored backwards
    apart = _labels(*CC.csr(np.concatenate([left, right]), n), n)
    assert (apart[:300] == 0).all() and (apart[300:] == 300).all()
    for bridge in ((450, 17), (17, 450)):                                               # u -> v stored, v -> u not
        joined = _labels(*CC.csr(np.concatenate([left, right, [bridge]]), n), n)
        assert not joined.any(), bridge


def test_the_bit_reversed_path_converges_inside_the_first_call():
    from molkgnn_amd import _lib
    from molkgnn_amd.readout import graph_components
    n = 4097
    name, row_ptr, col = CC.graphs(n)[3]
    assert name == f"path-bit_reversed-{n}"
    state = torch.full((4,), -1, dtype=torch.int32, device=DEV)
    labels = graph_components(*_dev(row_ptr, col), n, state=state)                     # the raw form: ONE call
    rounds, converged, skipped, zero = state.tolist()
    assert converged == 1 and skipped == 0 and zero == 0 and not bool(labels.any())
    assert rounds == CC.hook_compress(row_ptr, col, n)[1] <= CC.round_bound(n) < _lib.components_rounds(n)
    assert rounds >= 12                                                                 # (it is the worst graph known: log2 n + 1)


def test_resume_reaches_the_same_labels():
    from molkgnn_amd.readout import graph_components
    from molkgnn_amd.screening import components_reference
    n = 1025
    name, row_ptr, col = CC.graphs(n)[3]
    want = components_reference(row_ptr, col, n)
    need = CC.hook_compress(row_ptr, col, n)[1]
    assert need >= 4
    ptr, c = _dev(row_ptr, col)
    state = torch.empty(4, dtype=torch.int32, device=DEV)
    out = torch.empty(n, dtype=torch.int32, device=DEV)
    graph_components(ptr, c, n, out=out, state=state, _max_rounds=2)                   # two rounds only: not converged
    assert state.tolist() == [2, 0, 0, 0]
    part = out.cpu().numpy()
    assert not np.array_equal(part, want) and np.array_equal(part, CC.hook_compress(row_ptr, col, n, max_rounds=2)[0])
    calls, rounds = 1, 2
    for _ in range(need):                                                               # (a bounded loop: every call lowers a label or converges)
        graph_components(ptr, c, n, out=out, state=state, resume=True, _max_rounds=2)
        more, converged, skipped, _ = state.tolist()
        calls, rounds = calls + 1, rounds + more
        assert skipped == 0
        if converged:
            break
    assert converged and rounds == need and calls == need // 2 + 1 and np.array_equal(out.cpu().numpy(), want)
    # the eager form loops by itself and counts the same rounds
    labels, counted = _labels(row_ptr, col, n, return_rounds=True, _max_rounds=1)
    assert np.array_equal(labels, want) and counted == need
    # labels that cannot be labels are not used as an index on resume: replaced, and reported
    out.fill_(1 << 30)
    out[5] = -7
    graph_components(ptr, c, n, out=out, state=state, resume=True)
    assert state.tolist()[1:3] == [1, 1] and np.array_equal(out.cpu().numpy(), want)
    with pytest.raises(ValueError, match="resume"):
        graph_components(ptr, c, n, resume=True)


def test_input_that_cannot_be_indexed_is_skipped_and_raises():
    from molkgnn_amd.readout import graph_components
    n = 300
    edges = np.stack([np.arange(0, n - 1), np.arange(1, n)], axis=1)
    row_ptr, col = CC.csr(edges, n)
    buf = torch.full((n + 8,), -77, dtype=torch.int32, device=DEV)

    def run(bad_ptr, bad_col):
        buf.fill_(-77)
        with pytest.raises(ValueError, match="skipped"):
            graph_components(*_dev(bad_ptr, bad_col), n, out=buf[4:4 + n])
        torch.cuda.synchronize()
        host = buf.cpu().numpy()
        assert (host[:4] == -77).all() and (host[4 + n:] == -77).all()                 # only the labels were touched
        assert ((host[4:4 + n] >= 0) & (host[4:4 + n] <= np.arange(n))).all()          # and hold vertices

    for value in (n, -1, 1 << 30, -(1 << 31)):                                          # a column outside [0, n)
        bad = col.copy()
        bad[137] = value
        run(row_ptr, bad)
    bad = row_ptr.copy()
    bad[100] = bad[101] + 3                                                             # not monotone: segment 100 runs backwards
    run(bad, col)
    for value in (-5, 1 << 40):                                                         # a segment outside [0, row_ptr[n]]
        bad = row_ptr.copy()
        bad[200] = value
        run(bad, col)
    for value in (col.shape[0] + 1, -1):                                                # lists longer than col: refused before the launch
        bad = row_ptr.copy()
        bad[n] = value
        with pytest.raises(ValueError, match="length of col"):
            graph_components(*_dev(bad, col), n)
    # the same graph without the damage is fine in the same buffers
    assert not bool(graph_components(*_dev(row_ptr, col), n, out=buf[4:4 + n]).any())


def test_one_captured_call_follows_two_graphs_in_the_same_buffers():
    from molkgnn_amd.readout import graph_components
    from molkgnn_amd.screening import components_reference
    n = 257
    first, second = CC.graphs(n)[3], CC.graphs(n)[-1]
    room = max(first[2].shape[0], second[2].shape[0])
    ptr = torch.zeros(n + 1, dtype=torch.int64, device=DEV)
    col = torch.zeros(room, dtype=torch.int32, device=DEV)
    out = torch.empty(n, dtype=torch.int32, device=DEV)
    state = torch.empty(4, dtype=torch.int32, device=DEV)

    def load(graph):
        ptr.copy_(torch.from_numpy(graph[1]))
        col.fill_(-1)
        col[:graph[2].shape[0]] = torch.from_numpy(graph[2])

    load(first)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        graph_components(ptr, col, n, out=out, state=state)
        captured = torch.cuda.CUDAGraph()
        with torch.cuda.graph(captured, stream=side):
            graph_components(ptr, col, n, out=out, state=state)
    torch.cuda.current_stream(DEV).wait_stream(side)
    seen = []
    for graph in (second, first, second):
        load(graph)
        out.fill_(-9)
        state.fill_(-9)
        captured.replay()
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), components_reference(graph[1], graph[2], n)), graph[0]
        assert state.tolist() == [CC.hook_compress(graph[1], graph[2], n)[1], 1, 0, 0]
        seen.append(tuple(out.cpu().tolist()))
    assert seen[0] == seen[2] != seen[1]


def _off_diagonal(m):
    return int(m.sum() - m.diagonal().sum())


@pytest.mark.parametrize("H", CC.CHAIN_WIDTHS)
def test_the_chains_are_the_components_and_only_a_split_over_them_does_not_leak(H):
    from molkgnn_amd.sampling import cluster_split
    from molkgnn_amd.screening import (cluster_butina_embeddings, cluster_components_embeddings, components_reference, rank_order,
                                       split_leakage)
    emb, chain, _, margin = CC.chain_case(H)
    n, t = emb.shape[0], CC.CHAIN_MIN_SIM
    assert margin > 4
    e = torch.tensor(emb, device=DEV)
    scores = torch.from_numpy(np.random.default_rng(H).standard_normal(n).astype(np.float32)).to(DEV)
    scores[::17] = float("nan")
    got = cluster_components_embeddings(e, t, scores=scores)
    comp = got["component"].cpu().numpy()
    assert got["component"].dtype == torch.int64 and got["n_components"] == CC.N_CHAINS == len(set(comp.tolist()))
    smallest = np.array([np.nonzero(chain == chain[i])[0].min() for i in range(n)])
    assert np.array_equal(comp, smallest)                          # every label is the smallest row of its chain
    assert got["component_size"].tolist() == [CC.CHAIN_LENGTH] * CC.N_CHAINS
    assert np.array_equal(got["components"].cpu().numpy(), np.unique(smallest))
    # the lists are the self-join's, and the labels the union-symmetrised definition over embed_cosine's own matrix
    sim = CC.cosine_matrix(e, e)
    with np.errstate(invalid="ignore"):
        above = sim > np.float32(t)
    row_ptr, nbr = got["row_ptr"].cpu().numpy(), got["neighbour"].cpu().numpy()
    assert np.array_equal(np.diff(row_ptr), above.sum(axis=1)) and np.array_equal(nbr, np.nonzero(above)[1])
    assert np.array_equal(got["neighbour_sim"].cpu().numpy().view(np.int32), sim[above].view(np.int32))
    assert np.array_equal(got["neighbour_count"].cpu().numpy(), above.sum(axis=1)) and got["neighbour_count"].dtype == torch.int64
    assert np.array_equal(comp, components_reference(*CC.symmetrised(above), n))
    # the best member of every component: the first of its rows in rank_order(scores)
    ranked = rank_order(scores).cpu().numpy()
    best = [next(int(i) for i in ranked if comp[i] == c) for c in np.unique(smallest)]
    assert got["component_best"].tolist() == best
    assert np.array_equal(got["component_best_score"].cpu().numpy().view(np.int32), scores.cpu().numpy()[best].view(np.int32))
    # ids rename rows, not the grouping
    ids = torch.arange(n, device=DEV) * 3 + 1000
    named = cluster_components_embeddings(e, t, ids=ids)
    assert np.array_equal(named["component"].cpu().numpy(), 3 * comp + 1000) and named["components"].tolist() == (3 * np.unique(smallest) + 1000).tolist()
    # THE POINT: whole Butina clusters per fold still put linked rows into different folds; whole components do not
    butina = cluster_butina_embeddings(e, t)
    assert CC.N_CHAINS < butina["centroids"].numel() <= n // 2 and int(butina["leader"].min()) >= 0
    by_butina = cluster_split(butina["leader"], seed=0)
    by_component = cluster_split(got["component"], seed=0)
    leak_butina = split_leakage(got["row_ptr"], got["neighbour"], by_butina)
    leak_component = split_leakage(got["row_ptr"], got["neighbour"], by_component)
    nnz = int(got["row_ptr"][-1])
    assert int(leak_butina.sum()) == int(leak_component.sum()) == nnz == got["neighbour"].numel()
    assert _off_diagonal(leak_butina) > 0 and _off_diagonal(leak_component) == 0
    assert sorted(torch.bincount(by_component, minlength=3).tolist()) == [25, 25, 250]


@pytest.mark.parametrize("H", CC.CHAIN_WIDTHS)
def test_a_threshold_at_which_the_graph_is_one_directional_in_its_last_bit(H):
    """``sim(i, j)`` and ``sim(j, i)`` share their dot product and round their two scalings in different orders.  With the threshold
    at the smaller of such a pair the lists hold ``i -> j`` and not ``j -> i`` (or the reverse), and the components must still be
    those of the union.  (The widths are those of a real embedding; at ``H = 1`` every similarity is 1 or -1 up to its last bit and a
    threshold graph says nothing.)"""
    from molkgnn_amd.screening import cluster_components_embeddings, components_reference
    rows, _, _ = CC.tiling()
    n = 2 * rows + 37
    emb, _, _ = CC.float64_self_case(n, H)
    e = torch.tensor(emb, device=DEV)
    sim = CC.cosine_matrix(e, e)
    lower = np.minimum(sim, sim.T)
    uneven = np.argwhere((sim != sim.T) & ~np.isnan(lower))
    if uneven.shape[0] == 0:
        pytest.fail(f"no pair with S[i, j] != S[j, i] among the {n} rows of width {H}: the fixture does not exercise the union")
    i, j = uneven[np.argmax(lower[uneven[:, 0], uneven[:, 1]])]    # the closest such pair: the sparsest graph
    t = float(lower[i, j])
    with np.errstate(invalid="ignore"):
        above = sim > np.float32(t)
    assert above[i, j] != above[j, i]                               # stored in one direction only
    got = cluster_components_embeddings(e, t)
    assert np.array_equal(got["neighbour"].cpu().numpy(), np.nonzero(above)[1])
    comp = got["component"].cpu().numpy()
    assert np.array_equal(comp, components_reference(*CC.symmetrised(above), n)) and comp[i] == comp[j]
