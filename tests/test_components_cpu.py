"""Linked components without a GPU: ``components_reference``; the operator's scheme restated in numpy (snapshot hook, full
compress) against it, and its rounds against the bound the operator's fixed round count rests on; ``split_leakage`` against a
double loop; and, on the chain fixture, what this is all for -- a ``cluster_split`` over Butina clusters leaks pairs above the
threshold across folds, one over the linked components does not."""
import numpy as np
import pytest
import torch

from tests import _components_cases as CC


def test_components_reference_on_small_graphs():
    from molkgnn_amd.screening import components_reference
    assert components_reference([0], [], 0).shape == (0,)
    assert components_reference([0, 0], [], 1).tolist() == [0]
    assert components_reference([0, 0, 0, 0], [], 3).tolist() == [0, 1, 2]
    # 4 -> 2 and 3 -> 4 stored in one direction only; a self-loop on 1; 0 -> 5 twice
    row_ptr, col = CC.csr([(4, 2), (3, 4), (1, 1), (0, 5), (0, 5)], 7)
    got = components_reference(row_ptr, col, 7)
    assert got.dtype == np.int32 and got.tolist() == [0, 1, 2, 2, 2, 0, 6]
    assert components_reference(torch.from_numpy(row_ptr), torch.from_numpy(col), 7).tolist() == got.tolist()
    for bad_ptr, bad_col, n in (([0, 1], [1], 1), ([0, 1], [-1], 1), ([0, 2, 1], [0, 0], 2), ([0, 3], [0], 1), ([0, 0], [], 2), ([-1, 0], [], 1)):
        with pytest.raises(ValueError):
            components_reference(bad_ptr, bad_col, n)


@pytest.mark.parametrize("n", CC.GRAPH_SIZES)
def test_hook_and_compress_reaches_union_find_within_the_round_bound(n):
    from molkgnn_amd.screening import components_reference
    worst = 0
    for name, row_ptr, col in CC.graphs(n):
        labels, rounds, converged = CC.hook_compress(row_ptr, col, n)
        assert converged and np.array_equal(labels, components_reference(row_ptr, col, n)), name
        assert rounds <= CC.round_bound(n), (name, rounds)
        worst = max(worst, rounds)
        if name.startswith(("path", "star", "tree")):
            assert not labels.any(), name                          # one component, named by vertex 0
    assert worst >= 1
    # a capped run has not converged where more rounds were needed, and is a valid intermediate state: every label is a member of
    # its vertex's component, no larger than the vertex
    name, row_ptr, col = CC.graphs(n)[3]                           # the bit-reversed path
    full, rounds, _ = CC.hook_compress(row_ptr, col, n)
    part, _, converged = CC.hook_compress(row_ptr, col, n, max_rounds=1)
    assert rounds >= 1 and not converged
    assert (part <= np.arange(n)).all() and np.array_equal(full[part], full)


def test_bit_reversed_path_needs_about_log_n_rounds():
    """The worst graph known: its changing rounds grow with log2 n -- so the fixed count cannot be a small constant -- and stay at
    half the bound."""
    seen = []
    for n in (17, 257, 4097):
        name, row_ptr, col = CC.graphs(n)[3]
        assert name == f"path-bit_reversed-{n}"
        seen.append(CC.hook_compress(row_ptr, col, n)[1])
        assert seen[-1] <= CC.round_bound(n) // 2 + 1
    assert seen[0] < seen[1] < seen[2]


def test_split_leakage_is_the_double_loop():
    from molkgnn_amd.screening import split_leakage
    rng = np.random.default_rng(11)
    n, R, F = 37, 29, 4
    above = rng.uniform(size=(n, R)) < 0.2
    above[5] = False
    row_ptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(above.sum(axis=1), out=row_ptr[1:])
    nbr = np.nonzero(above)[1].astype(np.int32)
    folds, ref_folds = rng.integers(0, F, size=n), rng.integers(0, F - 1, size=R)
    folds[0] = F - 1
    want = np.zeros((F, F), dtype=np.int64)
    for i in range(n):
        for r in np.nonzero(above[i])[0]:
            want[folds[i], ref_folds[r]] += 1
    got = split_leakage(torch.from_numpy(row_ptr), torch.from_numpy(nbr), torch.from_numpy(folds), torch.from_numpy(ref_folds))
    assert got.dtype == torch.int64 and tuple(got.shape) == (F, F) and np.array_equal(got.numpy(), want) and int(got.sum()) == nbr.shape[0]
    # a self-join: the references' folds are the rows'
    square = rng.uniform(size=(n, n)) < 0.15
    ptr2 = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(square.sum(axis=1), out=ptr2[1:])
    nbr2 = np.nonzero(square)[1].astype(np.int32)
    want2 = np.zeros((F, F), dtype=np.int64)
    for i, j in zip(*np.nonzero(square)):
        want2[folds[i], folds[j]] += 1
    got2 = split_leakage(torch.from_numpy(ptr2), torch.from_numpy(nbr2), torch.from_numpy(folds).int())
    assert np.array_equal(got2.numpy(), want2)
    empty = split_leakage(torch.zeros(n + 1, dtype=torch.int64), torch.zeros(0, dtype=torch.int32), torch.from_numpy(folds))
    assert tuple(empty.shape) == (F, F) and not empty.any()
    t = torch.from_numpy
    for args in ((t(row_ptr)[:-1], t(nbr), t(folds)), (t(row_ptr).float(), t(nbr), t(folds)), (t(row_ptr), t(nbr).float(), t(folds)),
                 (t(row_ptr), t(nbr), t(folds).float()), (t(row_ptr), t(nbr)[:-1], t(folds), t(ref_folds)),
                 (t(row_ptr), t(nbr), t(folds), t(ref_folds)[:5]), (t(row_ptr), t(nbr), t(folds) - 1, t(ref_folds)),
                 (t(row_ptr), t(nbr), t(folds), t(ref_folds).float()), (t(row_ptr) + 1, t(nbr), t(folds), t(ref_folds))):
        with pytest.raises(ValueError):
            split_leakage(*args)


@pytest.mark.parametrize("H", CC.CHAIN_WIDTHS)
def test_on_the_chains_a_butina_split_leaks_and_a_component_split_does_not(H):
    from molkgnn_amd.sampling import cluster_split
    from molkgnn_amd.screening import butina_reference, components_reference, neighbours_reference, split_leakage
    emb, chain, sim, margin = CC.chain_case(H)
    n = emb.shape[0]
    assert n == CC.N_CHAINS * CC.CHAIN_LENGTH and margin > 4      # float32 inside its bound decides every pair as float64 does
    row_ptr, nbr, _ = neighbours_reference(sim, CC.CHAIN_MIN_SIM)
    linked = sim > CC.CHAIN_MIN_SIM
    assert not (linked & (chain[:, None] != chain[None, :])).any() and linked.diagonal().all()
    # the linked components are the chains, each named by its smallest row
    comp = components_reference(row_ptr, nbr, n)
    assert len(set(comp.tolist())) == CC.N_CHAINS
    for c in range(CC.N_CHAINS):
        members = np.nonzero(chain == c)[0]
        assert (comp[members] == members.min()).all() and members.shape[0] == CC.CHAIN_LENGTH
    labels, rounds, converged = CC.hook_compress(row_ptr, nbr, n)
    assert converged and np.array_equal(labels, comp) and rounds <= CC.round_bound(n)
    # Butina cuts every chain into several clusters ...
    _, n_clusters, leader, _, _, _ = butina_reference(sim, CC.CHAIN_MIN_SIM, n)
    assert (leader >= 0).all() and CC.N_CHAINS < n_clusters <= n // 2
    # ... so a split over them puts linked rows into different folds; over the components, none
    t = torch.from_numpy
    by_butina = cluster_split(t(leader.astype(np.int64)), seed=0)
    by_component = cluster_split(t(comp.astype(np.int64)), seed=0)
    leak_butina = split_leakage(t(row_ptr), t(nbr), by_butina)
    leak_component = split_leakage(t(row_ptr), t(nbr), by_component)
    assert int(leak_butina.sum()) == int(leak_component.sum()) == nbr.shape[0]
    off = lambda m: int(m.sum() - m.diagonal().sum())              # noqa: E731
    assert off(leak_butina) > 0 and off(leak_component) == 0
    assert sorted(torch.bincount(by_component, minlength=3).tolist()) == [25, 25, 250]
