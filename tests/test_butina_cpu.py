"""Host side of the Butina clustering (``screening.butina_reference`` / ``cluster_butina_embeddings``, ``sampling.cluster_split``):
the numpy definition on planted cases against a brute-force loop, the cluster-based split's promises, and everything that is
refused before a launch."""
import numpy as np
import pytest
import torch

NAN = float("nan")


def _brute_butina(sim, bound, k_max):
    """Count, sort by (count descending, row), walk: one comparison at a time, ``sim[i, c]`` with the walked row as the row."""
    n = len(sim)
    counts = [sum(1 for s in row if not np.isnan(s) and s > bound) for row in sim]
    order = sorted(range(n), key=lambda i: (-counts[i], i))
    centroids, leader = [], [-1] * n
    for i in order:
        if np.isnan(sim[i, i]):
            continue
        for c in centroids:
            if not np.isnan(sim[i, c]) and sim[i, c] > bound:
                leader[i] = c
                break
        else:
            if len(centroids) < k_max:
                centroids.append(i)
                leader[i] = i
    return centroids, leader, counts, order


def _butina(sim, bound, k_max):
    from molkgnn_amd.screening import butina_reference
    centroids, n_clusters, leader, leader_sim, counts, order = butina_reference(sim, bound, k_max)
    n = len(sim)
    assert centroids.dtype == np.int32 and centroids.shape == (k_max,) and (centroids[n_clusters:] == -1).all()
    assert leader.dtype == np.int32 and leader.shape == (n,) and leader_sim.dtype == sim.dtype and leader_sim.shape == (n,)
    assert counts.dtype == np.int64 and order.dtype == np.int64 and sorted(order.tolist()) == list(range(n))
    for i in range(n):                                             # the similarity is the walked row's, with its centroid as the query
        if leader[i] >= 0:
            assert leader_sim[i] == sim[i, leader[i]]
        else:
            assert np.isnan(leader_sim[i])
    return centroids[:n_clusters].tolist(), leader.tolist(), counts.tolist(), order.tolist()


def test_butina_reference_on_planted_cases():
    for dtype in (np.float32, np.float64):
        # a dense series 1-2-3 with 2 between its ends, an outlier 0 beside 1, a NaN row 4, a singleton 5; 1 and 2 tie in their counts
        sim = np.full((6, 6), 0.1, dtype=dtype)
        np.fill_diagonal(sim, 1.0)
        for a, b, s in ((1, 2, 0.95), (2, 3, 0.95), (1, 3, 0.8), (0, 1, 0.92)):
            sim[a, b] = sim[b, a] = s
        sim[4, :] = sim[:, 4] = NAN
        got = _butina(sim, 0.9, 6)
        assert got == ([1, 3, 5], [1, 1, 1, 3, -1, 5], [2, 3, 3, 2, 0, 1], [1, 2, 0, 3, 5, 4])          # the tie goes to the lower row
        assert got == _brute_butina(sim, dtype(0.9), 6)
        # the threshold EQUAL to sim[0, 1]: strict, so 0 is no neighbour of 1 any more -- 2 is the densest row alone
        at = sim[0, 1]
        got = _butina(sim, at, 6)
        assert got == ([2, 0, 5], [0, 2, 2, 2, -1, 5], [1, 2, 3, 2, 0, 1], [2, 1, 3, 0, 5, 4]) and got == _brute_butina(sim, at, 6)
        below = np.nextafter(at, dtype(-1))
        assert _butina(sim, below, 6)[2] == [2, 3, 3, 2, 0, 1]                                          # ... and counts again just below it
        # a full list: the rows behind it are assigned where a centroid covers them, the others keep (-1, NaN)
        assert _butina(sim, 0.9, 1) == ([1], [1, 1, 1, -1, -1, -1], [2, 3, 3, 2, 0, 1], [1, 2, 0, 3, 5, 4])
        assert _butina(sim, 0.9, 2)[:2] == ([1, 3], [1, 1, 1, 3, -1, -1])
        # -0.0 against +0.0: neither lies above the other
        zeros = np.array([[1, 0.0], [-0.0, 1]], dtype=dtype)
        assert _butina(zeros, 0.0, 2)[:3] == ([0, 1], [0, 1], [1, 1]) and _butina(zeros, -0.0, 2)[:3] == ([0, 1], [0, 1], [1, 1])
        assert _butina(zeros, -1e-30, 2)[:3] == ([0], [0, 0], [2, 2])
        # a zero row (every similarity 0, its own included) counts nothing, comes last, and still becomes a centroid: the walk's rule
        assert _butina(np.array([[0.0, 0.0], [0.0, 1.0]], dtype=dtype), 0.5, 2)[:3] == ([1, 0], [0, 1], [0, 1])
        # matrices that are NOT symmetric, with ties and NaNs: the count reads row i, the walk reads sim[i, centroid]
        rng = np.random.default_rng(17)
        for n in (1, 2, 9, 40):
            m = np.round(rng.uniform(-1, 1, (n, n)), 1).astype(dtype)                                   # (one decimal: many equal elements)
            np.fill_diagonal(m, 1.0)
            if n >= 9:
                m[3, :] = m[:, 3] = NAN
                m[5, 7] = NAN
            for bound in (0.0, 0.5, float(m[n // 2, 0]) if not np.isnan(m[n // 2, 0]) else 0.3):
                for k_max in sorted({1, max(n // 3, 1), n}):
                    assert _butina(m, bound, k_max) == _brute_butina(m, dtype(bound), k_max), (n, bound, k_max)
    from molkgnn_amd.screening import butina_reference
    for bad in (np.zeros((2, 3)), np.zeros(4), np.zeros((2, 2), dtype=np.int32)):
        with pytest.raises(ValueError):
            butina_reference(bad, 0.5, 1)
    for k in (0, 3):
        with pytest.raises(ValueError):
            butina_reference(np.eye(2), 0.5, k)
    with pytest.raises(ValueError):
        butina_reference(np.eye(2), NAN, 1)
    assert butina_reference(torch.eye(3), 0.5, 3)[1] == 3          # tensors are taken as they are


def _check_split(leader, fractions, seed):
    from molkgnn_amd.sampling import cluster_split
    folds = cluster_split(leader, fractions, seed)
    lead = torch.as_tensor(leader).long().cpu()
    n = lead.numel()
    assert folds.dtype == torch.int64 and tuple(folds.shape) == (n,) and folds.device == torch.as_tensor(leader).device
    f = folds.cpu()
    assert n == 0 or (0 <= int(f.min()) and int(f.max()) < len(fractions))
    sizes = {}
    for name in set(lead[lead >= 0].tolist()):
        members = f[lead == name]
        assert len(set(members.tolist())) == 1, name               # no cluster straddles folds
        sizes[name] = len(members)
    largest = max(list(sizes.values()) + [1 if bool((lead < 0).any()) else 0])
    total = float(sum(fractions))
    for j, share in enumerate(fractions):                          # within the largest cluster's size of its target
        assert abs(int((f == j).sum()) - share / total * n) <= largest, (j, fractions, seed)
    assert torch.equal(cluster_split(leader, fractions, seed), folds)          # the same arguments, the same folds
    return f


def test_cluster_split_keeps_clusters_whole_and_folds_near_their_targets():
    from molkgnn_amd.sampling import cluster_split
    rng = np.random.default_rng(23)
    n = 600
    centres = rng.choice(n, 70, replace=False)
    leader = centres[rng.integers(0, 70, n)]                       # clusters of uneven sizes, named by arbitrary rows
    leader[rng.choice(n, 50, replace=False)] = -1                  # and 50 rows without a cluster
    leader[:40] = int(centres[0])                                  # one large cluster
    lead = torch.from_numpy(leader)
    seen = set()
    for seed in (0, 1, 2):
        for fractions in ((0.8, 0.1, 0.1), (0.5, 0.5), (1.0,), (3, 1, 1, 1), (0.9, 0.0, 0.1)):
            f = _check_split(lead, fractions, seed)
            if fractions == (0.9, 0.0, 0.1):
                assert not bool((f == 1).any())                    # a fold with no share gets nothing
            if fractions == (0.8, 0.1, 0.1):
                seen.add(tuple(f.tolist()))
                alone = f[lead < 0]                                # -1 rows are singletons: they are not kept together
                assert len(set(alone.tolist())) == 3
    assert len(seen) == 3                                          # another seed, another split
    assert torch.equal(cluster_split(lead.int(), (0.8, 0.1, 0.1), 1), cluster_split(lead, (0.8, 0.1, 0.1), 1))
    # names need not be rows: ids far beyond n work alike
    assert torch.equal(cluster_split(torch.where(lead >= 0, lead * 1000 + 7, lead), (0.8, 0.1, 0.1), 1), cluster_split(lead, (0.8, 0.1, 0.1), 1))
    # every row alone, one cluster, nothing
    _check_split(torch.full((30,), -1), (0.8, 0.1, 0.1), 0)
    assert cluster_split(torch.zeros(30, dtype=torch.int64), (0.8, 0.1, 0.1), 5).tolist() == [0] * 30
    assert tuple(cluster_split(torch.zeros(0, dtype=torch.int64)).shape) == (0,)
    two = cluster_split(torch.tensor([0, 0, 2, 2]), (0.5, 0.5), 3)
    assert two[0] == two[1] and two[2] == two[3] and two[0] != two[2]
    for bad in (torch.zeros(4), torch.zeros(2, 2, dtype=torch.int64), torch.tensor([0, -2])):
        with pytest.raises(ValueError):
            cluster_split(bad)
    for fractions in ((), (0.0, 0.0), (-0.1, 1.1), (NAN, 1.0), (float("inf"), 1.0)):
        with pytest.raises(ValueError):
            cluster_split(torch.tensor([0, 0, 1]), fractions)


def test_rejections_before_any_launch(monkeypatch):
    """A NaN or infinite threshold, no rows or more than 2^20, ``k`` beyond the rows, wrong shapes and dtypes, CPU tensors:
    ``ValueError`` before the library is even loaded."""
    from molkgnn_amd import _lib, screening

    def no_load():
        raise AssertionError("the library was loaded before the refusal")

    monkeypatch.setattr(_lib, "load", no_load)
    emb, scores = torch.zeros(10, 32), torch.zeros(10)
    for bad in (NAN, float("inf"), float("-inf")):
        with pytest.raises(ValueError, match="finite"):
            screening.cluster_butina_embeddings(emb, bad)
    with pytest.raises(ValueError, match="GPU"):
        screening.cluster_butina_embeddings(emb, 0.9)
    with pytest.raises(ValueError, match="GPU"):
        screening.cluster_butina_embeddings(emb, 0.9, 4, scores, torch.arange(10))
    with pytest.raises(ValueError, match="rows"):
        screening.cluster_butina_embeddings(torch.zeros(0, 32), 0.9)
    with pytest.raises(ValueError, match="rows"):
        screening.cluster_butina_embeddings(torch.zeros(1, 1).expand((1 << 20) + 1, 1), 0.9)
    for args in ((emb.double(), 0.9), (emb[0], 0.9), (torch.zeros(10, 0), 0.9), (emb, 0.9, 0), (emb, 0.9, 11), (emb, 0.9, 4, scores.double()),
                 (emb, 0.9, 4, scores[:9]), (emb, 0.9, 4, None, torch.zeros(10)), (emb, 0.9, 4, None, torch.zeros(9, dtype=torch.int32)),
                 (emb.numpy(), 0.9)):
        with pytest.raises(ValueError):
            screening.cluster_butina_embeddings(*args)
    assert screening.BUTINA_MAX_ROWS == _lib.DIVERSE_MAX_ROWS == _lib.MAX_COSINE_MAX_REFS and screening.NEIGHBOUR_SLICE == _lib.MAX_COSINE_MAX_REFS
