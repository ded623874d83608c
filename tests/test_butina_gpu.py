"""``screening.cluster_butina_embeddings`` and ``neighbour_counts`` on the GPU: the clustering against the host definition
(``butina_reference``) over ``mkgnn_embed_cosine``'s own float32 similarities -- exactly, every row, at the walk's tile edges -- a
planted series where Butina and the score-ordered leader walk must differ, the ``ids`` mapping, the cap, NaN rows, and the sliced
count."""
import numpy as np
import pytest
import torch

from tests import _count_cases as CC
from tests import _diverse_cases as DC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _agree(res, sim, min_sim, k):
    """The clustering is the host definition over ``sim``: indices equal, ``leader_sim`` by bit pattern apart from NaN."""
    from molkgnn_amd.screening import butina_reference
    n = sim.shape[0]
    centroids, n_clusters, leader, leader_sim, counts, order = butina_reference(sim, min_sim, k)
    for key in ("centroids", "neighbour_count", "leader", "cluster_size", "order"):
        assert res[key].dtype == torch.int64, key
    assert res["leader_sim"].dtype == torch.float32
    assert res["centroids"].cpu().tolist() == centroids[:n_clusters].tolist(), (n, min_sim, k)
    assert np.array_equal(res["neighbour_count"].cpu().numpy(), counts), (n, min_sim, k)
    assert np.array_equal(res["order"].cpu().numpy(), order), (n, min_sim, k)
    assert np.array_equal(res["leader"].cpu().numpy(), leader), (n, min_sim, k)
    got = res["leader_sim"].cpu().numpy()
    some = ~np.isnan(leader_sim)
    assert np.array_equal(_bits(got)[some], _bits(leader_sim)[some]) and np.isnan(got[~some]).all(), (n, min_sim, k)
    sizes = np.bincount(leader[leader >= 0], minlength=n)[centroids[:n_clusters]]
    assert np.array_equal(res["cluster_size"].cpu().numpy(), sizes) and (k < n_clusters or sizes.sum() == (leader >= 0).sum())
    return centroids[:n_clusters], leader


@pytest.mark.parametrize("H", DC.WIDTHS)
def test_clusters_are_the_definition_over_embed_cosines_own_similarities(H):
    from molkgnn_amd.screening import cluster_butina_embeddings
    for n in DC.sizes(H):
        e = torch.tensor(DC.float64_case(n, H)[0], device=DEV)         # (a copy: the cached array is read-only)
        sim = CC.cosine_matrix(e, e)
        centroids, leader = _agree(cluster_butina_embeddings(e, DC.MAX_SIM), sim, DC.MAX_SIM, n)
        assert (leader >= 0).all() and (H < 2 or n < 100 or 16 <= len(centroids) < n)
        # a cap: the clusters before it are unchanged, the rows no centroid before it covers get -1
        k = max(len(centroids) // 2, 1)
        capped = cluster_butina_embeddings(e, DC.MAX_SIM, k)
        cc, cl = _agree(capped, sim, DC.MAX_SIM, k)
        assert np.array_equal(cc, centroids[:k]) and np.array_equal(cl, np.where(np.isin(leader, centroids[:k]), leader, -1))
        assert k == len(centroids) or (cl == -1).any()


def _series(H, rng):
    """Eleven rows 0.08 rad apart on an arc -- neighbours up to five steps, cos 0.40 = 0.921 > 0.9 > cos 0.48 = 0.887, so the sixth
    row alone is a neighbour of all -- and an outlier 0.36 rad before the arc's first row: above 0.9 to the first two rows only (cos
    0.44 = 0.905, cos 0.52 = 0.868), and far from the centre (cos 0.76 = 0.725).  Every row at a scale of its own."""
    u = rng.standard_normal(H)
    u /= np.linalg.norm(u)
    v = rng.standard_normal(H)
    v -= (v @ u) * u
    v /= np.linalg.norm(v)
    angles = np.concatenate([0.08 * np.arange(11), [-0.36]])[:, None]
    rows = np.cos(angles) * u[None, :] + np.sin(angles) * v[None, :]
    return (rows * np.exp(rng.uniform(-2.0, 2.0, 12))[:, None]).astype(np.float32)


def test_butina_finds_the_centre_where_the_leader_walk_starts_at_the_outlier():
    from molkgnn_amd.screening import cluster_butina_embeddings, pick_diverse_embeddings
    H = 32
    rng = np.random.default_rng(41)
    place = rng.permutation(12)                                    # series row j sits at place[j]
    emb = np.empty((12, H), dtype=np.float32)
    emb[place] = _series(H, rng)
    score = np.empty(12, dtype=np.float32)
    score[place] = np.concatenate([np.arange(11), [100.0]])        # the outlier scores best; along the arc the last row does
    CENTRE, OUTLIER, FIRST, SECOND, LAST = (int(place[j]) for j in (5, 11, 0, 1, 10))
    e, s = torch.from_numpy(emb).to(DEV), torch.from_numpy(score).to(DEV)
    sim = CC.cosine_matrix(e, e)
    assert sorted(np.flatnonzero(sim[OUTLIER] > np.float32(0.9)).tolist()) == sorted([OUTLIER, FIRST, SECOND])
    res = cluster_butina_embeddings(e, 0.9, scores=s)
    _agree(res, sim, 0.9, 12)
    assert res["centroids"].tolist() == [CENTRE, OUTLIER] and res["cluster_size"].tolist() == [11, 1]
    assert res["neighbour_count"][CENTRE] == 11 and res["neighbour_count"][OUTLIER] == 3 and res["order"][0] == CENTRE
    assert res["leader"].tolist() == [OUTLIER if i == OUTLIER else CENTRE for i in range(12)]
    assert res["cluster_best"].tolist() == [LAST, OUTLIER] and res["cluster_best_score"].tolist() == [10.0, 100.0]
    # the score-ordered leader walk starts at the outlier, which takes the arc's first two rows with it
    walk = pick_diverse_embeddings(e, s, 0.9, 12)
    assert walk["picks"][0] == OUTLIER and CENTRE not in walk["picks"].tolist()
    assert walk["leader"][FIRST] == OUTLIER and walk["leader"][SECOND] == OUTLIER and walk["cluster_size"][0] == 3
    # a NaN score ranks last: the best member is the best of the others
    s2 = s.clone()
    s2[LAST] = float("nan")
    assert cluster_butina_embeddings(e, 0.9, scores=s2)["cluster_best"].tolist() == [int(place[9]), OUTLIER]


def test_ids_nan_rows_and_scores():
    from molkgnn_amd.screening import cluster_butina_embeddings, rank_order
    n, H = 300, 33
    emb = DC.clustered(n, H, 21).copy()
    NAN_ROW, INF_ROW, ZERO = 20, 30, 10
    emb[NAN_ROW, 7] = np.nan
    emb[INF_ROW, 32] = np.inf
    emb[ZERO] = 0.0
    e = torch.from_numpy(emb).to(DEV)
    sim = CC.cosine_matrix(e, e)
    rng = np.random.default_rng(3)
    score = rng.standard_normal(n).astype(np.float32)
    score[[4, 5]] = np.nan
    s = torch.from_numpy(score).to(DEV)
    plain = cluster_butina_embeddings(e, DC.MAX_SIM, scores=s)
    centroids, leader = _agree(plain, sim, DC.MAX_SIM, n)
    for bad in (NAN_ROW, INF_ROW):                                 # never a centroid, never in a cluster, a neighbour of nobody
        assert leader[bad] == -1 and bad not in centroids and not (leader == bad).any() and plain["neighbour_count"][bad] == 0
    assert leader[ZERO] == ZERO and plain["neighbour_count"][ZERO] == 0 and plain["order"][-3:].sort().values.tolist() == sorted([ZERO, NAN_ROW, INF_ROW])
    # the best member of every cluster: the first of its rows in rank_order(scores)
    ranked = rank_order(s).cpu().numpy()
    best = [int(next(r for r in ranked if leader[r] == c)) for c in centroids]
    assert plain["cluster_best"].cpu().tolist() == best
    assert np.array_equal(_bits(plain["cluster_best_score"].cpu().numpy()), _bits(score[best]))
    # ids: every row index in the result is replaced by the caller's name of it, -1 stays; order keeps the rows
    names = (1000 + 7 * np.arange(n)[::-1]).astype(np.int64)
    for ids in (torch.from_numpy(names).to(DEV), torch.from_numpy(names.astype(np.int32)).to(DEV)):
        named = cluster_butina_embeddings(e, DC.MAX_SIM, scores=s, ids=ids)
        assert named["centroids"].cpu().tolist() == names[centroids].tolist()
        assert np.array_equal(named["leader"].cpu().numpy(), np.where(leader >= 0, names[np.maximum(leader, 0)], -1))
        assert named["cluster_best"].cpu().tolist() == names[best].tolist()
        for key in ("neighbour_count", "leader_sim", "cluster_size", "order", "cluster_best_score"):
            assert np.array_equal(named[key].cpu().numpy(), plain[key].cpu().numpy(), equal_nan=True), key
    assert "cluster_best" not in cluster_butina_embeddings(e, DC.MAX_SIM)


def test_neighbour_counts_in_slices_is_the_unsliced_count(monkeypatch):
    from molkgnn_amd import screening
    from molkgnn_amd.readout import embedding_count_within
    n, R, H = 70, 173, 31
    pool = DC.clustered(n + R, H, 5)
    e, r = torch.from_numpy(pool[:n].copy()).to(DEV), torch.from_numpy(pool[n:].copy()).to(DEV)
    whole = screening.neighbour_counts(e, r, DC.MAX_SIM)
    assert whole.dtype == torch.int64 and tuple(whole.shape) == (n,) and int(whole.max()) >= 2
    assert torch.equal(whole, embedding_count_within(e, r, DC.MAX_SIM).long())
    with np.errstate(invalid="ignore"):
        assert np.array_equal(whole.cpu().numpy(), (CC.cosine_matrix(e, r) > np.float32(DC.MAX_SIM)).sum(axis=1))
    for size in (50, 172, 1):
        monkeypatch.setattr(screening, "NEIGHBOUR_SLICE", size)
        assert torch.equal(screening.neighbour_counts(e, r, DC.MAX_SIM), whole), size
