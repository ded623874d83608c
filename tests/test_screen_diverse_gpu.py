"""``screening.screen_diverse`` and ``pick_diverse_embeddings`` end to end on the GPU: two small resident shards (short tails
included), a seeded model, a pool of 64.  The pool is ``screen``'s list bit for bit, its embeddings are the rows of the per-shard
matrices, and the picks and leaders are the host walk over ``mkgnn_embed_cosine``'s similarities of the pool."""
import numpy as np
import pytest
import torch

from tests._resident_library import bits as _bits, build_library

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
POOL, BATCH = 64, 16


@pytest.fixture(scope="module")
def library(tmp_path_factory):
    model, residents, _ = build_library(tmp_path_factory.mktemp("diverse"), DEV, counts=(70, 33), shard_seed=60,
                                        labels=lambda n: (torch.arange(n) % 3 == 0).float(), model_seed=2, batch_size=BATCH, num_layers=2)
    return model, residents


def _all_sims(e):
    from molkgnn_amd.readout import embedding_cosine
    n = e.shape[0]
    out = torch.empty(n, n, dtype=torch.float32, device=e.device)
    for a in range(0, n, 32):
        out[:, a:a + 32] = embedding_cosine(e, e[a:a + 32])
    return out.cpu().numpy()


def _median_off_diagonal(sim):
    """A threshold that splits the pool: the median similarity below the diagonal (as an exact float32 value)."""
    low = sim[np.tril_indices(len(sim), -1)]
    return float(np.sort(low[~np.isnan(low)])[low.size // 2])


@pytest.fixture(scope="module")
def screened(library):
    """One ``screen`` for the pool, one ``screen_diverse`` without a cap to read the pool's similarities from, and the threshold."""
    from molkgnn_amd.screening import screen, screen_diverse
    model, residents = library
    plain = screen(model, residents, POOL, BATCH, return_scores=True)
    first = screen_diverse(model, residents, POOL, BATCH, 0.5, pool=POOL)
    return plain, _median_off_diagonal(_all_sims(first["pool_emb"]))


def test_pool_is_the_screens_list_and_the_picks_are_the_host_walk(library, screened):
    from molkgnn_amd.screening import diverse_pick_reference, screen_diverse
    model, residents = library
    plain, max_sim = screened
    model.train()                                                  # it comes back in the mode it came in
    res = screen_diverse(model, residents, POOL, BATCH, max_sim, pool=POOL, return_embeddings=True)
    assert model.training
    model.eval()
    assert res["n_scored"] == 103 and res["pool_score"].shape == (POOL,)
    assert np.array_equal(_bits(res["pool_score"]), _bits(plain["top_score"]))
    assert torch.equal(res["pool_shard"], plain["top_shard"]) and torch.equal(res["pool_mol"], plain["top_mol"])
    assert bool((res["pool_shard"] == 0).any()) and bool((res["pool_shard"] == 1).any())
    # the pool's embeddings are the rows of the per-shard matrices (the short tails included: every row was written)
    embs = res["embeddings"]
    assert [tuple(e.shape) for e in embs] == [(70, 32), (33, 32)] and not any(bool(torch.isnan(e).any()) for e in embs)
    for j in range(POOL):
        assert np.array_equal(_bits(res["pool_emb"][j]), _bits(embs[int(res["pool_shard"][j])][int(res["pool_mol"][j])])), j
    # picks and leaders: the host walk over embed_cosine's similarities of the pool
    sim = _all_sims(res["pool_emb"])
    wp, wn, wl, ws = diverse_pick_reference(sim, max_sim, POOL)
    assert 1 < wn < POOL                                           # the threshold splits the pool: neither one cluster nor sixty-four
    assert res["picks"].dtype == torch.int64 and np.array_equal(res["picks"].cpu().numpy(), wp[:wn])
    assert res["pool_leader"].dtype == torch.int64 and np.array_equal(res["pool_leader"].cpu().numpy(), wl)
    assert np.array_equal(_bits(res["pool_leader_sim"]), ws.view(np.int32))        # (no cap: every row has a leader, no NaN)
    for name, source in (("top_score", "pool_score"), ("top_shard", "pool_shard"), ("top_mol", "pool_mol")):
        assert np.array_equal(_bits(res[name].float()), _bits(res[source][res["picks"]].float())), name
    sizes = res["cluster_size"].cpu().numpy()
    assert sizes.shape == (wn,) and (sizes >= 1).all() and sizes.sum() == int((wl >= 0).sum()) == POOL
    assert np.array_equal(sizes, np.array([(wl == p).sum() for p in wp[:wn]]))
    # capped: the same pool, the first k picks, and the rows nothing covers keep -1
    k = wn // 2
    capped = screen_diverse(model, residents, k, BATCH, max_sim, pool=POOL)
    cp, cn, cl, cs = diverse_pick_reference(sim, max_sim, k)
    assert cn == k and np.array_equal(capped["picks"].cpu().numpy(), wp[:k]) and np.array_equal(capped["pool_leader"].cpu().numpy(), cl)
    assert np.array_equal(_bits(capped["pool_score"]), _bits(plain["top_score"])) and "embeddings" not in capped
    assert (cl == -1).any() and capped["cluster_size"].sum().item() == int((cl >= 0).sum()) < POOL
    assert bool(torch.isnan(capped["pool_leader_sim"][torch.from_numpy(cl == -1).to(DEV)]).all())


def test_stored_embeddings_of_one_shard(library):
    from molkgnn_amd.screening import diverse_pick_reference, embed_resident, pick_diverse_embeddings, score_resident, topk_update_reference, empty_top
    model, residents = library
    model.eval()
    shard = residents[0]
    n = int(shard.n_molecules)
    emb = embed_resident(model, shard, BATCH)
    scores = score_resident(model, shard, BATCH).clone()
    scores[3] = float("nan")                                       # ranked last, wherever torch's sort would put it
    scores[5] = scores[4]                                          # a tie: the lower row first
    ids = (1000 + 7 * torch.arange(n, device=DEV)).to(torch.int32)
    max_sim = _median_off_diagonal(_all_sims(emb))
    host = scores.cpu().numpy()
    order = topk_update_reference(empty_top(n), host, np.arange(n, dtype=np.int32), n, 0)[2].astype(np.int64)
    assert order[-1] == 3 and list(order).index(4) + 1 == list(order).index(5)
    sim = _all_sims(emb[torch.from_numpy(order).to(DEV)])          # the similarities of the rows in rank order
    uncapped = diverse_pick_reference(sim, max_sim, n)[1]
    assert 2 < uncapped < n
    # by ids with and without a cap, then by row numbers
    for k, by_ids in ((n, True), (uncapped // 2, True), (n, False)):
        names = ids.cpu().numpy().astype(np.int64) if by_ids else np.arange(n)
        res = pick_diverse_embeddings(emb, scores, max_sim, k, ids=ids if by_ids else None)
        assert res["order"].dtype == torch.int64 and np.array_equal(res["order"].cpu().numpy(), order)
        wp, wn, wl, ws = diverse_pick_reference(sim, max_sim, k)
        assert wn == min(k, uncapped)
        assert res["picks"].dtype == torch.int64 and np.array_equal(res["picks"].cpu().numpy(), names[order[wp[:wn]]])
        assert np.array_equal(_bits(res["pick_score"]), host[order[wp[:wn]]].view(np.int32))
        want_leader = np.full(n, -1, dtype=np.int64)
        want_leader[order] = np.where(wl >= 0, names[order[np.maximum(wl, 0)]], -1)
        want_sim = np.empty(n, dtype=np.float32)
        want_sim[order] = ws
        assert np.array_equal(res["leader"].cpu().numpy(), want_leader)
        got_sim = res["leader_sim"].cpu().numpy()
        some = ~np.isnan(want_sim)
        assert np.array_equal(got_sim.view(np.int32)[some], want_sim.view(np.int32)[some]) and np.isnan(got_sim[~some]).all()
        assert some.all() == (k == n)
        sizes = res["cluster_size"].cpu().numpy()
        assert sizes.sum() == int((wl >= 0).sum()) and np.array_equal(sizes, np.array([(wl == p).sum() for p in wp[:wn]]))
