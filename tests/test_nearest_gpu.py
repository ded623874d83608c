"""Analogue search on the GPU: ``GNNModel.embed`` / ``screening.embed_resident`` against ``predict_tasks`` on the same gathered
batches (bits), ``screening.nearest`` against the numpy ranking (``topk_update_tasks_reference``, bits) and the float64 cosine
(``cosine_reference`` within ``cosine_bound``), the tensor and the shard form of the queries, and the stored-embedding route."""
import numpy as np
import pytest
import torch

from tests import _screen_cases as SC
from tests._resident_library import bits as _bits, build_library, eval_model

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
G = 32


def _host(topk):
    return (topk.top_score.cpu().numpy(), topk.top_shard.cpu().numpy(), topk.top_mol.cpu().numpy())


def _empty(T, K):
    from molkgnn_amd.screening import empty_top
    return tuple(np.stack([a] * T) for a in empty_top(K))


def _same_lists(a, b):
    return all(SC.same_list(tuple(x[t] for x in a), tuple(x[t] for x in b)) for t in range(len(a[0])))


@pytest.fixture(scope="module")
def library(tmp_path_factory):
    """The fixture shape of test_screen_tasks_gpu.py -- two resident shards (70 and 33 synthetic molecules), batch 32, 3-layer models
    with non-trivial running statistics: a nine-task and a one-task model -- a three-molecule query shard and, computed ONCE,
    eagerly, ``predict_tasks(data)[1]`` and ``embed(data)`` of both models on the gathered batches of each shard (live slots only)."""
    nine, residents, gathered = build_library(tmp_path_factory.mktemp("library_nearest"), DEV, counts=(70, 33, 3), shard_seed=40,
                                              labels=lambda n: (torch.arange(n) % 3 == 0).float(), model_seed=9, num_layers=3, task_dim=9)
    query_shard = residents.pop()
    models = {9: nine, 1: eval_model(DEV, 1, num_layers=3, task_dim=1)}

    tails = {T: [] for T in models}                                # predict_tasks(data)[1]
    embeds = {T: [] for T in models}                               # embed(data)
    for r in residents:
        parts, own = {T: [] for T in models}, {T: [] for T in models}
        for data, live in gathered(r):
            for T, model in models.items():
                emb = model.embed(data)
                assert emb.shape == (32, G) and emb.dtype == torch.float32
                own[T].append(emb[:live].clone())
                parts[T].append(model.predict_tasks(data)[1][:live].clone())
        for T in models:
            tails[T].append(torch.cat(parts[T]))
            embeds[T].append(torch.cat(own[T]))
    for model in models.values():
        model.train()
    return models, residents, tails, embeds, query_shard


@pytest.mark.parametrize("T", [9, 1])
def test_embed_is_the_embedding_of_predict_tasks(library, T):
    models, residents, tails, embeds, _ = library
    for j in range(2):
        assert embeds[T][j].shape == (residents[j].n_molecules, G)
        assert np.array_equal(_bits(embeds[T][j]), _bits(tails[T][j])), j
        assert not bool(torch.isnan(embeds[T][j]).any())
    assert models[T].training
    with pytest.raises(ValueError):
        models[T].embed(None)                                      # training mode: refused before the batch is looked at


@pytest.mark.parametrize("T", [9, 1])
def test_embed_resident_equals_embed_on_the_gathered_batches(library, T):
    from molkgnn_amd.screening import embed_resident
    models, residents, _, embeds, _ = library
    model = models[T]
    assert model.training
    emb = embed_resident(model, residents[0], 32)
    assert model.training                                          # handed back in the mode it came in
    assert emb.shape == (70, G) and emb.dtype == torch.float32 and emb.is_cuda
    assert not bool(torch.isnan(emb).any())
    assert np.array_equal(_bits(emb), _bits(embeds[T][0]))
    # another batch size: other batches, a full last one (70 = 2 * 35), the same molecules -- every slot is written
    assert not bool(torch.isnan(embed_resident(model, residents[0], 35)).any())
    out = torch.zeros(70, G, dtype=torch.float32, device=DEV)
    again = embed_resident(model, residents[0], 32, out=out)
    assert again is out and np.array_equal(_bits(out), _bits(emb))
    model.eval()
    embed_resident(model, residents[1], 32)
    assert not model.training
    model.train()
    with pytest.raises(ValueError):
        embed_resident(model, residents[0], 32, out=torch.zeros(70, device=DEV))
    with pytest.raises(ValueError):
        embed_resident(model, residents[0], 0)


def _five_queries(embeds):
    """The embeddings of molecules 0, 7 and 69 of shard 0 and molecule 32 of shard 1, and a zero vector; and where each lives."""
    homes = [(0, 0), (0, 7), (0, 69), (1, 32)]
    q = torch.stack([embeds[s][m] for s, m in homes] + [torch.zeros(G, device=DEV)]).contiguous()
    return q, homes


@pytest.mark.parametrize("k", [16, 200])
def test_nearest_ranks_two_shards_for_five_queries(library, k):
    from molkgnn_amd.screening import cosine_bound, cosine_reference, nearest, topk_update_tasks_reference
    models, residents, _, embeds, _ = library
    model, Q = models[9], 5
    queries, homes = _five_queries(embeds[9])
    r = nearest(model, queries, (s for s in residents), k, 32, return_sims=True)     # (a generator: shards one at a time)
    assert model.training
    assert r["n_searched"] == 103 and len(r["sims"]) == 2 and r["query_emb"] is queries
    want = _empty(Q, k)
    bounds = []
    for tag, sim in enumerate(r["sims"]):
        assert sim.shape == (residents[tag].n_molecules, Q) and not bool(torch.isnan(sim).any())
        s = sim.cpu().numpy()
        e, q = embeds[9][tag].cpu(), queries.cpu()
        err, bound = np.abs(s.astype(np.float64) - cosine_reference(e, q)), cosine_bound(e, q)
        assert (err <= bound).all(), (tag, float((err / bound).max()))
        bounds.append(bound)
        assert (s[:, 4].view(np.int32) == 0).all()                 # the zero query: +0.0 by bits
        want = topk_update_tasks_reference(want, s.T, np.arange(len(s), dtype=np.int32), len(s), tag)
    occupied = min(k, 103)
    assert r["top_sim"].shape == r["top_shard"].shape == r["top_mol"].shape == (Q, k)
    assert r["n_occupied"].tolist() == [occupied] * Q
    got = (r["top_sim"].cpu().numpy(), r["top_shard"].cpu().numpy(), r["top_mol"].cpu().numpy())
    assert _same_lists(got, want)
    everyone = [(0, m) for m in range(70)] + [(1, m) for m in range(33)]
    for t in range(Q):
        assert (got[1][t][occupied:] == -1).all() and (got[2][t][occupied:] == -1).all()     # empty slots stay (-inf, -1, -1)
        assert (SC.bits(got[0][t][occupied:]) == SC.bits([-np.inf])[0]).all()
        pairs = list(zip(got[1][t][:occupied].tolist(), got[2][t][:occupied].tolist()))
        if k == 200:
            assert sorted(pairs) == everyone
        if t < 4:
            # the query is in the library and is not excluded: its own pair is in its list at 1 to within the bound, and so is the
            # head of the list (cos(e, e) is not exactly 1, and a neighbour may tie with it inside the bound)
            shard, mol = homes[t]
            at = pairs.index((shard, mol))
            assert abs(float(got[0][t][at]) - 1.0) <= bounds[shard][mol, t]
            assert abs(float(got[0][t][0]) - 1.0) <= bounds[got[1][t][0]][got[2][t][0], t]
    assert pairs == everyone[:occupied]                            # the zero query's list: all ties, by shard and molecule
    assert any(got[2][t].tolist() != got[2][0].tolist() for t in range(1, Q))      # the queries rank differently


def test_queries_as_a_tensor_and_as_a_shard_agree(library):
    from molkgnn_amd.screening import embed_resident, nearest
    models, residents, _, _, query_shard = library
    model = models[9]
    assert query_shard.n_molecules == 3
    by_shard = nearest(model, query_shard, residents, 16, 32, return_sims=True)
    q = embed_resident(model, query_shard, 32)
    assert q.shape == (3, G) and np.array_equal(_bits(by_shard["query_emb"]), _bits(q))
    by_tensor = nearest(model, q, residents, 16, 32, return_sims=True)
    for name in ("top_sim", "top_shard", "top_mol"):
        assert by_shard[name].shape == (3, 16) and np.array_equal(_bits(by_shard[name]), _bits(by_tensor[name])), name
    assert by_shard["n_occupied"].tolist() == by_tensor["n_occupied"].tolist() == [16] * 3
    for a, b in zip(by_shard["sims"], by_tensor["sims"]):
        assert np.array_equal(_bits(a), _bits(b))
    assert model.training


def test_rank_embeddings_is_nearest_resident_without_the_network(library):
    from molkgnn_amd.screening import TopK, TopKTasks, embed_resident, nearest_resident, rank_embeddings
    models, residents, _, embeds, _ = library
    model, k = models[9], 16
    queries, _ = _five_queries(embeds[9])
    stored = embed_resident(model, residents[0], 32)
    live = TopKTasks(k, 5, DEV)
    sim = nearest_resident(model, residents[0], queries, 32, topk=live, shard_tag=3)
    assert sim.shape == (70, 5) and int(live.result()[3].min()) == k
    again = TopKTasks(k, 5, DEV)
    rank_embeddings(stored, queries, again, shard_tag=3, chunk=32)
    assert _same_lists(_host(again), _host(live))
    # two groups of queries, a list set per group: the lists of the corresponding columns; ids given, another chunk
    first, second = TopKTasks(k, 2, DEV), TopKTasks(k, 3, DEV)
    ids = torch.arange(70, dtype=torch.int32, device=DEV)
    rank_embeddings(stored, queries[:2], first, ids=ids, shard_tag=3, chunk=50)
    rank_embeddings(stored, queries[2:], second, ids=ids, shard_tag=3, chunk=4096)
    whole = _host(live)
    assert _same_lists(_host(first), tuple(a[:2] for a in whole)) and _same_lists(_host(second), tuple(a[2:] for a in whole))
    # what is refused on the GPU, before a launch: lists of another kind or number, a wrong output
    for bad in (TopK(k, DEV), TopKTasks(k, 4, DEV)):
        with pytest.raises(ValueError):
            nearest_resident(model, residents[0], queries, 32, topk=bad)
        with pytest.raises(ValueError):
            rank_embeddings(stored, queries, bad)
    with pytest.raises(ValueError):
        nearest_resident(model, residents[0], queries, 32, out=torch.zeros(70, 4, device=DEV))
    with pytest.raises(ValueError):
        rank_embeddings(stored, queries, again, ids=torch.arange(70, device=DEV))          # (int64 ids)
    assert model.training
