"""``screening.select_maxmin`` end to end on the GPU: two small resident shards (short tails included), seeded models, batches of
32.  The picks are ``pick_maxmin_embeddings`` over the concatenated ``embed_resident`` outputs and map to the right (shard, molecule);
a ``ResidentShard`` serves as a deck; a nine-task model is accepted; a library beyond the limit is refused before any pass."""
import numpy as np
import pytest
import torch

from tests._resident_library import bits as _bits, build_library, eval_model

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BATCH, K = 32, 12
COUNTS = (70, 45)


@pytest.fixture(scope="module")
def library(tmp_path_factory):
    model, residents, _ = build_library(tmp_path_factory.mktemp("maxmin"), DEV, counts=COUNTS, shard_seed=80,
                                        labels=lambda n: (torch.arange(n) % 3 == 0).float(), model_seed=3, batch_size=BATCH, num_layers=2)
    return model, residents


def test_picks_are_the_selection_over_the_concatenated_embeddings(library):
    from molkgnn_amd.screening import embed_resident, pick_maxmin_embeddings, select_maxmin
    model, residents = library
    model.train()                                                  # it comes back in the mode it came in
    res = select_maxmin(model, residents, K, BATCH)
    assert model.training
    model.eval()
    embs = [embed_resident(model, r, BATCH) for r in residents]
    emb = torch.cat(embs)
    assert res["n_embedded"] == sum(COUNTS) == emb.shape[0] and not bool(torch.isnan(emb).any())
    want = pick_maxmin_embeddings(emb, K)
    assert res["n_picks"] == want["n_picks"] == K
    assert torch.equal(res["picks"], want["picks"]) and np.array_equal(_bits(res["pick_sim"]), _bits(want["pick_sim"]))
    assert torch.equal(res["cluster_size"], want["cluster_size"]) and int(res["cluster_size"].sum()) == sum(COUNTS)
    assert torch.equal(torch.cat(res["leader"]), want["leader"]) and [t.shape[0] for t in res["leader"]] == list(COUNTS)
    assert np.array_equal(_bits(torch.cat(res["leader_sim"])), _bits(want["leader_sim"]))
    assert res["top_shard"].dtype == res["top_mol"].dtype == torch.int32
    assert bool((res["top_shard"] == 0).any()) and bool((res["top_shard"] == 1).any())
    for t in range(K):                                             # (shard, molecule) name the row that was picked
        shard, mol = int(res["top_shard"][t]), int(res["top_mol"][t])
        assert 0 <= mol < COUNTS[shard] and int(res["picks"][t]) == sum(COUNTS[:shard]) + mol
        assert np.array_equal(_bits(embs[shard][mol]), _bits(emb[int(res["picks"][t])]))
    # a stop ends the walk early and is handed on
    at = float(res["pick_sim"][K // 2])
    fewer = select_maxmin(model, residents, K, BATCH, stop_sim=at)
    assert 1 <= fewer["n_picks"] <= K // 2 and torch.equal(fewer["picks"], res["picks"][:fewer["n_picks"]])


def test_a_resident_shard_serves_as_the_deck(library):
    from molkgnn_amd.screening import embed_resident, pick_maxmin_embeddings, select_maxmin
    model, residents = library
    res = select_maxmin(model, residents[:1], K, BATCH, deck=residents[1])
    emb, deck = embed_resident(model, residents[0], BATCH), embed_resident(model, residents[1], BATCH)
    want = pick_maxmin_embeddings(emb, K, deck=deck)
    assert np.array_equal(_bits(res["deck_emb"]), _bits(deck))
    assert torch.equal(res["picks"], want["picks"]) and np.array_equal(_bits(res["pick_sim"]), _bits(want["pick_sim"]))
    assert np.array_equal(_bits(res["deck_sim"][0]), _bits(want["deck_sim"])) and bool((res["top_shard"] == 0).all())
    assert float(res["pick_sim"][0]) == float(want["deck_sim"].min()) > -1.0      # the walk starts at what the deck lacks most
    same = select_maxmin(model, residents[:1], K, BATCH, deck=deck)              # ... and so does the tensor it embeds to
    assert torch.equal(same["picks"], res["picks"])
    with pytest.raises(ValueError, match="deck"):
        select_maxmin(model, residents[:1], K, BATCH, deck=deck[:, :31])
    with pytest.raises(ValueError, match="deck"):
        select_maxmin(model, residents[:1], K, BATCH, deck=deck.cpu())


def test_a_nine_task_model_is_accepted(library):
    from molkgnn_amd.screening import embed_resident, pick_maxmin_embeddings, select_maxmin
    _, residents = library
    nine = eval_model(DEV, 4, num_layers=2, task_dim=9)
    res = select_maxmin(nine, residents, K, BATCH)
    want = pick_maxmin_embeddings(torch.cat([embed_resident(nine, r, BATCH) for r in residents]), K)
    assert res["n_picks"] == K and torch.equal(res["picks"], want["picks"])


def test_a_library_beyond_the_limit_is_refused_before_any_pass(library, monkeypatch):
    from molkgnn_amd import screening
    model, residents = library

    def no_pass(*args, **kwargs):
        raise AssertionError("a shard was embedded before the refusal")

    monkeypatch.setattr(screening, "embed_resident", no_pass)
    monkeypatch.setattr(screening, "MAXMIN_MAX_ROWS", sum(COUNTS) - 1)
    with pytest.raises(ValueError, match="at most"):
        screening.select_maxmin(model, residents, K, BATCH)
    with pytest.raises(ValueError, match="at most"):
        screening.select_maxmin(model, iter(residents), K, BATCH, deck=residents[1])
    with pytest.raises(ValueError, match="k = "):                  # more picks than molecules
        screening.select_maxmin(model, residents[1:], COUNTS[1] + 1, BATCH)
