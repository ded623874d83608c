"""The novelty filter end to end on the GPU: ``screening.reference_similarity_resident`` against ``embedding_max_cosine`` on the
eagerly gathered batches (bits), and ``screening.screen_novel`` against ``score_resident``'s scores (bits), the numpy compaction and
ranking (``select_rows_reference``, ``topk_update_reference``) and ``screen`` itself, in both directions of the filter."""
import numpy as np
import pytest
import torch

from tests import _screen_cases as SC
from tests._resident_library import bits as _bits, build_library, eval_model

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
G = 32
COUNTS = (70, 45)


@pytest.fixture(scope="module")
def library(tmp_path_factory):
    """Two resident shards (70 and 45 synthetic molecules: batch 32 leaves short tails of 6 and 13), a three-molecule shard of "known
    actives", a one-task and a nine-task model; computed ONCE, eagerly: ``embed(data)`` of both models on the gathered batches, and
    the references -- the embeddings of six library molecules plus random rows, 40 in all, per model."""
    one, residents, gathered = build_library(tmp_path_factory.mktemp("library_novel"), DEV, counts=(*COUNTS, 3), shard_seed=60,
                                             labels=lambda n: (torch.arange(n) % 3 == 0).float(), model_seed=4, num_layers=3, task_dim=1)
    known = residents.pop()
    models = {1: one, 9: eval_model(DEV, 9, num_layers=3, task_dim=9)}
    embeds = {T: [] for T in models}
    for r in residents:
        parts = {T: [] for T in models}
        for data, live in gathered(r):
            for T, model in models.items():
                parts[T].append(model.embed(data)[:live].clone())
        for T in models:
            embeds[T].append(torch.cat(parts[T]))
    homes = [(0, 0), (0, 33), (0, 69), (1, 5), (1, 32), (1, 44)]
    gen = torch.Generator(device=DEV).manual_seed(8)
    refs = {}
    for T in models:
        own = torch.stack([embeds[T][s][m] for s, m in homes])
        scale = float(embeds[T][0].abs().mean())
        refs[T] = torch.cat([own, torch.randn(34, G, generator=gen, device=DEV) * scale]).contiguous()
    for model in models.values():
        model.train()
    return models, residents, embeds, refs, homes, known


@pytest.mark.parametrize("T", [1, 9])
def test_reference_similarity_resident_equals_the_eager_batches(library, T):
    from molkgnn_amd.readout import embedding_max_cosine
    from molkgnn_amd.screening import cosine_bound, reference_similarity_resident
    models, residents, embeds, refs, homes, _ = library
    model = models[T]
    for j, r in enumerate(residents):
        sim, arg = reference_similarity_resident(model, r, refs[T], 32)
        assert model.training                                      # handed back in the mode it came in
        assert sim.shape == arg.shape == (COUNTS[j],) and sim.dtype == torch.float32 and arg.dtype == torch.int32
        want_sim, want_arg = embedding_max_cosine(embeds[T][j], refs[T])
        assert np.array_equal(_bits(sim), _bits(want_sim)) and np.array_equal(arg.cpu().numpy(), want_arg.cpu().numpy())
        assert not bool(torch.isnan(sim).any()) and int(arg.min()) >= 0
        bound = cosine_bound(embeds[T][j].cpu(), refs[T].cpu())
        for at, (s, m) in enumerate(homes):                        # a molecule that is a reference finds itself, at 1 within the bound
            if s == j:
                assert abs(float(sim[m]) - 1.0) <= bound[m, at]
    out = (torch.zeros(70, device=DEV), torch.zeros(70, dtype=torch.int32, device=DEV))
    sim2, arg2 = reference_similarity_resident(model, residents[0], refs[T], 35, out=out)      # (another batch size: 70 = 2 * 35)
    assert sim2 is out[0] and arg2 is out[1] and not bool(torch.isnan(sim2).any()) and int(arg2.min()) >= 0
    with pytest.raises(ValueError):
        reference_similarity_resident(model, residents[0], refs[T], 32, out=(out[0], out[1].long()))
    with pytest.raises(ValueError):
        reference_similarity_resident(model, residents[0], refs[T][:, :G - 1], 32)


def _expected(scores, sims, k, lo, hi):
    """The lists ``topk_update_reference`` makes of the per-shard scores, batch by batch as the pass feeds them, restricted by
    ``select_rows_reference`` to the molecules whose reference similarity passes; and how many passed."""
    from molkgnn_amd.screening import empty_top, select_rows_reference, topk_update_reference
    want, kept = empty_top(k), 0
    for tag, (s, key) in enumerate(zip(scores, sims)):
        for a in range(0, len(s), 32):
            ids = np.arange(a, min(a + 32, len(s)), dtype=np.int32)
            ks, ki, n = select_rows_reference(s[a:a + 32], ids, key[a:a + 32], len(ids), lo, hi)
            want = topk_update_reference(want, ks, ki, n, tag)
            kept += n
    return want, kept


def _threshold(sims):
    """A similarity between two measured ones, near the median: about half of the molecules lie below it."""
    flat = np.sort(np.concatenate(sims))
    return float((flat[len(flat) // 2 - 1] + flat[len(flat) // 2]) / 2)


@pytest.mark.parametrize("k", [16, 200])
def test_screen_novel_ranks_the_molecules_that_pass(library, k):
    from molkgnn_amd.screening import cosine_bound, score_resident, screen_novel
    models, residents, embeds, refs, homes, _ = library
    model = models[1]
    sims = [torch_sim.cpu().numpy() for torch_sim in
            (screen_novel(model, residents, 4, 32, refs[1], max_sim=float("inf"), return_scores=True)["ref_sims"])]
    c = _threshold(sims)
    r = screen_novel(model, (s for s in residents), k, 32, refs[1], max_sim=c, return_scores=True)      # (a generator of shards)
    assert model.training
    assert r["n_scored"] == sum(COUNTS) and r["ref_emb"] is refs[1] and len(r["scores"]) == len(r["ref_sims"]) == len(r["refs"]) == 2
    scores = []
    for j, res in enumerate(residents):
        assert np.array_equal(_bits(r["scores"][j]), _bits(score_resident(model, res, 32)))          # bit for bit score_resident's
        assert np.array_equal(_bits(r["ref_sims"][j]), sims[j].view(np.int32))
        scores.append(r["scores"][j].cpu().numpy())
    share = float(np.mean(np.concatenate(sims) <= np.float32(c)))
    assert 0.25 <= share <= 0.75, share
    want, kept = _expected(scores, sims, k, -np.inf, c)
    assert r["n_kept"] == kept == int(round(share * sum(COUNTS)))
    occupied = min(k, kept)
    got = (r["top_score"].cpu().numpy(), r["top_shard"].cpu().numpy(), r["top_mol"].cpu().numpy())
    assert len(got[0]) == occupied and SC.same_list(got, tuple(a[:occupied] for a in want))
    if k == 200:
        assert occupied == kept < k                                # more slots than survivors: every survivor, no one else
    # the nearest reference of every hit: the per-shard values at the hits
    refs_host = [a.cpu().numpy() for a in r["refs"]]
    assert np.array_equal(r["top_ref_sim"].cpu().numpy().view(np.int32),
                          np.array([sims[s][m] for s, m in zip(got[1], got[2])], dtype=np.float32).view(np.int32))
    assert np.array_equal(r["top_ref"].cpu().numpy(), np.array([refs_host[s][m] for s, m in zip(got[1], got[2])], dtype=np.int32))
    assert (r["top_ref_sim"].cpu().numpy() <= np.float32(c)).all()
    # a library molecule that is itself a reference is absent when c < 1 - bound
    hits = set(zip(got[1].tolist(), got[2].tolist()))
    for at, (s, m) in enumerate(homes):
        assert c < 1.0 - cosine_bound(embeds[1][s][m:m + 1].cpu(), refs[1][at:at + 1].cpu())[0, 0]
        assert (s, m) not in hits


def test_an_infinite_bound_is_screen_itself(library):
    from molkgnn_amd.screening import screen, screen_novel
    models, residents, _, refs, _, _ = library
    model = models[1]
    for k in (16, 200):
        plain = screen(model, residents, k, 32)
        novel = screen_novel(model, residents, k, 32, refs[1], max_sim=float("inf"))
        assert novel["n_kept"] == novel["n_scored"] == plain["n_scored"] == sum(COUNTS)
        for name in ("top_score", "top_shard", "top_mol"):
            assert np.array_equal(_bits(novel[name].float()) if name == "top_score" else novel[name].cpu().numpy(),
                                  _bits(plain[name].float()) if name == "top_score" else plain[name].cpu().numpy()), name
        assert "scores" not in novel and novel["top_ref"].shape == novel["top_ref_sim"].shape == novel["top_mol"].shape


def test_min_sim_keeps_the_complement(library):
    """The applicability-domain direction: with the same ``c`` the kept set is the complement of the ``max_sim`` set, apart from keys
    equal to ``c`` (kept by both) and NaN keys (kept by neither); both bounds at once keep the band."""
    from molkgnn_amd.screening import screen_novel
    models, residents, _, refs, _, _ = library
    model = models[1]
    k = 200
    near = screen_novel(model, residents, k, 32, refs[1], min_sim=0.0, return_scores=True)
    sims = [a.cpu().numpy() for a in near["ref_sims"]]
    c = float(sims[0][10])                                         # a measured similarity: a key EQUAL to the bound
    low = screen_novel(model, residents, k, 32, refs[1], max_sim=c)
    high = screen_novel(model, residents, k, 32, refs[1], min_sim=c)
    pairs = lambda r: set(zip(r["top_shard"].tolist(), r["top_mol"].tolist()))         # noqa: E731
    everyone = {(s, m) for s in range(2) for m in range(COUNTS[s])}
    equal = {(s, m) for s, m in everyone if sims[s][m] == np.float32(c)}
    nan = {(s, m) for s, m in everyone if np.isnan(sims[s][m])}
    assert (0, 10) in equal and not nan
    assert pairs(low) & pairs(high) == equal and pairs(low) | pairs(high) == everyone - nan
    assert low["n_kept"] + high["n_kept"] == sum(COUNTS) + len(equal)
    assert pairs(low) == {(s, m) for s, m in everyone if sims[s][m] <= np.float32(c)}
    flat = np.sort(np.concatenate(sims))
    lo, hi = float(flat[20]), float(flat[80])
    band = screen_novel(model, residents, k, 32, refs[1], min_sim=lo, max_sim=hi)
    assert band["n_kept"] == int(((np.concatenate(sims) >= np.float32(lo)) & (np.concatenate(sims) <= np.float32(hi))).sum()) >= 61
    assert pairs(band) == {(s, m) for s, m in everyone if np.float32(lo) <= sims[s][m] <= np.float32(hi)}
    assert model.training


def test_references_as_a_shard_and_as_its_embeddings_agree(library):
    from molkgnn_amd.screening import embed_resident, screen_novel
    models, residents, _, _, _, known = library
    model = models[1]
    model.eval()
    by_shard = screen_novel(model, residents, 16, 32, known, min_sim=-1.0, return_scores=True)
    assert not model.training                                      # the mode it came in, either way
    model.train()
    emb = embed_resident(model, known, 32)
    assert emb.shape == (3, G) and np.array_equal(_bits(by_shard["ref_emb"]), _bits(emb))
    by_tensor = screen_novel(model, residents, 16, 32, emb, min_sim=-1.0, return_scores=True)
    assert model.training
    for name in ("top_score", "top_ref_sim"):
        assert np.array_equal(_bits(by_shard[name]), _bits(by_tensor[name])), name
    for name in ("top_shard", "top_mol", "top_ref"):
        assert np.array_equal(by_shard[name].cpu().numpy(), by_tensor[name].cpu().numpy()), name
    assert by_shard["n_kept"] == by_tensor["n_kept"]
    for name in ("scores", "ref_sims"):
        for a, b in zip(by_shard[name], by_tensor[name]):
            assert np.array_equal(_bits(a), _bits(b))
    assert int(torch.cat(by_shard["refs"]).max()) <= 2
    # what is refused on the GPU, before a pass: the bounds, the head, the references
    for kw in ({}, {"max_sim": 0.1, "min_sim": 0.2}):
        with pytest.raises(ValueError):
            screen_novel(model, residents, 16, 32, emb, **kw)
    with pytest.raises(ValueError):
        screen_novel(models[9], residents, 16, 32, emb, max_sim=0.5)
    with pytest.raises(ValueError):
        screen_novel(model, residents, 16, 32, emb[:, :G - 1], max_sim=0.5)
    with pytest.raises(ValueError):
        screen_novel(model, [], 16, 32, emb, max_sim=0.5)
