"""Library screening on the GPU: ``mkgnn_topk_update`` against its numpy definition (``screening.topk_update_reference``), bit for
bit; ``score_resident`` / ``screen`` / ``evaluate_resident`` against ``model.predict`` on the same gathered batches.  No tolerance
anywhere: integers and float bit patterns."""
import copy

import numpy as np
import pytest
import torch

from tests import _screen_cases as SC
from tests._resident_library import bits as _bits, build_library

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _lib():
    from molkgnn_amd import _lib
    return _lib


def _host(topk):
    return (topk.top_score.cpu().numpy(), topk.top_shard.cpu().numpy(), topk.top_mol.cpu().numpy())


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV).to(dtype)


def _shapes():
    return [(1, 1), (63, 2), (64, 64), (65, 100), (256, 1024), (4096, 1024), (100, _lib().TOPK_MAX_K)]


@pytest.mark.parametrize("B,K", [(1, 1), (63, 2), (64, 64), (65, 100), (256, 1024), (4096, 1024), (100, None)])
def test_kernel_matches_the_definition(B, K):
    """From an empty list, then three further updates with a changing shard tag, for every n_valid of {0, 1, B - 1, B} and on
    every kind of input (special values, all equal, 8 levels, repeated ids, normal)."""
    from molkgnn_amd.screening import TopK, empty_top, topk_update_reference
    K = _lib().TOPK_MAX_K if K is None else K
    for kind in SC.CASES:
        for nv in sorted({0, 1, B - 1, B}):
            topk = TopK(K, DEV)
            want = empty_top(K)
            assert SC.same_list(_host(topk), want)
            for u in range(4):
                scores, ids = SC.case_inputs(kind, B, seed=7 * B + K + u)
                n_valid = nv if u != 2 else B                 # (one full batch in between, so that a sparse n_valid meets a filled list)
                tag = (3, 0, 5, 1)[u]
                topk.update(_dev(scores, torch.float32), _dev(ids, torch.int32), n_valid=n_valid, shard_tag=tag)
                want = topk_update_reference(want, scores, ids, n_valid, tag)
                got = _host(topk)
                assert SC.same_list(got, want), (kind, B, K, nv, u)


def test_kernel_limits_and_rejections():
    from molkgnn_amd.screening import TopK, topk_update_reference
    L = _lib()
    lib = L.load()
    B, K = 100, 8
    scores, ids = SC.case_inputs("normal", B, 1)
    topk = TopK(K, DEV)
    topk.update(_dev(scores, torch.float32), _dev(ids, torch.int32), n_valid=B + 1000, shard_tag=2)       # clamped to B
    want = topk_update_reference(_host(TopK(K, DEV)), scores, ids, B, 2)
    assert SC.same_list(_host(topk), want)
    topk.update(_dev(scores, torch.float32), _dev(ids, torch.int32), n_valid=-4, shard_tag=2)             # nothing counts
    assert SC.same_list(_host(topk), want)
    # rejected sizes: non-zero, a message, the list untouched
    s, i = _dev(scores, torch.float32), _dev(ids, torch.int32)
    big = [torch.zeros(L.TOPK_MAX_K + 1, dtype=dt, device=DEV) for dt in (torch.float32, torch.int32, torch.int32)]
    ws = torch.zeros(1 << 20, dtype=torch.uint8, device=DEV)
    stream = L.stream_ptr(torch.device(DEV))
    rc = lib.mkgnn_topk_update(s.data_ptr(), i.data_ptr(), 0, topk.n_valid.data_ptr(), topk.shard_tag.data_ptr(), K,
                               topk.top_score.data_ptr(), topk.top_shard.data_ptr(), topk.top_mol.data_ptr(), ws.data_ptr(), ws.numel(), stream)
    assert rc != 0 and b"B = 0" in lib.mkgnn_last_error()
    rc = lib.mkgnn_topk_update(s.data_ptr(), i.data_ptr(), B, topk.n_valid.data_ptr(), topk.shard_tag.data_ptr(), L.TOPK_MAX_K + 1,
                               big[0].data_ptr(), big[1].data_ptr(), big[2].data_ptr(), ws.data_ptr(), ws.numel(), stream)
    assert rc != 0 and b"K = " in lib.mkgnn_last_error()
    rc = lib.mkgnn_topk_update(s.data_ptr(), i.data_ptr(), B, topk.n_valid.data_ptr(), topk.shard_tag.data_ptr(), K,
                               topk.top_score.data_ptr(), topk.top_shard.data_ptr(), topk.top_mol.data_ptr(), ws.data_ptr(), 16, stream)
    assert rc != 0 and b"workspace" in lib.mkgnn_last_error()
    torch.cuda.synchronize()
    assert SC.same_list(_host(topk), want)
    assert all(int(t.abs().sum()) == 0 for t in big)


@pytest.mark.parametrize("B,K", [(65, 100), (4096, 1024), (2500, 300)])
def test_poisoned_workspace_and_dead_slots_change_nothing(B, K):
    from molkgnn_amd.screening import TopK
    nv = B - 37 if B > 64 else B - 1
    first, ids0 = SC.case_inputs("special", B, 3)
    scores, ids = SC.case_inputs("quantised", B, 4)
    results = []
    for poison in (False, True):
        topk = TopK(K, DEV)
        topk.update(_dev(first, torch.float32), _dev(ids0, torch.int32), n_valid=B, shard_tag=0)
        s, i = scores.copy(), ids.copy()
        if poison:
            s.view(np.int32)[nv:] = np.int32(0x7FC0BEEF)
            i[nv:] = np.int32(2 ** 31 - 5)
            topk.workspace.view(torch.int32).fill_(0x7FC0BEEF)
        topk.update(_dev(s, torch.float32), _dev(i, torch.int32), n_valid=nv, shard_tag=1)
        results.append(_host(topk))
    assert SC.same_list(results[0], results[1])


@pytest.mark.parametrize("B,K", [(300, 50), (2048, 1024)])
def test_one_captured_update_serves_every_batch(B, K):
    from molkgnn_amd.screening import TopK
    feeds = [(*SC.case_inputs(SC.CASES[u % len(SC.CASES)], B, 20 + u), (B, B - 3, 1, 0, B)[u], u) for u in range(5)]
    eager = TopK(K, DEV)
    for scores, ids, nv, tag in feeds:
        eager.update(_dev(scores, torch.float32), _dev(ids, torch.int32), n_valid=nv, shard_tag=tag)
    replayed = TopK(K, DEV)
    replayed.reserve(B)
    s = torch.zeros(B, dtype=torch.float32, device=DEV)
    i = torch.zeros(B, dtype=torch.int32, device=DEV)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side), torch.cuda.graph(graph, stream=side):
        replayed.update(s, i)                                  # (n_valid and shard_tag: the list's own device scalars)
    torch.cuda.current_stream().wait_stream(side)
    assert SC.same_list(_host(replayed), _host(TopK(K, DEV)))  # a capture launches nothing
    for scores, ids, nv, tag in feeds:
        s.copy_(_dev(scores, torch.float32))
        i.copy_(_dev(ids, torch.int32))
        replayed.n_valid.fill_(nv)
        replayed.shard_tag.fill_(tag)
        graph.replay()
    assert SC.same_list(_host(replayed), _host(eager))
    top = _host(replayed)
    assert replayed.result()[3] == int((top[1] >= 0).sum())


@pytest.fixture(scope="module")
def library(tmp_path_factory):
    """Two resident shards (70 and 33 synthetic molecules), a 3-layer default model with non-trivial running statistics, and
    -- computed ONCE, eagerly -- ``model.predict`` on the gathered batches of each shard (live slots only)."""
    model, residents, gathered = build_library(tmp_path_factory.mktemp("library"), DEV, counts=(70, 33), shard_seed=40,
                                               labels=lambda n: (torch.arange(n) % 3 == 0).float(), model_seed=0, num_layers=3)
    eager = []
    for r in residents:
        eager.append(torch.cat([model.predict(data)[0].view(-1)[:live].clone() for data, live in gathered(r)]))
    model.train()
    return model, residents, eager, gathered


def test_score_resident_equals_predict_on_the_gathered_batches(library):
    from molkgnn_amd.screening import score_resident
    model, residents, eager, _ = library
    assert model.training
    scores = score_resident(model, residents[0], 32)
    assert model.training                                      # handed back in the mode it came in
    assert scores.shape == (70,) and scores.dtype == torch.float32 and scores.is_cuda
    assert not bool(torch.isnan(scores).any())
    assert np.array_equal(_bits(scores), _bits(eager[0]))
    out = torch.zeros(70, dtype=torch.float32, device=DEV)
    again = score_resident(model, residents[0], 32, out=out)
    assert again is out and np.array_equal(_bits(out), _bits(scores))
    # another batch size: other batches, a full last one (70 = 2 * 35), the same molecules -- every slot is written
    assert not bool(torch.isnan(score_resident(model, residents[0], 35)).any())


@pytest.mark.parametrize("k", [16, 200])
def test_screen_ranks_two_shards(library, k):
    from molkgnn_amd.screening import empty_top, screen, topk_update_reference
    model, residents, eager, _ = library
    model.eval()
    r = screen(model, (s for s in residents), k, 32, return_scores=True)     # (a generator: shards one at a time)
    assert not model.training
    model.train()
    assert r["n_scored"] == 103 and len(r["scores"]) == 2
    want = empty_top(k)
    for tag, s in enumerate(r["scores"]):
        assert np.array_equal(_bits(s), _bits(eager[tag]))
        s = s.cpu().numpy()
        want = topk_update_reference(want, s, np.arange(len(s), dtype=np.int32), len(s), tag)
    occupied = min(k, 103)
    assert r["top_score"].shape == r["top_shard"].shape == r["top_mol"].shape == (occupied,)
    got = (r["top_score"].cpu().numpy(), r["top_shard"].cpu().numpy(), r["top_mol"].cpu().numpy())
    assert SC.same_list(got, tuple(a[:occupied] for a in want))
    assert (want[1][occupied:] == -1).all()                    # exactly `occupied` slots are occupied
    if k == 200:
        assert sorted(zip(got[1].tolist(), got[2].tolist())) == [(0, m) for m in range(70)] + [(1, m) for m in range(33)]


def test_screen_rejects_a_two_task_model_before_any_launch(library):
    from molkgnn_amd import screening
    from molkgnn_amd.train import GNNModel
    _, residents, _, _ = library
    two = GNNModel(num_layers=1, task_dim=2).to(DEV)
    launched = []
    real = screening.score_resident
    screening.score_resident = lambda *a, **k: launched.append(1)
    try:
        with pytest.raises(ValueError):
            screening.screen(two, residents, 4, 32)
    finally:
        screening.score_resident = real
    assert not launched
    with pytest.raises(ValueError):
        screening.score_resident(two, residents[0], 32)


def test_evaluate_resident_equals_evaluate(library):
    from molkgnn_amd.train import evaluate, evaluate_resident
    model, residents, eager, gathered = library
    metrics = ("accuracy", "RMSE", "logAUC_0.001_0.1", "logAUC_0.001_1", "ppv", "f1_score", "AUC")

    def batches():
        for data, live in gathered(residents[0]):
            b = copy.copy(data)                                # (the static buffers are refilled: this batch's labels are kept)
            b.y, b.n_valid_molecules = data.y.clone(), live
            yield b

    want = evaluate(model, batches(), metrics)
    got = evaluate_resident(model, residents[0], 32, metrics)
    assert model.training
    assert np.array_equal(_bits(got["pred_y"]), _bits(want["pred_y"])) and np.array_equal(_bits(got["pred_y"]), _bits(eager[0]))
    assert np.array_equal(_bits(got["true_y"].float()), _bits(want["true_y"].float()))
    assert set(got) == set(want)
    for name in ("loss",) + metrics:
        a, b = torch.as_tensor(got[name]).double().cpu(), torch.as_tensor(want[name]).double().cpu()
        assert a.view(torch.int64).equal(b.view(torch.int64)), (name, got[name], want[name])
