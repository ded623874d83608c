"""Per-task library screening on the GPU: ``mkgnn_topk_update_tasks`` against its numpy definition
(``screening.topk_update_tasks_reference``) and against ``mkgnn_topk_update`` list by list, bit for bit; ``predict_tasks`` /
``score_resident_tasks`` / ``screen_tasks`` / ``evaluate_resident_tasks`` against the task-indexed head and the forward-only tail
on the same gathered batches.  No tolerance anywhere: integers and float bit patterns."""
import numpy as np
import pytest
import torch

from tests import _screen_cases as SC
from tests._resident_library import bits as _bits, build_library, eval_model

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _L():
    from molkgnn_amd import _lib
    return _lib


def _host(topk):
    return (topk.top_score.cpu().numpy(), topk.top_shard.cpu().numpy(), topk.top_mol.cpu().numpy())


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV).to(dtype)


def _task_inputs(B, T, seed):
    """``(scores float32 [T, B], ids int32 [B])``: a different kind and seed per task, so the lists differ and some tasks pass a
    run over while others merge it."""
    per_task = [SC.case_inputs(SC.CASES[(t + seed) % len(SC.CASES)], B, seed=seed + 17 * t) for t in range(T)]
    return np.stack([p[0] for p in per_task]), per_task[0][1]


def _empty(T, K):
    from molkgnn_amd.screening import empty_top
    return tuple(np.stack([a] * T) for a in empty_top(K))


# (1025, 100, 9): two tiles, K not a power of two; (2500, 1024, 2): three tiles at the longest list; (1, 1, 32) and (63, 100, 32):
# every task the head takes, inside one tile; (1024, 100, 1) / (1025, 1, 2): the last one-launch size, the first two-launch one
@pytest.mark.parametrize("layout", ["BT", "TB"])
@pytest.mark.parametrize("B,K,T", [(1025, 100, 9), (2500, 1024, 2), (1, 1, 32), (63, 100, 32), (1024, 100, 1), (1025, 1, 2), (63, 1024, 9)])
def test_kernel_matches_the_definition_and_the_single_list_kernel(B, K, T, layout):
    """Three successive updates with n_valid in {B, B // 2, 0} and two shard tags; after each, every list equals the numpy
    definition and a ``TopK`` fed that task's column through ``mkgnn_topk_update``."""
    from molkgnn_amd.screening import TopK, TopKTasks, topk_update_tasks_reference
    lists = TopKTasks(K, T, DEV)
    singles = [TopK(K, DEV) for _ in range(T)]
    want = _empty(T, K)
    assert all(SC.same_list(tuple(a[t] for a in _host(lists)), tuple(a[t] for a in want)) for t in range(T))
    for u, (n_valid, tag) in enumerate(((B, 3), (B // 2, 0), (0, 3))):
        scores, ids = _task_inputs(B, T, seed=5 * B + K + u)
        s_tb = _dev(scores, torch.float32)                             # [T, B]
        s = s_tb if layout == "TB" else s_tb.t().contiguous()          # [B, T] rows
        i = _dev(ids, torch.int32)
        lists.update(s, i, n_valid=n_valid, shard_tag=tag)
        want = topk_update_tasks_reference(want, scores, ids, n_valid, tag)
        got = _host(lists)
        for t in range(T):
            assert SC.same_list(tuple(a[t] for a in got), tuple(a[t] for a in want)), (B, K, T, layout, u, t)
            singles[t].update(s_tb[t].contiguous(), i, n_valid=n_valid, shard_tag=tag)
            assert SC.same_list(tuple(a[t] for a in got), _host(singles[t])), (B, K, T, layout, u, t)
    occupied = lists.result()[3]
    assert occupied.tolist() == [min(K, B + B // 2)] * T


def test_transposed_views_are_read_in_place_and_other_strides_are_refused():
    from molkgnn_amd.screening import TopKTasks, topk_update_tasks_reference
    B, K, T = 70, 16, 9
    scores, ids = _task_inputs(B, T, 3)
    i = _dev(ids, torch.int32)
    want = topk_update_tasks_reference(_empty(T, K), scores, ids, B, 1)
    s_tb = _dev(scores, torch.float32)
    wide = torch.full((T, B + 6), float("nan"), device=DEV)
    wide[:, :B] = s_tb
    for s in (s_tb.t(), s_tb.t().contiguous().t(), wide[:, :B], wide[:, :B].t()):       # views: nothing is copied
        lists = TopKTasks(K, T, DEV)
        lists.update(s, i, n_valid=B, shard_tag=1)
        got = _host(lists)
        assert all(SC.same_list(tuple(a[t] for a in got), tuple(a[t] for a in want)) for t in range(T)), s.stride()
    lists = TopKTasks(K, T, DEV)
    rows = torch.zeros(B, 2 * T, device=DEV)
    for bad in (rows[:, :T], rows[:, ::2], torch.zeros(B, T + 1, device=DEV), torch.zeros(B, device=DEV), torch.zeros(B, T, dtype=torch.float64, device=DEV)):
        with pytest.raises(ValueError):
            lists.update(bad, i, n_valid=B, shard_tag=1)
    with pytest.raises(ValueError):
        lists.update(s_tb, i[:-1], n_valid=B, shard_tag=1)
    assert lists.result()[3].tolist() == [0] * T


@pytest.mark.parametrize("B,K,T", [(65, 100, 9), (2500, 300, 2)])
def test_poisoned_workspace_dead_slots_and_a_large_n_valid(B, K, T):
    from molkgnn_amd.screening import TopKTasks, topk_update_tasks_reference
    nv = B - 37
    first, ids0 = _task_inputs(B, T, 3)
    scores, ids = _task_inputs(B, T, 4)
    results = []
    for poison in (False, True):
        lists = TopKTasks(K, T, DEV)
        lists.update(_dev(first, torch.float32), _dev(ids0, torch.int32), n_valid=B + 1000, shard_tag=0)     # clamped to B
        s, i = scores.copy(), ids.copy()
        if poison:
            s.view(np.int32)[:, nv:] = np.int32(0x7FC0BEEF)            # NaN scores and garbage ids past n_valid
            i[nv:] = np.int32(2 ** 31 - 5)
            lists.workspace.fill_(0xFF)
        lists.update(_dev(s, torch.float32), _dev(i, torch.int32), n_valid=nv, shard_tag=1)
        results.append(_host(lists))
    want = topk_update_tasks_reference(topk_update_tasks_reference(_empty(T, K), first, ids0, B, 0), scores, ids, nv, 1)
    for t in range(T):
        assert SC.same_list(tuple(a[t] for a in results[0]), tuple(a[t] for a in want)), t
        assert SC.same_list(tuple(a[t] for a in results[1]), tuple(a[t] for a in want)), t


def test_one_captured_update_serves_every_batch():
    from molkgnn_amd.screening import TopKTasks
    B, K, T = 64, 16, 9
    feeds = [(*_task_inputs(B, T, 20 + u), (B, B - 3, 1, 0, B)[u], u) for u in range(5)]
    eager = TopKTasks(K, T, DEV)
    for scores, ids, nv, tag in feeds:
        eager.update(_dev(scores, torch.float32).t().contiguous(), _dev(ids, torch.int32), n_valid=nv, shard_tag=tag)
    replayed = TopKTasks(K, T, DEV)
    replayed.reserve(B)
    s = torch.zeros(B, T, dtype=torch.float32, device=DEV)
    i = torch.zeros(B, dtype=torch.int32, device=DEV)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side), torch.cuda.graph(graph, stream=side):
        replayed.update(s, i)                                          # (n_valid and shard_tag: the lists' own device scalars)
    torch.cuda.current_stream().wait_stream(side)
    assert replayed.result()[3].tolist() == [0] * T                    # a capture launches nothing
    for scores, ids, nv, tag in feeds:
        s.copy_(_dev(scores, torch.float32).t())
        i.copy_(_dev(ids, torch.int32))
        replayed.n_valid.fill_(nv)
        replayed.shard_tag.fill_(tag)
        graph.replay()
    a, b = _host(replayed), _host(eager)
    assert all(SC.same_list(tuple(x[t] for x in a), tuple(x[t] for x in b)) for t in range(T))


def test_kernel_rejections_launch_nothing():
    from molkgnn_amd.screening import TopKTasks
    L = _L()
    lib = L.load()
    B, K, T = 100, 8, 3
    scores, ids = _task_inputs(B, T, 1)
    lists = TopKTasks(K, T, DEV)
    lists.update(_dev(scores, torch.float32), _dev(ids, torch.int32), n_valid=B, shard_tag=2)
    want = _host(lists)
    s, i = _dev(scores, torch.float32), _dev(ids, torch.int32)
    big = [torch.zeros(33 * (L.TOPK_MAX_K + 1), dtype=dt, device=DEV) for dt in (torch.float32, torch.int32, torch.int32)]
    ws = torch.zeros(1 << 20, dtype=torch.uint8, device=DEV)
    stream = L.stream_ptr(torch.device(DEV))
    nv, tag = lists.n_valid.data_ptr(), lists.shard_tag.data_ptr()
    own = (lists.top_score.data_ptr(), lists.top_shard.data_ptr(), lists.top_mol.data_ptr())
    other = tuple(t.data_ptr() for t in big)

    def call(B=B, T=T, K=K, top=own, ws_ptr=ws.data_ptr(), ws_bytes=ws.numel(), rs=1, ts=B):
        return lib.mkgnn_topk_update_tasks(s.data_ptr(), rs, ts, i.data_ptr(), B, T, nv, tag, K, *top, ws_ptr, ws_bytes, stream)

    assert call(T=33, top=other) != 0 and b"T = 33" in lib.mkgnn_last_error()
    assert call(T=0) != 0 and b"T = 0" in lib.mkgnn_last_error()
    assert call(K=L.TOPK_MAX_K + 1, top=other) != 0 and b"K = " in lib.mkgnn_last_error()
    assert call(B=0) != 0 and b"B = 0" in lib.mkgnn_last_error()
    assert call(ws_ptr=ws.data_ptr() + 4) != 0 and b"aligned" in lib.mkgnn_last_error()
    assert call(ws_bytes=16) != 0 and b"workspace" in lib.mkgnn_last_error()
    assert call(rs=-1) != 0 and b"stride" in lib.mkgnn_last_error()
    # two tiles: the runs of all three tasks must fit, not only those of one
    need = int(lib.mkgnn_topk_tasks_workspace_bytes(2000, K, T))
    assert need > int(lib.mkgnn_topk_workspace_bytes(2000, K))
    assert call(B=2000, ws_bytes=need - 1) != 0 and b"workspace" in lib.mkgnn_last_error()
    torch.cuda.synchronize()
    got = _host(lists)
    assert all(SC.same_list(tuple(a[t] for a in got), tuple(a[t] for a in want)) for t in range(T))
    assert all(int(t.abs().sum()) == 0 for t in big)


# ------------------------------------------------------------------------------------------------ end to end --
@pytest.fixture(scope="module")
def library(tmp_path_factory):
    """The fixture shape of test_screen_gpu.py -- two resident shards (70 and 33 synthetic molecules; the first also held with its
    molecules' tasks), batch 32, 3-layer models with non-trivial running statistics: a nine-task and a two-task model and a
    one-task model that shares the nine-task model's network -- and, computed ONCE, eagerly, ``predict_tasks`` of the nine-task
    model and ``predict`` of the one-task model on the gathered batches of each shard (live slots only)."""
    from molkgnn_amd import shards as S
    from molkgnn_amd.synthetic import NINE_ASSAYS
    from molkgnn_amd.train import GNNModel
    d = tmp_path_factory.mktemp("library_tasks")
    nine, residents, gathered = build_library(d, DEV, counts=(70, 33), shard_seed=40, labels=lambda n: (torch.arange(n) % 3 == 0).float(),
                                              model_seed=9, num_layers=3, task_dim=9)
    labelled = S.ResidentShard(str(d / "lib-0.mkgs"), DEV, assays=[int(a) for a in NINE_ASSAYS][:8])    # (one assay is not listed)
    models = {9: nine, 2: eval_model(DEV, 2, num_layers=3, task_dim=2)}
    one = GNNModel(num_layers=3, task_dim=1).to(DEV)
    one.gnn_model = models[9].gnn_model                            # the same network, a one-task head
    one.eval()

    eager = {T: [] for T in models}
    emb9, emb1 = [], []
    for r in residents:
        parts = {T: [] for T in models}
        for data, live in gathered(r):
            for T, model in models.items():
                pred, emb = model.predict_tasks(data)
                assert pred.shape == (32, T) and emb.shape[0] == 32
                parts[T].append(pred[:live].clone())
                if T == 9:
                    emb9.append(emb[:live].clone())
            emb1.append(one.predict(data)[1][:live].clone())
        for T in models:
            eager[T].append(torch.cat(parts[T]))
    for model in models.values():
        model.train()
    return models, residents, eager, (torch.cat(emb9), torch.cat(emb1)), labelled


def test_predict_tasks_takes_the_tail_for_the_embedding_and_the_head_for_every_column(library):
    models, residents, eager, (emb9, emb1), _ = library
    L = _L()
    lib = L.load()
    assert emb9.shape == (103, 32) and np.array_equal(_bits(emb9), _bits(emb1))       # the forward-only tail supplied it
    model = models[9]
    pred = torch.cat(eager[9])
    n, H, T = 103, 32, 9
    w, b = model.ffn.weight.detach().contiguous(), model.ffn.bias.detach()
    ws = torch.empty(int(lib.mkgnn_task_head_workspace_bytes(n, H, T)), dtype=torch.uint8, device=DEV)
    y, loss, col = torch.zeros(n, device=DEV), torch.empty(1, device=DEV), torch.empty(n, device=DEV)
    for t in range(T):
        task = torch.full((n,), t, dtype=torch.int32, device=DEV)
        L.check(lib.mkgnn_task_head_forward(L.LOSS_BCE_MEAN, emb9.data_ptr(), H, n, H, T, w.data_ptr(), b.data_ptr(), y.data_ptr(),
                                            task.data_ptr(), None, n, 0.0, None, None, col.data_ptr(), loss.data_ptr(), ws.data_ptr(),
                                            ws.numel(), L.stream_ptr(torch.device(DEV))), "mkgnn_task_head_forward")
        assert np.array_equal(_bits(pred[:, t]), _bits(col)), t
    assert model.training
    with pytest.raises(ValueError):
        model.predict_tasks(None)                                  # training mode: refused before the batch is looked at


@pytest.mark.parametrize("T", [9, 2])
def test_score_resident_tasks_equals_predict_tasks_on_the_gathered_batches(library, T):
    from molkgnn_amd.screening import score_resident_tasks
    models, residents, eager, _, _ = library
    model = models[T]
    assert model.training
    scores = score_resident_tasks(model, residents[0], 32)
    assert model.training                                          # handed back in the mode it came in
    assert scores.shape == (70, T) and scores.dtype == torch.float32 and scores.is_cuda
    assert not bool(torch.isnan(scores).any())
    assert np.array_equal(_bits(scores), _bits(eager[T][0]))
    if T == 9:
        out = torch.zeros(70, T, dtype=torch.float32, device=DEV)
        again = score_resident_tasks(model, residents[0], 32, out=out)
        assert again is out and np.array_equal(_bits(out), _bits(scores))
        # another batch size: other batches, a full last one (70 = 2 * 35), the same molecules -- every slot is written
        assert not bool(torch.isnan(score_resident_tasks(model, residents[0], 35)).any())
        model.eval()
        score_resident_tasks(model, residents[0], 32)
        assert not model.training
        model.train()
        with pytest.raises(ValueError):
            score_resident_tasks(model, residents[0], 32, out=torch.zeros(70, device=DEV))
        with pytest.raises(ValueError):
            from molkgnn_amd.screening import TopK
            score_resident_tasks(model, residents[0], 32, topk=TopK(4, DEV))


@pytest.mark.parametrize("k", [16, 200])
def test_screen_tasks_ranks_two_shards_in_every_task(library, k):
    from molkgnn_amd.screening import screen_tasks, topk_update_tasks_reference
    models, residents, eager, _, _ = library
    model, T = models[9], 9
    r = screen_tasks(model, (s for s in residents), k, 32, return_scores=True)     # (a generator: shards one at a time)
    assert model.training
    assert r["n_scored"] == 103 and len(r["scores"]) == 2
    want = _empty(T, k)
    for tag, s in enumerate(r["scores"]):
        assert np.array_equal(_bits(s), _bits(eager[T][tag]))
        s = s.cpu().numpy()
        want = topk_update_tasks_reference(want, s.T, np.arange(len(s), dtype=np.int32), len(s), tag)
    occupied = min(k, 103)
    assert r["top_score"].shape == r["top_shard"].shape == r["top_mol"].shape == (T, k)
    assert r["n_occupied"].tolist() == [occupied] * T
    got = (r["top_score"].cpu().numpy(), r["top_shard"].cpu().numpy(), r["top_mol"].cpu().numpy())
    everyone = [(0, m) for m in range(70)] + [(1, m) for m in range(33)]
    for t in range(T):
        assert SC.same_list(tuple(a[t] for a in got), tuple(a[t] for a in want)), t
        assert (got[1][t][occupied:] == -1).all() and (got[2][t][occupied:] == -1).all()     # empty slots stay (-inf, -1, -1)
        assert (SC.bits(got[0][t][occupied:]) == SC.bits([-np.inf])[0]).all()
        if k == 200:
            assert sorted(zip(got[1][t][:occupied].tolist(), got[2][t][:occupied].tolist())) == everyone
    assert any(got[2][t].tolist() != got[2][0].tolist() for t in range(1, T))      # the tasks rank differently


def test_evaluate_resident_tasks_is_the_shared_helper_on_the_resident_scores(library):
    from molkgnn_amd import train
    from molkgnn_amd.screening import score_resident_tasks
    models, residents, eager, _, labelled = library
    model, T = models[9], 9
    metrics = ("accuracy", "RMSE", "logAUC_0.001_0.1", "logAUC_0.001_1", "ppv", "f1_score", "AUC")
    got = train.evaluate_resident_tasks(model, labelled, 32, metrics)
    assert model.training
    pred = score_resident_tasks(model, labelled, 32)
    assert np.array_equal(_bits(pred), _bits(eager[T][0]))
    task = labelled.task.to(DEV).view(-1).long()
    assert int(task.min()) == -1 and int(task.max()) == 7          # (a molecule of the unlisted assay has no label)
    want = train._task_results(pred, labelled.y.to(DEV).view(-1), task, T, "bce", metrics, train._metric_functions())
    keys = {"loss", "pred_y", "true_y", "task"} | set(metrics) | {m + "_mean" for m in metrics}
    assert set(got) == set(want) == keys                           # evaluate_tasks' keys
    assert np.array_equal(_bits(got["pred_y"]), _bits(want["pred_y"]))
    lab = task >= 0
    assert np.array_equal(_bits(got["pred_y"][lab]), _bits(pred[lab].gather(1, task[lab][:, None]).view(-1)))
    assert bool(torch.isnan(got["pred_y"][~lab]).all())
    assert torch.equal(got["task"], task) and torch.equal(got["true_y"], labelled.y.to(DEV).view(-1))
    for name in ("loss",) + metrics + tuple(m + "_mean" for m in metrics):
        a, b = torch.as_tensor(got[name]).double().cpu(), torch.as_tensor(want[name]).double().cpu()
        assert a.view(torch.int64).equal(b.view(torch.int64)), (name, got[name], want[name])
