"""The refusals of screening that lie behind the device check, on a GPU model and a GPU shard: for each of the four ``*_resident``
entry points a batch size of 0, an ``out`` of the wrong shape, dtype or layout and a running list of the wrong class or count -- a
``ValueError`` with its word, the model handed back in its mode, the running lists untouched bit for bit -- then the refusals of
``rank_embeddings``, ``nearest`` and the lists' ``update`` that need a device, a ``predict`` that raises in the eager step, and one
positive pass per entry point over a shard with a short tail (40 molecules, batch 16).  The cells a CPU-only process reaches:
test_screening_refusals_cpu.py; what the passes compute, bit for bit: test_screen_gpu.py, test_screen_tasks_gpu.py,
test_nearest_gpu.py."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests._resident_library import bits

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N, BS, T, Q, G, K = 40, 16, 3, 5, 32, 8


@pytest.fixture(scope="module")
def ctx(tmp_path_factory):
    from molkgnn_amd import shards as S
    from molkgnn_amd.screening import TopK, TopKTasks
    from molkgnn_amd.synthetic import make_batch
    from molkgnn_amd.train import GNNModel
    path = str(tmp_path_factory.mktemp("refusals_gpu") / "lib.mkgs")
    S.write_shard(path, make_batch(N, seed=6, assay="all9", with_receptive_fields=False))
    torch.manual_seed(0)
    c = SimpleNamespace(shard=S.ResidentShard(path, DEV), cpu_shard=S.ResidentShard(path, "cpu"),
                        one=GNNModel(num_layers=1).to(DEV), three=GNNModel(num_layers=1, task_dim=T).to(DEV),
                        queries=torch.randn(Q, G, generator=torch.Generator().manual_seed(1)).to(DEV))
    # running lists that hold something: what a refusal must leave as it is
    ids = torch.arange(N, dtype=torch.int32, device=DEV)
    scores = torch.randn(N, Q, generator=torch.Generator().manual_seed(2)).to(DEV)
    c.lists = {"TopK": TopK(K, DEV), "TopKTasks 2": TopKTasks(K, 2, DEV), "TopKTasks 3": TopKTasks(K, T, DEV),
               "TopKTasks 4": TopKTasks(K, 4, DEV), "TopKTasks 5": TopKTasks(K, Q, DEV)}
    for name, lists in c.lists.items():
        lists.update(scores[:, 0].contiguous() if name == "TopK" else scores[:, :lists.n_tasks].contiguous(), ids, n_valid=N, shard_tag=7)
    return c


def _snapshot(lists):
    return [bits(lists.top_score), lists.top_shard.cpu().numpy(), lists.top_mol.cpu().numpy(), lists.n_valid.cpu().numpy(),
            lists.shard_tag.cpu().numpy()]


def _entry(c, name):
    """``(call(**kw), model, the shape of its result, the lists it takes)`` of one of the four entry points."""
    from molkgnn_amd import screening
    if name == "score_resident":
        return (lambda bs=BS, **kw: screening.score_resident(c.one, c.shard, bs, **kw)), c.one, (N,), "TopK"
    if name == "score_resident_tasks":
        return (lambda bs=BS, **kw: screening.score_resident_tasks(c.three, c.shard, bs, **kw)), c.three, (N, T), "TopKTasks 3"
    if name == "embed_resident":
        return (lambda bs=BS, **kw: screening.embed_resident(c.three, c.shard, bs, **kw)), c.three, (N, G), None
    return (lambda bs=BS, **kw: screening.nearest_resident(c.three, c.shard, c.queries, bs, **kw)), c.three, (N, Q), "TopKTasks 5"


ENTRIES = ("score_resident", "score_resident_tasks", "embed_resident", "nearest_resident")
WRONG_LISTS = {            # entry point -> (lists of the wrong class, lists of the wrong count, the word of both refusals)
    "score_resident": ("TopKTasks 3", None, "^score_resident: the running list must be a TopK$"),
    "score_resident_tasks": ("TopK", "TopKTasks 2", "^score_resident_tasks: the running list must be a TopKTasks of 3 tasks$"),
    "nearest_resident": ("TopK", "TopKTasks 4", "^nearest_resident: the running lists must be a TopKTasks of 5 lists, one per query$"),
}


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("name", ENTRIES)
def test_refused_behind_the_device_check(ctx, name, training):
    call, model, shape, own = _entry(ctx, name)
    good = {} if own is None else {"topk": ctx.lists[own]}
    before = {k: _snapshot(v) for k, v in ctx.lists.items()}
    out_word = rf"^out: a contiguous float32 tensor of shape \({', '.join(map(str, shape))},?\) on cuda:0$"
    wide = torch.zeros(shape[0], 2 * shape[-1] if len(shape) == 2 else 2, device=DEV)
    strided = wide[:, ::2] if len(shape) == 2 else wide[:, 0]
    assert tuple(strided.shape) == shape and not strided.is_contiguous()
    cells = [(dict(bs=0, **good), "^batch_size >= 1$"),
             (dict(out=torch.zeros(N + 1, *shape[1:], device=DEV), **good), out_word),
             (dict(out=torch.zeros(N, 7, device=DEV), **good), out_word),
             (dict(out=torch.zeros(shape, dtype=torch.float64, device=DEV), **good), out_word),
             (dict(out=strided, **good), out_word),
             (dict(out=torch.zeros(shape), **good), out_word),                                   # (an ``out`` on the CPU)
             (dict(bs=0, out=torch.zeros(3, device=DEV), **good), "^batch_size >= 1$")]          # the batch size is named first
    if own is not None:
        wrong_class, wrong_count, word = WRONG_LISTS[name]
        cells += [(dict(topk=ctx.lists[wrong_class]), word),
                  (dict(topk=ctx.lists[wrong_class], out=torch.zeros(3, device=DEV)), word),     # the lists before ``out``
                  (dict(bs=0, topk=ctx.lists[wrong_class]), "^batch_size >= 1$")]                # the batch size before the lists
        if wrong_count is not None:
            cells.append((dict(topk=ctx.lists[wrong_count]), word))
    model.train(training)
    for kw, word in cells:
        with pytest.raises(ValueError, match=word):
            call(**kw)
        assert model.training is training, kw
    model.train()
    for k, lists in ctx.lists.items():
        assert all(np.array_equal(a, b) for a, b in zip(_snapshot(lists), before[k])), k


def test_shard_and_model_on_different_devices(ctx):
    from molkgnn_amd import screening
    from molkgnn_amd.train import GNNModel
    word = "^the shard is resident on cpu, the model is on cuda:0$"
    for call in (lambda: screening.score_resident(ctx.one, ctx.cpu_shard, BS),
                 lambda: screening.score_resident_tasks(ctx.three, ctx.cpu_shard, BS),
                 lambda: screening.embed_resident(ctx.three, ctx.cpu_shard, BS),
                 lambda: screening.nearest_resident(ctx.three, ctx.cpu_shard, ctx.queries, BS),
                 lambda: screening.screen(ctx.one, [ctx.cpu_shard], K, BS),
                 lambda: screening.screen_tasks(ctx.three, [ctx.cpu_shard], K, BS),
                 lambda: screening.nearest(ctx.three, ctx.queries, [ctx.cpu_shard], K, BS),
                 lambda: screening.nearest_resident(ctx.three, ctx.cpu_shard, ctx.queries, 0)):   # (the shard before the batch size)
        with pytest.raises(ValueError, match=word):
            call()
    # queries on the GPU: what is refused behind them
    with pytest.raises(ValueError, match="^nearest needs at least one shard$"):
        screening.nearest(ctx.three, ctx.queries, [], K, BS)
    with pytest.raises(ValueError, match=r"^nearest runs on the GPU: move the model there \(there is no CPU path\)$"):
        screening.nearest(GNNModel(num_layers=1), ctx.queries, [ctx.shard], K, BS)
    with pytest.raises(ValueError, match=r"^nearest: the queries are on cpu; they belong on the GPU of the library \(cuda:0\)$"):
        screening.nearest(ctx.three, ctx.queries.cpu(), [ctx.shard], K, BS)
    with pytest.raises(ValueError, match=r"^nearest_resident: the queries are on cpu; they belong on the GPU of the library$"):
        screening.nearest_resident(ctx.three, ctx.shard, ctx.queries.cpu(), BS)
    assert ctx.one.training and ctx.three.training


def test_rank_embeddings_refusals_on_the_device(ctx):
    from molkgnn_amd.screening import rank_embeddings
    emb, lists = torch.zeros(N, G, device=DEV), ctx.lists["TopKTasks 5"]
    before = _snapshot(lists)
    wrong = r"^rank_embeddings: the running lists must be a TopKTasks of 5 lists on cuda:0$"
    ids_word = r"^rank_embeddings: ids is a contiguous int32 \[40\] tensor on cuda:0$"
    cells = [(dict(topk=ctx.lists["TopK"]), wrong), (dict(topk=ctx.lists["TopKTasks 4"]), wrong), (dict(topk=None), wrong),
             (dict(topk=ctx.lists["TopK"], chunk=0), wrong),                                     # the lists before the chunk
             (dict(topk=lists, chunk=0), "^chunk >= 1$"),
             (dict(topk=lists, chunk=0, ids=torch.arange(N, device=DEV)), "^chunk >= 1$"),       # the chunk before the ids
             (dict(topk=lists, ids=torch.arange(N, device=DEV)), ids_word),                      # (int64 ids)
             (dict(topk=lists, ids=torch.arange(N - 1, dtype=torch.int32, device=DEV)), ids_word),
             (dict(topk=lists, ids=torch.arange(2 * N, dtype=torch.int32, device=DEV)[::2]), ids_word),
             (dict(topk=lists, ids=torch.arange(N, dtype=torch.int32)), ids_word)]
    for kw, word in cells:
        with pytest.raises(ValueError, match=word):
            rank_embeddings(emb, ctx.queries, **kw)
    with pytest.raises(ValueError, match=r"^rank_embeddings: the queries are on cpu; they belong on the GPU of the library$"):
        rank_embeddings(emb, ctx.queries.cpu(), lists)
    with pytest.raises(ValueError, match=r"^rank_embeddings: emb is on cpu; the ranking runs on the GPU \(there is no CPU path\)$"):
        rank_embeddings(emb.cpu(), ctx.queries, lists)
    rank_embeddings(emb[:0], ctx.queries, lists)                                                  # no row: nothing to do
    assert all(np.array_equal(a, b) for a, b in zip(_snapshot(lists), before))


def test_update_refusals(ctx):
    one, three = ctx.lists["TopK"], ctx.lists["TopKTasks 3"]
    before = _snapshot(one), _snapshot(three)
    s, i = torch.zeros(N, device=DEV), torch.zeros(N, dtype=torch.int32, device=DEV)
    device_word = "^scores float32 and ids int32 on the list's device$"
    for scores, ids, kw, word in [(s.double(), i, {}, device_word), (s, i.long(), {}, device_word), (s.cpu(), i, {}, device_word),
                                  (s, i.cpu(), {}, device_word), (s.double()[:3], i, {}, device_word),
                                  (s[:-1], i, {}, "^scores and ids: contiguous, one id per score$"),
                                  (torch.zeros(2 * N, device=DEV)[::2], i, {}, "^scores and ids: contiguous, one id per score$"),
                                  (s[:0], i[:0], {}, "^an update needs at least one slot$"),
                                  (s, i, dict(n_valid=torch.zeros(1, dtype=torch.int64, device=DEV)),
                                   "^a device scalar of an update is one int32 on the list's device$"),
                                  (s, i, dict(shard_tag=torch.zeros(2, dtype=torch.int32, device=DEV)),
                                   "^a device scalar of an update is one int32 on the list's device$")]:
        with pytest.raises(ValueError, match=word):
            one.update(scores, ids, **kw)
    m = torch.zeros(N, T, device=DEV)
    lists_word = "^scores float32 and ids int32 on the lists' device$"
    for scores, ids, kw, word in [(m.double(), i, {}, lists_word), (m, i.long(), {}, lists_word), (m.cpu(), i, {}, lists_word),
                                  (m.double()[:, :2], i, {}, lists_word),
                                  (m[:0], i[:0], {}, "^an update needs at least one slot and contiguous ids$"),
                                  (m, torch.zeros(2 * N, dtype=torch.int32, device=DEV)[::2], {},
                                   "^an update needs at least one slot and contiguous ids$"),
                                  (m[:, :2], i, {}, r"^scores: \[40, 3\] or \[3, 40\], one row of 3 scores per id$"),
                                  (s, i, {}, r"^scores: \[40, 3\] or \[3, 40\], one row of 3 scores per id$"),
                                  (torch.zeros(N, 2 * T, device=DEV)[:, ::2], i, {}, r"^scores: strides \(6, 2\) are neither \[B, T\] rows"),
                                  (m, i, dict(n_valid=torch.zeros(1, dtype=torch.int64, device=DEV)),
                                   "^a device scalar of an update is one int32 on the list's device$")]:
        with pytest.raises(ValueError, match=word):
            three.update(scores, ids, **kw)
    after = _snapshot(one), _snapshot(three)
    assert all(np.array_equal(a, b) for x, y in zip(after, before) for a, b in zip(x, y))


def test_a_predict_that_raises_in_the_eager_step(ctx, monkeypatch):
    """On the host, in the warm-up step, before any capture begins: the exception comes through and the model is back in training
    mode."""
    from molkgnn_amd.screening import embed_resident

    def stop(data):
        raise RuntimeError("stop")

    model = ctx.three
    monkeypatch.setattr(model, "embed", stop)
    assert model.training
    with pytest.raises(RuntimeError, match="^stop$"):
        embed_resident(model, ctx.shard, BS)
    assert model.training
    torch.cuda.synchronize()


@pytest.mark.parametrize("name", ENTRIES)
def test_a_pass_over_a_shard_with_a_short_tail(ctx, name):
    """40 molecules in batches of 16: a tail of 8.  The shape, no NaN, and ``out`` is what comes back."""
    call, model, shape, _ = _entry(ctx, name)
    got = call()
    assert tuple(got.shape) == shape and got.dtype == torch.float32 and got.is_cuda
    assert not bool(torch.isnan(got).any())
    out = torch.full(shape, float("nan"), device=DEV)
    assert call(out=out) is out
    assert not bool(torch.isnan(out).any())
    assert model.training
