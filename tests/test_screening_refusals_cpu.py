"""What screening and resident evaluation refuse before the device is reached, cell by cell: every public entry point of
``molkgnn_amd.screening`` plus ``train.evaluate_resident`` / ``evaluate_resident_tasks`` against each bad argument a CPU-only process
can hand it -- the exception type and a word of its message -- and, where two arguments are bad at once, which refusal wins.  The
library is never loaded on the way to a refusal.  (The cells behind the device check: test_screening_refusals_gpu.py.)"""
from types import SimpleNamespace

import pytest
import torch

G = 32                                                  # hidden_dim of the default model: the embedding's width


@pytest.fixture(scope="module")
def ctx(tmp_path_factory):
    """One CPU shard of 40 molecules, held plainly and with its molecules' tasks, and a query shard of 3 molecules."""
    from molkgnn_amd import shards as S
    from molkgnn_amd.synthetic import NINE_ASSAYS, make_batch
    d = tmp_path_factory.mktemp("refusals")
    path, few = str(d / "lib.mkgs"), str(d / "few.mkgs")
    S.write_shard(path, make_batch(40, seed=6, assay="all9", with_receptive_fields=False))
    S.write_shard(few, make_batch(3, seed=7, assay="all9", with_receptive_fields=False))
    return SimpleNamespace(plain=S.ResidentShard(path, "cpu"), few=S.ResidentShard(few, "cpu"),
                           nine=S.ResidentShard(path, "cpu", assays=[int(a) for a in NINE_ASSAYS]))


def _model(task_dim=1, **kw):
    from molkgnn_amd.train import GNNModel
    return GNNModel(num_layers=1, task_dim=task_dim, **kw)


def _headless():
    return torch.nn.Linear(2, 2)                        # (a module without ``ffn``)


def _sc():
    from molkgnn_amd import screening
    return screening


def _tr():
    from molkgnn_amd import train
    return train


def _max_k():
    from molkgnn_amd import _lib
    return _lib.TOPK_MAX_K


QUERIES = {                                             # a malformed query matrix -> the word that names it
    "no queries": (lambda: torch.zeros(0, G), "0 queries outside"),
    "33 queries": (lambda: torch.zeros(33, G), "33 queries outside"),
    "too wide": (lambda: torch.zeros(3, G + 1), "the queries are 33 wide, the embedding is 32 wide"),
    "float64": (lambda: torch.zeros(3, G, dtype=torch.float64), "the queries are float32, not torch.float64"),
    "a vector": (lambda: torch.zeros(G), r"the queries are a \[Q, 32\] tensor of embeddings"),
    "not a tensor": (lambda: [[0.0] * G], r"the queries are a \[Q, 32\] tensor of embeddings"),
}
GOOD = lambda: torch.zeros(3, G)                        # noqa: E731  (well-formed, on the CPU)
ON_CPU = "the queries are on cpu; they belong on the GPU of the library"
NO_CPU_PATH = r"screening runs on the GPU: move the model there \(there is no CPU path\)"
ONE_TASK = r"screening ranks ONE score per molecule: a one-task model \(task_dim = 1\) is needed"
OUTPUTS = r"per-task screening takes a model with 1 to 32 outputs \(task_dim\), not "
NO_HEAD = r"a model whose head \(ffn\) reads the graph embedding is needed"
METRIC = r"unknown metric\(s\) \['no such metric'\]: one of \['AUC', 'RMSE', 'accuracy', 'f1_score', "
LOSS_KINDS = r" needs one of the head's loss kinds \(BCEWithLogitsLoss\(\), MSELoss\(\), MSELoss\('sum'\)\)"

# name -> (call(ctx), the word of the refusal): every one a ValueError
CELLS = {
    # ---------------------------------------------------------------------------------------------- score_resident
    "score_resident: a CPU model": (lambda c: _sc().score_resident(_model(), c.plain, 32), NO_CPU_PATH),
    "score_resident: a two-task model": (lambda c: _sc().score_resident(_model(2), c.plain, 32), ONE_TASK),
    "score_resident: a model without a head": (lambda c: _sc().score_resident(_headless(), c.plain, 32), ONE_TASK),
    "score_resident: a two-task model wins over batch_size 0": (lambda c: _sc().score_resident(_model(2), c.plain, 0), ONE_TASK),
    "score_resident: a CPU model wins over batch_size 0": (lambda c: _sc().score_resident(_model(), c.plain, 0), NO_CPU_PATH),
    # ---------------------------------------------------------------------------------------- score_resident_tasks
    "score_resident_tasks: a CPU model": (lambda c: _sc().score_resident_tasks(_model(9), c.plain, 32), NO_CPU_PATH),
    "score_resident_tasks: a CPU one-task model": (lambda c: _sc().score_resident_tasks(_model(1), c.plain, 32), NO_CPU_PATH),
    "score_resident_tasks: 33 outputs": (lambda c: _sc().score_resident_tasks(_model(33), c.plain, 32), OUTPUTS + "33"),
    "score_resident_tasks: a model without a head": (lambda c: _sc().score_resident_tasks(_headless(), c.plain, 32), OUTPUTS + "None"),
    # ---------------------------------------------------------------------------------------------- embed_resident
    "embed_resident: a CPU model": (lambda c: _sc().embed_resident(_model(9), c.plain, 32), NO_CPU_PATH),
    "embed_resident: a model without a head": (lambda c: _sc().embed_resident(_headless(), c.plain, 32), NO_HEAD),
    "embed_resident: a CPU model wins over batch_size 0": (lambda c: _sc().embed_resident(_model(), c.plain, 0), NO_CPU_PATH),
    # -------------------------------------------------------------------------------------------- nearest_resident
    **{f"nearest_resident: {name}": (lambda c, q=q: _sc().nearest_resident(_model(9), c.plain, q(), 32), "nearest_resident: " + word)
       for name, (q, word) in QUERIES.items()},
    "nearest_resident: queries on the CPU win over a CPU model":
        (lambda c: _sc().nearest_resident(_model(9), c.plain, GOOD(), 32), "nearest_resident: " + ON_CPU + "$"),
    "nearest_resident: a model without a head wins over the queries":
        (lambda c: _sc().nearest_resident(_headless(), c.plain, torch.zeros(G), 32), NO_HEAD),
    # ------------------------------------------------------------------------------------------------------ screen
    "screen: a CPU model": (lambda c: _sc().screen(_model(), [c.plain], 4, 32), NO_CPU_PATH),
    "screen: a two-task model": (lambda c: _sc().screen(_model(2), [c.plain], 4, 32), ONE_TASK),
    "screen: no shard": (lambda c: _sc().screen(_model(), [], 4, 32), "^screen needs at least one shard$"),
    "screen: no shard, from a generator": (lambda c: _sc().screen(_model(), (s for s in ()), 4, 32), "^screen needs at least one shard$"),
    "screen: a CPU model wins over k = 0": (lambda c: _sc().screen(_model(), [c.plain], 0, 32), NO_CPU_PATH),
    # ------------------------------------------------------------------------------------------------ screen_tasks
    "screen_tasks: a CPU model": (lambda c: _sc().screen_tasks(_model(9), [c.plain], 4, 32), NO_CPU_PATH),
    "screen_tasks: 33 outputs": (lambda c: _sc().screen_tasks(_model(33), [c.plain], 4, 32), OUTPUTS + "33"),
    "screen_tasks: no shard": (lambda c: _sc().screen_tasks(_model(9), [], 4, 32), "^screen_tasks needs at least one shard$"),
    # ----------------------------------------------------------------------------------------------------- nearest
    **{f"nearest: {name}": (lambda c, q=q: _sc().nearest(_model(9), q(), [c.plain], 4, 32), "nearest: " + word)
       for name, (q, word) in QUERIES.items()},
    "nearest: queries on the CPU win over a CPU model": (lambda c: _sc().nearest(_model(9), GOOD(), [c.plain], 4, 32), "nearest: " + ON_CPU + "$"),
    "nearest: queries on the CPU win over no shard": (lambda c: _sc().nearest(_model(9), GOOD(), [], 4, 32), "nearest: " + ON_CPU + "$"),
    "nearest: a query shard of 40 molecules":
        (lambda c: _sc().nearest(_model(9), c.plain, [c.plain], 4, 32), "nearest: a query shard holds 1 to 32 molecules, not 40"),
    "nearest: a query shard and a CPU model": (lambda c: _sc().nearest(_model(9), c.few, [c.plain], 4, 32), NO_CPU_PATH),
    "nearest: a model without a head": (lambda c: _sc().nearest(_headless(), GOOD(), [c.plain], 4, 32), NO_HEAD),
    # --------------------------------------------------------------------------------------------- rank_embeddings
    "rank_embeddings: emb is a list": (lambda c: _sc().rank_embeddings([[0.0] * G], GOOD(), None), r"rank_embeddings: emb is a float32 \[n, G\] tensor"),
    "rank_embeddings: emb is a vector": (lambda c: _sc().rank_embeddings(torch.zeros(G), GOOD(), None), r"rank_embeddings: emb is a float32 \[n, G\] tensor"),
    "rank_embeddings: emb is float64":
        (lambda c: _sc().rank_embeddings(torch.zeros(10, G, dtype=torch.float64), GOOD(), None), r"rank_embeddings: emb is a float32 \[n, G\] tensor"),
    "rank_embeddings: emb of width 0": (lambda c: _sc().rank_embeddings(torch.zeros(10, 0), GOOD(), None), r"rank_embeddings: emb is a float32 \[n, G\] tensor"),
    "rank_embeddings: a malformed emb wins over malformed queries":
        (lambda c: _sc().rank_embeddings(torch.zeros(G), torch.zeros(G), None), r"rank_embeddings: emb is a float32 \[n, G\] tensor"),
    **{f"rank_embeddings: {name}": (lambda c, q=q: _sc().rank_embeddings(torch.zeros(10, G), q(), None), "rank_embeddings: " + word)
       for name, (q, word) in QUERIES.items()},
    "rank_embeddings: queries on the CPU win over emb on the CPU":
        (lambda c: _sc().rank_embeddings(torch.zeros(10, G), GOOD(), None), "rank_embeddings: " + ON_CPU + "$"),
    # ------------------------------------------------------------------------------------------- evaluate_resident
    "evaluate_resident: an unknown metric wins over a CPU model":
        (lambda c: _tr().evaluate_resident(_model(), c.plain, 32, metrics=("accuracy", "no such metric")), METRIC),
    "evaluate_resident: a CPU model": (lambda c: _tr().evaluate_resident(_model(), c.plain, 32, metrics=("AUC",)), NO_CPU_PATH),
    "evaluate_resident: a two-task model": (lambda c: _tr().evaluate_resident(_model(2), c.plain, 32), ONE_TASK),
    # ------------------------------------------------------------------------------------- evaluate_resident_tasks
    "evaluate_resident_tasks: an unknown metric wins over a shard without assays":
        (lambda c: _tr().evaluate_resident_tasks(_model(9), c.plain, 32, metrics=("no such metric",)), METRIC),
    "evaluate_resident_tasks: a shard without assays wins over the loss":
        (lambda c: _tr().evaluate_resident_tasks(_model(9, loss_func=torch.nn.L1Loss()), c.plain, 32),
         r"evaluate_resident_tasks needs a shard that knows every molecule's task: ResidentShard\(\.\.\., assays=\.\.\.\)"),
    "evaluate_resident_tasks: a loss that is none of the head's kinds wins over a CPU model":
        (lambda c: _tr().evaluate_resident_tasks(_model(9, loss_func=torch.nn.L1Loss()), c.nine, 32), "^evaluate_resident_tasks" + LOSS_KINDS),
    "evaluate_resident_tasks: a CPU model": (lambda c: _tr().evaluate_resident_tasks(_model(9), c.nine, 32), NO_CPU_PATH),
    "evaluate_resident_tasks: 33 outputs": (lambda c: _tr().evaluate_resident_tasks(_model(33), c.nine, 32), OUTPUTS + "33"),
    # ----------------------------------------------------------------------- evaluate / evaluate_tasks (the shared checks)
    "evaluate: an unknown metric": (lambda c: _tr().evaluate(_model(), [], metrics=("no such metric",)), METRIC),
    "evaluate: no batch": (lambda c: _tr().evaluate(_model(), []), "^evaluate needs at least one batch$"),
    "evaluate_tasks: an unknown metric wins over the loss":
        (lambda c: _tr().evaluate_tasks(_model(9, loss_func=torch.nn.L1Loss()), [], metrics=("no such metric",)), METRIC),
    "evaluate_tasks: a loss that is none of the head's kinds":
        (lambda c: _tr().evaluate_tasks(_model(9, loss_func=torch.nn.L1Loss()), []), "^evaluate_tasks" + LOSS_KINDS),
    "evaluate_tasks: no batch": (lambda c: _tr().evaluate_tasks(_model(9), []), "^evaluate_tasks needs at least one batch$"),
    # -------------------------------------------------------------------------------------------- TopK / TopKTasks
    "TopK: k = 0": (lambda c: _sc().TopK(0, "cuda:0"), r"k = 0 outside \[1, \d+\] \(MKGNN_TOPK_MAX_K\)"),
    "TopK: k above the limit": (lambda c: _sc().TopK(_max_k() + 1, "cuda:0"), r"k = \d+ outside \[1, \d+\] \(MKGNN_TOPK_MAX_K\)"),
    "TopK: on the CPU": (lambda c: _sc().TopK(4, "cpu"), r"a running list lives on the GPU \(topk_update_reference is the host form\)"),
    "TopK: k = 0 wins over the CPU": (lambda c: _sc().TopK(0, "cpu"), r"k = 0 outside"),
    "TopKTasks: no task": (lambda c: _sc().TopKTasks(4, 0, "cuda:0"), r"n_tasks = 0 outside \[1, 32\] \(MKGNN_TASK_HEAD_MAX_TASKS\)"),
    "TopKTasks: 33 tasks": (lambda c: _sc().TopKTasks(4, 33, "cuda:0"), r"n_tasks = 33 outside \[1, 32\] \(MKGNN_TASK_HEAD_MAX_TASKS\)"),
    "TopKTasks: 33 tasks win over k = 0": (lambda c: _sc().TopKTasks(0, 33, "cpu"), r"n_tasks = 33 outside"),
    "TopKTasks: k above the limit": (lambda c: _sc().TopKTasks(_max_k() + 1, 9, "cuda:0"), r"k = \d+ outside \[1, \d+\] \(MKGNN_TOPK_MAX_K\)"),
    "TopKTasks: k = 0 wins over the CPU": (lambda c: _sc().TopKTasks(0, 9, "cpu"), r"k = 0 outside"),
    "TopKTasks: on the CPU": (lambda c: _sc().TopKTasks(4, 9, "cpu"), r"a running list lives on the GPU \(topk_update_reference is the host form\)"),
    # ------------------------------------------------------------------------ GNNModel's scoring calls in training mode
    "predict: training mode":
        (lambda c: _model().predict(object()), r"^GNNModel\.predict needs evaluation mode: call model\.eval\(\) first \(train\.evaluate does\)$"),
    "embed: training mode": (lambda c: _model().embed(object()), r"^GNNModel\.embed needs evaluation mode: call model\.eval\(\) first$"),
    "predict_tasks: training mode":
        (lambda c: _model(9).predict_tasks(object()), r"^GNNModel\.predict_tasks needs evaluation mode: call model\.eval\(\) first$"),
}


@pytest.mark.parametrize("name", list(CELLS))
def test_refused_before_the_library_is_loaded(name, ctx, monkeypatch):
    from molkgnn_amd import _lib

    def no_load():
        raise AssertionError("the library was loaded before the refusal")

    monkeypatch.setattr(_lib, "load", no_load)
    torch.manual_seed(0)
    call, word = CELLS[name]
    with pytest.raises(ValueError, match=word):
        call(ctx)


@pytest.mark.parametrize("entry", ["score_resident", "score_resident_tasks", "embed_resident", "screen", "screen_tasks",
                                   "evaluate_resident", "evaluate_resident_tasks"])
@pytest.mark.parametrize("training", [True, False])
def test_a_refused_model_keeps_its_mode(entry, training, ctx):
    model = _model(9).train(training)
    module = _tr() if entry.startswith("evaluate") else _sc()
    args = ([ctx.nine], 4, 32) if entry.startswith("screen") else (ctx.nine, 32)
    with pytest.raises(ValueError):
        getattr(module, entry)(model, *args)
    assert model.training is training


@pytest.mark.parametrize("training", [True, False])
def test_evaluation_mode_restores_the_mode_after_a_body_that_raises(training):
    from molkgnn_amd.train import evaluation_mode
    model = _model().train(training)
    with pytest.raises(RuntimeError, match="stop"):
        with evaluation_mode(model):
            assert not model.training
            raise RuntimeError("stop")
    assert model.training is training
    with evaluation_mode(model):                          # ... and after one that does not
        assert not model.training
    assert model.training is training
