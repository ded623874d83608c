"""Training and evaluating on a label matrix with holes (``GNNModel.loss`` on ``batch.labels`` / ``label_table``;
``shards.ResidentShard(labels=...)``; ``train.evaluate_resident_labels``) on the GPU.  ``pytest -m gpu``.

About 40 synthetic molecules, T = 9, 30 % of the entries present.  Bound of every value check: ``tests/_f64.check`` against
``readout.label_head_reference`` in float64 on the model's own float32 embedding."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import _f64 as F64
from tests import _label_training_child as LT

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dev():
    assert torch.cuda.is_available(), "pytest -m gpu needs the MI355X"
    return torch.device("cuda:0")


def _spy(monkeypatch):
    from molkgnn_amd import _lib
    calls = []
    real = _lib.check
    monkeypatch.setattr(_lib, "check", lambda rc, what: (calls.append(what), real(rc, what))[1])
    return calls


def _legs(got, model, labels, kind="bce", **kw):
    """The float32 and float64 legs of ``got`` (``LT.loss_and_head_gradients``): the definition on ``got['emb']``."""
    from molkgnn_amd.readout import label_head_reference
    legs = []
    for dt in (torch.float32, torch.float64):
        w = model.ffn.weight.detach().cpu().to(dt).requires_grad_(True)
        b = model.ffn.bias.detach().cpu().to(dt).requires_grad_(True)
        cast = {k: (None if v is None else v.detach().cpu().to(dt)) for k, v in kw.items()}
        loss, _ = label_head_reference(got["emb"].cpu().to(dt), w, b, labels.cpu().to(dt), kind, **cast)
        loss.backward()
        legs.append({"loss": loss.detach(), "ffn.weight": w.grad, "ffn.bias": b.grad})
    return legs


@pytest.mark.parametrize("weighted", [False, True])
def test_model_loss_is_the_definition_on_its_own_embedding(weighted, monkeypatch):
    dev = _dev()
    kw = {}
    if weighted:
        from molkgnn_amd.sampling import label_pos_weights
        kw = dict(loss_func=torch.nn.BCEWithLogitsLoss(pos_weight=label_pos_weights(LT.label_matrix(40, 8))))
    model, batch = LT.model_and_batch(dev, **kw)
    extra = {}
    if weighted:
        batch.weight = torch.rand(40, generator=torch.Generator().manual_seed(3)) + 0.5
        extra = dict(sample_weight=batch.weight, pos_weight=model.loss_func.pos_weight)
    bd = batch.to(dev)
    calls = _spy(monkeypatch)
    got = LT.loss_and_head_gradients(model, bd)
    assert "mkgnn_label_head_fused" in calls and not [c for c in calls if "tail" in c or "molecule" in c or "task_head" in c], calls
    assert float(got["loss"]) > 0.0
    for n, p in model.named_parameters():                     # every parameter the PyTorch formulation reaches gets a gradient
        if n.startswith("gnn_model.") or n.startswith("ffn."):
            assert p.grad is None or bool(torch.isfinite(p.grad).all()), n
    assert sum(p.grad is not None for n, p in model.named_parameters() if n.startswith("gnn_model.")) > 10
    n = F64.check({k: got[k] for k in ("loss", "ffn.weight", "ffn.bias")}, *_legs(got, model, batch.labels, **extra),
                  f"label_head:model:weighted={weighted}")
    assert n == 3
    # n_valid_molecules: only the leading molecules enter the loss
    bd.n_valid_molecules = 33
    got = LT.loss_and_head_gradients(model, bd)
    trimmed = batch.labels.clone()
    trimmed[33:] = LT.NAN
    assert F64.check({k: got[k] for k in ("loss", "ffn.weight", "ffn.bias")}, *_legs(got, model, trimmed, **extra),
                     f"label_head:model:n_valid:weighted={weighted}") == 3


def test_a_batch_with_labels_and_tasks_raises():
    dev = _dev()
    model, batch = LT.model_and_batch(dev)
    batch.task = torch.zeros(40, dtype=torch.int32)
    with pytest.raises(ValueError, match="both tasks"):
        model.loss(batch.to(dev))


def test_a_batch_without_labels_keeps_its_route_and_bits(monkeypatch):
    """With the label fields absent -- never set, or cleared to None as ``gather`` leaves them -- the task-indexed route and the
    single-task route run what they ran: the same launches and the same bits as the operators they are made of."""
    from molkgnn_amd import readout as R
    from molkgnn_amd.sampling import task_index
    from molkgnn_amd.synthetic import NINE_ASSAYS, make_batch
    from molkgnn_amd.train import GNNModel
    dev = _dev()
    nine = [int(a) for a in NINE_ASSAYS]
    for task_dim in (9, 1):
        batch = make_batch(40, seed=7, assay="all9")
        if task_dim == 9:
            batch.task = task_index(batch.assay_id, nine)
        bd = batch.to(dev)
        torch.manual_seed(0)
        model = GNNModel(num_layers=2, task_dim=task_dim, dropout_ratio=0.0, ffn_dropout_rate=0.0).to(dev).train()
        calls = _spy(monkeypatch)
        plain = model.loss(bd).detach().clone()
        first = list(calls)
        bd.labels = bd.label_table = bd.label_rows = None
        del calls[:]
        cleared = model.loss(bd).detach().clone()
        torch.cuda.synchronize()
        heads = lambda names: [c for c in names if "head" in c or "tail" in c or "molecule" in c]     # (plans are cached: not compared)
        assert heads(calls) == heads(first) and not [c for c in calls if "label_head" in c], (task_dim, calls, first)
        assert torch.equal(plain, cleared), task_dim
        if task_dim == 9:
            assert "mkgnn_task_head_fused" in calls
            want = R.task_head_loss(model.gnn_model(bd), model.ffn, bd.y, bd.task, "bce").detach()
            assert torch.equal(plain, want)
        else:
            assert [c for c in calls if c in ("mkgnn_molecule_step", "mkgnn_tail_fused", "mkgnn_bce_head_fused")], calls
        monkeypatch.undo()


def test_the_torch_route_in_a_fresh_process_agrees_with_the_kernels(tmp_path):
    """``MKGNN_LABEL_HEAD=0`` is read once at import: a child process runs the same loss on the definition in torch operators;
    both routes are inside the bound of the definition in float64 on their own embedding."""
    dev = _dev()
    model, batch = LT.model_and_batch(dev)
    here = LT.loss_and_head_gradients(model, batch.to(dev))
    out = tmp_path / "child.pt"
    done = subprocess.run([sys.executable, "-m", "tests._label_training_child", str(out)], cwd=REPO,
                          env=dict(os.environ, MKGNN_LABEL_HEAD="0"), capture_output=True, text=True, timeout=300)
    assert done.returncode == 0, (done.returncode, done.stderr[-2000:])
    there = torch.load(out)
    assert there["label_head"] is False
    for tag, got in (("kernels", here), ("torch", there)):
        assert F64.check({k: got[k] for k in ("loss", "ffn.weight", "ffn.bias")}, *_legs(got, model, batch.labels),
                         f"label_head:model:{tag}") == 3
    assert abs(float(here["loss"]) - float(there["loss"])) <= 1e-5 * abs(float(here["loss"]))


# ------------------------------------------------------------------------------ the resident captured step --
def _resident(tmp_path, dev, mols=48):
    from molkgnn_amd import shards as S
    from molkgnn_amd.synthetic import make_batch
    whole = make_batch(mols, seed=12, assay="all9", with_receptive_fields=False)
    path = str(tmp_path / "all9.mkgs")
    S.write_shard(path, whole)
    labels = LT.label_matrix(mols, 21)
    return S.ResidentShard(S.Shard(path), dev, labels=labels), labels


def test_one_captured_graph_serves_label_matrix_batches(tmp_path):
    """gather -> expand -> receptive fields -> ``train.training_step`` captured ONCE on a resident shard with a label matrix, fed
    by a ``ResidentLoader``, and replayed on two id rows (one with a repeated id): each replay's loss and ffn gradients equal, bit
    for bit, an eager step from the same state on the same ids with ``data.labels = label_table[ids]`` set directly."""
    from molkgnn_amd import padding as P, shards as S
    from molkgnn_amd.receptive_field import attach_receptive_fields
    from molkgnn_amd.train import GNNModel, training_step
    dev = _dev()
    res, labels = _resident(tmp_path, dev)
    assert res.tensors["labels"].dtype == torch.float32 and res.tensors["labels"].shape == (48, LT.T)
    assert torch.equal(res.tensors["labels"].cpu().nan_to_num(-1.0), labels.nan_to_num(-1.0)) and "task" not in res.tensors
    rows = np.random.default_rng(3).integers(0, 48, size=(3, 16))
    rows[2, 5] = rows[2, 11]                                  # (a repeated id)
    loader = S.ResidentLoader(res, 16, rows.reshape(-1), dev)
    batches = list(loader)
    torch.manual_seed(1)
    model = GNNModel(num_layers=2, task_dim=LT.T, dropout_ratio=0.0, ffn_dropout_rate=0.0).to(dev).train()
    csb = P.CompactStaticBatch(loader.shape, 16, res.x_dim, res.p_dim, res.e_dim, dev, max_mol_atoms=loader.max_mol_atoms,
                               max_mol_edges=loader.max_mol_edges)

    def step():
        csb.gather(res)
        csb.expand()
        attach_receptive_fields(csb.data, sizes=csb.data.bucket_sizes, overlap=True)
        return training_step(model, csb.data)                 # (no optimiser: the state stays what it is)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        csb.gather(res, batches[0])
        assert csb.data.label_table is res.tensors["labels"] and csb.data.label_rows is csb.ids
        for _ in range(2):
            step()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            static_loss = step()
        got = []
        for k in (1, 2):
            csb.ids.copy_(batches[k])
            g.replay()
            got.append((static_loss.detach().clone(), model.ffn.weight.grad.detach().clone(), model.ffn.bias.grad.detach().clone()))
        want = []
        for k in (1, 2):
            csb.ids.copy_(batches[k])
            csb.data.labels = res.tensors["labels"][csb.ids.long()]       # (given directly: taken before the table)
            loss = step()
            want.append((loss.detach().clone(), model.ffn.weight.grad.detach().clone(), model.ffn.bias.grad.detach().clone()))
            del csb.data.labels
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for k in range(2):
        assert torch.equal(got[k][0], want[k][0]), (k, float(got[k][0]), float(want[k][0]))
        assert torch.equal(got[k][1], want[k][1]) and torch.equal(got[k][2], want[k][2]), k
    assert float(got[0][0]) != float(got[1][0]) and float(got[0][0]) > 0.0
    assert csb.gather_status() == 0
    # a shard without labels clears the fields: the batch is back on the route it had
    plain = S.ResidentShard(res.shard, dev)
    csb.gather(plain)
    assert csb.data.label_table is None and csb.data.label_rows is None


def test_evaluate_resident_labels_scores_every_task(tmp_path):
    from molkgnn_amd import evaluation as E
    from molkgnn_amd.screening import score_resident_tasks
    from molkgnn_amd.train import GNNModel, evaluate_resident_labels
    dev = _dev()
    res, labels = _resident(tmp_path, dev)
    labels = labels.to(dev)
    torch.manual_seed(0)
    model = GNNModel(num_layers=2, task_dim=LT.T, dropout_ratio=0.0, ffn_dropout_rate=0.0).to(dev).train()
    out = evaluate_resident_labels(model, res, 16, metrics=("AUC",))
    assert model.training
    pred = score_resident_tasks(model, res, 16)
    assert pred.shape == (48, LT.T)
    lab = ~torch.isnan(labels)
    assert out["n_labelled"] == lab.sum(dim=0).tolist() and sum(out["n_labelled"]) == out["pred_y"].numel() == out["task"].numel()
    for t in range(LT.T):
        rows = lab[:, t]
        want = E.calculate_auc(labels[rows, t], pred[rows, t]) if bool(rows.any()) else float("nan")
        assert out["AUC"][t] == want or (want != want and out["AUC"][t] != out["AUC"][t]), t
    assert bool(torch.isfinite(out["loss"])) and set(out) >= {"loss", "AUC", "AUC_mean", "pred_y", "true_y", "task", "n_labelled"}
    with pytest.raises(ValueError, match="labels"):
        evaluate_resident_labels(model, type(res)(res.shard, dev), 16)
