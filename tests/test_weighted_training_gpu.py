"""Weighted losses through ``train.GNNModel.loss``: ``BCEWithLogitsLoss(pos_weight=...)`` and per-molecule weights on the HIP head
and fused tail, a nine-task model with per-task positive weights, a resident shard's weights inside one captured step, and the
unweighted models under ``MKGNN_WEIGHTED_LOSS=0``.  64-molecule synthetic batches.  ``pytest -m gpu``."""
import copy
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import _f64 as F64
from tests.test_regression_tail import _close

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dev():
    assert torch.cuda.is_available(), "pytest -m gpu needs the MI355X"
    return torch.device("cuda:0")


@pytest.mark.parametrize("route", ["tail", "head"])
@pytest.mark.parametrize("weights", [False, True])
def test_pos_weight_model_takes_the_weighted_hip_route(route, weights, monkeypatch):
    """``GNNModel(loss_func=BCEWithLogitsLoss(pos_weight=tensor([7.])))``: the weighted fused tail (or, with the tail switched
    off, the separate operators + the weighted head), and torch's own loss of ``model(batch)[0]`` at dropout 0 in evaluation-mode
    batch norm -- the loss and every parameter gradient inside ``_close``."""
    from molkgnn_amd import readout as R
    from molkgnn_amd.synthetic import make_batch
    from molkgnn_amd.train import GNNModel
    dev = _dev()
    if route == "head":
        monkeypatch.setattr(R, "_FUSED_TAIL", False)
    torch.manual_seed(0)
    model = GNNModel(dropout_ratio=0.0, ffn_dropout_rate=0.0, loss_func=torch.nn.BCEWithLogitsLoss(pos_weight=torch.tensor([7.0])))
    model = model.to(dev).eval()
    assert model._loss_kind() is None and model.loss_func.pos_weight.device == dev
    ref = copy.deepcopy(model)
    b = make_batch(64, seed=21).to(dev)
    s = None
    if weights:
        # (zeros among them, none above 1 -- label confidences: the loss, every gradient and its float32 rounding keep the scale of
        # the pos_weight-only case, which is what _close's absolute floor of 2e-11 is sized for.  Measured with weights up to 3:
        # layers.0...center_attr_sc_weight, whose gradient is 1.5e-7 at its largest, differed from torch's by 3.3e-11 on the tail
        # route and by 2.5e-11 on the separate operators -- float32 rounding of the convolution's backward, scaled by the weights)
        s = (torch.arange(64, device=dev) % 5).float() * 0.25
        b.weight = s
    model.zero_grad(set_to_none=True)
    loss = model.loss(b)
    assert type(loss.grad_fn).__name__ == ("_WeightedTailFnBackward" if route == "tail" else "_WeightedTaskHeadFnBackward")
    loss.backward()
    ref.zero_grad(set_to_none=True)
    want = F.binary_cross_entropy_with_logits(ref(b)[0].view(-1), b.y.view(-1).float(), weight=s, pos_weight=ref.loss_func.pos_weight)
    want.backward()
    torch.cuda.synchronize()
    print(f"pos_weight model {route} weights={weights}: loss {float(loss)!r} torch {float(want)!r}")
    _close(loss.detach().reshape(1), want.detach().reshape(1))
    checked = 0
    for (n, p), (_, q) in zip(model.named_parameters(), ref.named_parameters()):
        if q.grad is not None:
            assert p.grad is not None, n
            print(f"  {n}: err {float((p.grad - q.grad).abs().max()):.3e} max|torch| {float(q.grad.abs().max()):.3e}")
            _close(p.grad, q.grad)
            checked += 1
    assert checked > 70


def _nine_task_batch(dev, seed=7):
    from molkgnn_amd.sampling import task_index
    from molkgnn_amd.synthetic import NINE_ASSAYS, make_batch
    batch = make_batch(64, seed=seed, assay="all9")
    batch.task = task_index(batch.assay_id, [int(a) for a in NINE_ASSAYS])
    batch.task[::7] = -1                                                 # (some without a label)
    g = torch.Generator().manual_seed(seed)
    batch.weight = torch.rand(64, generator=g) * 2
    batch.weight[::5] = 0.0
    return batch


def test_nine_task_model_with_positive_weights_and_sample_weights():
    """``[9]`` positive weights, ``batch.task`` and ``batch.weight``: the weighted task-indexed head, against
    ``task_head_reference`` on the model's own embedding (float32 and float64 legs, ``tests/_f64.check``)."""
    from molkgnn_amd import readout as R
    from molkgnn_amd.sampling import pos_weights
    from molkgnn_amd.train import GNNModel, backward
    dev = _dev()
    batch = _nine_task_batch(dev)
    pw = pos_weights(batch.y, batch.task, 9).clamp(0.5, 40.0) + torch.arange(9) * 0.25
    bd = batch.to(dev)
    torch.manual_seed(0)
    model = GNNModel(num_layers=2, task_dim=9, dropout_ratio=0.0, ffn_dropout_rate=0.0,
                     loss_func=torch.nn.BCEWithLogitsLoss(pos_weight=pw.clone())).to(dev).train()
    model.zero_grad(set_to_none=True)
    loss = model.loss(bd)
    assert type(loss.grad_fn).__name__ == "_WeightedTaskHeadFnBackward"
    emb = loss.grad_fn.saved_tensors[0].detach().clone()
    backward(loss)
    torch.cuda.synchronize()
    legs = []
    for dt in (torch.float32, torch.float64):
        w = model.ffn.weight.detach().cpu().to(dt).requires_grad_(True)
        b = model.ffn.bias.detach().cpu().to(dt).requires_grad_(True)
        l, _ = R.task_head_reference(emb.cpu().to(dt), w, b, batch.y.to(dt), batch.task, "bce", sample_weight=batch.weight.to(dt),
                                     pos_weight=pw.to(dt))
        l.backward()
        legs.append({"loss": l.detach(), "ffn.weight": w.grad, "ffn.bias": b.grad})
    got = {"loss": loss.detach(), "ffn.weight": model.ffn.weight.grad, "ffn.bias": model.ffn.bias.grad}
    assert F64.check(got, *legs, "weighted_head:model9") == 3
    grads = [p.grad for n, p in model.named_parameters() if n.startswith("gnn_model") and p.grad is not None]
    assert len(grads) > 30 and all(bool(torch.isfinite(g).all()) for g in grads) and any(float(g.abs().max()) > 0 for g in grads)


def test_one_captured_step_reads_a_resident_shards_weights(tmp_path):
    """``ResidentShard(..., assays=..., weights=w)`` + ``CompactStaticBatch.gather`` inside ONE captured step replayed with three
    id lists (one with repeats): each replay's loss and ``ffn.weight.grad`` equal, bit for bit, an eager run on the same ids with
    ``data.task`` and ``data.weight`` set directly, whose loss is the definition's on its own embedding."""
    from molkgnn_amd import padding as P, readout as R, shards as S
    from molkgnn_amd.receptive_field import attach_receptive_fields
    from molkgnn_amd.synthetic import NINE_ASSAYS, make_batch
    from molkgnn_amd.train import GNNModel, backward
    dev = _dev()
    whole = make_batch(64, seed=12, assay="all9", with_receptive_fields=False)
    path = str(tmp_path / "all9.mkgs")
    S.write_shard(path, whole)
    w = np.random.default_rng(5).random(64).astype(np.float32) * 3
    w[::6] = 0.0
    res = S.ResidentShard(S.Shard(path), dev, assays=[int(a) for a in NINE_ASSAYS], weights=w)
    assert res.tensors["weight"].dtype == torch.float32 and torch.equal(res.tensors["weight"].cpu(), torch.from_numpy(w))
    rows = np.random.default_rng(3).integers(0, 64, size=(4, 16))
    rows[2, 5] = rows[2, 11] = rows[2, 12]                    # (repeated ids)
    loader = S.ResidentLoader(res, 16, rows.reshape(-1), dev)
    batches = list(loader)
    pw = torch.linspace(0.5, 40.0, 9)
    torch.manual_seed(1)
    model = GNNModel(num_layers=2, task_dim=9, dropout_ratio=0.0, ffn_dropout_rate=0.0,
                     loss_func=torch.nn.BCEWithLogitsLoss(pos_weight=pw.clone())).to(dev).train()
    csb = P.CompactStaticBatch(loader.shape, 16, res.x_dim, res.p_dim, res.e_dim, dev, max_mol_atoms=loader.max_mol_atoms,
                               max_mol_edges=loader.max_mol_edges)

    def step():
        csb.gather(res)
        csb.expand()
        attach_receptive_fields(csb.data, sizes=csb.data.bucket_sizes, overlap=True)
        model.zero_grad(set_to_none=True)
        loss = model.loss(csb.data)
        backward(loss)
        return loss

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        csb.gather(res, batches[0])
        assert csb.data.weight_table is res.tensors["weight"] and csb.data.weight_rows is csb.ids
        assert csb.data.task_table is res.tensors["task"] and csb.data.task_rows is csb.ids
        for _ in range(2):
            loss = step()
        assert type(loss.grad_fn).__name__ == "_WeightedTaskHeadFnBackward"
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            static_loss = step()
        got = []
        for k in (1, 2, 3):
            csb.ids.copy_(batches[k])
            g.replay()
            got.append((static_loss.detach().clone(), model.ffn.weight.grad.detach().clone()))
        want, defined = [], []
        for k in (1, 2, 3):
            csb.ids.copy_(batches[k])
            csb.data.task = res.tensors["task"][csb.ids.long()]
            csb.data.weight = res.tensors["weight"][csb.ids.long()]
            loss = step()
            with torch.no_grad():
                emb = model.gnn_model(csb.data)              # (training-mode batch norm: the embedding the step's head saw)
            ref, _ = R.task_head_reference(emb.double(), model.ffn.weight.detach().double(), model.ffn.bias.detach().double(),
                                           csb.data.y.double(), csb.data.task, "bce", n_rows=16, sample_weight=csb.data.weight.double(),
                                           pos_weight=pw.to(dev).double())
            want.append((loss.detach().clone(), model.ffn.weight.grad.detach().clone()))
            defined.append(ref)
            del csb.data.task, csb.data.weight
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for k in range(3):
        assert torch.equal(got[k][0], want[k][0]), (k, float(got[k][0]), float(want[k][0]))
        assert torch.equal(got[k][1], want[k][1]), k
        assert abs(float(want[k][0]) - float(defined[k])) <= 1e-5 * abs(float(defined[k])), (k, float(want[k][0]), float(defined[k]))
    assert len({float(l) for l, _ in got}) == 3 and float(got[0][0]) > 0.0
    assert csb.gather_status() == 0
    # a shard without weights clears the table again
    csb.gather(S.ResidentShard(S.Shard(path), dev, assays=[int(a) for a in NINE_ASSAYS]), batches[0])
    assert csb.data.weight_table is None and csb.data.weight_rows is None


_CHILD = r"""
import hashlib, json, sys
sys.path.insert(0, {repo!r})
import torch
from molkgnn_amd import readout as R
from molkgnn_amd.sampling import task_index
from molkgnn_amd.synthetic import NINE_ASSAYS, make_batch
from molkgnn_amd.train import GNNModel, backward
dev = torch.device("cuda:0")
out = {{"switch": R._WEIGHTED_LOSS}}
def digest(model, loss):
    h = hashlib.sha256(loss.detach().cpu().numpy().tobytes())
    for n, p in model.named_parameters():
        if p.grad is not None:
            h.update(n.encode()); h.update(p.grad.detach().cpu().numpy().tobytes())
    return h.hexdigest()
for name, task_dim, assay in (("single", 1, None), ("mixed", 9, "all9")):
    torch.manual_seed(4)
    model = GNNModel(num_layers=2, task_dim=task_dim).to(dev).train()
    b = make_batch(64, seed=31, **({{}} if assay is None else {{"assay": assay}}))
    if assay is not None:
        b.task = task_index(b.assay_id, [int(a) for a in NINE_ASSAYS])
    b = b.to(dev)
    R.reset_head_rng(dev, seed=77)
    model.zero_grad(set_to_none=True)
    loss = model.loss(b)
    out[name + "_fn"] = type(loss.grad_fn).__name__
    backward(loss)
    torch.cuda.synchronize()
    out[name] = digest(model, loss)
# a weighted model: the kernels, or (switch off) the definition in torch operators
torch.manual_seed(4)
model = GNNModel(num_layers=2, ffn_dropout_rate=0.0, loss_func=torch.nn.BCEWithLogitsLoss(pos_weight=torch.tensor([7.0]))).to(dev).train()
b = make_batch(64, seed=31).to(dev)
loss = model.loss(b)
out["weighted_fn"], out["weighted_loss"] = type(loss.grad_fn).__name__, float(loss)
print("RESULT " + json.dumps(out))
"""


def _child(switch):
    import json
    env = dict(os.environ)
    env.pop("MKGNN_WEIGHTED_LOSS", None)
    if switch is not None:
        env["MKGNN_WEIGHTED_LOSS"] = switch
    done = subprocess.run([sys.executable, "-c", _CHILD.format(repo=REPO)], env=env, cwd=REPO, capture_output=True, text=True, timeout=300)
    assert done.returncode == 0, done.stderr[-2000:]
    line = [l for l in done.stdout.splitlines() if l.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


def test_unweighted_models_do_not_see_the_switch():
    """An unweighted ``GNNModel`` and an unweighted mixed-assay model: bit-identical loss and gradients with and without
    ``MKGNN_WEIGHTED_LOSS=0`` (fresh child processes: the switch is read once).  The weighted model leaves the kernels under it and
    keeps its loss."""
    on, off = _child(None), _child("0")
    assert on["switch"] is True and off["switch"] is False
    for name in ("single", "mixed"):
        assert on[name] == off[name], name
        assert on[name + "_fn"] == off[name + "_fn"] and "Weighted" not in on[name + "_fn"]
    assert on["mixed_fn"] == "_TaskHeadFnBackward"
    assert on["weighted_fn"] in ("_WeightedTailFnBackward", "_WeightedTaskHeadFnBackward")
    assert "Weighted" not in off["weighted_fn"]
    assert abs(on["weighted_loss"] - off["weighted_loss"]) <= 2e-5 * abs(off["weighted_loss"])
