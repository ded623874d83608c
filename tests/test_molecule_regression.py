"""The molecule-resident step (molkgnn_amd.molecule, csrc/kgnn_molecule.hip) with the squared-error loss kinds
(MKGNN_MOLECULE_SQERR / MKGNN_MOLECULE_SUM): ``loss_forward`` against the per-operator path and float64, and the docking-score
training step at 16 molecules end to end.  (The file name carries ``test_molecule``: tests/conftest.py leaves the
molecule-resident path on for it.)  ``pytest -m gpu``."""
import copy

import pytest
import torch

from tests.test_regression_tail import _e2e

pytestmark = pytest.mark.gpu


def _dev():
    assert torch.cuda.is_available(), "pytest -m gpu needs the MI355X"
    return torch.device("cuda:0")


@pytest.mark.parametrize("loss", ["mse", "mse_sum"])
@pytest.mark.parametrize("mols", [16, 256])
def test_loss_forward_against_the_per_operator_path_and_float64(loss, mols, monkeypatch):
    from molkgnn_amd import _lib
    from molkgnn_amd import molecule as M
    from molkgnn_amd import readout as R
    from molkgnn_amd.synthetic import make_batch
    from molkgnn_amd.train import GNNModel
    from molkgnn_amd.train import backward as train_backward
    dev = _dev()
    torch.manual_seed(50 + mols)
    lf = torch.nn.MSELoss(reduction="mean" if loss == "mse" else "sum")
    model = GNNModel(ffn_dropout_rate=0.0, loss_func=lf).to(dev).train()
    ref_model = copy.deepcopy(model)
    b = make_batch(mols, seed=700 + mols, target="docking_score").to(dev)
    b.num_graphs = mols
    # the one-launch step (HEAD | BACKWARD with the kind's mode bits), the embedding captured
    monkeypatch.setattr(M, "_MODE", "1")
    cap = {}
    monkeypatch.setattr(M, "debug_capture", cap)
    calls = []
    orig = M._run
    monkeypatch.setattr(M, "_run", lambda *a, **k: (calls.append(a[6]), orig(*a, **k))[1])
    kind_bits = _lib.MOLECULE_SQERR | (_lib.MOLECULE_SUM if loss == "mse_sum" else 0)
    out = M.loss_forward(model, b, 0.0, loss)
    assert out is not None and calls == [_lib.MOLECULE_HEAD | _lib.MOLECULE_BACKWARD | kind_bits], calls
    train_backward(out)
    assert len(calls) == 1                                 # the backward launched nothing
    got = {n: p.grad for n, p in model.named_parameters() if p.grad is not None}
    # float64 on the step's own embedding: loss, pred and the head's gradients
    e64 = cap["emb"].detach().double().requires_grad_(True)
    w64 = model.ffn.weight.detach().double().requires_grad_(True)
    b64 = model.ffn.bias.detach().double().requires_grad_(True)
    p64 = (e64 @ w64.t() + b64).view(-1)
    l64 = torch.nn.MSELoss(reduction=lf.reduction)(p64, b.y.double())
    gw, gb = torch.autograd.grad(l64, [w64, b64])
    assert abs(float(out) - float(l64)) <= 2e-6 * max(1.0, abs(float(l64))), (float(out), float(l64))
    assert float((cap["pred"].double() - p64.detach()).abs().max()) <= 2e-5 * max(float(p64.abs().max()), 1.0)
    for g, w in ((model.ffn.weight.grad, gw), (model.ffn.bias.grad, gb)):
        assert float((g.double() - w).abs().max()) <= 2e-5 * max(float(w.abs().max()), 1e-6)
    # the per-operator head kernels fed the same embedding: the same loss and head gradients
    emb = cap["emb"].detach().clone().requires_grad_(True)
    ffn = copy.deepcopy(ref_model.ffn)
    out2 = R.head_loss(emb, ffn, b.y, loss)
    out2.backward()
    assert abs(float(out) - float(out2)) <= 2e-6 * max(1.0, abs(float(out2))), (float(out), float(out2))
    for g, w in ((model.ffn.weight.grad, ffn.weight.grad), (model.ffn.bias.grad, ffn.bias.grad)):
        assert float((g - w).abs().max()) <= 2e-5 * max(float(w.abs().max()), 1e-6)
    # ... and the whole per-operator network (other kernels, other summation orders -- and where two neighbour orders score
    # within rounding, possibly the other choice: a loose bound) on the same parameters gives the same loss
    monkeypatch.setattr(M, "_MODE", "0")
    monkeypatch.setattr(M, "debug_capture", None)
    ref = ref_model.loss(b)
    assert len(calls) == 1
    assert abs(float(out) - float(ref)) <= 1e-3 * abs(float(ref)), (float(out), float(ref))
    assert len(got) > 70 and all(torch.isfinite(g).all() for g in got.values())


def test_molecule_step_rejects_sum_without_squared_error(monkeypatch):
    """MKGNN_MOLECULE_SUM alone (a summed BCE) is not a loss kind: refused on the host."""
    from molkgnn_amd import _lib
    from molkgnn_amd import molecule as M
    from molkgnn_amd.synthetic import make_batch
    from molkgnn_amd.train import GNNModel
    dev = _dev()
    torch.manual_seed(1)
    model = GNNModel(ffn_dropout_rate=0.0).to(dev).train()
    b = make_batch(8, seed=8).to(dev)
    b.num_graphs = 8
    monkeypatch.setattr(M, "_MODE", "1")
    monkeypatch.setitem(M._KIND_MODE, _lib.LOSS_BCE_MEAN, _lib.MOLECULE_SUM)
    with pytest.raises(_lib.MolKGNNLibraryError, match="SUM needs SQERR"):
        M.loss_forward(model, b, 0.0, "bce")


@pytest.mark.parametrize("captured", [False, True])
def test_docking_step_at_16_molecules(captured, monkeypatch):
    from molkgnn_amd import molecule as M
    monkeypatch.setattr(M, "_MODE", "1")
    calls = []
    orig = M._run
    monkeypatch.setattr(M, "_run", lambda *a, **k: (calls.append(a[6]), orig(*a, **k))[1])
    tails = _e2e(16, captured, monkeypatch)
    assert not tails and calls                              # the molecule-resident step took it, not the fused tail
