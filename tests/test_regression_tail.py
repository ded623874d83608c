"""The fused tail with the squared-error loss kinds (readout.tail_loss(..., loss=...); csrc/kgnn_tail.hip, template parameter LK)
and the docking-score training step end to end (``GNNModel(loss_func=MSELoss(reduction='sum'))``, reference data.py:49-53,
model.py:156).  ``pytest -m gpu``."""
import copy

import pytest
import torch

from tests.test_tail import _block_rows, _modules

pytestmark = pytest.mark.gpu

LS = (10, 20, 30, 50)


def _dev():
    assert torch.cuda.is_available(), "pytest -m gpu needs the MI355X"
    return torch.device("cuda:0")


def _close(got, want, rel=2e-5):
    err, scale = float((got.double() - want.double()).abs().max()), max(float(want.abs().max()), 1e-6)
    assert err <= rel * scale, (err, scale)


def _setup(mols, n_pad, seed):
    from molkgnn_amd import readout as R
    from molkgnn_amd.plan import plan_from_data
    from molkgnn_amd.synthetic import make_batch
    dev = _dev()
    b = make_batch(mols, seed=seed, target="docking_score").to(dev)
    plan = plan_from_data(b)
    seg = R.molecule_segments(b.batch, mols)
    assert R.tail_supported(110, 32, 32, LS) and R._tail_limits_ok(seg, plan)
    lin1, lin2, ffn = _modules(dev)
    sim0, inblock = _block_rows(b, plan, LS, dev, seed)
    n_rows = mols - n_pad
    return dev, b, plan, seg, (lin1, lin2, ffn), sim0, inblock, b.y[:n_rows].contiguous(), n_rows


def _run(how, loss, mods, plan, seg, sim0, inblock, y, n_rows, p_drop, dev):
    """(loss, block-row grad_sim, the six parameter gradients, generator state) of one forward + backward."""
    from molkgnn_amd import readout as R
    from molkgnn_amd.train import backward
    lin1, lin2, ffn = mods
    params = list(lin1.parameters()) + list(lin2.parameters()) + list(ffn.parameters())
    R.reset_head_rng(dev, seed=1234)
    for p in params:
        p.grad = None
    sim = sim0.detach().requires_grad_(True)
    if how == "separate":
        emb = R.readout_blocks(sim, plan, LS, lin1, lin2, None, seg)
        out = R.head_loss(emb, ffn, y, loss, dropout_p=p_drop, n_rows=n_rows)
        out.backward()
    elif how == "deferred":
        with R.deferred_tail_reduce(dev):
            out = R.tail_loss(sim, plan, LS, lin1, lin2, ffn, y, seg, p_drop, n_rows, loss=loss)
            backward(out)
    else:
        out = R.tail_loss(sim, plan, LS, lin1, lin2, ffn, y, seg, p_drop, n_rows, loss=loss)
        out.backward()
    torch.cuda.synchronize()
    gsim = torch.where(inblock, sim.grad, torch.zeros((), device=dev))
    return out.detach().clone(), gsim, [p.grad.clone() for p in params], R.head_rng_state(dev).clone()


@pytest.mark.parametrize("loss", ["mse", "mse_sum"])
@pytest.mark.parametrize("mols,n_pad,p_drop", [(4096, 0, 0.0), (4096, 0, 0.25), (5, 0, 0.0), (300, 7, 0.0), (300, 7, 0.25)])
def test_fused_tail_matches_the_separate_operators(loss, mols, n_pad, p_drop):
    dev, b, plan, seg, mods, sim0, inblock, y, n_rows = _setup(mols, n_pad, 61 + mols)
    l0, gs0, gp0, st0 = _run("separate", loss, mods, plan, seg, sim0, inblock, y, n_rows, p_drop, dev)
    l1, gs1, gp1, st1 = _run("fused", loss, mods, plan, seg, sim0, inblock, y, n_rows, p_drop, dev)
    assert torch.isfinite(l1) and abs(float(l0) - float(l1)) <= 2e-6 * max(1.0, abs(float(l0))), (float(l0), float(l1))
    _close(gs1, gs0)
    for a, c in zip(gp1, gp0):
        _close(a, c)
    assert torch.equal(st0, st1)
    # bit-reproducible, and the same bits inside a deferred region (the reduction launched later, same order)
    for how in ("fused", "deferred"):
        l2, gs2, gp2, st2 = _run(how, loss, mods, plan, seg, sim0, inblock, y, n_rows, p_drop, dev)
        assert torch.equal(l1, l2) and torch.equal(gs1, gs2) and all(torch.equal(u, v) for u, v in zip(gp1, gp2)), how
        assert torch.equal(st1, st2)


@pytest.mark.parametrize("loss", ["mse", "mse_sum"])
@pytest.mark.parametrize("mols,n_pad", [(4096, 0), (5, 0), (300, 7)])
def test_fused_tail_against_the_float64_formula(loss, mols, n_pad):
    dev, b, plan, seg, mods, sim0, inblock, y, n_rows = _setup(mols, n_pad, 71 + mols)
    lin1, lin2, ffn = mods
    params = list(lin1.parameters()) + list(lin2.parameters()) + list(ffn.parameters())
    l1, gs1, gp1, _ = _run("fused", loss, mods, plan, seg, sim0, inblock, y, n_rows, 0.0, dev)
    dense = torch.where(inblock, sim0, torch.zeros((), device=dev)).double().requires_grad_(True)
    p64 = [p.detach().double().requires_grad_(True) for p in params]
    w1, b1, w2, b2, wh, bh = p64
    src, dst = b.edge_index[0], b.edge_index[1]
    h = torch.zeros_like(dense).index_add_(0, dst, dense[src])                       # KernelLayer.py:119-123
    z = h @ w1.t() + b1
    z = z * torch.sigmoid(z)
    z = z @ w2.t() + b2
    emb = torch.zeros(mols, 32, dtype=torch.float64, device=dev).index_add_(0, b.batch, z)     # MolKGNNNet.py:144-146
    pred = (emb[:n_rows] @ wh.t() + bh).view(-1)
    ref = torch.nn.MSELoss(reduction="mean" if loss == "mse" else "sum")(pred, y.double())
    grads = torch.autograd.grad(ref, [dense] + p64)
    assert abs(float(l1) - float(ref)) <= 2e-5 * max(1.0, abs(float(ref))), (float(l1), float(ref))
    _close(gs1, torch.where(inblock, grads[0], torch.zeros((), device=dev, dtype=torch.float64)))
    for g, w in zip(gp1, grads[1:]):
        _close(g, w)


def test_bce_kind_is_the_default_tail_bit_for_bit():
    """tail_loss(loss='bce') == tail_loss() as it was, and == the BCE kind's separate operators."""
    from molkgnn_amd import readout as R
    dev, b, plan, seg, mods, sim0, inblock, _, n_rows = _setup(1000, 9, 83)
    y = (torch.rand(n_rows, device=dev) < 0.3).float()
    lin1, lin2, ffn = mods
    res = []
    for kw in ({}, {"loss": "bce"}):
        R.reset_head_rng(dev, seed=5)
        for p in list(lin1.parameters()) + list(lin2.parameters()) + list(ffn.parameters()):
            p.grad = None
        sim = sim0.detach().requires_grad_(True)
        out = R.tail_loss(sim, plan, LS, lin1, lin2, ffn, y, seg, 0.25, n_rows, **kw)
        out.backward()
        gsim = torch.where(inblock, sim.grad, torch.zeros((), device=dev))
        res.append([out.detach().clone(), gsim] + [p.grad.clone() for p in list(lin1.parameters()) + list(lin2.parameters()) + list(ffn.parameters())])
    assert all(torch.equal(u, v) for u, v in zip(*res))


# ---------------------------------------------------------------------------------------------- end to end ----
def _e2e(mols, captured, monkeypatch, seed=5):
    """GNNModel(loss_func=MSELoss(reduction='sum')) on a docking-score batch: the HIP step (training_step, or CapturedSteps
    replaying it) never calls GNNModel.forward, and gives the loss and every parameter gradient of the PyTorch route
    ``loss_func(model(data)[0].view(-1), data.y.view(-1))`` on the same parameters."""
    from molkgnn_amd import readout as R
    from molkgnn_amd.synthetic import make_batch
    from molkgnn_amd.train import CapturedSteps, GNNModel, training_step
    dev = _dev()
    torch.manual_seed(seed)
    model = GNNModel(ffn_dropout_rate=0.0, loss_func=torch.nn.MSELoss(reduction="sum")).to(dev).train()
    ref_model = copy.deepcopy(model)
    b = make_batch(mols, seed=seed + mols, target="docking_score").to(dev)
    tails = []
    real_tail = R.tail_loss
    monkeypatch.setattr(R, "tail_loss", lambda *a, **k: (tails.append(a[10] if len(a) > 10 else k.get("loss")), real_tail(*a, **k))[1])

    def no_forward(self, data):
        raise AssertionError("the HIP loss path called GNNModel.forward")
    with monkeypatch.context() as m:
        m.setattr(GNNModel, "forward", no_forward)
        if captured:
            steps = CapturedSteps(model, None, warmup=1)
            for _ in range(3):                          # eager, capture (+ replay), replay
                loss = steps(b)
            assert len(steps._graphs) == 1
        else:
            loss = training_step(model, b)
        torch.cuda.synchronize()
    grads = {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}
    ref_model.zero_grad(set_to_none=True)
    ref = ref_model.loss_func(ref_model(b)[0].view(-1), b.y.view(-1))
    ref.backward()
    want = {n: p.grad for n, p in ref_model.named_parameters() if p.grad is not None}
    assert abs(float(loss) - float(ref)) <= 1e-5 * abs(float(ref)), (float(loss), float(ref))
    assert set(grads) == set(want) and len(grads) > 70
    for n in want:
        assert float((grads[n] - want[n]).abs().max()) <= 1e-4 * max(float(want[n].abs().max()), 1e-6), n
    return tails


@pytest.mark.parametrize("captured", [False, True])
def test_docking_step_at_4096_molecules(captured, monkeypatch):
    tails = _e2e(4096, captured, monkeypatch)
    assert tails and set(tails) == {"mse_sum"}            # the fused tail took it, with the kind


def test_mean_squared_error_step_at_4096_molecules(monkeypatch):
    """MSELoss() (mean) through the same route."""
    from molkgnn_amd.synthetic import make_batch
    from molkgnn_amd.train import GNNModel, training_step
    dev = _dev()
    torch.manual_seed(9)
    model = GNNModel(ffn_dropout_rate=0.0, loss_func=torch.nn.MSELoss()).to(dev).train()
    ref_model = copy.deepcopy(model)
    b = make_batch(4096, seed=19, target="docking_score").to(dev)
    loss = training_step(model, b)
    ref = ref_model.loss_func(ref_model(b)[0].view(-1), b.y.view(-1))
    ref.backward()
    assert abs(float(loss) - float(ref)) <= 1e-5 * abs(float(ref))
    for (n, p), (_, q) in zip(model.named_parameters(), ref_model.named_parameters()):
        if q.grad is not None:
            assert float((p.grad - q.grad).abs().max()) <= 1e-4 * max(float(q.grad.abs().max()), 1e-6), n


def test_training_lowers_the_docking_loss():
    """A short run of the HIP step with the fused AdamW on one docking batch lowers the summed squared error."""
    from molkgnn_amd.synthetic import make_batch
    from molkgnn_amd.train import GNNModel, configure_optimizer, training_step
    dev = _dev()
    torch.manual_seed(2)
    model = GNNModel(ffn_dropout_rate=0.0, loss_func=torch.nn.MSELoss(reduction="sum")).to(dev).train()
    opt = configure_optimizer(model, lr=3e-3)
    b = make_batch(512, seed=3, target="docking_score").to(dev)
    losses = [float(training_step(model, b, opt)) for _ in range(40)]
    assert all(l == l for l in losses) and min(losses[-10:]) < 0.5 * losses[0], losses
