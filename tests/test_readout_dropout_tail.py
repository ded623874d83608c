"""The readout's dropout (MolKGNNNet's ``drop_ratio``, reference MolKGNNNet.py:144-146) inside the fused tail
(``readout.tail_loss(..., readout_dropout_p=...)``, ``mkgnn_tail_fused_readout_dropout``): the mask export against the host
mirror, the fused tail against the separate operators fed that mask and against float64, padding, deferral, reproducibility
and the dispatch of ``GNNModel.loss``.  ``pytest -m gpu``."""
import numpy as np
import pytest
import torch

from tests import _philox as P
from tests.test_tail import _block_rows, _modules

pytestmark = pytest.mark.gpu

LS = (10, 20, 30, 50)


def _dev():
    assert torch.cuda.is_available(), "pytest -m gpu needs the MI355X"
    return torch.device("cuda:0")


def _close(got, want, rel=2e-5):
    err, scale = float((got.double() - want.double()).abs().max()), max(float(want.abs().max()), 1e-6)
    assert err <= rel * scale, (err, scale)


@pytest.mark.parametrize("n,H,p", [(1, 32, 0.2), (4097, 32, 0.2), (300, 32, 0.5), (77, 30, 0.2), (50, 7, 0.9)])
def test_mask_export_equals_the_host_mirror(n, H, p):
    from molkgnn_amd import readout as R
    dev = _dev()
    seed, offset = 0x1234_5678_9ABC_DEF1 & ((1 << 62) - 1), (5 << 32) + 3
    pair = torch.tensor([seed, offset], dtype=torch.int64, device=dev)
    got = R.readout_dropout_mask(pair, n, H, p).cpu().numpy()
    want = P.readout_mask(seed, offset, n, H, p)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert torch.equal(pair.cpu(), torch.tensor([seed, offset]))          # read, not advanced
    # a strided output: only the [n, H] window is written
    out = torch.full((n, H + 5), -1.0, device=dev)[:, :H]
    R.readout_dropout_mask(pair, n, H, p, out=out)
    assert np.array_equal(out.cpu().numpy(), want)
    if n * H >= 100_000:
        frac = float((got == 0).mean())
        assert abs(frac - p) <= 5 * (p * (1 - p) / got.size) ** 0.5, frac


def _setup(mols, n_pad, seed, kind):
    from molkgnn_amd import readout as R
    from molkgnn_amd.plan import plan_from_data
    from molkgnn_amd.synthetic import make_batch
    dev = _dev()
    b = make_batch(mols, seed=seed, target="docking_score" if kind != "bce" else "activity").to(dev)
    plan = plan_from_data(b)
    seg = R.molecule_segments(b.batch, mols)
    assert R.tail_supported(110, 32, 32, LS) and R._tail_limits_ok(seg, plan)
    mods = _modules(dev)
    sim0, inblock = _block_rows(b, plan, LS, dev, seed)
    n_rows = mols - n_pad
    y = b.y[:n_rows].float().contiguous()
    if kind == "bce":
        y = (torch.rand(n_rows, generator=torch.Generator().manual_seed(seed)) < 0.3).float().to(dev)
    return dev, b, plan, seg, mods, sim0, inblock, y, n_rows


def _params(mods):
    lin1, lin2, ffn = mods
    return list(lin1.parameters()) + list(lin2.parameters()) + list(ffn.parameters())


def _run(how, kind, mods, plan, seg, sim0, inblock, y, n_rows, p_head, p_ro, dev, seed=1234):
    """(loss, block-row grad_sim, the six parameter gradients, generator state after) of one forward + backward."""
    from molkgnn_amd import readout as R
    from molkgnn_amd.train import backward
    lin1, lin2, ffn = mods
    params = _params(mods)
    R.reset_head_rng(dev, seed=seed)
    for p in params:
        p.grad = None
    sim = sim0.detach().requires_grad_(True)
    if how == "separate":
        keep = R.readout_dropout_mask(R.head_rng_state(dev).clone(), sim.shape[0], 32, p_ro)
        emb = R._ReadoutBlocksFn.apply(sim, lin1.weight, lin1.bias, lin2.weight, lin2.bias, keep, seg, plan, LS)
        out = R.head_loss(emb, ffn, y, kind, dropout_p=p_head, n_rows=n_rows)
        out.backward()
        if p_head == 0.0:                                       # (the fused paths advance once for either dropout)
            R.head_rng_state(dev)[1] += 1
    elif how == "deferred":
        with R.deferred_tail_reduce(dev):
            out = R.tail_loss(sim, plan, LS, lin1, lin2, ffn, y, seg, p_head, n_rows, loss=kind, readout_dropout_p=p_ro)
            backward(out)
    else:
        out = R.tail_loss(sim, plan, LS, lin1, lin2, ffn, y, seg, p_head, n_rows, loss=kind, readout_dropout_p=p_ro)
        out.backward()
    torch.cuda.synchronize()
    gsim = torch.where(inblock, sim.grad, torch.zeros((), device=dev))
    return out.detach().clone(), gsim, [p.grad.clone() for p in params], R.head_rng_state(dev).clone()


@pytest.mark.parametrize("kind", ["bce", "mse", "mse_sum"])
@pytest.mark.parametrize("p_ro", [0.2, 0.5])
@pytest.mark.parametrize("p_head", [0.0, 0.25])
@pytest.mark.parametrize("n_pad", [0, 7])
def test_fused_tail_matches_the_separate_operators_with_the_same_mask(kind, p_ro, p_head, n_pad):
    mols = 300
    dev, b, plan, seg, mods, sim0, inblock, y, n_rows = _setup(mols, n_pad, 500 + n_pad, kind)
    l0, gs0, gp0, st0 = _run("separate", kind, mods, plan, seg, sim0, inblock, y, n_rows, p_head, p_ro, dev)
    l1, gs1, gp1, st1 = _run("fused", kind, mods, plan, seg, sim0, inblock, y, n_rows, p_head, p_ro, dev)
    assert torch.isfinite(l1) and abs(float(l0) - float(l1)) <= 2e-6 * max(1.0, abs(float(l0))), (float(l0), float(l1))
    _close(gs1, gs0)
    for a, c in zip(gp1, gp0):
        _close(a, c)
    assert st1.tolist() == [1234, 1] and torch.equal(st0, st1)          # advanced by exactly one
    # two runs from one seed: the same bits; inside a deferred region too
    for how in ("fused", "deferred"):
        l2, gs2, gp2, st2 = _run(how, kind, mods, plan, seg, sim0, inblock, y, n_rows, p_head, p_ro, dev)
        assert torch.equal(l1, l2) and torch.equal(gs1, gs2) and all(torch.equal(u, v) for u, v in zip(gp1, gp2)), how
        assert torch.equal(st1, st2)


def test_readout_dropout_changes_the_step_and_p_zero_is_todays_tail():
    from molkgnn_amd import readout as R
    dev, b, plan, seg, mods, sim0, inblock, y, n_rows = _setup(257, 0, 77, "bce")
    base = _run("fused", "bce", mods, plan, seg, sim0, inblock, y, n_rows, 0.25, 0.0, dev)
    # p = 0: the mkgnn_tail_fused call of before, whatever the keyword
    lin1, lin2, ffn = mods
    R.reset_head_rng(dev, seed=1234)
    sim = sim0.detach().requires_grad_(True)
    out = R.tail_loss(sim, plan, LS, lin1, lin2, ffn, y, seg, 0.25, n_rows)
    assert torch.equal(out.detach(), base[0])
    drop = _run("fused", "bce", mods, plan, seg, sim0, inblock, y, n_rows, 0.25, 0.2, dev)
    assert not torch.equal(drop[0], base[0])
    assert torch.equal(drop[3], base[3])                                 # one advance either way


def test_masked_formula_against_float64_autograd():
    from molkgnn_amd import readout as R
    mols, p_ro = 1000, 0.2
    dev, b, plan, seg, mods, sim0, inblock, y, n_rows = _setup(mols, 0, 91, "bce")
    l1, gs1, gp1, _ = _run("fused", "bce", mods, plan, seg, sim0, inblock, y, n_rows, 0.0, p_ro, dev, seed=31)
    keep = R.readout_dropout_mask(torch.tensor([31, 0], dtype=torch.int64, device=dev), sim0.shape[0], 32, p_ro).double()
    dense = torch.where(inblock, sim0, torch.zeros((), device=dev)).double().requires_grad_(True)
    p64 = [p.detach().double().requires_grad_(True) for p in _params(mods)]
    w1, b1, w2, b2, wh, bh = p64
    src, dst = b.edge_index[0], b.edge_index[1]
    h = torch.zeros_like(dense).index_add_(0, dst, dense[src])                       # KernelLayer.py:119-123
    z = h @ w1.t() + b1
    z = keep * (z * torch.sigmoid(z))                                                # MolKGNNNet.py:144-146 with the dropout
    z = z @ w2.t() + b2
    emb = torch.zeros(mols, 32, dtype=torch.float64, device=dev).index_add_(0, b.batch, z)
    pred = (emb[:n_rows] @ wh.t() + bh).view(-1)
    ref = torch.nn.functional.binary_cross_entropy_with_logits(pred, y.double())
    grads = torch.autograd.grad(ref, [dense] + p64)
    assert abs(float(l1) - float(ref)) <= 2e-5 * max(1.0, abs(float(ref))), (float(l1), float(ref))
    _close(gs1, torch.where(inblock, grads[0], torch.zeros((), device=dev, dtype=torch.float64)))
    for g, w in zip(gp1, grads[1:]):
        _close(g, w)


def _spy(monkeypatch, R, M=None):
    calls = []
    real = R._TailFn.apply
    monkeypatch.setattr(R._TailFn, "apply", lambda *a: (calls.append(("tail", a[-1])), real(*a))[1])
    return calls


@pytest.mark.parametrize("drop_ratio", [0.2, 1.0])
def test_model_loss_takes_the_fused_tail_with_readout_dropout(drop_ratio, monkeypatch):
    """GNNModel(dropout_ratio=0.2).loss in training mode at 4096 molecules: the fused tail (_TailFn), the readout's p handed
    over; p = 1 keeps the separate operators."""
    from molkgnn_amd import readout as R
    from molkgnn_amd.synthetic import make_batch
    from molkgnn_amd.train import GNNModel
    dev = _dev()
    torch.manual_seed(12)
    model = GNNModel(dropout_ratio=drop_ratio, ffn_dropout_rate=0.25).to(dev).train()
    b = make_batch(4096, seed=4096).to(dev)
    calls = _spy(monkeypatch, R)
    R.reset_head_rng(dev, seed=3)
    loss = model.loss(b)
    loss.backward()
    torch.cuda.synchronize()
    assert torch.isfinite(loss)
    if drop_ratio < 1.0:
        assert calls == [("tail", drop_ratio)], calls
        assert R.head_rng_state(dev).tolist() == [3, 1]
    else:
        assert calls == [], calls


def test_model_step_is_padding_invariant_and_deferral_exact():
    """A padded batch (padding.pad_batch) gives the unpadded batch's loss bit for bit with readout dropout (the real atoms keep
    their rows, so their masks); training_step's deferred reduction gives the bits of the three separate calls."""
    from molkgnn_amd import padding as PD
    from molkgnn_amd import readout as R
    from molkgnn_amd.receptive_field import attach_receptive_fields
    from molkgnn_amd.synthetic import make_batch
    from molkgnn_amd.train import GNNModel, backward as train_backward, configure_optimizer, training_step
    dev = _dev()
    torch.manual_seed(3)
    model = GNNModel(dropout_ratio=0.2, ffn_dropout_rate=0.25).to(dev).train()
    B = 700
    raw = make_batch(B, seed=4100, with_receptive_fields=False)
    raw.y = (torch.arange(B) % 5 == 0).long()
    other = make_batch(B, seed=4101, with_receptive_fields=False)
    shape = PD.fixed_shape([PD.degree_histogram(raw), PD.degree_histogram(other)])
    res = []
    for batch in (attach_receptive_fields(raw.to(dev)),
                  attach_receptive_fields(PD.pad_batch(raw, shape, B).to(dev), sizes=[shape[f"n{d}"] for d in range(1, 5)])):
        state = {k: v.clone() for k, v in model.state_dict().items()}
        model.zero_grad(set_to_none=True)
        R.reset_head_rng(dev, seed=21)
        loss = model.loss(batch)
        loss.backward()
        torch.cuda.synchronize()
        model.load_state_dict(state)
        res.append((loss.detach().clone(), {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}))
    assert torch.equal(res[0][0], res[1][0]), (float(res[0][0]), float(res[1][0]))
    for n, g in res[0][1].items():
        assert float((g - res[1][1][n]).abs().max()) <= 2e-5 * max(float(g.abs().max()), 1e-3) + 1e-7, n

    b = make_batch(600, seed=47).to(dev)

    def fresh():
        torch.manual_seed(1798)
        m = GNNModel(dropout_ratio=0.2, ffn_dropout_rate=0.0).to(dev).train()
        R.reset_head_rng(dev, seed=99)
        return m, configure_optimizer(m, lr=1e-3, capturable=True)

    m, opt = fresh()
    m.zero_grad(set_to_none=True)
    la = m.loss(b)
    train_backward(la)
    opt.step()
    torch.cuda.synchronize()
    pa = {n: p.detach().clone() for n, p in m.named_parameters()}
    sa = R.head_rng_state(dev).clone()
    m, opt = fresh()
    lb = training_step(m, b, opt)                       # readout dropout only: the deferred reduction still advances
    torch.cuda.synchronize()
    assert float(lb) == float(la)
    assert torch.equal(R.head_rng_state(dev), sa) and sa.tolist() == [99, 1]
    for n, p in m.named_parameters():
        assert torch.equal(p.detach(), pa[n]), n
