"""The head's squared-error loss kinds (readout.head_loss; mkgnn_head_loss_*, csrc/kgnn_head.hip): ``MSELoss()`` and
``MSELoss(reduction='sum')`` of ``ffn(dropout(emb))`` -- the reference's docking-score task (data.py:49-53) -- against float64
autograd, the fused form against the split one, the dropout mask against BCE's, and the BCE kind against ``bce_head_loss``.
``pytest -m gpu``."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _dev():
    assert torch.cuda.is_available(), "pytest -m gpu needs the MI355X"
    return torch.device("cuda:0")


def _close(got, want, rel=2e-5):
    err, scale = float((got.double() - want.double()).abs().max()), max(float(want.abs().max()), 1e-6)
    assert err <= rel * scale, (err, scale)


@pytest.mark.parametrize("loss", ["mse", "mse_sum"])
@pytest.mark.parametrize("B,H,n_pad,scale", [(4096, 32, 0, 1.0), (37, 5, 3, 1.7), (1, 40, 0, 1.0), (300, 64, 11, -0.6)])
def test_head_loss_against_float64_autograd(loss, B, H, n_pad, scale):
    """pred, loss, grad_emb (zero on the padding rows), grad_weight, grad_bias; n_rows < rows and d loss != 1 included."""
    from molkgnn_amd import readout as R
    dev = _dev()
    torch.manual_seed(B + H + n_pad)
    ffn = torch.nn.Linear(H, 1).to(dev)
    emb = (torch.randn(B + n_pad, H, device=dev) * 2).requires_grad_(True)
    y = torch.randn(B, device=dev) * 1.5 - 8.0
    out = R.head_loss(emb, ffn, y, loss, n_rows=B)
    pred = out.grad_fn.saved_tensors[3]
    got = torch.autograd.grad(out * scale, [emb, ffn.weight, ffn.bias])
    e64 = emb.detach().double().requires_grad_(True)
    w64, b64 = ffn.weight.detach().double().requires_grad_(True), ffn.bias.detach().double().requires_grad_(True)
    p64 = (e64[:B] @ w64.t() + b64).view(-1)
    ref = torch.nn.MSELoss(reduction="mean" if loss == "mse" else "sum")(p64, y.double())
    want = torch.autograd.grad(ref * scale, [e64, w64, b64])
    assert abs(float(out) - float(ref)) <= 2e-6 * max(1.0, abs(float(ref))), (float(out), float(ref))
    _close(pred, p64.detach())
    for g, w in zip(got, want):
        assert g.shape == w.shape
        _close(g, w)
    if n_pad:
        assert float(got[0][B:].abs().max()) == 0.0


@pytest.mark.parametrize("loss", ["mse", "mse_sum"])
@pytest.mark.parametrize("B,H,p", [(4096, 32, 0.25), (300, 40, 0.25), (37, 5, 0.5)])
def test_fused_split_and_dropout_entry_points_agree(loss, B, H, p, monkeypatch):
    """Dropout 0.25: the fused form (mkgnn_head_loss_fused) against the split one (MKGNN_SPLIT_HEAD: the dropout forward and
    backward entry points) from the same generator state -- gradients bit for bit through the unit seed, scaled otherwise."""
    from molkgnn_amd import readout as R
    from molkgnn_amd.train import backward
    dev = _dev()
    torch.manual_seed(B + H)
    ffn = torch.nn.Linear(H, 1).to(dev)
    emb0 = torch.randn(B + 3, H, device=dev) * 2
    y = torch.randn(B, device=dev) - 8.0

    def run(split, scale):
        monkeypatch.setattr(R, "_SPLIT_HEAD", split)
        R.reset_head_rng(dev, seed=1234)
        emb = emb0.clone().requires_grad_(True)
        ffn.zero_grad(set_to_none=True)
        out = R.head_loss(emb, ffn, y, loss, dropout_p=p, n_rows=B)
        if scale is None:
            backward(out)
        else:
            (out * scale).backward()
        torch.cuda.synchronize()
        return out.detach().clone(), emb.grad.clone(), ffn.weight.grad.clone(), ffn.bias.grad.clone(), R.head_rng_state(dev).clone()

    for scale in (None, 1.7):
        a, c = run(True, scale), run(False, scale)
        assert torch.isfinite(a[0]) and abs(float(a[0]) - float(c[0])) <= 1e-6 * abs(float(c[0]))
        if scale is None:
            assert all(torch.equal(u, v) for u, v in zip(a[1:4], c[1:4]))
        else:
            assert all(float((u - v).abs().max()) <= 2e-6 * float(v.abs().max()) for u, v in zip(a[1:4], c[1:4]))
        assert float(a[1][B:].abs().max()) == 0.0 and float(c[1][B:].abs().max()) == 0.0
        assert torch.equal(a[4], c[4]) and int(a[4][1]) == 1          # one draw each
        # the mask is really applied: about p of the counted rows' elements get no gradient
        zero = float((c[1][:B] == 0).double().mean())
        assert abs(zero - p) < 0.05 + 3.0 / (B * H) ** 0.5, zero


@pytest.mark.parametrize("loss", ["mse", "mse_sum"])
def test_squared_error_draws_the_bce_mask(loss):
    """The same generator state gives the same dropout mask whatever the loss: the zero pattern of grad_emb."""
    from molkgnn_amd import readout as R
    dev = _dev()
    torch.manual_seed(3)
    B, H = 1000, 32
    ffn = torch.nn.Linear(H, 1).to(dev)
    emb0 = torch.randn(B, H, device=dev)
    y = (torch.rand(B, device=dev) < 0.5).float()
    grads = []
    for fn in (lambda e: R.bce_head_loss(e, ffn, y, dropout_p=0.25), lambda e: R.head_loss(e, ffn, y, loss, dropout_p=0.25)):
        R.reset_head_rng(dev, seed=4321)
        emb = emb0.clone().requires_grad_(True)
        fn(emb).backward()
        grads.append(emb.grad)
    zb, zm = grads[0] == 0, grads[1] == 0
    assert 0.2 < float(zb.double().mean()) < 0.3
    assert torch.equal(zb, zm)


@pytest.mark.parametrize("B,H,p,n_pad", [(4096, 32, 0.25, 0), (37, 5, 0.0, 4), (300, 40, 0.5, 0)])
@pytest.mark.parametrize("split", [False, True])
def test_bce_kind_is_bce_head_loss_bit_for_bit(B, H, p, n_pad, split, monkeypatch):
    """head_loss(loss='bce') through the v8 entry points with kind 0 == bce_head_loss through the v7 ones, to the bit."""
    from molkgnn_amd import readout as R
    from molkgnn_amd.train import backward
    monkeypatch.setattr(R, "_SPLIT_HEAD", split)
    dev = _dev()
    torch.manual_seed(B)
    ffn = torch.nn.Linear(H, 1).to(dev)
    emb0 = torch.randn(B + n_pad, H, device=dev) * 2
    y = (torch.rand(B, device=dev) < 0.3).float()
    res = []
    for fn in (lambda e: R.bce_head_loss(e, ffn, y, dropout_p=p, n_rows=B), lambda e: R.head_loss(e, ffn, y, "bce", p, B)):
        R.reset_head_rng(dev, seed=99)
        emb = emb0.clone().requires_grad_(True)
        ffn.zero_grad(set_to_none=True)
        out = fn(emb)
        pred = out.grad_fn.saved_tensors[3].clone()
        backward(out)
        res.append((out.detach().clone(), pred, emb.grad.clone(), ffn.weight.grad.clone(), ffn.bias.grad.clone()))
    assert all(torch.equal(u, v) for u, v in zip(*res))
