"""The float64 batch norm reference of ``tests/_bn_f64.py`` checked WITHOUT a GPU: against ``torch.nn.BatchNorm1d`` run in
float64, against itself on a padded batch, and the exactness claims of the ``constant_exact`` and ``mean_rows`` families.  A wrong
reference would bless a wrong kernel; this is what keeps it right."""
import numpy as np
import pytest
import torch

from tests import _bn_f64 as B

FAMILIES = sorted(B.FAMILIES)
REL = 1e-12


def _close(a, b, tag, terms=0.0):
    """1e-12 relative to the tensor's largest entry -- or to the largest of the TERMS it is a sum of, where the caller gives it: the
    input gradient of two rows is zero but for the eps in the variance, a sum of terms 1e4 times its own size."""
    a, b = a.detach().double(), b.detach().double()
    assert a.shape == b.shape, tag
    if b.numel() == 0:
        return
    err, scale = float((a - b).abs().max()), max(float(b.abs().max()), float(terms))
    assert err <= REL * scale, (tag, err, scale)


def _module(C, affine, seed):
    g = torch.Generator().manual_seed(seed)
    bn = torch.nn.BatchNorm1d(C, affine=affine).double()
    with torch.no_grad():
        if affine:
            bn.weight.copy_(torch.rand(C, generator=g).double() + 0.5)
            bn.bias.copy_(torch.randn(C, generator=g).double())
        bn.running_mean.copy_(torch.randn(C, generator=g).double() * 0.2)
        bn.running_var.copy_(torch.rand(C, generator=g).double() + 0.5)
    return bn


# (two rows of ``offset`` are left out: 1e3 +- 1e-1 in float64 is known to 1e-13 of a value whose two-sample deviation may be 1e-2 or
# less -- the comparison would measure BatchNorm1d's own float64 rounding at a condition number nobody chose.  ``mean_rows`` needs
# eight rows for its zero rows.)
@pytest.mark.parametrize("affine", [True, False])
@pytest.mark.parametrize("family,n,C", [(f, n, C) for f in FAMILIES for n, C in [(2, 3), (257, 7), (1000, 28)]
                                        if not (n == 2 and f in ("offset", "mean_rows"))] + [("mean_rows", 10, 3)])
def test_reference_is_batchnorm1d_in_float64(family, n, C, affine):
    """Forward, saved statistics, the buffers after each of three training calls, all gradients; then the same in eval mode."""
    bn = _module(C, affine, 5)
    g = torch.Generator().manual_seed(9)
    for call in range(4):
        training = call < 3
        bn.train(training)
        x = B.make(family, n, C, seed=call)
        cot = torch.randn(n, C, generator=g)
        rm, rv = bn.running_mean.clone(), bn.running_var.clone()
        ref = B.reference(x, bn.weight, bn.bias, rm, rv, bn.momentum, bn.eps, training, cot=cot)
        xin = x.double().requires_grad_(True)
        bn.zero_grad()
        y = bn(xin)
        (y * cot.double()).sum().backward()
        tag = (family, n, C, affine, call)
        _close(ref["out"], y, tag + ("out",))
        _close(ref["running_mean"], bn.running_mean, tag + ("running_mean",))
        _close(ref["running_var"], bn.running_var, tag + ("running_var",))
        k0 = ref["save_invstd"] * (bn.weight.detach() if affine else 1.0)
        _close(ref["grad_x"], xin.grad, tag + ("grad_x",), terms=float((cot.double().abs() * k0).max()))
        if affine:
            _close(ref["grad_weight"], bn.weight.grad, tag + ("grad_weight",))
            _close(ref["grad_bias"], bn.bias.grad, tag + ("grad_bias",))
        else:
            assert ref["grad_weight"] is None and ref["grad_bias"] is None
        if training:
            xd = x.double()
            _close(ref["save_mean"], xd.mean(0), tag + ("save_mean",))
            _close(ref["save_invstd"], 1.0 / torch.sqrt(xd.var(0, unbiased=False) + bn.eps), tag + ("save_invstd",))
        else:
            assert torch.equal(ref["running_mean"], rm) and torch.equal(ref["running_var"], rv)
        _close(ref["inv_norm"], 1.0 / y.detach().norm(dim=1).clamp_min(1e-8), tag + ("inv_norm",))
    assert int(bn.num_batches_tracked) == 3


def test_reference_without_running_statistics_uses_batch_statistics():
    x = B.make("plain", 300, 5)
    bn = torch.nn.BatchNorm1d(5, track_running_stats=False).double().eval()
    ref = B.reference(x, bn.weight, bn.bias, None, None, 0.1, bn.eps, True)
    _close(ref["out"], bn(x.double()), "no running statistics")
    assert ref["running_mean"] is None and ref["running_var"] is None


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("n,nv", [(300, 2), (300, 257), (4097, 3000), (300, 300)])
def test_n_valid_reference_is_the_plain_reference_on_the_counted_rows(family, n, nv):
    """Statistics, buffers, counted output rows, counted grad_x rows and the parameter gradients of a padded batch are those of
    the batch without its padding; padding rows are normalised with the same statistics; their grad_x is zero by definition."""
    C = 6
    x = B.make(family, n, C) if family != "mean_rows" else torch.cat([B.make(family, max(nv, 8), C), torch.ones(n - max(nv, 8), C)])[:n]
    g = torch.Generator().manual_seed(3)
    w, b = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g)
    rm, rv = torch.randn(C, generator=g) * 0.1, torch.rand(C, generator=g) + 0.5
    cot = torch.randn(n, C, generator=g)
    pad = B.reference(x, w, b, rm, rv, 0.1, 1e-5, True, n_valid=nv, cot=cot)
    cut = B.reference(x[:nv], w, b, rm, rv, 0.1, 1e-5, True, cot=cot[:nv])
    for k in ("save_mean", "save_invstd", "running_mean", "running_var", "grad_weight", "grad_bias"):
        _close(pad[k], cut[k], (family, n, nv, k))
    for k in ("out", "grad_x", "inv_norm"):
        _close(pad[k][:nv], cut[k], (family, n, nv, k))
    want = (x[nv:].double() - pad["save_mean"]) * pad["save_invstd"] * w.double() + b.double()
    _close(pad["out"][nv:], want, (family, n, nv, "padding rows"))
    if nv < n:
        assert float(pad["grad_x"][nv:].abs().max()) == 0.0


ROW_COUNTS = (2, 3, 255, 256, 257, 300, 511, 1537, 3000, 4096, 4097, 65_537, 101_241, 102_584)


@pytest.mark.parametrize("n", ROW_COUNTS)
def test_constant_exact_has_exact_fp32_partial_sums_for_every_share(n):
    """Whatever the order in which a block adds the rows of its share and the blocks' sums are added: every partial sum is j * v, j
    <= n.  All of them are fp32 numbers; every share's mean ``fp32(cnt * v) / fp32(cnt)`` and the batch mean are exactly v; every
    centred value is exactly 0.  So the normalised column is ``fma(0, scale, bias) = bias`` bit for bit."""
    x = B.constant_exact(n, len(B.DYADIC)).numpy()
    assert x.dtype == np.float32
    v64 = x[0].astype(np.float64)
    assert np.array_equal(x, np.broadcast_to(x[0], x.shape))
    j = np.arange(1, n + 1, dtype=np.float64)[:, None]
    prod = j * v64                                        # exact in float64 (24 + 3 bits)
    assert np.array_equal(prod.astype(np.float32).astype(np.float64), prod)
    sh = B.shares(n)
    assert sum(hi - lo for lo, hi in sh) == n and sh[0][0] == 0 and all(a[1] == b[0] or b[0] == b[1] for a, b in zip(sh, sh[1:]))
    for cnt in sorted({hi - lo for lo, hi in sh if hi > lo} | {n}):
        mean = (np.float32(cnt) * x[0]) / np.float32(cnt)
        assert np.array_equal(mean, x[0]), cnt
    # the same block sums added up in the kernel's fixed order (8 interleaved accumulators, then a tree) stay exact: any subset sum
    # of the shares' counts is <= n
    counts = np.array([hi - lo for lo, hi in sh], dtype=np.float64)
    assert np.array_equal(np.cumsum(counts)[:, None] * v64, (np.cumsum(counts)[:, None] * v64).astype(np.float32).astype(np.float64))


@pytest.mark.parametrize("n", [300, 1537, 4097, 102_584])
def test_mean_rows_sums_are_small_integers_and_the_mean_is_zero(n):
    C = 8
    x = B.make("mean_rows", n, C)
    assert set(np.unique(x.numpy()).tolist()) == {-1.0, 0.0, 1.0}
    assert float(x.sum(0).abs().max()) == 0.0                        # as many +1 as -1: any order of integer sums below 2^24 is exact
    zero = B.mean_rows_zero_rows(n)
    assert 3 <= len(zero) <= 4 and len(set(zero)) == len(zero)
    assert float(x[zero].abs().max()) == 0.0 and int((x.abs().sum(1) == 0).sum()) == len(zero)
    ref = B.reference(x, torch.rand(C) + 0.5, torch.zeros(C), None, None, 0.1, 1e-5, True)
    assert float(ref["save_mean"].abs().max()) == 0.0
    assert float(ref["out"][zero].abs().max()) == 0.0
    assert bool((ref["inv_norm"][zero] == 1e8).all())


def test_fp32_clamp_of_a_zero_row_is_one_hundred_million():
    """``1.f / fmaxf(0.f, 1e-8f)``: what the apply pass hands for a zero row, the value ``split_row_scale_of`` is commented as safe
    for."""
    assert B.fp32_inv_clamp() == 1e8


@pytest.mark.parametrize("keep", ["all", "some", "one", "none"])
def test_masked_statistics_is_batchnorm1d_on_the_kept_rows(keep):
    n, C = 500, 7
    x = B.make("plain", n, C)
    mask = {"all": None, "some": torch.arange(n) % 10 < 7, "one": torch.arange(n) == 123, "none": torch.zeros(n, dtype=torch.bool)}[keep]
    bn = torch.nn.BatchNorm1d(C).double().train()
    rm, rv, moved = B.masked_statistics(x, mask, bn.running_mean, bn.running_var, bn.momentum)
    xs = x.double() if mask is None else x.double()[mask]
    if xs.shape[0] > 1:
        bn(xs)
    assert moved == (xs.shape[0] > 1)
    _close(rm, bn.running_mean, keep)
    _close(rv, bn.running_var, keep)
