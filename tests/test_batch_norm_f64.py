"""The batch norm kernels (``csrc/kgnn_batchnorm.hip``: ``mkgnn_batchnorm_forward_with_stats``, ``mkgnn_batchnorm_backward``,
``mkgnn_batchnorm_update_stats``) on the operator alone, against the float64 reference of ``tests/_bn_f64.py``, at every edge of
their dispatch: widths and row alignments (16-byte row passes or column passes, mixed in the backward), row counts around the
256-block grid, ``n_valid``, every mode of ``BatchNorm1d``, ill-conditioned columns, the statistics-only companion in both of its
forms with every kind of key, the handed row norms and pre-split rows, and the riders of the statistics launch.  ``pytest -m gpu``.

Criterion: ``tests/_f64.check`` with its constants as they are -- per tensor
``max|build - f64| <= 10 * max|fp32 torch - f64| + 2^-16 * max(max|f64|, 1e-3)``, the fp32 yardstick being
``torch.nn.functional.batch_norm`` and its autograd in fp32 ON THE CPU on the same inputs, computed here.  The families
``constant_exact`` and ``mean_rows`` get exact assertions instead.  ``MKGNN_BN_ONE_LAUNCH=1`` (the opt-in grid-barrier form) is not
run by this module.
"""
import pytest
import torch

from tests import _bn_f64 as B
from tests import _f64 as F64

pytestmark = pytest.mark.gpu

EPS = 1e-5
MOM = 0.1
STAT_NAMES = ("out", "save_mean", "save_invstd", "running_mean", "running_var", "grad_x", "grad_weight", "grad_bias", "inv_norm")


def _dev():
    assert torch.cuda.is_available(), "pytest -m gpu needs the MI355X"
    return torch.device("cuda:0")


def _params(C, seed, affine=True, track=True):
    g = torch.Generator().manual_seed(seed)
    w = torch.rand(C, generator=g) + 0.5 if affine else None
    b = torch.randn(C, generator=g) if affine else None
    rm = torch.randn(C, generator=g) * 0.2 if track else None
    rv = torch.rand(C, generator=g) + 0.5 if track else None
    return w, b, rm, rv


def _module(C, dev, w, b, rm, rv):
    bn = torch.nn.BatchNorm1d(C, eps=EPS, momentum=MOM, affine=w is not None, track_running_stats=rm is not None).to(dev)
    with torch.no_grad():
        if w is not None:
            bn.weight.copy_(w); bn.bias.copy_(b)
        if rm is not None:
            bn.running_mean.copy_(rm); bn.running_var.copy_(rv)
    return bn


def _lay(t, layout, dev):
    """``t`` [n, C] on the device in a storage form -> (leaf that owns the storage, first column of ``t`` in it).  ``aligned``: contiguous
    (16-byte rows iff C % 4 == 0); ``offset1``: the column slice [1, 1 + C) of a tensor four columns wider (rows start 4 bytes off
    a 16-byte boundary); ``stride1``: row stride C + 1."""
    n, C = t.shape
    if layout == "aligned":
        return t.to(dev).contiguous().clone(), 0
    big = torch.zeros(n, C + (4 if layout == "offset1" else 1), device=dev)
    lo = 1 if layout == "offset1" else 0
    big[:, lo:lo + C] = t.to(dev)
    return big, lo


def _view(leaf, lo, C):
    return leaf if leaf.shape[1] == C else leaf[:, lo:lo + C]


def yardstick(x, w, b, rm, rv, training, nv=None, cot=None):
    """``torch.nn.functional.batch_norm`` and its autograd in fp32 on the CPU (the saved statistics from
    ``torch.native_batch_norm``, the kernel behind it) -> the dict of ``_bn_f64.reference``.  A padded batch: the operator on the
    counted rows, the padding rows normalised in fp32 with its saved statistics."""
    x = x.detach().cpu().float()
    n, C = x.shape
    nv = n if nv is None else nv
    xin = x[:nv].clone().requires_grad_(cot is not None)
    w_ = None if w is None else w.detach().cpu().clone().requires_grad_(cot is not None)
    b_ = None if b is None else b.detach().cpu().clone().requires_grad_(cot is not None)
    rm_ = None if rm is None else rm.detach().cpu().clone()
    rv_ = None if rv is None else rv.detach().cpu().clone()
    out = torch.nn.functional.batch_norm(xin, rm_, rv_, w_, b_, training, MOM, EPS)
    if training:
        _, sm, si = torch.native_batch_norm(x[:nv], None, None, None, None, True, MOM, EPS)
    else:
        sm, si = rm_.clone(), 1.0 / torch.sqrt(rv_ + EPS)
    res = {"save_mean": sm, "save_invstd": si, "running_mean": rm_, "running_var": rv_, "grad_x": None, "grad_weight": None, "grad_bias": None}
    if cot is not None:
        (out * cot.detach().cpu().float()[:nv]).sum().backward()
        res["grad_x"] = xin.grad
        res["grad_weight"] = None if w_ is None else w_.grad
        res["grad_bias"] = None if b_ is None else b_.grad
    out = out.detach()
    if nv < n:
        pad = (x[nv:] - sm) * si
        if w_ is not None:
            pad = pad * w_.detach() + b_.detach()
        out = torch.cat([out, pad])
    res["out"] = out
    res["inv_norm"] = 1.0 / out.norm(dim=1).clamp_min(B.ROW_EPS)
    return res


def run_build(view, leaf, bn, n_valid=None, cot=None, split_out=False, companion=None):
    """One call of ``readout.batch_norm`` (+ backward with the cotangent ``cot``, a device tensor in whatever layout) -> dict."""
    from molkgnn_amd import functional as Fn
    from molkgnn_amd import readout as R
    for p in bn.parameters():
        p.grad = None
    leaf.grad = None
    nvt = None if n_valid is None else torch.tensor([n_valid], dtype=torch.int64, device=view.device)
    out = R.batch_norm(view, bn, n_valid=nvt, companion=companion, split_out=split_out)
    got = dict.fromkeys(STAT_NAMES)
    got["out"] = out.detach()
    got["inv_norm"] = Fn._handed_inv_norm(out)
    if out.grad_fn is not None:
        saved = out.grad_fn.saved_tensors
        got["save_mean"], got["save_invstd"] = saved[2].clone(), saved[3].clone()
    if cot is not None and out.requires_grad:
        torch.autograd.backward(out, grad_tensors=cot)
        if leaf.grad is not None:
            off = (view.data_ptr() - leaf.data_ptr()) // 4
            got["grad_x"] = leaf.grad[:, off:off + view.shape[1]].clone()
        if bn.weight is not None:
            got["grad_weight"], got["grad_bias"] = bn.weight.grad, bn.bias.grad
    torch.cuda.synchronize()
    got["running_mean"] = None if bn.running_mean is None else bn.running_mean.clone()
    got["running_var"] = None if bn.running_var is None else bn.running_var.clone()
    return got


def _cut(d, nv):
    d = dict(d)
    if d.get("grad_x") is not None:
        d["grad_x"] = d["grad_x"][:nv]
    return d


def hold(x, C, *, tag, dev, affine=True, track=True, training=True, calls=1, n_valid=None, x_grad=True, w_grad=True,
         layout="aligned", g_layout="aligned", seed=1):
    """``calls`` calls in a row of the build on ``x`` (CPU, fp32) in the given storage form, each against the float64 reference and the
    fp32 yardstick fed the SAME buffers the build started the call with.  Returns the last call's results."""
    n = x.shape[0]
    w, b, rm, rv = _params(C, seed, affine, track)
    bn = _module(C, dev, w, b, rm, rv).train(training)
    if affine and not w_grad:
        bn.weight.requires_grad_(False)
    g = torch.Generator().manual_seed(seed + 17)
    got = None
    for call in range(calls):
        cot = torch.randn(n, C, generator=g)
        leaf, lo = _lay(x, layout, dev)
        leaf.requires_grad_(x_grad)
        view = _view(leaf, lo, C)
        cot_dev = _view(*_lay(cot, g_layout, dev), C)
        if n_valid is not None:
            cot_dev[n_valid:] = 0.0
        before = None if not track else (bn.running_mean.clone(), bn.running_var.clone(), int(bn.num_batches_tracked))
        want_grad = x_grad or affine                      # (a frozen weight leaves the bias)
        got = run_build(view, leaf, bn, n_valid, cot_dev if want_grad else None)
        rm0, rv0 = (None, None) if before is None else before[:2]
        ref = B.reference(x, w, b, rm0, rv0, MOM, EPS, training or not track, n_valid, cot if want_grad else None)
        f32 = yardstick(x, w, b, rm0, rv0, training or not track, n_valid, cot if want_grad else None)
        if not x_grad:
            assert got["grad_x"] is None
            ref["grad_x"] = f32["grad_x"] = None
        if affine and not w_grad:
            assert got["grad_weight"] is None
            ref["grad_weight"] = f32["grad_weight"] = None
        nv = n if n_valid is None else n_valid
        handed = C <= 32 and C % 4 == 0 and layout == "aligned"
        assert (got["inv_norm"] is not None) == handed, (tag, "which apply pass ran")
        checked = F64.check(_cut(got, nv), _cut(f32, nv), _cut(ref, nv), f"bn/{tag}/call{call}")
        assert checked >= 2
        if track:
            assert int(bn.num_batches_tracked) == before[2] + (1 if training else 0), tag
            if not training:
                assert torch.equal(bn.running_mean, before[0]) and torch.equal(bn.running_var, before[1])
    return got, bn


# ------------------------------------------------------------------------------------ widths and alignments --
WIDTHS = (1, 3, 4, 7, 8, 12, 28, 32, 33, 64, 110, 128, 130, 132, 200, 256)
LAYOUTS = [(C, lay, gl) for C in WIDTHS for lay, gl in
           ([("aligned", "aligned")] + ([("offset1", "aligned"), ("stride1", "aligned"), ("aligned", "offset1"), ("aligned", "stride1"),
                                         ("offset1", "offset1")] if C % 4 == 0 else [("offset1", "aligned")]))]


@pytest.mark.parametrize("family", ["plain", "sorted"])
@pytest.mark.parametrize("C,layout,g_layout", LAYOUTS)
def test_widths_and_alignments(C, layout, g_layout, family):
    """Every width class of the dispatch (LW = CL / 4 of 1, 2, 4, 8, 16, 32, 64; the column passes for C % 4 != 0) and, for widths
    that could be read 16 bytes at a time, storage that cannot: a column slice one float into a wider tensor, a row stride of C + 1 --
    for x, for the cotangent only (the backward takes the column passes, the forward the 16-byte ones) and for both.  1 537 rows:
    256 shares of 7, the last non-empty one of 4, 36 empty."""
    x = B.make(family, 1537, C)
    hold(x, C, tag=f"width/{family}/{C}/{layout}/{g_layout}", dev=_dev(), layout=layout, g_layout=g_layout)


# ------------------------------------------------------------------------------------------------ row counts --
ROWS = (2, 3, 255, 256, 257, 511, 4096, 4097, 65_537, 102_584)


@pytest.mark.parametrize("family", ["plain", "offset", "sorted", "scales", "spike"])
@pytest.mark.parametrize("n", ROWS)
@pytest.mark.parametrize("C", [28, 7])
def test_row_counts_and_families(C, n, family):
    """Fewer rows than blocks, one row per block, a ragged last share, the headline batch's atom count; well- and ill-conditioned
    columns; the 16-byte passes (28) and the column passes (7)."""
    hold(B.make(family, n, C), C, tag=f"rows/{family}/{C}/{n}", dev=_dev())


# ----------------------------------------------------------------------------------------------------- modes --
@pytest.mark.parametrize("C", [28, 7, 132])
@pytest.mark.parametrize("mode", ["train3", "eval", "no_affine", "no_affine_eval", "no_tracking", "no_tracking_eval", "x_no_grad",
                                  "x_no_grad_eval", "weight_no_grad"])
def test_modes(mode, C):
    """Three training calls in a row (buffers and counter after each); eval forward AND backward (statistics from the running
    buffers, ``k0 * dy``); ``affine=False``; ``track_running_stats=False`` (batch statistics in both modes, no buffers); an input
    that needs no gradient (``bn_bwd_final_kernel`` in one block: the case of every real step); a frozen weight."""
    x = B.make("plain", 1537, C, seed=3)
    kw = {"train3": dict(calls=3), "eval": dict(training=False, calls=2), "no_affine": dict(affine=False),
          "no_affine_eval": dict(affine=False, training=False), "no_tracking": dict(track=False),
          "no_tracking_eval": dict(track=False, training=False), "x_no_grad": dict(x_grad=False),
          "x_no_grad_eval": dict(x_grad=False, training=False), "weight_no_grad": dict(w_grad=False)}[mode]
    hold(x, C, tag=f"mode/{mode}/{C}", dev=_dev(), **kw)


@pytest.mark.parametrize("family", ["offset", "sorted", "scales", "spike"])
@pytest.mark.parametrize("n", [257, 102_584])
def test_parameter_gradients_without_input_gradient(family, n):
    """The weight and bias gradients of a step whose input needs no gradient, on ill-conditioned columns."""
    hold(B.make(family, n, 28), 28, tag=f"paramgrad/{family}/{n}", dev=_dev(), x_grad=False)


# --------------------------------------------------------------------------------------------------- n_valid --
NVALID = [(300, 2), (300, 257), (4097, 4096), (4097, 3000), (102_584, 101_241), (300, 300), (4097, 4097)]


@pytest.mark.parametrize("family", ["plain", "offset", "sorted", "scales", "spike"])
@pytest.mark.parametrize("n,nv", NVALID)
@pytest.mark.parametrize("C", [28, 7])
def test_n_valid(C, n, nv, family):
    """A padded batch: statistics over the counted rows, every output row (padding rows: same statistics), the gradients as
    ``_bn_f64.reference`` defines them -- and ``out[:nv]``, the saved statistics and the running buffers BIT FOR BIT those of the call
    on ``x[:nv]`` alone (``bn_block_stats`` deals the COUNTED rows to the blocks; the padded-graph tests rely on it)."""
    dev = _dev()
    x = B.make(family, n, C)
    got, _ = hold(x, C, tag=f"nvalid/{family}/{C}/{n}/{nv}", dev=dev, n_valid=nv, seed=4)
    w, b, rm, rv = _params(C, 4)
    bn = _module(C, dev, w, b, rm, rv).train()
    leaf = x[:nv].to(dev).contiguous().requires_grad_(True)
    alone = run_build(leaf, leaf, bn, None, torch.zeros(nv, C, device=dev))
    for k in ("save_mean", "save_invstd", "running_mean", "running_var"):
        assert torch.equal(got[k], alone[k]), k
    assert torch.equal(got["out"][:nv], alone["out"])
    if got["inv_norm"] is not None:
        assert torch.equal(got["inv_norm"][:nv], alone["inv_norm"])


# --------------------------------------------------------------------------------------------- exact families --
@pytest.mark.parametrize("n", [2, 257, 1537, 4097, 102_584])
@pytest.mark.parametrize("C", [28, 7, 8, 132])
def test_constant_columns_come_out_as_the_bias_bit_for_bit(C, n):
    """``constant_exact``: every partial sum a kernel can form is exact (tests/test_bn_reference_cpu.py), so the batch mean is the
    column's value, the variance 0, ``save_invstd = 1 / sqrt(eps)`` and every output ``fma(0, scale, bias) = bias``."""
    from molkgnn_amd import readout as R
    dev = _dev()
    x = B.constant_exact(n, C)
    w, b, rm, rv = _params(C, 2)
    bn = _module(C, dev, w, b, rm, rv).train()
    leaf = x.to(dev).requires_grad_(True)
    cot = torch.randn(n, C, generator=torch.Generator().manual_seed(n))
    got = run_build(leaf, leaf, bn, None, cot.to(dev))
    assert torch.equal(got["out"], b.to(dev).expand(n, C))
    assert torch.equal(got["save_mean"], x[0].to(dev))
    F64.check(got, yardstick(x, w, b, rm, rv, True, None, cot), B.reference(x, w, b, rm, rv, MOM, EPS, True, None, cot),
              f"bn/constant/{C}/{n}", names=("save_invstd", "running_mean", "running_var", "grad_x", "grad_bias"))
    # xhat is exactly 0: the input gradient is k0 (dy - mean(dy)), the weight gradient exactly 0
    assert float(got["grad_weight"].abs().max()) == 0.0
    bn.eval()
    with torch.no_grad():
        bn.running_mean.copy_(x[0]); bn.running_var.fill_(1.0)
        assert torch.equal(R.batch_norm(x.to(dev), bn), b.to(dev).expand(n, C))


@pytest.mark.parametrize("n", [300, 1537, 4097, 102_584])
@pytest.mark.parametrize("C", [4, 8, 16, 28, 32])
def test_rows_equal_to_the_batch_mean_come_out_zero_with_the_clamped_norm(C, n):
    """``mean_rows`` with bias 0: the batch mean is exactly 0, so the all-zero rows are normalised to exactly zero rows; their handed
    norm is ``1 / 1e-8 = 1e8`` (the one value ``split_row_scale_of`` is commented as safe for) and their pre-split bytes are zero.  The
    other rows are held to the float64 bound like any input."""
    from molkgnn_amd import functional as Fn
    dev = _dev()
    x = B.make("mean_rows", n, C)
    zero = B.mean_rows_zero_rows(n)
    w, _, rm, rv = _params(C, 6)
    b = torch.zeros(C)
    for split in (False, True):
        bn = _module(C, dev, w, b, rm, rv).train()
        leaf = x.to(dev).requires_grad_(True)
        cot = torch.randn(n, C, generator=torch.Generator().manual_seed(n + C))
        got = run_build(leaf, leaf, bn, None, cot.to(dev), split_out=split)
        assert got["inv_norm"] is not None and float(got["save_mean"].abs().max()) == 0.0
        assert bool((got["inv_norm"][zero] == 1e8).all()), got["inv_norm"][zero]
        assert int(got["out"][zero].view(torch.int32).abs().max()) == 0       # (+0.0 in fp32; hi = lo = +0 in the pre-split form)
        assert torch.equal(got["inv_norm"], Fn.row_inv_norm(got["out"])) or split
        if not split:
            ref = B.reference(x, w, b, rm, rv, MOM, EPS, True, None, cot)
            f32 = yardstick(x, w, b, rm, rv, True, None, cot)
            F64.check(got, f32, ref, f"bn/meanrows/{C}/{n}")


# ------------------------------------------------------------------------------------------------- companion --
def _key(kind, n, dev, g):
    """-> (key, limit, boolean keep mask on the CPU) or (None, None, None)"""
    if kind == "all":
        return None, None, None
    if kind == "70":
        key = torch.randint(0, 1000, (n,), generator=g)
        lim = 700
    elif kind == "one":
        key = torch.ones(n, dtype=torch.int64)
        key[(2 * n) // 3] = 0
        lim = 1
    elif kind == "none":
        key = torch.full((n,), 5, dtype=torch.int64)
        lim = 5
    else:                                                   # "blocks": a sorted key -- the blocks behind the limit count nothing
        key = torch.arange(n, dtype=torch.int64)
        lim = max(n // 3, min(n, 2))
    return key.to(dev), torch.tensor([lim], dtype=torch.int64, device=dev), key < lim


def _companion_case(n, C, kind, forms):
    from molkgnn_amd import readout as R
    dev = _dev()
    g = torch.Generator().manual_seed(n * 31 + C)
    x = torch.randn(n, C, generator=g) * torch.linspace(0.5, 3.0, C) + torch.linspace(-2.0, 40.0, C)
    key, lim, keep = _key(kind, n, dev, g)
    _, _, rm, rv = _params(C, 8)
    rm64, rv64, moved = B.masked_statistics(x, keep, rm, rv, MOM)
    ref = {"running_mean": rm64, "running_var": rv64}
    cpu = torch.nn.BatchNorm1d(C, eps=EPS, momentum=MOM)
    with torch.no_grad():
        cpu.running_mean.copy_(rm); cpu.running_var.copy_(rv)
    xs = x if keep is None else x[keep]
    if xs.shape[0] > 1:
        cpu(xs)
    f32 = {"running_mean": cpu.running_mean, "running_var": cpu.running_var}
    assert moved == (xs.shape[0] > 1)
    main_x = B.make("plain", 500, 28, seed=5)
    for form in forms:
        store = x.to(dev) if form != "column" else _view(*_lay(x, "stride1", dev), C)
        for via in ("alone", "riding"):
            bn = _module(C, dev, None, None, rm, rv).train()
            if via == "alone":
                R.update_running_stats(store, bn, key, lim)
            else:
                w, b, rm2, rv2 = _params(28, 9)
                main = _module(28, dev, w, b, rm2, rv2).train()
                leaf = main_x.to(dev)
                got_main = run_build(leaf, leaf, main, companion=(store, bn, key, lim))
                F64.check(got_main, yardstick(main_x, w, b, rm2, rv2, True), B.reference(main_x, w, b, rm2, rv2, MOM, EPS, True),
                          f"bn/companion-main/{form}/{n}/{C}/{kind}")
            torch.cuda.synchronize()
            tag = f"bn/companion/{form}/{via}/{n}/{C}/{kind}"
            assert int(bn.num_batches_tracked) == (1 if moved else 0), tag
            if not moved:                                 # a degenerate batch: buffers and counter stand still
                assert torch.equal(bn.running_mean.cpu(), rm) and torch.equal(bn.running_var.cpu(), rv), tag
            F64.check({"running_mean": bn.running_mean, "running_var": bn.running_var}, f32, ref, tag)


KEYS = ("all", "70", "one", "none", "blocks")


@pytest.mark.parametrize("kind", KEYS)
@pytest.mark.parametrize("n", [1, 2, 300, 16_385, 218_000, 1_100_000])
@pytest.mark.parametrize("C", [1, 2, 3, 4, 5, 6, 7, 8])
def test_companion_narrow_rows(C, n, kind):
    """``update_running_stats`` and ``batch_norm(..., companion=...)`` against float64 (not against each other): contiguous rows of 1
    .. 8 floats take the flat form (``bn_side_block_stats_flat<C>``), the same rows at a stride of C + 1 the column form
    (``bn_side_block_stats``, up to 1 024 blocks of several trips at 1.1 M rows); one block, several, the companion's blocks behind
    the batch norm's own.  Keys that keep 70 % of the rows, one row, none (nothing may move), and a sorted key whose limit leaves
    whole blocks without a counted row."""
    _companion_case(n, C, kind, ("flat", "column"))


@pytest.mark.parametrize("kind", KEYS)
@pytest.mark.parametrize("n", [1, 2, 300, 16_385])
@pytest.mark.parametrize("C", [16, 33, 200])
def test_companion_wide_rows(C, n, kind):
    """The column form in one block and in several (64, 128 and 1 024 blocks), with every kind of key."""
    _companion_case(n, C, kind, ("contiguous",))


# -------------------------------------------------------------------------------------------------- hand-off --
@pytest.mark.parametrize("family", ["plain", "scales", "mean_rows"])
@pytest.mark.parametrize("C", [4, 8, 16, 28, 32])
def test_handed_norms_and_presplit_rows(C, family):
    """The row norms the apply pass hands on: bit-equal to ``row_inv_norm(out)`` AND within the float64 bound of
    ``1 / max(|out_f64 row|, 1e-8)`` (lanes with ``col >= C`` take part in the xor tree with zeros).  With ``split_out=True`` the rows
    decode -- ``(hi + lo) / scale`` -- to the un-split call's rows within ``kgnn_split.h``'s bound: 2^-22 |x| per element (an element
    below 2^-3 after scaling -- 2^-11 of its row's norm -- loses its lo half to fp16 subnormals: 2^-25 scaled, absolute), and where the
    library takes pre-split rows of this width the first convolution on them is bit for bit the convolution on the fp32 rows."""
    from molkgnn_amd import functional as Fn
    from tests._csr_reference import decode_split
    from tests.test_rows_split import _setup
    dev, b, plan, first, _, _ = _setup(C, dup=0.0)
    n = b.x.shape[0]
    x = B.make(family, n, C, seed=2)
    w, bias, rm, rv = _params(C, 11)
    if family == "mean_rows":
        bias = torch.zeros(C)
    res = []
    for split in (False, True):
        bn = _module(C, dev, w, bias, rm, rv).train()
        leaf = x.to(dev)
        from molkgnn_amd import readout as R
        out = R.batch_norm(leaf, bn, split_out=split)
        assert Fn.is_rows_split(out) == split
        res.append((out, Fn._handed_inv_norm(out)))
    (x0, i0), (x1, i1) = res
    assert i0 is not None and torch.equal(i0, i1) and torch.equal(i0, Fn.row_inv_norm(x0.detach()))
    ref = B.reference(x, w, bias, rm, rv, MOM, EPS, True)
    F64.check({"out": x0, "inv_norm": i0}, yardstick(x, w, bias, rm, rv, True), ref, f"bn/handoff/{family}/{C}")
    back = decode_split(x1.detach(), C, i1)
    e = (i1.view(torch.int32) >> 23) & 0xFF
    scale = torch.exp2((e - 127 + 8).float())[:, None]
    a0 = x0.detach().abs()
    err = (back - x0.detach()).abs()
    assert bool((err * scale <= 2.0 ** -22 * a0 * scale + 2.0 ** -25).all()), float((err / a0.clamp_min(1e-30)).max())
    big = a0 * scale >= 0.125
    assert bool((err[big] <= 2.0 ** -22 * a0[big]).all())
    p1, E = first._bank_params("train", x0.detach())
    supported = Fn.rows_split_supported(plan, p1, C, E, plan.n_atoms)
    assert supported or C != 28, "the first layer of the network takes pre-split rows"
    if supported:
        with torch.no_grad():
            o0 = Fn.kernelsetconv(x0.detach(), plan, False, p1, E, "auto", block_rows=True, propagate=True)
            o1 = Fn.kernelsetconv(x1, plan, False, p1, E, "auto", block_rows=True, propagate=True)
        assert torch.equal(o0, o1)


# ---------------------------------------------------------------------------------------------------- riders --
@pytest.mark.parametrize("rider", ["touch", "prepare", "both"])
def test_riders_behind_the_statistics_launch_leave_the_float64_bound(rider):
    """A pending ``mkgnn_touch_hint`` and a pending ``mkgnn_bank_prepare_deferred`` ride behind the statistics launch
    (``bn_stats_kernel`` / ``bn_stats_prep_kernel``) together with a multi-block companion: the batch norm's own results and the
    companion's buffers are bit for bit those of the bare call AND within the float64 bound."""
    from molkgnn_amd import functional as Fn
    from molkgnn_amd.plan import plan_from_data
    from molkgnn_amd.synthetic import make_batch
    from molkgnn_amd.train import GNNModel
    from molkgnn_amd import readout as R
    dev = _dev()
    b = make_batch(300, seed=5).to(dev)
    plan = plan_from_data(b)
    n = b.x.shape[0]
    x = B.make("offset", n, 28, seed=7)
    side = torch.randn(20_000, 7, generator=torch.Generator().manual_seed(1)) * 2 + 3
    w, bias, rm, rv = _params(28, 12)
    _, _, srm, srv = _params(7, 13)
    cot = torch.randn(n, 28, generator=torch.Generator().manual_seed(2))
    torch.manual_seed(3)
    gnn = GNNModel().to(dev).gnn_model.gnn
    pl = [layer._bank_params("train", b.x) for layer in gnn.layers]
    args = ([p for p, _ in pl], [28, 110, 110], pl[0][1], n, plan.n_slots)
    lib = R._lib.load()

    def run(with_rider):
        bn = _module(28, dev, w, bias, rm, rv).train()
        sbn = _module(7, dev, None, None, srm, srv).train()
        leaf = x.to(dev).requires_grad_(True)
        comp = (side.to(dev), sbn, None, None)
        if not with_rider:
            got = run_build(leaf, leaf, bn, None, cot.to(dev), companion=comp)
        else:
            if rider in ("prepare", "both"):
                Fn.prepare_banks(*args, defer=True)
            if rider in ("touch", "both"):
                with Fn.touch_hint(Fn.plan_touch_list(plan)) as h:
                    got = run_build(leaf, leaf, bn, None, cot.to(dev), companion=comp)
                assert h.taken
            else:
                got = run_build(leaf, leaf, bn, None, cot.to(dev), companion=comp)
            if rider in ("prepare", "both"):
                assert int(lib.mkgnn_bank_prepare_withdraw()) == 0       # the statistics launch carried it
        torch.cuda.synchronize()
        return got, sbn
    bare, sbn0 = run(False)
    got, sbn1 = run(True)
    for k in STAT_NAMES:
        assert bare[k] is not None and torch.equal(bare[k], got[k]), k
    assert torch.equal(sbn0.running_mean, sbn1.running_mean) and torch.equal(sbn0.running_var, sbn1.running_var)
    assert int(sbn1.num_batches_tracked) == 1
    F64.check(got, yardstick(x, w, bias, rm, rv, True, None, cot), B.reference(x, w, bias, rm, rv, MOM, EPS, True, None, cot),
              f"bn/rider/{rider}")
    srm64, srv64, _ = B.masked_statistics(side, None, srm, srv, MOM)
    cpu = torch.nn.BatchNorm1d(7, eps=EPS, momentum=MOM)
    with torch.no_grad():
        cpu.running_mean.copy_(srm); cpu.running_var.copy_(srv)
    cpu(side)
    F64.check({"running_mean": sbn1.running_mean, "running_var": sbn1.running_var},
              {"running_mean": cpu.running_mean, "running_var": cpu.running_var}, {"running_mean": srm64, "running_var": srv64},
              f"bn/rider-companion/{rider}")
