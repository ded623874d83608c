"""The batch norm's register forms (``csrc/kgnn_batchnorm.hip``: ``bn_merge_held``, ``bn_total_pair_held``,
``bn_side_totals_held``) against its loop forms IN ONE PROCESS: every case calls the C ABI twice on the same inputs, once
behind ``mkgnn_debug_set_bn_merge(0)`` and once on the default
dispatch, every output buffer and the workspaces pre-filled with NaN, and compares every tensor the calls write on its raw bits
-- ``out`` (fp32 or pre-split), ``inv_norm``, ``save_mean``, ``save_invstd``, the running statistics, ``num_batches_tracked``,
``grad_x``, ``grad_weight``, ``grad_bias``, the companion's running statistics and counter.  No tolerance anywhere; the float64
bound of the default dispatch is ``tests/test_batch_norm_f64.py``'s.  ``pytest -m gpu``.

Shapes: the smallest at which the two forms can differ.  A thread of the merge holds ``ceil(256 / RS)`` terms, ``RS = 256 / CL``:
one trip of eight for CL <= 8, two at 16, four at 32 (C = 28, 32), the loop form from CL = 64 on.  257 rows at 256 blocks are
shares of two rows with empty blocks behind them (the ``left == 0`` term); 131 072 rows of 28 floats (16 384 of 256) are the last
share of one trip of the statistics pass, one row more is the first of two (that pass is the same code in both forms: holding
a one-trip share in registers was measured and left out, DESIGN 4.4 -- the row counts stay as the boundary of the share sizes
the merge's ``left`` terms see).
"""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

EPS = 1e-5
MOM = 0.1
NAN = float("nan")


@pytest.fixture(scope="module")
def _pool():
    pool = torch.cuda.MemPool()
    yield pool
    torch.cuda.synchronize()
    del pool


@pytest.fixture(autouse=True)
def _private_pool(request, _pool):
    """The module allocates many odd sizes; they come from a memory pool of its own, so that the modules behind it find the
    caching allocator as they would without it (``tests/test_neighbours_gpu.py`` has a case that depends on which buffers
    end up next to each other).  The capture test opens the pool itself, around what it runs eagerly."""
    if "captured" in request.node.name:
        yield
        return
    with torch.cuda.use_mem_pool(_pool):
        yield


def _dev():
    assert torch.cuda.is_available(), "pytest -m gpu needs the MI355X"
    return torch.device("cuda:0")


def _lib():
    from molkgnn_amd import _lib as L
    return L, L.load()


def _nan(*shape, dev):
    return torch.full(shape, NAN, dtype=torch.float32, device=dev)


def _strided(t, layout, dev):
    """[n, C] on the device: contiguous (``aligned``: float4-readable iff C % 4 == 0) or at a row stride of C + 1 (``stride1``)."""
    n, C = t.shape
    if layout == "aligned":
        return t.to(dev).contiguous()
    big = torch.zeros(n, C + 1, device=dev)
    big[:, :C] = t.to(dev)
    return big[:, :C]


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def _companion_struct(L, c, dev):
    """c: dict(x=[m, Cs] device tensor, key, lim) -> (struct, workspace, the buffers it moves)"""
    Cs = c["x"].shape[1]
    g = torch.Generator().manual_seed(Cs)
    rm = (torch.randn(Cs, generator=g) * 0.2).to(dev)
    rv = (torch.rand(Cs, generator=g) + 0.5).to(dev)
    nbt = torch.zeros(1, dtype=torch.int64, device=dev)
    st = L.BnStats(c["x"].data_ptr(), c["x"].stride(0), c["x"].shape[0], Cs, rm.data_ptr(), rv.data_ptr(), MOM, nbt.data_ptr(),
                   L.ptr(c.get("key")), L.ptr(c.get("lim")))
    return st, {"side_running_mean": rm, "side_running_var": rv, "side_num_batches_tracked": nbt}


def _params(C, dev):
    g = torch.Generator().manual_seed(100 + C)
    return ((torch.rand(C, generator=g) + 0.5).to(dev), torch.randn(C, generator=g).to(dev), (torch.randn(C, generator=g) * 0.2).to(dev),
            (torch.rand(C, generator=g) + 0.5).to(dev))


def call(x, *, affine=True, track=True, training=True, n_valid=None, inv=False, split=False, companion=None, cot=None, grad_x=True,
         before=None, params=None):
    """One forward (and, with ``cot``, one backward) through the C ABI on fresh NaN-filled outputs -> {name: tensor}.  ``params``:
    ``_params`` made ahead (a capture cannot copy from the host); the running statistics are cloned on the device."""
    L, lib = _lib()
    dev = x.device
    n, C = x.shape
    w, b, rm, rv = params if params is not None else _params(C, dev)
    if not affine:
        w = b = None
    rm = rm.clone() if (track or not training) else None
    rv = rv.clone() if (track or not training) else None
    nbt = torch.zeros(1, dtype=torch.int64, device=dev) if track else None
    nv = None if n_valid is None else torch.tensor([n_valid], dtype=torch.int64, device=dev)
    res = {"out": _nan(n, C, dev=dev), "save_mean": _nan(C, dev=dev), "save_invstd": _nan(C, dev=dev)}
    if inv:
        res["inv_norm"] = _nan(n, dev=dev)
    ws_bytes = int(lib.mkgnn_batchnorm_workspace_bytes(C))
    ws = _nan(ws_bytes // 4, dev=dev)
    st, cws, cws_bytes = None, None, 0
    if companion is not None:
        st, moved = _companion_struct(L, companion, dev)
        res.update(moved)
        cws_bytes = int(lib.mkgnn_batchnorm_stats_workspace_bytes(st.C))
        cws = _nan(cws_bytes // 4, dev=dev)
    stream = L.stream_ptr(dev)
    if before is not None:
        before()
    L.check(lib.mkgnn_batchnorm_forward_with_stats(
        x.data_ptr(), x.stride(0), n, C, L.ptr(w), L.ptr(b), L.ptr(rm), L.ptr(rv), MOM, EPS, int(training) | (2 if split else 0),
        res["out"].data_ptr(), C, res["save_mean"].data_ptr(), res["save_invstd"].data_ptr(), L.ptr(res.get("inv_norm")),
        L.ptr(nbt if training else None), L.ptr(nv), ws.data_ptr(), ws_bytes, None if st is None else ctypes.byref(st), L.ptr(cws),
        cws_bytes, stream), "mkgnn_batchnorm_forward_with_stats")
    if rm is not None:
        res["running_mean"], res["running_var"] = rm, rv
    if nbt is not None:
        res["num_batches_tracked"] = nbt
    if cot is not None:
        if grad_x:
            res["grad_x"] = _nan(n, C, dev=dev)
        if affine:
            res["grad_weight"] = _nan(C, dev=dev)
        res["grad_bias"] = _nan(C, dev=dev)
        ws2 = _nan(ws_bytes // 4, dev=dev)
        L.check(lib.mkgnn_batchnorm_backward(
            cot.data_ptr(), cot.stride(0), x.data_ptr(), x.stride(0), n, C, L.ptr(w), res["save_mean"].data_ptr(),
            res["save_invstd"].data_ptr(), int(training), L.ptr(res.get("grad_x")), C, L.ptr(res.get("grad_weight")),
            res["grad_bias"].data_ptr(), L.ptr(nv), ws2.data_ptr(), ws_bytes, stream), "mkgnn_batchnorm_backward")
        res["_keep"] = (ws2,)
    res["_keep"] = res.get("_keep", ()) + (ws, cws, w, b, nv, st)
    return res


def both(x, tag, **kw):
    """The call in the loop forms and on the default dispatch; every tensor equal on its bits.  Returns the default's results."""
    _, lib = _lib()
    try:
        assert lib.mkgnn_debug_set_bn_merge(0) == 0
        loop = call(x, **kw)
        torch.cuda.synchronize()
    finally:
        lib.mkgnn_debug_set_bn_merge(-1)
    held = call(x, **kw)
    torch.cuda.synchronize()
    same(loop, held, tag)
    return held


def same(a, b, tag):
    assert a.keys() == b.keys(), tag
    names = [k for k in a if not k.startswith("_")]
    assert "out" in names and "save_mean" in names
    for k in names:
        assert torch.equal(_bits(a[k]), _bits(b[k])), (tag, k)


def _x(n, C, seed=0):
    g = torch.Generator().manual_seed(1000 * C + n % 997 + seed)
    return torch.randn(n, C, generator=g) * torch.linspace(0.3, 3.0, C) + torch.linspace(-5.0, 50.0, C)


def _cot(n, C, dev, layout="aligned"):
    return _strided(torch.randn(n, C, generator=torch.Generator().manual_seed(n + C)), layout, dev)


def _written(res):
    """Nothing the call should have written is left NaN (fp32 outputs only)."""
    for k, v in res.items():
        if not k.startswith("_") and v.dtype == torch.float32 and k != "out":
            assert not bool(torch.isnan(v).any()), k


# ------------------------------------------------------------------------------------------------------ widths --
@pytest.mark.parametrize("layout", ["aligned", "stride1"])
@pytest.mark.parametrize("C", [1, 3, 4, 7, 8, 28, 32, 33, 64, 256])
def test_widths(C, layout):
    """One, two and four trips of held terms (CL <= 8, 16, 32) and the loop form (CL >= 64, untouched), on float4-readable rows and
    on rows at a stride of C + 1; 1 537 rows: 256 shares of 7, the last non-empty one of 4, 36 empty blocks."""
    dev = _dev()
    n = 1537
    x = _strided(_x(n, C), layout, dev)
    inv = C <= 32 and C % 4 == 0 and layout == "aligned"
    got = both(x, f"width/{C}/{layout}", inv=inv, cot=_cot(n, C, dev, layout))
    _written(got)
    assert not bool(torch.isnan(got["out"]).any())
    assert int(got["num_batches_tracked"]) == 1


# -------------------------------------------------------------------------------------------------- row counts --
@pytest.mark.parametrize("grad_x", [True, False])
@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 511, 4097, 131_072, 131_073])
def test_row_counts_at_28(n, grad_x):
    dev = _dev()
    x = _x(n, 28).to(dev)
    _written(both(x, f"rows28/{n}/{grad_x}", inv=True, cot=_cot(n, 28, dev), grad_x=grad_x))


@pytest.mark.parametrize("n", [16_384, 16_385])
def test_row_counts_at_256(n):
    """The same boundary of the held share at RS = 4 (the merge itself is the loop form at this width)."""
    dev = _dev()
    _written(both(_x(n, 256).to(dev), f"rows256/{n}", cot=_cot(n, 256, dev)))


@pytest.mark.parametrize("grad_x", [True, False])
@pytest.mark.parametrize("n,nv", [(300, 1), (300, 255), (300, 257), (103_865, 102_241)])
def test_n_valid(n, nv, grad_x):
    """Padded batches: the shares are dealt over the counted rows, the apply pass over all of them."""
    dev = _dev()
    cot = _cot(n, 28, dev)
    cot[nv:] = 0.0
    _written(both(_x(n, 28).to(dev), f"nvalid/{n}/{nv}/{grad_x}", n_valid=nv, inv=True, cot=cot, grad_x=grad_x))


# ------------------------------------------------------------------------------------------------------- modes --
@pytest.mark.parametrize("C", [28, 32])
@pytest.mark.parametrize("mode", ["no_tracking", "no_affine", "no_inv", "inv", "split", "eval"])
def test_modes(mode, C):
    dev = _dev()
    n = 1537
    x = _x(n, C, seed=3).to(dev)
    kw = {"no_tracking": dict(track=False, inv=True), "no_affine": dict(affine=False, inv=True), "no_inv": dict(), "inv": dict(inv=True),
          "split": dict(inv=True, split=True), "eval": dict(training=False, inv=True)}[mode]
    got = both(x, f"mode/{mode}/{C}", cot=_cot(n, C, dev), **kw)
    if mode == "split":                                   # (the rows are split fp16 pairs: not the fp32 call's bits)
        plain = call(x, inv=True)
        torch.cuda.synchronize()
        assert not torch.equal(_bits(plain["out"]), _bits(got["out"])) and torch.equal(_bits(plain["inv_norm"]), _bits(got["inv_norm"]))


# --------------------------------------------------------------------------------------------------- companion --
def _side(kind, dev):
    """-> companion dict.  flat: [53 * 4096 + 1, 7] contiguous (54 blocks of the flat form, the odd row last); wide16: [16 385, 16]
    (129 blocks of the column form: two trips of held terms); wide33: [16 385, 33] (the loop form); one: 300 rows (one block: the
    totals in the statistics launch itself)."""
    n, C = {"flat": (53 * 4096 + 1, 7), "wide16": (16_385, 16), "wide33": (16_385, 33), "one": (300, 7)}[kind]
    g = torch.Generator().manual_seed(n + C)
    return {"x": (torch.randn(n, C, generator=g) * 2 + 3).to(dev)}


@pytest.mark.parametrize("keyed", [False, True])
@pytest.mark.parametrize("kind", ["flat", "wide16", "wide33", "one"])
def test_companion(kind, keyed):
    """The companion riding on the batch norm's launches, and alone (``mkgnn_batchnorm_update_stats``)."""
    L, lib = _lib()
    dev = _dev()
    c = _side(kind, dev)
    if keyed:
        m = c["x"].shape[0]
        c["key"] = torch.randint(0, 1000, (m,), generator=torch.Generator().manual_seed(m)).to(dev)
        c["lim"] = torch.tensor([700], dtype=torch.int64, device=dev)
    got = both(_x(500, 28).to(dev), f"companion/{kind}/{keyed}", inv=True, companion=c)
    assert int(got["side_num_batches_tracked"]) == 1

    def alone():
        st, moved = _companion_struct(L, c, dev)
        nbytes = int(lib.mkgnn_batchnorm_stats_workspace_bytes(st.C))
        ws = _nan(nbytes // 4, dev=dev)
        L.check(lib.mkgnn_batchnorm_update_stats(ctypes.byref(st), ws.data_ptr(), nbytes, L.stream_ptr(dev)), "mkgnn_batchnorm_update_stats")
        torch.cuda.synchronize()
        return moved
    try:
        lib.mkgnn_debug_set_bn_merge(0)
        loop = alone()
    finally:
        lib.mkgnn_debug_set_bn_merge(-1)
    held = alone()
    for k in loop:
        assert torch.equal(_bits(loop[k]), _bits(held[k])), k
        assert torch.equal(_bits(held[k]), _bits(got[k])), k       # (riding or alone: the same statistics)


# ------------------------------------------------------------------------------------------------------ riders --
@pytest.mark.parametrize("rider", ["touch", "prepare", "both"])
def test_riders(rider):
    """A pending touch hint and a pending bank preparation behind the statistics launch: the batch norm's bits are those of the
    bare call, in either form."""
    from molkgnn_amd import functional as Fn
    from molkgnn_amd.plan import plan_from_data
    from molkgnn_amd.synthetic import make_batch
    from molkgnn_amd.train import GNNModel
    _, lib = _lib()
    dev = _dev()
    b = make_batch(300, seed=5).to(dev)
    plan = plan_from_data(b)
    n = b.x.shape[0]
    torch.manual_seed(3)
    gnn = GNNModel().to(dev).gnn_model.gnn
    pl = [layer._bank_params("train", b.x) for layer in gnn.layers]
    args = ([p for p, _ in pl], [28, 110, 110], pl[0][1], n, plan.n_slots)
    x = _x(n, 28, seed=7).to(dev)
    c = _side("wide16", dev)
    bare = call(x, inv=True, companion=c)
    torch.cuda.synchronize()

    def ridden():
        def before():
            if rider in ("prepare", "both"):
                Fn.prepare_banks(*args, defer=True)
        if rider in ("touch", "both"):
            with Fn.touch_hint(Fn.plan_touch_list(plan)) as h:
                got = call(x, inv=True, companion=c, before=before)
            assert h.taken
        else:
            got = call(x, inv=True, companion=c, before=before)
        if rider in ("prepare", "both"):
            assert int(lib.mkgnn_bank_prepare_withdraw()) == 0       # the statistics launch carried it
        torch.cuda.synchronize()
        return got
    try:
        lib.mkgnn_debug_set_bn_merge(0)
        loop = ridden()
    finally:
        lib.mkgnn_debug_set_bn_merge(-1)
    held = ridden()
    same(bare, loop, f"rider/{rider}/loop")
    same(bare, held, f"rider/{rider}/held")


# ----------------------------------------------------------------------------------------------------- capture --
def test_captured_forward_and_backward_replay_the_eager_bits(_pool):
    dev = _dev()
    n = 4097
    side = torch.cuda.Stream()
    with torch.cuda.use_mem_pool(_pool):
        x = _x(n, 28).to(dev)
        cot = _cot(n, 28, dev)
        eager = both(x, "capture/eager", inv=True, cot=cot)
        params = _params(28, dev)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            call(x, inv=True, cot=cot, params=params)     # (warm-up on the capture's stream)
        torch.cuda.synchronize()
    with torch.cuda.stream(side):
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            got = call(x, inv=True, cot=cot, params=params)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for k, v in got.items():                              # (the capture ran nothing: poison what the replay must write)
        if not k.startswith("_") and v.dtype == torch.float32 and not k.startswith("running"):
            v.fill_(NAN)
    graph.replay()
    torch.cuda.synchronize()
    for k in ("out", "inv_norm", "save_mean", "save_invstd", "grad_x", "grad_weight", "grad_bias"):
        assert torch.equal(_bits(eager[k]), _bits(got[k])), k
