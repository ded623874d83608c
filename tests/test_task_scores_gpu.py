"""``mkgnn_task_scores`` (``readout.task_scores``): every task's logit of every row.  Bit equality with the task-indexed head
(``mkgnn_task_head_forward``, row i labelled with task t, dropout 0), a derived float64 bound, both output layouts, untouched
cells outside the written region, rejections, and the torch route beyond the kernels' limits."""
from functools import lru_cache

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# rows around a block's 16, columns around a half-wave's 32 and at the limit, T at 1, 2, 9 and the limit
CASES = [(1, 1, 1), (15, 32, 9), (16, 32, 32), (17, 33, 2), (250, 64, 9), (4096, 32, 9)]
EPS = 2.0 ** -24


def _L():
    from molkgnn_amd import _lib
    return _lib


def _bits(t):
    return t.detach().contiguous().view(torch.int32).cpu().numpy()


@lru_cache(maxsize=None)
def _inputs(n, H, T):
    """float32 CPU inputs of a case (never written to): ``emb [n, H]`` whose last rows are the hazards -- zeros, a 1e30 / -1e30
    pair, denormals -- where there is room for them; ``w [T, H]``; ``b [T]``."""
    g = torch.Generator().manual_seed(1000 * n + 10 * H + T)
    emb = torch.randn(n, H, generator=g) * 2
    w = torch.randn(T, H, generator=g) * H ** -0.5
    b = torch.randn(T, generator=g)
    if n >= 15:
        emb[n - 1] = 0.0
        emb[n - 2] = 1e-41 * torch.arange(1, H + 1)                 # denormals
        emb[n - 3, 0] = 1e30
        if H > 1:
            emb[n - 3, H - 1] = -1e30
    return emb, w, b


def _call(emb, w, b, n, H, T, pred, rs, ts):
    L = _L()
    rc = L.load().mkgnn_task_scores(emb.data_ptr(), emb.stride(0) if emb.dim() == 2 and emb.shape[0] > 1 else max(H, emb.shape[-1]), n, H, T,
                                    w.data_ptr(), None if b is None else b.data_ptr(), pred.data_ptr(), rs, ts,
                                    L.stream_ptr(torch.device(DEV)))
    return rc


def _padded(emb, pad):
    """The same rows with ``pad`` NaN columns behind them: an ``emb_stride`` larger than H."""
    n, H = emb.shape
    store = torch.full((n, H + pad), float("nan"), dtype=torch.float32, device=DEV)
    store[:, :H] = emb
    return store[:, :H]


def _head_column(emb, w, b, t, n, H, T):
    """``pred`` of ``mkgnn_task_head_forward`` with every row labelled with task ``t`` (kind mse, dropout 0)."""
    L = _L()
    lib = L.load()
    task = torch.full((n,), t, dtype=torch.int32, device=DEV)
    y = torch.zeros(n, dtype=torch.float32, device=DEV)
    pred = torch.empty(n, dtype=torch.float32, device=DEV)
    loss = torch.empty(1, dtype=torch.float32, device=DEV)
    ws = torch.empty(int(lib.mkgnn_task_head_workspace_bytes(n, H, T)), dtype=torch.uint8, device=DEV)
    L.check(lib.mkgnn_task_head_forward(L.LOSS_SQERR_MEAN, emb.data_ptr(), emb.stride(0) if n > 1 else emb.shape[1] + 3, n, H, T,
                                        w.data_ptr(), None if b is None else b.data_ptr(), y.data_ptr(), task.data_ptr(), None, n, 0.0,
                                        None, None, pred.data_ptr(), loss.data_ptr(), ws.data_ptr(), ws.numel(),
                                        L.stream_ptr(torch.device(DEV))), "mkgnn_task_head_forward")
    return pred


@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("n,H,T", CASES)
def test_bit_equal_to_the_task_head_and_inside_the_float64_bound(n, H, T, bias):
    from molkgnn_amd.readout import task_scores
    emb_c, w_c, b_c = _inputs(n, H, T)
    emb, w = _padded(emb_c.to(DEV), 3), w_c.to(DEV)
    b = b_c.to(DEV) if bias else None
    ffn = torch.nn.Linear(H, T, bias=bias).to(DEV)
    with torch.no_grad():
        ffn.weight.copy_(w)
        if bias:
            ffn.bias.copy_(b)
        pred = task_scores(emb, ffn)
    assert pred.shape == (n, T) and pred.dtype == torch.float32
    # every column against the head's pred for that task: int32 bit patterns
    for t in range(T):
        want = _head_column(emb, w, b, t, n, H, T)
        assert np.array_equal(_bits(pred[:, t]), _bits(want)), (n, H, T, t)
    # |pred - exact| <= (H + 2) 2^-24 (|emb| |w|^T + |b|): a length-H float32 sum in any order, with or without fused
    # multiply-adds, plus the bias add (Higham, Accuracy and Stability of Numerical Algorithms, 3.1: gamma_(H+1), first order).
    # That model, fl(x op y) = (x op y)(1 + d), holds only while nothing underflows; the row of denormals is there to underflow.
    # With gradual underflow (Higham 2.8) a product is (x y)(1 + d) + e with |e| <= 2^-150, half the spacing of the denormals, and
    # a sum that lands among the denormals is exact: H products add at most H 2^-150, carried through the later additions by a
    # factor <= 1 + (H + 2) 2^-24.  Without that term no correct float32 evaluation of the denormal row without bias can pass
    # (measured on the kernel there: 3.3e-45, 2.4 denormal spacings, against a relative bound of 1e-47); everywhere else the term
    # is more than 30 orders of magnitude below the relative bound.
    e64, w64 = emb_c.double(), w_c.double()
    b64 = b_c.double() if bias else torch.zeros(T, dtype=torch.float64)
    exact = e64 @ w64.T + b64
    bound = (H + 2) * EPS * (e64.abs() @ w64.abs().T + b64.abs()) + H * 2.0 ** -150 * (1 + (H + 2) * EPS)
    err = (pred.double().cpu() - exact).abs()
    print(f"n={n} H={H} T={T} bias={bias}: max err / bound = {float((err / bound.clamp(min=1e-300)).max()):.3f}")
    assert bool((err <= bound).all()), float((err - bound).max())
    if n >= 15 and not bias:
        assert int(pred[n - 1].abs().sum()) == 0                        # the row of zeros


@pytest.mark.parametrize("n,H,T", [(17, 33, 2), (250, 64, 9), (16, 32, 32), (1, 1, 1)])
def test_both_layouts_hold_the_same_bits_and_nothing_else_is_written(n, H, T):
    from molkgnn_amd.readout import task_scores
    emb_c, w_c, b_c = _inputs(n, H, T)
    ffn = torch.nn.Linear(H, T).to(DEV)
    with torch.no_grad():
        ffn.weight.copy_(w_c)
        ffn.bias.copy_(b_c)
        emb = emb_c.to(DEV)
        rows = task_scores(emb, ffn)
        tasks = task_scores(emb, ffn, task_major=True)
        assert tasks.shape == (T, n) and np.array_equal(_bits(tasks.t()), _bits(rows))
        # into the middle of larger, NaN-prefilled buffers, the leading n - 1 rows only: every other cell stays NaN
        m = max(n - 1, 1)
        big_r = torch.full((n + 2, T + 3), float("nan"), device=DEV)
        got = task_scores(emb, ffn, n_rows=m, out=big_r[1:1 + m, 2:2 + T])
        assert got.data_ptr() == big_r[1:, 2:].data_ptr()
        big_t = torch.full((T + 2, n + 5), float("nan"), device=DEV)
        task_scores(emb, ffn, n_rows=m, out=big_t[1:1 + T, 3:3 + m], task_major=True)
    inside = torch.zeros_like(big_r, dtype=torch.bool)
    inside[1:1 + m, 2:2 + T] = True
    assert bool(torch.isnan(big_r[~inside]).all()) and np.array_equal(_bits(big_r[1:1 + m, 2:2 + T]), _bits(rows[:m]))
    inside = torch.zeros_like(big_t, dtype=torch.bool)
    inside[1:1 + T, 3:3 + m] = True
    assert bool(torch.isnan(big_t[~inside]).all()) and np.array_equal(_bits(big_t[1:1 + T, 3:3 + m].t()), _bits(rows[:m]))


def test_rejections_and_the_empty_call():
    lib = _L().load()
    n, H, T = 16, 8, 3
    emb = torch.zeros(n, H, device=DEV)
    w, b = torch.zeros(T, H, device=DEV), torch.zeros(T, device=DEV)
    pred = torch.full((n, 40), float("nan"), device=DEV)
    for change, word in ((dict(T=0), b"tasks"), (dict(T=33), b"tasks"), (dict(H=0), b"width"), (dict(H=65), b"width")):
        a = dict(dict(H=H, T=T), **change)
        rc = _call(emb, w, b, n, a["H"], a["T"], pred, 40, 1)
        assert rc != 0 and word in lib.mkgnn_last_error(), change
    stream = _L().stream_ptr(torch.device(DEV))
    for args in ((None, H, n, H, T, w.data_ptr(), b.data_ptr(), pred.data_ptr(), 40, 1),
                 (emb.data_ptr(), H, n, H, T, None, b.data_ptr(), pred.data_ptr(), 40, 1),
                 (emb.data_ptr(), H, n, H, T, w.data_ptr(), b.data_ptr(), None, 40, 1)):
        assert lib.mkgnn_task_scores(*args, stream) != 0 and b"null" in lib.mkgnn_last_error()
    # a row stride smaller than the row, strides under which two outputs share an element, a negative row count
    assert lib.mkgnn_task_scores(emb.data_ptr(), H - 1, n, H, T, w.data_ptr(), b.data_ptr(), pred.data_ptr(), 40, 1, stream) != 0
    assert lib.mkgnn_task_scores(emb.data_ptr(), H, n, H, T, w.data_ptr(), b.data_ptr(), pred.data_ptr(), 2, 1, stream) != 0
    assert b"share" in lib.mkgnn_last_error()
    assert lib.mkgnn_task_scores(emb.data_ptr(), H, n, H, T, w.data_ptr(), b.data_ptr(), pred.data_ptr(), 0, 1, stream) != 0
    assert lib.mkgnn_task_scores(emb.data_ptr(), H, -1, H, T, w.data_ptr(), b.data_ptr(), pred.data_ptr(), 40, 1, stream) != 0
    # no rows: a no-op that returns 0
    assert lib.mkgnn_task_scores(emb.data_ptr(), H, 0, H, T, w.data_ptr(), b.data_ptr(), pred.data_ptr(), 40, 1, stream) == 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(pred).all())                                # nothing was launched by any of them


def test_python_wrapper_refuses_a_recorded_gradient_and_wrong_shapes():
    from molkgnn_amd.readout import task_scores
    ffn = torch.nn.Linear(8, 3).to(DEV)
    emb = torch.zeros(4, 8, device=DEV)
    with pytest.raises(RuntimeError):
        task_scores(emb, ffn)                                           # (the parameters require a gradient and grad mode is on)
    with torch.no_grad():
        assert task_scores(emb, ffn, n_rows=0).shape == (0, 3)
        with pytest.raises(ValueError):
            task_scores(emb, ffn, n_rows=5)
        with pytest.raises(ValueError):
            task_scores(emb, ffn, out=torch.zeros(3, 4, device=DEV))    # (that is the task-major shape)
        with pytest.raises(ValueError):
            task_scores(torch.zeros(4, 7, device=DEV), ffn)
        with pytest.raises(_L().MolKGNNLibraryError):
            task_scores(torch.zeros(4, 8), ffn)


@pytest.mark.parametrize("T,H", [(40, 32), (9, 70)])
def test_torch_route_beyond_the_limits_meets_the_same_bound(T, H):
    from molkgnn_amd.readout import task_head_supported, task_scores
    assert not task_head_supported(T, H)
    n = 37
    g = torch.Generator().manual_seed(T)
    emb_c, w_c, b_c = torch.randn(n, H, generator=g) * 2, torch.randn(T, H, generator=g) * H ** -0.5, torch.randn(T, generator=g)
    ffn = torch.nn.Linear(H, T).to(DEV)
    with torch.no_grad():
        ffn.weight.copy_(w_c)
        ffn.bias.copy_(b_c)
        pred = task_scores(emb_c.to(DEV), ffn)
        tasks = task_scores(emb_c.to(DEV), ffn, task_major=True)
    assert pred.shape == (n, T) and np.array_equal(_bits(tasks.t()), _bits(pred))
    e64, w64, b64 = emb_c.double(), w_c.double(), b_c.double()
    err = (pred.double().cpu() - (e64 @ w64.T + b64)).abs()
    assert bool((err <= (H + 2) * EPS * (e64.abs() @ w64.abs().T + b64.abs())).all())
