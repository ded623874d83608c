"""Gradient clipping by global norm and the non-finite guard of the fused AdamW step, everything that needs no GPU: the C ABI's
declarations and exports, the host-only workspace size, the argument errors of the entry, of ``FusedAdamW`` and of
``configure_optimizer``, and the reference module ``tests/_clip_f64.py`` pinned to ``torch.nn.utils.clip_grad_norm_``."""
import ctypes
import math
import os
import re

import pytest
import torch

from tests import _adamw_f64 as A
from tests import _clip_f64 as K

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("mkgnn_adamw_clip_workspace_bytes", "mkgnn_adamw_step_clipped")


def test_header_declares_both_entries_and_abi_stays_8():
    text = open(os.path.join(REPO, "include", "molkgnn_hip.h")).read()
    assert re.search(r"\bsize_t mkgnn_adamw_clip_workspace_bytes\(const mkgnn_adamw_tensor\* tensors, int32_t n_tensors\);", text)
    assert re.search(r"\bint mkgnn_adamw_step_clipped\(const mkgnn_adamw_tensor\* tensors, int32_t n_tensors, const mkgnn_adamw_group\* "
                     r"groups,\s+int32_t n_groups, float max_norm, int32_t skip_nonfinite, void\* workspace, size_t workspace_bytes,\s+"
                     r"float\* stats, void\* stream\);", text)
    cap = re.search(r"#define MKGNN_ADAMW_CLIP_PROLOGUE_BLOCKS (\d+)\b", text)
    assert cap and int(cap.group(1)) >= 256
    assert re.search(r"#define MKGNN_ABI_VERSION 8\b", text)


def test_lib_types_both_entries_and_lists_them():
    from molkgnn_amd import _lib
    assert _lib.ABI_VERSION == 8
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRIES:
        assert name in _lib.EXPORTS, name
        assert hasattr(raw, name), name
    lib = _lib.load()
    assert lib.mkgnn_abi_version() == 8
    assert lib.mkgnn_adamw_clip_workspace_bytes.restype is ctypes.c_size_t and len(lib.mkgnn_adamw_clip_workspace_bytes.argtypes) == 2
    assert lib.mkgnn_adamw_step_clipped.restype is ctypes.c_int and len(lib.mkgnn_adamw_step_clipped.argtypes) == 10
    assert lib.mkgnn_adamw_step_clipped.argtypes[4] is ctypes.c_float and lib.mkgnn_adamw_step_clipped.argtypes[7] is ctypes.c_size_t


def _table(sizes, ptr=64):
    from molkgnn_amd import _lib
    t = (_lib.AdamWTensor * max(len(sizes), 1))()
    for e, n in zip(t, sizes):
        e.param, e.grad, e.state, e.numel, e.group, e.active = ptr, ptr, ptr, n, 0, None
    return t


def test_workspace_bytes_is_host_only():
    """No pointer of the table is followed: at least one double per block of ``ceil(n / 1024)``, nothing for an empty table."""
    from molkgnn_amd import _lib
    lib = _lib.load()
    assert lib.mkgnn_adamw_clip_workspace_bytes(None, 0) == 0
    assert lib.mkgnn_adamw_clip_workspace_bytes(_table([]), 0) == 0
    for sizes in ([1], [1024], [1025], list(A.BLOCK_SIZES), A.table_sizes(161), [513 * 1024, 3, 5]):
        blocks = sum((n + A.CHUNK - 1) // A.CHUNK for n in sizes)
        got = lib.mkgnn_adamw_clip_workspace_bytes(_table(sizes), len(sizes))
        assert 8 * blocks <= got <= 8 * blocks + 64 and got % 8 == 0, (sizes[:4], got)


def test_entry_refuses_bad_arguments_before_any_launch():
    """Every check comes before a launch, so host memory stands in for the device's: max_norm that is zero, negative or NaN, a
    workspace that is null, short or misaligned, null stats, a fifth group, a tensor without elements."""
    import numpy as np
    from molkgnn_amd import _lib
    lib = _lib.load()
    buf = np.zeros(1 << 12, dtype=np.float64)
    ws, stats = buf.ctypes.data, buf.ctypes.data + 2048
    sizes = [3, 1025]
    t = _table(sizes, ptr=ws)
    need = lib.mkgnn_adamw_clip_workspace_bytes(t, 2)
    g = (_lib.AdamWGroup * 5)()
    for e in g:
        e.lr_device, e.lr, e.beta1, e.beta2, e.eps, e.weight_decay, e.maximize, e.grad_scale = None, 1e-3, 0.9, 0.999, 1e-8, 0.0, 0, 1.0
    ok = dict(t=t, n=2, ng=1, m=1.0, ws=ws, wb=need, stats=stats)
    bad = [dict(m=0.0), dict(m=-1.0), dict(m=math.nan), dict(m=-math.inf), dict(ws=None), dict(wb=need - 1), dict(wb=0), dict(ws=ws + 4),
           dict(stats=None), dict(ng=5), dict(ng=0), dict(n=-1), dict(t=_table([3, 0], ptr=ws)), dict(t=None)]
    for change in bad:
        a = dict(ok, **change)
        rc = lib.mkgnn_adamw_step_clipped(a["t"], a["n"], g, a["ng"], a["m"], 1, a["ws"], a["wb"], a["stats"], None)
        assert rc != 0 and b"mkgnn_adamw_step_clipped" in lib.mkgnn_last_error(), change
    assert not buf.any()
    # an empty table is a no-op that needs no workspace
    assert lib.mkgnn_adamw_step_clipped(None, 0, g, 1, math.inf, 0, None, 0, stats, None) == 0


def test_fused_adamw_argument_errors():
    from molkgnn_amd.optim import FusedAdamW
    p = [torch.nn.Parameter(torch.zeros(3))]
    for bad in (0.0, -1.0, math.nan, -math.inf):
        with pytest.raises(ValueError, match="max_grad_norm"):
            FusedAdamW(p, max_grad_norm=bad)
    opt = FusedAdamW(p, max_grad_norm=2.5, skip_nonfinite=True)
    assert opt.max_grad_norm == 2.5 and opt.skip_nonfinite is True and opt.clipping
    # attributes of the optimiser, not of its groups: state_dict keeps its shape
    assert all("max_grad_norm" not in g and "skip_nonfinite" not in g for g in opt.param_groups)
    assert "max_grad_norm" not in opt.defaults and "skip_nonfinite" not in opt.defaults
    plain = FusedAdamW(p)
    assert plain.max_grad_norm is None and plain.skip_nonfinite is False and not plain.clipping
    assert set(opt.state_dict()["param_groups"][0]) == set(plain.state_dict()["param_groups"][0])
    assert FusedAdamW(p, skip_nonfinite=True).max_grad_norm is None
    assert FusedAdamW(p, max_grad_norm=math.inf).max_grad_norm == math.inf
    with pytest.raises(RuntimeError):
        plain.grad_norm


def test_configure_optimizer_refuses_clipping_on_the_torch_route():
    from molkgnn_amd.optim import FusedAdamW
    from molkgnn_amd.train import configure_optimizer
    model = torch.nn.Linear(3, 2)
    for kw in (dict(max_grad_norm=1.0), dict(skip_nonfinite=True)):
        with pytest.raises(ValueError, match="clip_grad_norm_"):
            configure_optimizer(model, fused=False, **kw)
    assert isinstance(configure_optimizer(model, fused=False), torch.optim.AdamW)
    with pytest.raises(ValueError, match="max_grad_norm"):
        configure_optimizer(model, fused=True, max_grad_norm=0.0)
    assert FusedAdamW.__init__.__doc__ and ".grad" in FusedAdamW.__init__.__doc__


# ------------------------------------------------------------------------------------- the reference, pinned to torch --
def _clip_in_f64(row, group_of, groups, max_norm):
    """``clip_grad_norm_(foreach=False)`` in float64 on the float32 ``gg`` of every tensor: (norm, the clipped gradients)."""
    ps = []
    for g, gi in zip(row, group_of):
        p = torch.nn.Parameter(torch.zeros(g.numel(), dtype=torch.float64))
        p.grad = K.scaled_fp32(g, groups[gi]).double()
        ps.append(p)
    norm = torch.nn.utils.clip_grad_norm_(ps, max_norm, foreach=False)
    return float(norm), [p.grad for p in ps]


@pytest.mark.parametrize("max_norm", [1e-3, 1.0, 1e3, 1e4, 1e9, math.inf])
def test_norm_and_coefficient_are_clip_grad_norm(max_norm):
    sizes = A.table_sizes(161)
    group_of = [i % 4 for i in range(161)]
    L = A.launched(A.FOUR_GROUPS)
    m = A.fp32(max_norm)
    clipped_some = False
    for row in A.make_grads(sizes, 6, 11):
        norm, coef = K.norm_and_coef(row, group_of, L, m)
        t_norm, t_grads = _clip_in_f64(row, group_of, L, m)
        assert abs(norm - t_norm) <= 1e-12 * t_norm
        want = min(1.0, m / (t_norm + 1e-6))
        assert coef == A.fp32(want) or abs(coef - want) <= 2.0 ** -23 * want
        clipped_some |= coef < 1.0
        for g, gi, tg in zip(row, group_of, t_grads):             # the clipped gradient itself, to the float32 rounding of coef
            mine = K.scaled_fp32(g, L[gi]).double() * coef
            assert float((mine - tg).abs().max()) <= 2.0 ** -23 * float(tg.abs().max()) + 1e-300
    assert clipped_some == (max_norm <= 1e4)


def test_stepped_tensors_alone_enter_the_norm():
    sizes = [3, 1025, 2, 5]
    row = A.make_grads(sizes, 1, 5)[0]
    G = [A.as_launched(A.group(grad_scale=0.5, maximize=True))]
    full, _ = K.norm_and_coef(row, [0] * 4, G, 1.0)
    off = list(row)
    off[1] = None
    flagged, _ = K.norm_and_coef(row, [0] * 4, G, 1.0, active_row=[1.0, 0.0, 1.0, 1.0])
    none, _ = K.norm_and_coef(off, [0] * 4, G, 1.0)
    want = math.sqrt(sum(float((0.5 * g.double()).square().sum()) for i, g in enumerate(row) if i != 1))
    assert flagged == none and abs(none - want) <= 1e-12 * want and full > none
    row[1][7] = math.inf                                           # a gradient that is not stepped cannot trip the guard
    assert math.isfinite(K.norm_and_coef(row, [0] * 4, G, 1.0, active_row=[1.0, 0.0, 1.0, 1.0])[0])


@pytest.mark.parametrize("bad", [math.inf, -math.inf, math.nan])
def test_non_finite_rules_are_torchs(bad):
    """Guard off: an ``inf`` in one element gives NaN there and exact zeros elsewhere; a NaN gives NaN everywhere."""
    sizes = [3, 1025, 2, 5, 1]
    G = [A.as_launched(A.group())]
    row = A.make_grads(sizes, 1, 7)[0]
    row[1][100] = bad
    norm, coef = K.norm_and_coef(row, [0] * 5, G, A.fp32(10.0))
    t_norm, t_grads = _clip_in_f64(row, [0] * 5, G, A.fp32(10.0))
    assert (math.isnan(norm) and math.isnan(t_norm)) or norm == t_norm == math.inf
    mine = K.clipped_row(row, coef)
    for i, (a, b) in enumerate(zip(mine, t_grads)):
        assert torch.equal(torch.isnan(a), torch.isnan(b)), i
        assert torch.equal(a[~torch.isnan(a)], b[~torch.isnan(b)]), i
    if math.isinf(bad):
        assert coef == 0.0
        nan_at = torch.cat([torch.isnan(a) for a in mine]).nonzero().flatten().tolist()
        assert nan_at == [3 + 100] and all(float(a[~torch.isnan(a)].abs().sum()) == 0.0 for a in mine)
    else:
        assert math.isnan(coef) and all(bool(torch.isnan(a).all()) for a in mine)
    # ... and max_norm = inf with a non-finite norm is torch's inf / inf as well
    assert math.isnan(K.norm_and_coef(row, [0] * 5, G, math.inf)[1])
    assert all(bool(torch.isnan(g).all()) for g in _clip_in_f64(row, [0] * 5, G, math.inf)[1])


def test_skip_rule():
    """A skipped step leaves parameters, moments and counts as they were and is counted; the next finite step continues from the old
    counts -- the trajectory equals the one that never saw the bad step."""
    sizes = [3, 1025, 2]
    G = [A.as_launched(A.group(lr=2e-3))]
    params0, grads = A.make_params(sizes, 3), A.make_grads(sizes, 3, 4)
    poisoned = [[g.clone() for g in row] for row in grads]
    poisoned[1][2][1] = math.nan
    ps, sts, stats = K.run_f64(params0, [0] * 3, G, poisoned, 1.0, skip_nonfinite=True)
    qs, rts, _ = K.run_f64(params0, [0] * 3, G, [grads[0], grads[2]], 1.0, skip_nonfinite=True)
    assert [s[2] for s in stats] == [0, 1, 1] and math.isnan(stats[1][0])
    assert all(torch.equal(p, q) for p, q in zip(ps, qs)) and [s.step for s in sts] == [2, 2, 2] == [s.step for s in rts]
    assert all(torch.equal(a.exp_avg, b.exp_avg) and torch.equal(a.exp_avg_sq, b.exp_avg_sq) for a, b in zip(sts, rts))
    assert K.is_skipped(math.inf, True) and K.is_skipped(math.nan, True) and not K.is_skipped(math.inf, False) and not K.is_skipped(1e300, True)
    # guard off: the same inputs poison every parameter, as torch's pair does
    ps, _, _ = K.run_f64(params0, [0] * 3, G, poisoned, 1.0)
    ts, _, _ = K.run_torch(params0, [0] * 3, G, poisoned, 1.0)
    assert all(torch.equal(torch.isnan(p), torch.isnan(t)) and bool(torch.isnan(p).all()) for p, t in zip(ps, ts))


def test_yardstick_equals_reference_in_float64():
    """``run_torch`` in float64 and ``run_f64`` are the same trajectory to rounding: the yardstick is the reference's arithmetic."""
    sizes = A.table_sizes(5)
    group_of = [0, 0, 1, 2, 3]
    L = A.launched(A.FOUR_GROUPS)
    params0, grads = A.make_params(sizes, 8), A.make_grads(sizes, 4, 9)
    m = A.fp32(1e-2)
    ps, sts, stats = K.run_f64(params0, group_of, L, grads, m)
    ts, tts, norms = K.run_torch(params0, group_of, L, grads, m, dtype=torch.float64)
    # (the reference rounds every gg to float32 as the launch does, the float64 yardstick does not: 2^-24 per element)
    assert all(abs(a[0] - b) <= 2.0 ** -23 * b for a, b in zip(stats, norms)) and any(s[1] < 1.0 for s in stats)
    for p, t, a, b in zip(ps, ts, sts, tts):
        assert float((p - t).abs().max()) <= 1e-6 * max(float(p.abs().max()), 1e-3)
        assert float((a.exp_avg - b.exp_avg).abs().max()) <= 1e-6 * max(float(b.exp_avg.abs().max()), 1e-30) and a.step == b.step


def test_ulps_apart():
    one = 1.0
    nxt = float(torch.nextafter(torch.tensor(1.0), torch.tensor(2.0)))
    assert K.ulps_apart(one, one) == 0 and K.ulps_apart(one, nxt) == 1 and K.ulps_apart(nxt, one) == 1
    assert K.ulps_apart(math.nan, math.nan) == 0 and K.ulps_apart(math.nan, 1.0) > 1 and K.ulps_apart(-1e-45, 1e-45) == 2
