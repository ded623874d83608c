"""The average of the weights kept inside the fused AdamW step, everything that needs no GPU: the C ABI's declarations and exports,
the host-only size of the average, the argument errors of ``mkgnn_adamw_step_averaged`` and ``mkgnn_flat_swap`` (raised before
any launch), of ``FusedAdamW`` and of ``configure_optimizer``, and the reference module ``tests/_avg_f64.py`` pinned to
``torch.optim.swa_utils.AveragedModel`` run in float64."""
import ctypes
import math
import os
import re

import pytest
import torch
from torch.optim.swa_utils import AveragedModel, get_ema_multi_avg_fn

from tests import _adamw_f64 as A
from tests import _avg_f64 as V

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("mkgnn_adamw_average_floats", "mkgnn_adamw_step_averaged", "mkgnn_flat_swap")


def test_header_declares_the_entries_and_abi_stays_8():
    text = open(os.path.join(REPO, "include", "molkgnn_hip.h")).read()
    assert re.search(r"\bint64_t mkgnn_adamw_average_floats\(int64_t numel\);", text)
    assert re.search(r"typedef struct \{ int32_t mode; float decay; int32_t warmup; int32_t start; \} mkgnn_adamw_average;", text)
    assert re.search(r"#define MKGNN_ADAMW_AVERAGE_EMA 0\b", text) and re.search(r"#define MKGNN_ADAMW_AVERAGE_MEAN 1\b", text)
    assert re.search(r"\bint mkgnn_adamw_step_averaged\(const mkgnn_adamw_tensor\* tensors, int32_t n_tensors, const mkgnn_adamw_group\* "
                     r"groups,\s+int32_t n_groups, const mkgnn_adamw_average\* avg, float max_norm, int32_t skip_nonfinite,\s+"
                     r"void\* workspace, size_t workspace_bytes, float\* stats, void\* stream\);", text)
    assert re.search(r"typedef struct mkgnn_swap_item \{ float\* a; float\* b; int64_t numel; \} mkgnn_swap_item;", text)
    assert re.search(r"\bint mkgnn_flat_swap\(const mkgnn_swap_item\* items, int32_t n_items, void\* stream\);", text)
    assert "overlap" in text[text.index("typedef struct mkgnn_swap_item") - 700:text.index("typedef struct mkgnn_swap_item")]
    assert re.search(r"#define MKGNN_ABI_VERSION 8\b", text)


def test_lib_types_the_entries_and_lists_them():
    from molkgnn_amd import _lib
    assert _lib.ABI_VERSION == 8
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRIES:
        assert name in _lib.EXPORTS and hasattr(raw, name), name
    lib = _lib.load()
    assert lib.mkgnn_abi_version() == 8
    assert lib.mkgnn_adamw_average_floats.restype is ctypes.c_int64 and len(lib.mkgnn_adamw_average_floats.argtypes) == 1
    assert lib.mkgnn_adamw_step_averaged.restype is ctypes.c_int and len(lib.mkgnn_adamw_step_averaged.argtypes) == 11
    assert lib.mkgnn_adamw_step_averaged.argtypes[5] is ctypes.c_float and lib.mkgnn_adamw_step_averaged.argtypes[8] is ctypes.c_size_t
    assert lib.mkgnn_flat_swap.restype is ctypes.c_int and len(lib.mkgnn_flat_swap.argtypes) == 3
    assert ctypes.sizeof(_lib.AdamWAverage) == 16 and ctypes.sizeof(_lib.SwapItem) == 24
    assert [f[0] for f in _lib.AdamWAverage._fields_] == ["mode", "decay", "warmup", "start"]
    assert (_lib.ADAMW_AVERAGE_EMA, _lib.ADAMW_AVERAGE_MEAN) == (0, 1)
    # the existing structs are as they were
    assert ctypes.sizeof(_lib.AdamWTensor) == 48 and ctypes.sizeof(_lib.AdamWGroup) == 40


def test_average_floats():
    from molkgnn_amd import _lib
    lib = _lib.load()
    want = {0: 0, -3: 0, 1: 3, 1024: 1026, 1025: 1028}
    for n, w in want.items():
        assert lib.mkgnn_adamw_average_floats(n) == w == V.average_floats(n), n
    from molkgnn_amd.optim import FusedAdamW
    assert all(FusedAdamW._average_floats(n) == w for n, w in want.items() if n > 0)


def _table(sizes, ptr=64):
    from molkgnn_amd import _lib
    t = (_lib.AdamWTensor * max(len(sizes), 1))()
    for e, n in zip(t, sizes):
        e.param, e.grad, e.state, e.numel, e.group, e.active = ptr, ptr, ptr, n, 0, None
    return t


def _groups(k=5):
    from molkgnn_amd import _lib
    g = (_lib.AdamWGroup * k)()
    for e in g:
        e.lr_device, e.lr, e.beta1, e.beta2, e.eps, e.weight_decay, e.maximize, e.grad_scale = None, 1e-3, 0.9, 0.999, 1e-8, 0.0, 0, 1.0
    return g


def test_averaged_entry_refuses_bad_arguments_before_any_launch():
    """Every check comes before a launch, so host memory stands in for the device's: the average's settings in both forms of the
    entry, what the unclipped entry refuses in the unclipped form, and the clipped entry's own checks in the clipped form."""
    import numpy as np
    from molkgnn_amd import _lib
    lib = _lib.load()
    buf = np.zeros(1 << 12, dtype=np.float64)
    ws, stats = buf.ctypes.data, buf.ctypes.data + 2048
    t = _table([3, 1025], ptr=ws)
    need = lib.mkgnn_adamw_clip_workspace_bytes(t, 2)
    g = _groups()

    def avg(mode=0, decay=0.9, warmup=0, start=0):
        return _lib.AdamWAverage(mode, decay, warmup, start)

    def call(a):
        return lib.mkgnn_adamw_step_averaged(a["t"], a["n"], g, a["ng"], a["avg"], a["m"], a["skip"], a["ws"], a["wb"], a["stats"], None)

    settings = [dict(avg=None), dict(avg=avg(mode=2)), dict(avg=avg(mode=-1)), dict(avg=avg(decay=1.0)), dict(avg=avg(decay=-0.1)),
                dict(avg=avg(decay=math.nan)), dict(avg=avg(decay=math.inf)), dict(avg=avg(start=-1))]
    unclipped = dict(t=t, n=2, ng=1, avg=avg(), m=math.inf, skip=0, ws=None, wb=0, stats=None)
    clipped = dict(t=t, n=2, ng=1, avg=avg(mode=1), m=1.0, skip=1, ws=ws, wb=need, stats=stats)
    bad_unclipped = settings + [dict(ng=5), dict(ng=0), dict(n=-1), dict(t=_table([3, 0], ptr=ws)), dict(t=None),
                                dict(t=_table([3] * 80 + [0], ptr=ws), n=81)]      # (a bad tensor of the second launch)
    bad_clipped = settings + [dict(m=0.0), dict(m=-1.0), dict(m=math.nan), dict(m=-math.inf), dict(ws=None), dict(wb=need - 1), dict(wb=0),
                              dict(ws=ws + 4), dict(stats=None), dict(ng=5), dict(ng=0), dict(n=-1), dict(t=_table([3, 0], ptr=ws)),
                              dict(t=None),
                              # not the unclipped form, so the clipped entry's needs hold: the guard alone, stats alone
                              dict(m=math.inf, skip=1, stats=None), dict(m=math.inf, skip=0, ws=None, wb=0)]
    for ok, bad in ((unclipped, bad_unclipped), (clipped, bad_clipped)):
        for change in bad:
            assert call(dict(ok, **change)) != 0 and b"mkgnn_adamw_step_averaged" in lib.mkgnn_last_error(), change
    assert not buf.any()
    # an empty table is a no-op in both forms
    assert call(dict(unclipped, t=None, n=0)) == 0 and call(dict(clipped, t=None, n=0, ws=None, wb=0)) == 0


def test_flat_swap_refuses_bad_arguments_before_any_launch():
    import numpy as np
    from molkgnn_amd import _lib
    lib = _lib.load()
    buf = np.arange(64, dtype=np.float32)
    a, b = buf.ctypes.data, buf.ctypes.data + 128

    def items(rows):
        t = (_lib.SwapItem * len(rows))()
        for e, r in zip(t, rows):
            e.a, e.b, e.numel = r
        return t
    good = (a, b, 8)
    for rows in ([(None, b, 8)], [(a, None, 8)], [(a, b, 0)], [(a, b, -1)], [(a, b, (1 << 30) + 1)], [good, (a, None, 8)],
                 [good] * 120 + [(a, b, 0)]):                  # (the bad item of a second launch is found before the first one)
        assert lib.mkgnn_flat_swap(items(rows), len(rows), None) != 0 and b"mkgnn_flat_swap" in lib.mkgnn_last_error(), rows[-1]
    assert lib.mkgnn_flat_swap(items([good]), -1, None) != 0 and b"mkgnn_flat_swap" in lib.mkgnn_last_error()
    assert lib.mkgnn_flat_swap(None, 1, None) != 0 and b"mkgnn_flat_swap" in lib.mkgnn_last_error()
    assert lib.mkgnn_flat_swap(None, 0, None) == 0
    assert buf.tolist() == list(range(64))


def test_fused_adamw_argument_errors():
    from molkgnn_amd.optim import FusedAdamW
    p = [torch.nn.Parameter(torch.zeros(3))]
    for bad in ("swa", "EMA", True, 1):
        with pytest.raises(ValueError, match="average"):
            FusedAdamW(p, average=bad)
    for bad in (1.0, -0.1, math.nan, math.inf):
        with pytest.raises(ValueError, match="average_decay"):
            FusedAdamW(p, average="ema", average_decay=bad)
    for bad in (-1, 0.5):
        with pytest.raises(ValueError, match="average_start"):
            FusedAdamW(p, average="mean", average_start=bad)
    opt = FusedAdamW(p, average="ema", average_decay=0.9, average_warmup=False, average_start=3)
    assert (opt.average, opt.average_decay, opt.average_warmup, opt.average_start) == ("ema", 0.9, False, 3)
    plain = FusedAdamW(p)
    assert plain.average is None and (plain.average_decay, plain.average_warmup, plain.average_start) == (0.999, True, 0)
    # settings of the optimiser, not of its groups: state_dict keeps its shape
    assert set(opt.state_dict()["param_groups"][0]) == set(plain.state_dict()["param_groups"][0])
    assert all(not k.startswith("average") for k in opt.defaults)
    assert plain._packed_floats(1025) == A.state_floats(1025) and opt._packed_floats(1025) == A.state_floats(1025) + V.average_floats(1025)
    for call in (plain.averaged_parameters, plain.swap_averaged):
        with pytest.raises(RuntimeError, match="average"):
            call()
    with pytest.raises(RuntimeError, match="average"):
        with plain.averaged_weights():
            pass
    assert opt.averaged_parameters() == {}                    # no state yet
    opt.swap_averaged()                                       # nothing to exchange: no launch, no GPU asked for


def test_configure_optimizer_refuses_averaging_on_the_torch_route():
    from molkgnn_amd import train
    model = torch.nn.Linear(3, 2)
    with pytest.raises(ValueError, match="AveragedModel"):
        train.configure_optimizer(model, fused=False, average="ema")
    assert isinstance(train.configure_optimizer(model, fused=False), torch.optim.AdamW)
    with pytest.raises(ValueError, match="average"):
        train.configure_optimizer(model, fused=True, average="polyak")
    with pytest.raises(ValueError, match="average_decay"):
        train.configure_optimizer(model, fused=True, average="ema", average_decay=1.0)
    plain = train.configure_optimizer(model, fused=False)
    with pytest.raises(ValueError, match="keeps no average"):
        with train.averaged_weights(model, plain):
            pass
    with pytest.raises(ValueError, match="keeps no average"):
        train.averaged_state_dict(model, plain)


# ------------------------------------------------------------------------------------- the reference, pinned to torch --
class _Three(torch.nn.Module):
    def __init__(self, params):
        super().__init__()
        self.ps = torch.nn.ParameterList([torch.nn.Parameter(p.clone()) for p in params])


def _walk(steps, seed):
    """A random walk of three tensors in float64: ``[step][tensor]``, and its start."""
    g = torch.Generator().manual_seed(seed)
    sizes = (1, 5, 1025)
    p = [torch.randn(n, generator=g, dtype=torch.float64) for n in sizes]
    start, out = [q.clone() for q in p], []
    for _ in range(steps):
        p = [q + 1e-2 * torch.randn(q.numel(), generator=g, dtype=torch.float64) for q in p]
        out.append([q.clone() for q in p])
    return start, out


AVERAGED_MODEL_MEASURED = {"ema": 2.220446049250313e-16, "mean": 4.440892098500626e-16}


@pytest.mark.parametrize("mode", ["ema", "mean"])
def test_float64_leg_is_averaged_model(mode):
    """300 updates of three tensors, ``start = 0``, EMA without warmup at ``decay = fl32(0.999)`` and the mean, against
    ``AveragedModel`` (``get_ema_multi_avg_fn`` / its default running mean) on float64 CPU tensors.  Largest absolute difference
    measured on the CPU (values of order 1): ema 2.22e-16, mean 4.44e-16 -- ``AVERAGED_MODEL_MEASURED``; asserted: 8 times that, ema
    1.78e-15, mean 3.55e-15.  (torch's lerp and its ``(p - avg) / (n + 1)`` round differently from ``avg + w (p - avg)`` in the last
    bit.)"""
    decay = A.fp32(0.999)
    start, walk = _walk(300, seed=31)
    model = _Three(start)
    kw = dict(multi_avg_fn=get_ema_multi_avg_fn(decay)) if mode == "ema" else {}
    swa = AveragedModel(model, **kw)
    for row in walk:
        with torch.no_grad():
            for p, q in zip(model.ps, row):
                p.copy_(q)
        swa.update_parameters(model)
    counts = [[s + 1] * 3 for s in range(300)]
    avgs, ns, _ = V.run(start, walk, counts, mode, decay, warmup=False, start=0, dtype=torch.float64)
    assert ns == [300] * 3 == [int(swa.n_averaged)] * 3
    worst = max(float((a - b.detach()).abs().max()) for a, b in zip(avgs, swa.module.ps))
    print("float64 leg against AveragedModel", mode, worst)
    assert worst <= 8.0 * AVERAGED_MODEL_MEASURED[mode], (mode, worst)
    # ... and the leg averages: it is not the last iterate
    assert all(float((a - q).abs().max()) > 1e-3 for a, q in zip(avgs, walk[-1]))


def test_warmup_formula_at_hand_values():
    d = A.fp32(0.999)
    assert V.decay_at(d, True, 1) == 2.0 / 11.0
    assert V.decay_at(d, True, 90) == 0.91
    assert V.decay_at(0.999, True, 8989) < 0.999 and V.decay_at(0.999, True, 8990) == 0.999 == V.decay_at(0.999, True, 10 ** 6)
    assert V.decay_at(d, True, 8990) == 0.999 and V.decay_at(d, True, 8991) == d      # (fl32(0.999) lies just above 0.999)
    assert V.decay_at(d, False, 1) == d
    assert V.weight("ema", d, True, 1) == A.fp32(9.0 / 11.0) and V.weight("ema", d, False, 7) == A.fp32(1.0 - d)
    assert V.weight("mean", d, True, 1) == 0.5 and V.weight("mean", d, False, 2) == A.fp32(1.0 / 3.0)
    assert V.weight("mean", d, False, 2, rounded=False) == 1.0 / 3.0


def test_w_of_one_copies_and_the_three_cases():
    """``decay = 0``: ``w = 1`` and the average is the parameter in bits, where ``avg + 1 * (p - avg)`` is not; before ``start`` the
    count stays 0; the first update counts 1; an untaken step changes nothing."""
    g = torch.Generator().manual_seed(5)
    avg = torch.randn(4096, generator=g) * 1e3
    p = torch.randn(4096, generator=g) * 1e-3
    assert not torch.equal(avg + 1.0 * (p - avg), p)           # the formula alone would not copy
    out, n = V.update(avg, 4, p, 9, "ema", 0.0)
    assert n == 5 and torch.equal(out.view(torch.int32), p.view(torch.int32)) and out.data_ptr() != p.data_ptr()
    out, n = V.update(avg, 0, p, 3, "mean", 0.5, start=3)
    assert n == 0 and torch.equal(out, p)
    out, n = V.update(avg, 0, p, 4, "mean", 0.5, start=3)
    assert n == 1 and torch.equal(out, p)
    out, n = V.update(avg, 1, p, 5, "mean", 0.5, start=3)
    assert n == 2 and torch.equal(out, avg + (p - avg) * torch.tensor(0.5))
    # a trajectory whose tensor 1 is not stepped at step 1: its average and count stand still
    snaps = [[p, p], [avg, avg], [p, p]]
    avgs, ns, hist = V.run([avg, avg], snaps, [[1, 1], [2, 1], [3, 2]], "ema", A.fp32(0.9))
    assert ns == [3, 2] and torch.equal(hist[0][0][1], hist[1][0][1]) and hist[1][1] == [2, 1]
    assert not torch.equal(avgs[0], avgs[1])
