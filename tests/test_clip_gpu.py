"""``mkgnn_adamw_step_clipped`` (csrc/kgnn_optim.hip): gradient clipping by global norm and the non-finite guard inside the fused
AdamW step, against float64 (``tests/_clip_f64.py``) and the float32 pair ``clip_grad_norm_(foreach=False)`` +
``torch.optim.AdamW(foreach=False, fused=False)``.  Driven through ``optim.FusedAdamW`` and, where the table's order or its
surroundings matter, through the C ABI with guard sentinels around every buffer.  ``pytest -m gpu``.

Parameters and moments are held with ``_adamw_f64.check`` and its constants as they stand, step counts exactly, ``stats[0]`` and
``stats[1]`` within one float32 ulp of the reference's norm and coefficient (the double sum's order may differ in the last bit).
"""
import copy
import math
import os
import re

import pytest
import torch

from tests import _adamw_f64 as A
from tests import _clip_f64 as K

pytestmark = pytest.mark.gpu

GUARD = 1024
SENTINEL = 1234567.0
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dev():
    assert torch.cuda.is_available(), "pytest -m gpu needs the MI355X"
    return torch.device("cuda:0")


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _cap():
    text = open(os.path.join(REPO, "include", "molkgnn_hip.h")).read()
    return int(re.search(r"#define MKGNN_ADAMW_CLIP_PROLOGUE_BLOCKS (\d+)\b", text).group(1))


def _hold(tag, params, states, f32, f64, names=None):
    """The build's parameters and moments to the bound; its step counts to the reference's, exactly."""
    n = A.check(A.quantities(params, states), A.quantities(*f32[:2]), A.quantities(*f64[:2]), tag, names)
    assert [st.step for st in states] == [st.step for st in f64[1]], tag
    return n


def _stats_hold(tag, got, want):
    """``got``: (norm, coef, skipped) read from the device; ``want``: the reference's."""
    assert K.ulps_apart(got[0], want[0]) <= 1, (tag, "norm", got[0], want[0])
    assert K.ulps_apart(got[1], want[1]) <= 1, (tag, "coef", got[1], want[1])
    assert got[2] == float(want[2]), (tag, "skipped", got[2], want[2])


# ------------------------------------------------------------------------------------------ the two drivers --
class _Direct:
    """A tensor table handed to ``mkgnn_adamw_step_clipped`` (or ``mkgnn_adamw_step``) as it stands: param, grad and packed state of
    every tensor cut out of three larger buffers, the workspace and the stats out of two more, ``GUARD`` sentinels on each side of
    each (the pattern of ``test_adamw_f64.py``)."""

    def __init__(self, dev, params0, group_of):
        from molkgnn_amd import _lib
        self.lib, self.dev, self.group_of = _lib.load(), dev, list(group_of)
        self.sizes = [p.numel() for p in params0]
        self.slens = [A.state_floats(n) for n in self.sizes]

        def layout(lens):
            offs, o = [], 0
            for L in lens:
                offs.append(o + GUARD)
                o += GUARD + L + GUARD
            guard = torch.ones(o, dtype=torch.bool)
            for off, L in zip(offs, lens):
                guard[off:off + L] = False
            return offs, o, guard.to(dev)
        self.poff, total, self.pguard = layout(self.sizes)
        self.soff, stotal, self.sguard = layout(self.slens)
        self.P = torch.full((total,), SENTINEL, device=dev)
        self.G = torch.full((total,), SENTINEL, device=dev)
        self.S = torch.full((stotal,), SENTINEL, device=dev)
        for p, off, n, so, sl in zip(params0, self.poff, self.sizes, self.soff, self.slens):
            self.P[off:off + n] = p.to(dev)
            self.S[so:so + sl] = 0.0
        self.table = (_lib.AdamWTensor * len(self.sizes))()
        for e, off, so, n, gi in zip(self.table, self.poff, self.soff, self.sizes, self.group_of):
            e.param, e.grad, e.state = self.P.data_ptr() + 4 * off, self.G.data_ptr() + 4 * off, self.S.data_ptr() + 4 * so
            e.numel, e.group, e.active = n, gi, None
        self._G_host = torch.full((total,), SENTINEL)
        self.ws_bytes = int(self.lib.mkgnn_adamw_clip_workspace_bytes(self.table, len(self.sizes)))
        assert self.ws_bytes % 8 == 0 and self.ws_bytes >= 8 * sum((n + A.CHUNK - 1) // A.CHUNK for n in self.sizes)
        self.W = torch.full((GUARD + self.ws_bytes // 8 + GUARD,), SENTINEL, dtype=torch.float64, device=dev)
        self.stats = torch.full((GUARD + 4 + GUARD,), SENTINEL, device=dev)
        self.stats[GUARD:GUARD + 4] = 0.0
        torch.cuda.synchronize()

    def _groups(self, groups):
        from molkgnn_amd import _lib
        arr = (_lib.AdamWGroup * len(groups))()
        for e, G in zip(arr, groups):
            e.lr_device, e.lr = None, G["lr"]
            e.beta1, e.beta2, e.eps, e.weight_decay = G["betas"][0], G["betas"][1], G["eps"], G["weight_decay"]
            e.maximize, e.grad_scale = int(G["maximize"]), G["grad_scale"]
        return arr

    def _fill(self, grads):
        for g, off, n in zip(grads, self.poff, self.sizes):
            self._G_host[off:off + n] = g
        self.G.copy_(self._G_host)

    def step(self, groups, grads, max_norm, skip_nonfinite=False):
        from molkgnn_amd import _lib
        self._fill(grads)
        with torch.cuda.device(self.dev):
            rc = self.lib.mkgnn_adamw_step_clipped(self.table, len(self.sizes), self._groups(groups), len(groups), max_norm,
                                                   int(skip_nonfinite), self.W.data_ptr() + 8 * GUARD, self.ws_bytes,
                                                   self.stats.data_ptr() + 4 * GUARD, _lib.stream_ptr(self.dev))
        torch.cuda.synchronize()
        return rc

    def step_unclipped(self, groups, grads):
        from molkgnn_amd import _lib
        self._fill(grads)
        with torch.cuda.device(self.dev):
            rc = self.lib.mkgnn_adamw_step(self.table, len(self.sizes), self._groups(groups), len(groups), _lib.stream_ptr(self.dev))
        torch.cuda.synchronize()
        return rc

    def read_stats(self):
        s = self.stats[GUARD:GUARD + 4].cpu().tolist()
        assert s[3] == 0.0                                    # reserved: not touched
        return s[0], s[1], s[2]

    def read(self):
        """(params, states, per-block counts) on the CPU."""
        P, S = self.P.cpu(), self.S.cpu()
        params, states, blocks = [], [], []
        for off, n, so, sl in zip(self.poff, self.sizes, self.soff, self.slens):
            st = S[so:so + sl]
            params.append(P[off:off + n].clone())
            states.append(A.State((n,), st[:n], st[n:2 * n], int(st[2 * n])))
            blocks.append(st[2 * n + 3:].tolist())
        return params, states, blocks

    def guards_intact(self):
        """The sentinels around every param, grad and state slot, around the workspace and the stats; the two reserved floats of
        every state (zero as handed over); the gradient buffer as it was filled."""
        want = _bits(torch.tensor([SENTINEL]))[0].item()
        S = self.S.cpu()
        reserved = all(S[so + 2 * n + 1:so + 2 * n + 3].tolist() == [0.0, 0.0] for so, n in zip(self.soff, self.sizes))
        tables = all(bool((_bits(buf)[mask] == want).all())
                     for buf, mask in ((self.P, self.pguard), (self.G, self.pguard), (self.S, self.sguard)))
        W, st = self.W.cpu(), self.stats.cpu()
        around = bool((W[:GUARD] == SENTINEL).all()) and bool((W[-GUARD:] == SENTINEL).all()) and \
            bool((st[:GUARD] == SENTINEL).all()) and bool((st[-GUARD:] == SENTINEL).all())
        grads = torch.equal(_bits(self.G.cpu()), _bits(self._G_host))
        return reserved and tables and around and grads


def _fused(dev, params0, group_of, groups0, **clip):
    """``FusedAdamW`` over device copies of ``params0``; the table's order is group by group, so ``group_of`` must not decrease."""
    from molkgnn_amd.optim import FusedAdamW
    assert list(group_of) == sorted(group_of)
    ps = [torch.nn.Parameter(p.to(dev)) for p in params0]
    pgs = [dict(params=[p for p, gi in zip(ps, group_of) if gi == k], lr=G["lr"], betas=G["betas"], eps=G["eps"],
                weight_decay=G["weight_decay"], maximize=G["maximize"], grad_scale=G["grad_scale"]) for k, G in enumerate(groups0)]
    return ps, FusedAdamW(pgs, **clip)


def _read_fused(ps, opt):
    torch.cuda.synchronize()
    params, states, blocks = [], [], []
    for p in ps:
        n, buf = p.numel(), opt.state[p]["_packed"].cpu()
        assert buf.numel() == A.state_floats(n)
        params.append(p.detach().cpu().reshape(-1))
        states.append(A.State((n,), buf[:n], buf[n:2 * n], int(buf[2 * n])))
        blocks.append(buf[2 * n + 3:].tolist())
    return params, states, blocks


def _fused_stats(opt):
    torch.cuda.synchronize()
    return float(opt.grad_norm), float(opt.clip_coef), float(opt.skipped_steps)


def _blocks_agree(states, blocks, sizes, tag):
    for i, (st, b, n) in enumerate(zip(states, blocks, sizes)):
        assert len(b) == (n + A.CHUNK - 1) // A.CHUNK and all(c == float(st.step) for c in b), (tag, i, n, st.step, b)


# ------------------------------------------------------------------------------- 1: three launches, one norm --
MAX_NORM_1 = 1e4


@pytest.fixture(scope="module")
def table161():
    """161 tensors over three launches, four groups interleaved (``maximize`` and four different ``grad_scale`` enter the norm), six
    steps of gradients, and both CPU legs at ``max_norm = 1e4`` -- computed once, shared, not modified."""
    sizes = A.table_sizes(161)
    group_of = [i % 4 for i in range(161)]
    L = A.launched(A.FOUR_GROUPS)
    params0, grads = A.make_params(sizes, seed=6), A.make_grads(sizes, 6, 11)
    m = A.fp32(MAX_NORM_1)
    f64 = K.run_f64(params0, group_of, L, grads, m, snapshots=True)
    return dict(sizes=sizes, group_of=group_of, L=L, params0=params0, grads=grads, m=m, f64=f64,
                f32=K.run_torch(params0, group_of, L, grads, m),
                f32_two=K.run_torch(params0, group_of, L, grads[:2], m))


def test_three_launches_one_norm(table161):
    """Some of the six steps clip and some do not -- only with the norm of the whole table: the reference's coefficient of every
    step is held to one ulp, and a per-launch norm would clip differently in each third of the table."""
    t = table161
    d = _Direct(_dev(), t["params0"], t["group_of"])
    coefs = [s[1] for s in t["f64"][2]]
    assert any(c < 1.0 for c in coefs) and any(c == 1.0 for c in coefs), coefs
    for s, row in enumerate(t["grads"]):
        assert d.step(t["L"], row, t["m"]) == 0
        _stats_hold(("one norm", s), d.read_stats(), t["f64"][2][s])
    params, states, blocks = d.read()
    assert _hold("three launches, one norm", params, states, t["f32"], t["f64"]) == 3 * 161
    _blocks_agree(states, blocks, t["sizes"], "one norm")
    assert all(st.step == 6 for st in states) and d.guards_intact()


# --------------------------------------------------------------------------------------------- 2: block edges --
@pytest.mark.parametrize("n", A.BLOCK_SIZES)
def test_block_edges_count_no_clamped_lane(n):
    """One tensor of all ones: the norm is ``fl32(sqrt(n))``; a clamped tail load that was counted would show."""
    dev = _dev()
    ps, opt = _fused(dev, [torch.zeros(n)], [0], [A.group()], skip_nonfinite=True)       # max_grad_norm None: +inf
    ps[0].grad = torch.ones(n, device=dev)
    opt.step()
    norm, coef, skipped = _fused_stats(opt)
    assert norm == A.fp32(math.sqrt(n)) and coef == 1.0 and skipped == 0.0, (n, norm, coef, skipped)
    _, states, blocks = _read_fused(ps, opt)
    assert states[0].step == 1
    _blocks_agree(states, blocks, [n], n)


# ---------------------------------------------------------------------- 3: the coefficient is the same everywhere --
def test_one_coefficient_in_every_block_of_every_launch(table161):
    """``beta1 = 0`` and a fresh state: ``exp_avg`` is the clipped gradient itself, ``fl32(gg * stats[1])`` bit for bit in every
    element of every tensor of all three launches."""
    t = table161
    dev = _dev()
    L = [A.as_launched(dict(G, betas=(0.0, G["betas"][1]))) for G in A.FOUR_GROUPS]
    d = _Direct(dev, t["params0"], t["group_of"])
    assert d.step(L, t["grads"][0], A.fp32(1.0)) == 0
    norm, coef, _ = d.read_stats()
    assert 0.0 < coef < 1.0 and K.ulps_apart(coef, K.norm_and_coef(t["grads"][0], t["group_of"], L, A.fp32(1.0))[1]) <= 1
    coef_t = d.stats[GUARD + 1]
    for i, (off, so, n, gi) in enumerate(zip(d.poff, d.soff, d.sizes, d.group_of)):
        g = d.G[off:off + n]
        gg = (-g if L[gi]["maximize"] else g) * torch.tensor(L[gi]["grad_scale"], dtype=torch.float32, device=dev)
        # (+ 0.0: the update forms m + (gg - m) with m = +0, which turns a gradient of -0 into +0 and changes nothing else)
        assert torch.equal(_bits(d.S[so:so + n]), _bits(gg * coef_t + 0.0)), i


# ------------------------------------------------------------------------------------ 4: coef = 1 is the old step --
def test_without_clipping_the_step_is_the_unclipped_one(table161):
    """``max_norm = inf``, guard off: parameters, moments and every step count bit-equal to ``mkgnn_adamw_step`` over three steps."""
    t = table161
    dev = _dev()
    old, new = _Direct(dev, t["params0"], t["group_of"]), _Direct(dev, t["params0"], t["group_of"])
    for s in range(3):
        assert old.step_unclipped(t["L"], t["grads"][s]) == 0
        assert new.step(t["L"], t["grads"][s], math.inf) == 0
        assert new.read_stats()[1:] == (1.0, 0.0)
        assert torch.equal(_bits(old.P), _bits(new.P)) and torch.equal(_bits(old.S), _bits(new.S)), s
    assert new.guards_intact() and all(st.step == 3 for st in new.read()[1])


# -------------------------------------------------------------------------------------------- 5: skips and None --
def test_skipped_tensors_are_outside_the_norm_and_untouched():
    """Device flags on tensor 0 (three blocks: the block that writes the stats is an idle one) and tensor 3, a ``None`` gradient on
    tensor 2; the flagged-off tensor 0 holds an ``inf`` in its gradient buffer, which must not trip the guard."""
    dev = _dev()
    sizes = [2049, 3, 5, 1025, 2, 1]
    T, steps = len(sizes), 3
    group_of, groups = [0] * T, [A.group(lr=2e-3, weight_decay=0.02, grad_scale=0.5)]
    L = A.launched(groups)
    params0, grads = A.make_params(sizes, seed=21), A.make_grads(sizes, steps, seed=22)
    grads = [[g * 1e3 for g in row] for row in grads]
    active = [[1.0] * T for _ in range(steps)]
    active[0][0] = 0.0
    grads[0][0][2048] = math.inf
    active[2][3] = 0.0
    grads[2][2] = None
    m = A.fp32(5.0)
    f64 = K.run_f64(params0, group_of, L, grads, m, skip_nonfinite=True, active=active)
    f32 = K.run_torch(params0, group_of, L, grads, m, skip_nonfinite=True, active=active)
    assert all(math.isfinite(s[0]) for s in f64[2]) and any(s[1] < 1.0 for s in f64[2])
    ps, opt = _fused(dev, params0, group_of, groups, max_grad_norm=5.0, skip_nonfinite=True)
    flags = torch.ones(2, device=dev)
    opt.set_grad_active({ps[0]: flags[0], ps[3]: flags[1]})
    opt.prepare_state()
    for s, row in enumerate(grads):
        flags.copy_(torch.tensor([active[s][0], active[s][3]]))
        for p, g in zip(ps, row):
            p.grad = None if g is None else g.to(dev)
        before = [(p.detach().clone(), opt.state[p]["_packed"].clone()) for p in ps]
        opt.step()
        _stats_hold(("skips", s), _fused_stats(opt), f64[2][s])
        for i in range(T):
            same = torch.equal(_bits(before[i][0]), _bits(ps[i])) and torch.equal(_bits(before[i][1]), _bits(opt.state[ps[i]]["_packed"]))
            assert same == (active[s][i] == 0.0 or row[i] is None), (s, i)
    params, states, blocks = _read_fused(ps, opt)
    assert _hold("skips and None", params, states, f32, f64) == 3 * T
    _blocks_agree(states, blocks, sizes, "skips")
    assert [st.step for st in states] == [2, 3, 2, 2, 3, 3]


# ------------------------------------------------------------------------------------------------------ 6: guard --
def _poison(name, row, group_of):
    row = [g.clone() for g in row]
    if name == "inf_last_of_third_launch":
        row[160][-1] = math.inf
    elif name == "nan_first_of_all":
        row[0][0] = math.nan
    else:
        i = next(i for i, gi in enumerate(group_of) if A.FOUR_GROUPS[gi]["grad_scale"] == 0.1)
        row[i][0] = -math.inf
    return row


@pytest.mark.parametrize("variant", ["inf_last_of_third_launch", "nan_first_of_all", "inf_in_a_group_scaled_by_a_tenth"])
def test_guard_skips_the_whole_step(table161, variant):
    """A finite step, the poisoned one, a finite one: the poisoned step changes no bit of any parameter or packed state (per-block
    counters included), counts one skip, and the trajectory is the one that never saw it."""
    t = table161
    d = _Direct(_dev(), t["params0"], t["group_of"])
    assert d.step(t["L"], t["grads"][0], t["m"], True) == 0
    _stats_hold((variant, 0), d.read_stats(), t["f64"][2][0])
    P0, S0 = d.P.clone(), d.S.clone()
    assert d.step(t["L"], _poison(variant, t["grads"][1], t["group_of"]), t["m"], True) == 0
    norm, coef, skipped = d.read_stats()
    assert not math.isfinite(norm) and skipped == 1.0, (norm, coef, skipped)
    assert torch.equal(_bits(P0), _bits(d.P)) and torch.equal(_bits(S0), _bits(d.S)) and d.guards_intact()
    assert d.step(t["L"], t["grads"][1], t["m"], True) == 0
    want = t["f64"][2][1]
    _stats_hold((variant, 2), d.read_stats(), (want[0], want[1], 1))
    params, states, blocks = d.read()
    assert _hold("guard " + variant, params, states, t["f32_two"], t["f64"][3][1]) == 3 * 161
    _blocks_agree(states, blocks, t["sizes"], variant)
    assert all(st.step == 2 for st in states) and d.guards_intact()


def test_huge_finite_gradients_are_not_skipped():
    """Gradients of 1e30: their float32 squares overflow, the float64 sum does not.  The norm is finite, nothing is skipped, and the
    clipped step goes to the bound (the float32 yardstick here is the float64 trajectory rounded: torch's float32 norm is ``inf``)."""
    dev = _dev()
    sizes = [3, 1025]
    groups = [A.group(lr=2e-3)]
    L = A.launched(groups)
    params0 = A.make_params(sizes, seed=23)
    grads = [[torch.full((n,), 1e30) for n in sizes]]
    f64 = K.run_f64(params0, [0, 0], L, grads, A.fp32(1.0), skip_nonfinite=True)
    assert math.isfinite(f64[2][0][0]) and 0.0 < f64[2][0][1] < 1e-29
    rounded = ([p.float() for p in f64[0]], [A.State(p.shape, st.exp_avg.float(), st.exp_avg_sq.float(), st.step) for p, st in zip(f64[0], f64[1])])
    ps, opt = _fused(dev, params0, [0, 0], groups, max_grad_norm=1.0, skip_nonfinite=True)
    for p, g in zip(ps, grads[0]):
        p.grad = g.to(dev)
    opt.step()
    _stats_hold("huge", _fused_stats(opt), f64[2][0])
    params, states, _ = _read_fused(ps, opt)
    assert _hold("huge", params, states, rounded, f64) == 6 and all(st.step == 1 for st in states)


# ------------------------------------------------------------------------- 7: guard off with a non-finite norm --
@pytest.mark.parametrize("bad", [math.inf, math.nan])
def test_guard_off_follows_torch(bad):
    """An ``inf`` gives ``coef = 0``: NaN in that element's parameter alone; a NaN gives ``coef = NaN``: NaN everywhere -- the NaN
    mask of the CPU pair ``clip_grad_norm_`` + ``torch.optim.AdamW``."""
    dev = _dev()
    sizes = A.table_sizes(5)
    groups = [A.group(lr=2e-3, weight_decay=0.02)]
    L = A.launched(groups)
    params0, grads = A.make_params(sizes, seed=24), A.make_grads(sizes, 1, seed=25)
    grads[0][4][1] = bad
    want, _, _ = K.run_torch(params0, [0] * 5, L, grads, A.fp32(10.0))
    masks = [torch.isnan(p) for p in want]
    assert sum(int(k.sum()) for k in masks) == (1 if math.isinf(bad) else sum(sizes))
    ps, opt = _fused(dev, params0, [0] * 5, groups, max_grad_norm=10.0)
    for p, g in zip(ps, grads[0]):
        p.grad = g.to(dev)
    opt.step()
    norm, coef, skipped = _fused_stats(opt)
    assert skipped == 0.0 and ((norm == math.inf and coef == 0.0) if math.isinf(bad) else (math.isnan(norm) and math.isnan(coef)))
    params, states, _ = _read_fused(ps, opt)
    assert all(torch.equal(torch.isnan(p), k) for p, k in zip(params, masks)) and all(st.step == 1 for st in states)
    if math.isinf(bad):                                        # the other elements took torch's step on a zero gradient
        f64 = K.run_f64(params0, [0] * 5, L, grads, A.fp32(10.0))
        for p, q, k in zip(params, f64[0], masks):
            assert float((p.double() - q)[~k].abs().max()) <= 2.0 ** -22 * max(float(q[~k].abs().max()), 1e-3)


# ---------------------------------------------------------------------------------- 8: beyond the prologue cap --
def test_table_beyond_the_prologue_cap():
    """One tensor of ``cap + 1`` blocks and two small ones: the finishing launch reduces the partials; norm, coefficient and one step."""
    dev = _dev()
    sizes = [(_cap() + 1) * A.CHUNK, 3, 1025]
    groups = [A.group(lr=2e-3, weight_decay=0.02, grad_scale=0.5)]
    L = A.launched(groups)
    params0, grads = A.make_params(sizes, seed=26), A.make_grads(sizes, 1, seed=27)
    grads[0][0] *= 1e6
    m = A.fp32(1.0)
    f64, f32 = K.run_f64(params0, [0] * 3, L, grads, m), K.run_torch(params0, [0] * 3, L, grads, m)
    assert f64[2][0][1] < 1.0
    ps, opt = _fused(dev, params0, [0] * 3, groups, max_grad_norm=1.0, skip_nonfinite=True)
    for p, g in zip(ps, grads[0]):
        p.grad = g.to(dev)
    opt.step()
    _stats_hold("beyond the cap", _fused_stats(opt), f64[2][0])
    params, states, blocks = _read_fused(ps, opt)
    assert _hold("beyond the cap", params, states, f32, f64) == 9
    _blocks_agree(states, blocks, sizes, "beyond the cap")


# ------------------------------------------------------------------------------------------------- 9: captured --
def test_captured_step_clips_and_skips_on_the_device():
    """ONE ``opt.step()`` captured, replayed four times over refilled gradients: below the threshold, above it, non-finite, finite."""
    dev = _dev()
    sizes = A.table_sizes(5)
    group_of = [0, 0, 1, 1, 1]
    groups = A.FOUR_GROUPS[:2]
    L = A.launched(groups)
    params0 = A.make_params(sizes, seed=28)
    base = A.make_grads(sizes, 3, seed=29)
    small = base[0]
    m = A.fp32(10.0 * K.norm_and_coef(small, group_of, L, math.inf)[0])
    big = [g * 100.0 for g in base[1]]
    bad = [g.clone() for g in big]
    bad[1][1] = math.inf
    grads = [small, big, bad, base[2]]
    f64 = K.run_f64(params0, group_of, L, grads, m, skip_nonfinite=True)
    f32 = K.run_torch(params0, group_of, L, grads, m, skip_nonfinite=True)
    assert f64[2][0][1] == 1.0 and f64[2][1][1] < 1.0 and [s[2] for s in f64[2]] == [0, 0, 1, 1]
    ps, opt = _fused(dev, params0, group_of, groups, max_grad_norm=m, skip_nonfinite=True)
    opt.prepare_state()
    for p in ps:
        p.grad = torch.zeros_like(p)
    scratch, warm = _fused(dev, [torch.ones(3)], [0], [A.group()], max_grad_norm=1.0, skip_nonfinite=True)
    scratch[0].grad = torch.ones(3, device=dev)
    warm.step()                                                # the kernels' first launch ever is not a captured one
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt.step()
    torch.cuda.synchronize()
    assert all(torch.equal(_bits(p.detach().cpu().reshape(-1)), _bits(q)) for p, q in zip(ps, params0)), "capturing must not step"
    assert float(opt.skipped_steps) == 0.0
    for s, row in enumerate(grads):
        for p, g in zip(ps, row):
            p.grad.copy_(g)
        graph.replay()
        _stats_hold(("captured", s), _fused_stats(opt), f64[2][s])
    params, states, blocks = _read_fused(ps, opt)
    assert _hold("captured", params, states, f32, f64) == 15
    _blocks_agree(states, blocks, sizes, "captured")
    assert all(st.step == 3 for st in states)


def test_buffers_are_not_allocated_inside_a_capture(monkeypatch):
    """Workspace and stats that do not exist yet are refused while the stream is capturing (no capture is started here: the
    question the optimiser asks is answered for it), and ``prepare_state`` makes them."""
    from molkgnn_amd import _lib
    dev = _dev()
    ps, opt = _fused(dev, [torch.ones(3)], [0], [A.group()], max_grad_norm=1.0)
    ps[0].grad = torch.ones(3, device=dev)
    opt._packed_state(ps[0])
    assert opt._clip_stats is None
    before = ps[0].detach().clone()
    with monkeypatch.context() as mp:
        mp.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
        with pytest.raises(_lib.MolKGNNLibraryError, match="prepare_state"):
            opt.step()
    torch.cuda.synchronize()
    assert torch.equal(_bits(before), _bits(ps[0])) and opt._clip_stats is None
    opt.prepare_state()
    assert opt._clip_stats is not None and float(opt.skipped_steps) == 0.0
    opt.step()
    assert _fused_stats(opt)[0] == A.fp32(math.sqrt(3.0))


# ------------------------------------------------------------------------------------------------ 10: the model --
def test_model_step_clips_and_replays():
    """``GNNModel(num_layers=2)`` on 16 molecules, ``max_grad_norm`` half the first step's gradient norm (measured on an unclipped
    twin): ``grad_norm`` is the norm of the ``.grad`` the step left unscaled, the parameters go to the bound, and two visits through
    ``CapturedSteps(warmup=1)`` -- the second one replayed from a graph -- keep the loss finite and refresh ``grad_norm``."""
    from molkgnn_amd.synthetic import make_batch
    from molkgnn_amd.train import CapturedSteps, GNNModel, configure_optimizer, training_step
    dev = _dev()
    torch.manual_seed(7)
    model = GNNModel(num_layers=2, ffn_dropout_rate=0.0).to(dev).train()
    twin = copy.deepcopy(model)
    batch = make_batch(16, seed=33).to(dev)
    training_step(twin, batch, None)
    torch.cuda.synchronize()
    norm0 = math.sqrt(sum(float(p.grad.double().square().sum()) for p in twin.parameters() if p.grad is not None))
    assert math.isfinite(norm0) and norm0 > 0.0
    m = A.fp32(0.5 * norm0)
    opt = configure_optimizer(model, lr=1e-3, max_grad_norm=m)
    assert opt.max_grad_norm == m and not opt.skip_nonfinite
    table = [(gi, p) for gi, g in enumerate(opt.param_groups) for p in g["params"] if p.numel()]
    params0 = [p.detach().cpu().reshape(-1).clone() for _, p in table]
    group_of = [gi for gi, _ in table]
    L = A.launched([A.group(lr=g["lr"], betas=g["betas"], eps=g["eps"], weight_decay=g["weight_decay"], maximize=g["maximize"],
                            grad_scale=g["grad_scale"]) for g in opt.param_groups])
    loss = training_step(model, batch, opt)
    torch.cuda.synchronize()
    assert math.isfinite(float(loss.detach()))
    row = [None if p.grad is None else p.grad.detach().cpu().reshape(-1).clone() for _, p in table]
    f64, f32 = K.run_f64(params0, group_of, L, [row], m), K.run_torch(params0, group_of, L, [row], m)
    got = _fused_stats(opt)
    _stats_hold("model", got, f64[2][0])
    assert got[1] < 0.75 and abs(got[0] - norm0) <= 1e-3 * norm0       # it clips; .grad was not written back (the twin's norm)
    params, states, _ = _read_fused([p for _, p in table], opt)
    assert _hold("model", params, states, f32, f64) == 3 * len(table)
    steps = CapturedSteps(model, opt, warmup=1)
    seen = [got[0]]
    for visit in range(2):
        loss = steps(batch)
        torch.cuda.synchronize()
        assert math.isfinite(float(loss.detach())), visit
        norm = float(opt.grad_norm)
        assert math.isfinite(norm) and norm > 0.0 and norm not in seen, (visit, norm, seen)
        seen.append(norm)
    assert len(steps._graphs) == 1 and float(opt.skipped_steps) == 0.0
