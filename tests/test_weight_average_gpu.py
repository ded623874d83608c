"""The average of the weights kept inside the fused AdamW launch (``mkgnn_adamw_step_averaged``, csrc/kgnn_optim.hip) and the exchange
``mkgnn_flat_swap``.  Tables are driven through the C ABI with guard sentinels around every buffer; a twin table goes through
``mkgnn_adamw_step`` / ``mkgnn_adamw_step_clipped`` -- the entries as they were -- and must stay bit-equal in parameters, moments,
step counts and stats, while its parameter snapshots feed the float32 leg of ``tests/_avg_f64.py`` (separate torch CPU operators)
that the averages are held to, bit for bit.  ``pytest -m gpu``."""
import copy
import math

import pytest
import torch

from tests import _adamw_f64 as A
from tests import _avg_f64 as V

pytestmark = pytest.mark.gpu

GUARD = 1024
SENTINEL = 1234567.0
MAX_NORM = A.fp32(1e4)                  # of the 161-tensor table's six steps some clip at this threshold and some do not


def _dev():
    assert torch.cuda.is_available(), "pytest -m gpu needs the MI355X"
    return torch.device("cuda:0")


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _settings(mode="ema", decay=0.9, warmup=False, start=0):
    return dict(mode=mode, decay=A.fp32(decay), warmup=bool(warmup), start=int(start))


# ------------------------------------------------------------------------------------------------- the driver --
class _Direct:
    """A tensor table handed to the C ABI as it stands: param, grad and packed state (``state_floats + average_floats`` per tensor,
    the average initialised to the parameter, every count 0) cut out of three larger buffers, workspace and stats out of two more,
    ``GUARD`` sentinels on each side of each (the pattern of ``test_clip_gpu.py``).  Group 0's learning rate is read from a device
    float that ``step`` refills; every tensor has an active flag on the device (1 unless ``step`` is told otherwise)."""

    def __init__(self, dev, params0, group_of):
        from molkgnn_amd import _lib
        self._lib = _lib
        self.lib, self.dev, self.group_of = _lib.load(), dev, list(group_of)
        self.sizes = [p.numel() for p in params0]
        self.slens = [A.state_floats(n) + V.average_floats(n) for n in self.sizes]
        assert all(A.state_floats(n) == self.lib.mkgnn_adamw_state_floats(n) and V.average_floats(n) == self.lib.mkgnn_adamw_average_floats(n)
                   for n in set(self.sizes))

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
        P = torch.full((total,), SENTINEL)
        S = torch.full((stotal,), SENTINEL)
        for p, off, n, so, sl in zip(params0, self.poff, self.sizes, self.soff, self.slens):
            P[off:off + n] = p
            S[so:so + sl] = 0.0
            S[so + A.state_floats(n):so + A.state_floats(n) + n] = p
        self.P, self.S = P.to(dev), S.to(dev)
        self.G = torch.full((total,), SENTINEL, device=dev)
        self._G_host = torch.full((total,), SENTINEL)
        self.flags = torch.ones(len(self.sizes), device=dev)
        self.lr0 = torch.zeros(1, device=dev)
        full = self._table(range(len(self.sizes)))
        self.ws_bytes = int(self.lib.mkgnn_adamw_clip_workspace_bytes(full, len(self.sizes)))
        self.W = torch.full((GUARD + self.ws_bytes // 8 + GUARD,), SENTINEL, dtype=torch.float64, device=dev)
        self.stats = torch.full((GUARD + 4 + GUARD,), SENTINEL, device=dev)
        self.stats[GUARD:GUARD + 4] = 0.0
        torch.cuda.synchronize()

    def _table(self, which):
        which = list(which)
        t = (self._lib.AdamWTensor * len(which))()
        for e, i in zip(t, which):
            off, so = self.poff[i], self.soff[i]
            e.param, e.grad, e.state = self.P.data_ptr() + 4 * off, self.G.data_ptr() + 4 * off, self.S.data_ptr() + 4 * so
            e.numel, e.group, e.active = self.sizes[i], self.group_of[i], self.flags.data_ptr() + 4 * i
        return t

    def _groups(self, groups):
        arr = (self._lib.AdamWGroup * len(groups))()
        for k, (e, G) in enumerate(zip(arr, groups)):
            e.lr_device, e.lr = (self.lr0.data_ptr(), 0.0) if k == 0 else (None, G["lr"])
            e.beta1, e.beta2, e.eps, e.weight_decay = G["betas"][0], G["betas"][1], G["eps"], G["weight_decay"]
            e.maximize, e.grad_scale = int(G["maximize"]), G["grad_scale"]
        self.lr0.fill_(groups[0]["lr"])
        return arr

    def step(self, groups, grads, avg=None, clip=None, active=None):
        """One step of the tensors whose gradient is not None.  ``avg``: None (``mkgnn_adamw_step`` / ``_clipped``) or ``_settings``
        (``mkgnn_adamw_step_averaged``); ``clip``: None (the unclipped form) or ``(max_norm, skip_nonfinite)``."""
        which = [i for i, g in enumerate(grads) if g is not None]
        for i in which:
            self._G_host[self.poff[i]:self.poff[i] + self.sizes[i]] = grads[i]
        self.G.copy_(self._G_host)
        self.flags.copy_(torch.ones(len(self.sizes)) if active is None else torch.tensor([float(a) for a in active]))
        table, garr, st = self._table(which), self._groups(groups), self._lib.stream_ptr(self.dev)
        ws, stats = self.W.data_ptr() + 8 * GUARD, self.stats.data_ptr() + 4 * GUARD
        with torch.cuda.device(self.dev):
            if avg is not None:
                v = self._lib.AdamWAverage(V.MODES.index(avg["mode"]), avg["decay"], int(avg["warmup"]), avg["start"])
                if clip is None:
                    rc = self.lib.mkgnn_adamw_step_averaged(table, len(which), garr, len(groups), v, math.inf, 0, None, 0, None, st)
                else:
                    rc = self.lib.mkgnn_adamw_step_averaged(table, len(which), garr, len(groups), v, clip[0], int(clip[1]), ws,
                                                            self.ws_bytes, stats, st)
            elif clip is None:
                rc = self.lib.mkgnn_adamw_step(table, len(which), garr, len(groups), st)
            else:
                rc = self.lib.mkgnn_adamw_step_clipped(table, len(which), garr, len(groups), clip[0], int(clip[1]), ws, self.ws_bytes, stats, st)
        torch.cuda.synchronize()
        assert rc == 0, self.lib.mkgnn_last_error()

    def read(self):
        """Per tensor, on the CPU: parameter, packed AdamW state, average, canonical count, per-block counts."""
        P, S = self.P.cpu(), self.S.cpu()
        out = []
        for off, n, so in zip(self.poff, self.sizes, self.soff):
            sf = A.state_floats(n)
            out.append(dict(p=P[off:off + n].clone(), state=S[so:so + sf].clone(), avg=S[so + sf:so + sf + n].clone(),
                            n_avg=float(S[so + sf + n]), n_blocks=S[so + sf + n + 1:so + sf + V.average_floats(n)].tolist(),
                            step=int(S[so + 2 * n]), reserved=S[so + 2 * n + 1:so + 2 * n + 3].tolist()))
        return out

    def read_stats(self):
        return self.stats[GUARD:GUARD + 4].cpu()

    def guards_intact(self):
        want = _bits(torch.tensor([SENTINEL]))[0].item()
        tables = all(bool((_bits(buf)[mask] == want).all()) for buf, mask in ((self.P, self.pguard), (self.G, self.pguard), (self.S, self.sguard)))
        W, st = self.W.cpu(), self.stats.cpu()
        around = bool((W[:GUARD] == SENTINEL).all()) and bool((W[-GUARD:] == SENTINEL).all()) and \
            bool((st[:GUARD] == SENTINEL).all()) and bool((st[-GUARD:] == SENTINEL).all())
        return tables and around and _same(self.G.cpu(), self._G_host)


def _hold(tag, new, twin, ref_avgs, ref_ns):
    """``new`` (averaged) against ``twin`` (the entries as they were) and the definition: every bit."""
    a, b = new.read(), twin.read()
    for i, (x, y) in enumerate(zip(a, b)):
        assert _same(x["p"], y["p"]), (tag, i, "param")
        assert _same(x["state"], y["state"]), (tag, i, "moments, step counts, reserved")
        assert x["reserved"] == [0.0, 0.0], (tag, i)
        assert _same(x["avg"], ref_avgs[i]), (tag, i, "avg", int((_bits(x["avg"]) != _bits(ref_avgs[i])).sum()))
        nb = (new.sizes[i] + A.CHUNK - 1) // A.CHUNK
        assert x["n_avg"] == float(ref_ns[i]) and x["n_blocks"] == [float(ref_ns[i])] * nb, (tag, i, x["n_avg"], x["n_blocks"], ref_ns[i])
        # the twin's average was never touched: its parameter at the start, counts 0
        assert y["n_avg"] == 0.0 and not any(y["n_blocks"]), (tag, i)
    assert _same(new.read_stats(), twin.read_stats()), (tag, new.read_stats(), twin.read_stats())
    assert new.guards_intact() and twin.guards_intact(), tag


def _trajectory(dev, params0, group_of, groups_at, grads, avg, clip=None, active=None, check_every_step=True, tag=""):
    """Both tables through ``grads``; the definition fed with the twin's snapshots; everything held after every step."""
    new, twin = _Direct(dev, params0, group_of), _Direct(dev, params0, group_of)
    snaps, counts = [], []
    for s, row in enumerate(grads):
        G, act = groups_at(s), None if active is None else active[s]
        twin.step(G, row, None, clip, act)
        new.step(G, row, avg, clip, act)
        t = twin.read()
        snaps.append([x["p"] for x in t])
        counts.append([x["step"] for x in t])
        if check_every_step or s == len(grads) - 1:
            ref_avgs, ref_ns, _ = V.run(params0, snaps, counts, **avg)
            _hold((tag, s), new, twin, ref_avgs, ref_ns)
    return new, twin, snaps, counts


# ------------------------------------------------------------------------------------ 1: block edges and launches --
@pytest.fixture(scope="module")
def tables():
    """The two tables of test 1 -- one tensor of every block-edge size, and 161 tensors over three launches -- with four groups
    interleaved and six steps of gradients; computed once, shared, not modified."""
    out = {}
    for name, sizes, seed in (("block_sizes", list(A.BLOCK_SIZES), 41), ("161", A.table_sizes(161), 6)):
        out[name] = dict(sizes=sizes, group_of=[i % 4 for i in range(len(sizes))], params0=A.make_params(sizes, seed=seed),
                         grads=A.make_grads(sizes, 6, seed + 5))
    return out


@pytest.mark.parametrize("form", ["unclipped", "clipped"])
@pytest.mark.parametrize("name", ["block_sizes", "161"])
def test_block_edges_and_launches(tables, name, form):
    """Four groups, group 0's learning rate refilled on the device step by step, six steps: the twin through the entry as it was
    is bit-equal in parameters, moments, every per-block step count and the stats; the averages are the definition's in bits, every
    per-block ``n_averaged`` and the canonical one are its count; sentinels and the reserved floats are intact."""
    t = tables[name]
    groups_at = A.launched(A.four_groups_at)
    clip = None if form == "unclipped" else (MAX_NORM, True)
    avg = _settings("ema", 0.9, warmup=True) if form == "unclipped" else _settings("mean")
    new, twin, _, counts = _trajectory(_dev(), t["params0"], t["group_of"], groups_at, t["grads"], avg, clip, tag=(name, form))
    assert counts[-1] == [6] * len(t["sizes"])
    if form == "clipped" and name == "161":
        assert float(new.read_stats()[2]) == 0.0


# ------------------------------------------------------------------------------------------- 2: modes and edges --
EDGE_SIZES = [1025, 3, 2049, 1]


@pytest.fixture(scope="module")
def edge_inputs():
    return dict(params0=A.make_params(EDGE_SIZES, seed=51), grads=A.make_grads(EDGE_SIZES, 6, seed=52), group_of=[0, 1, 0, 1])


@pytest.mark.parametrize("mode,warmup", [("ema", False), ("ema", True), ("mean", False)])
def test_modes_and_edges(edge_inputs, mode, warmup):
    """``decay`` 0 / 0.9 / 0.9999 and ``start`` 0 / 3 over six steps.  ``decay = 0`` (``w = 1``) tracks the parameter bit for
    bit; until the step count exceeds ``start`` the average is the parameter in bits and the count 0."""
    e = edge_inputs
    dev = _dev()
    groups = A.launched(A.FOUR_GROUPS[:2])
    for decay in ((0.0, 0.9, 0.9999) if mode == "ema" else (0.5,)):
        for start in (0, 3):
            avg = _settings(mode, decay, warmup, start)
            new, twin, snaps, counts = _trajectory(dev, e["params0"], e["group_of"], lambda s: groups, e["grads"], avg, tag=(mode, warmup, decay, start))
            _, _, hist = V.run(e["params0"], snaps, counts, **avg)
            for s, (avgs, ns) in enumerate(hist):
                tracks = s + 1 <= start or (mode == "ema" and decay == 0.0) or s + 1 == start + 1
                if s + 1 <= start:
                    assert ns == [0] * 4
                else:
                    assert ns == [s + 1 - start] * 4
                if tracks:
                    assert all(_same(a, p) for a, p in zip(avgs, snaps[s])), (decay, start, s)
            final = new.read()
            assert all(x["n_avg"] == 6.0 - start for x in final)
            if not (mode == "ema" and decay == 0.0):
                assert not any(_same(x["avg"], x["p"]) for x in final if x["p"].numel() > 1)      # it averages


# ----------------------------------------------------------------------------------- 3: steps that do not happen --
@pytest.mark.parametrize("form", ["unclipped", "clipped"])
def test_idle_tensors_and_missing_gradients_are_not_averaged(form):
    """Active flags of 0 on tensor 0 (three blocks; in the clipped form the block that writes the stats is an idle one) and on
    tensor 3, a ``None`` gradient on tensor 2: their averages and counts do not change by a bit while the others advance, and the
    counts end up different per tensor."""
    dev = _dev()
    sizes = [2049, 3, 5, 1025, 2, 1]
    T, steps = len(sizes), 4
    groups = A.launched([A.group(lr=2e-3, weight_decay=0.02, grad_scale=0.5)])
    params0, grads = A.make_params(sizes, seed=21), A.make_grads(sizes, steps, seed=22)
    active = [[1.0] * T for _ in range(steps)]
    active[0][0] = active[2][3] = active[3][3] = 0.0
    grads[0][0][2048] = math.inf                               # (flagged off: it must not reach the norm, the step or the average)
    grads[2][2] = None
    clip = None if form == "unclipped" else (A.fp32(5.0), True)
    avg = _settings("ema", 0.9, warmup=False, start=1)
    new, twin = _Direct(dev, params0, [0] * T), _Direct(dev, params0, [0] * T)
    snaps, counts = [], []
    for s, row in enumerate(grads):
        before = new.read()
        twin.step(groups, row, None, clip, active[s])
        new.step(groups, row, avg, clip, active[s])
        after, t = new.read(), twin.read()
        snaps.append([x["p"] for x in t])
        counts.append([x["step"] for x in t])
        for i in range(T):
            off = active[s][i] == 0.0 or row[i] is None
            same = _same(before[i]["avg"], after[i]["avg"]) and before[i]["n_avg"] == after[i]["n_avg"] and before[i]["n_blocks"] == after[i]["n_blocks"] \
                and _same(before[i]["p"], after[i]["p"]) and _same(before[i]["state"], after[i]["state"])
            assert same == off, (s, i)
    ref_avgs, ref_ns, _ = V.run(params0, snaps, counts, **avg)
    _hold(("idle", form), new, twin, ref_avgs, ref_ns)
    assert counts[-1] == [3, 4, 3, 2, 4, 4] and ref_ns == [2, 3, 2, 1, 3, 3]
    if form == "clipped":
        assert float(new.read_stats()[2]) == 0.0 and math.isfinite(float(new.read_stats()[0]))


@pytest.mark.parametrize("guard", [True, False])
def test_a_non_finite_step(tables, guard):
    """Two finite steps, one with an ``inf`` in the last gradient of the third launch, one finite.  Guard on: the bad step changes
    no bit of any parameter, state, average or count, and ``stats[2]`` goes up by one.  Guard off: the step follows the clipped
    entry (the twin, bit-equal, NaN included), and the average takes what the step produced -- NaN where the definition has NaN,
    the definition's bits elsewhere."""
    t = tables["161"]
    dev = _dev()
    groups = A.launched(A.FOUR_GROUPS)
    bad = [g.clone() for g in t["grads"][2]]
    bad[160][-1] = math.inf
    rows = [t["grads"][0], t["grads"][1], bad, t["grads"][3]]
    avg, clip = _settings("ema", 0.9, warmup=True), (MAX_NORM, guard)
    new, twin = _Direct(dev, t["params0"], t["group_of"]), _Direct(dev, t["params0"], t["group_of"])
    snaps, counts = [], []
    for s, row in enumerate(rows):
        P0, S0, skipped0 = new.P.clone(), new.S.clone(), float(new.read_stats()[2])
        twin.step(groups, row, None, clip)
        new.step(groups, row, avg, clip)
        tw = twin.read()
        snaps.append([x["p"] for x in tw])
        counts.append([x["step"] for x in tw])
        if s == 2 and guard:
            assert _same(P0, new.P) and _same(S0, new.S) and float(new.read_stats()[2]) == skipped0 + 1.0
            assert not math.isfinite(float(new.read_stats()[0]))
    assert _same(new.P, twin.P) and _same(new.read_stats(), twin.read_stats())
    ref_avgs, ref_ns, _ = V.run(t["params0"], snaps, counts, **avg)
    got = new.read()
    assert ref_ns == ([3] * 161 if guard else [4] * 161) and float(new.read_stats()[2]) == (1.0 if guard else 0.0)
    nans = 0
    for i, (x, y, r) in enumerate(zip(got, twin.read(), ref_avgs)):
        assert _same(x["state"], y["state"]) and x["n_avg"] == float(ref_ns[i]) and set(x["n_blocks"]) == {float(ref_ns[i])}, i
        k = torch.isnan(r)
        nans += int(k.sum())
        assert torch.equal(torch.isnan(x["avg"]), k) and _same(x["avg"][~k], r[~k]), i
    assert (nans == 0) == guard and new.guards_intact()


# ------------------------------------------------------------------------------------------------- 4: capture --
def _fused(dev, params0, group_of, groups0, **kw):
    from molkgnn_amd.optim import FusedAdamW
    assert list(group_of) == sorted(group_of)
    ps = [torch.nn.Parameter(p.to(dev)) for p in params0]
    pgs = [dict(params=[p for p, gi in zip(ps, group_of) if gi == k], lr=G["lr"], betas=G["betas"], eps=G["eps"],
                weight_decay=G["weight_decay"], maximize=G["maximize"], grad_scale=G["grad_scale"]) for k, G in enumerate(groups0)]
    return ps, FusedAdamW(pgs, **kw)


def _fused_equal(ps, opt, qs, opq):
    torch.cuda.synchronize()
    return all(_same(p, q) and _same(opt.state[p]["_packed"], opq.state[q]["_packed"]) for p, q in zip(ps, qs))


def test_captured_step_averages_as_the_eager_one():
    """ONE ``opt.step()`` captured (clipped, guarded, EMA with warmup), replayed over four rows of gradients -- small, large,
    non-finite, finite -- against the eager steps of a twin optimiser: parameters and packed states, averages and counts
    included, equal in every bit; the skipped step was not averaged."""
    dev = _dev()
    sizes, group_of, groups = A.table_sizes(5), [0, 0, 1, 1, 1], A.FOUR_GROUPS[:2]
    params0, base = A.make_params(sizes, seed=28), A.make_grads(sizes, 3, seed=29)
    bad = [g * 100.0 for g in base[1]]
    bad[1][1] = math.inf
    rows = [base[0], [g * 100.0 for g in base[1]], bad, base[2]]
    kw = dict(max_grad_norm=1e-3, skip_nonfinite=True, average="ema", average_decay=0.9, average_warmup=True)
    ps, opt = _fused(dev, params0, group_of, groups, **kw)
    qs, eager = _fused(dev, params0, group_of, groups, **kw)
    opt.prepare_state()
    for p, q in zip(ps, qs):
        p.grad, q.grad = torch.zeros_like(p), torch.zeros_like(q)
    for row in rows[:1]:                                       # (the kernels' first launch ever is an eager one: the twin's)
        for q, g in zip(qs, row):
            q.grad.copy_(g)
        eager.step()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt.step()
    torch.cuda.synchronize()
    assert all(_same(p.detach().cpu().reshape(-1), q) for p, q in zip(ps, params0)), "capturing must not step"
    assert all(float(opt.state[p]["n_averaged"]) == 0.0 and _same(opt.state[p]["param_avg"], p) for p in ps)
    for s, row in enumerate(rows):
        for p, q, g in zip(ps, qs, row):
            p.grad.copy_(g)
            q.grad.copy_(g)
        graph.replay()
        if s:
            eager.step()
        assert _fused_equal(ps, opt, qs, eager), s
    assert float(opt.skipped_steps) == 1.0 and all(float(opt.state[p]["n_averaged"]) == 3.0 and float(opt.state[p]["step"]) == 3.0 for p in ps)
    assert not any(_same(opt.state[p]["param_avg"], p) for p in ps if p.numel() > 1)


def test_the_average_is_not_allocated_inside_a_capture(monkeypatch):
    """State that does not exist yet is refused while the stream is capturing (no capture is started: the question the optimiser
    asks is answered for it); ``prepare_state`` makes it, the average a copy of the parameter with count 0."""
    from molkgnn_amd import _lib
    dev = _dev()
    ps, opt = _fused(dev, [torch.arange(1025.0)], [0], [A.group()], average="mean")
    ps[0].grad = torch.ones(1025, device=dev)
    with monkeypatch.context() as mp:
        mp.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
        with pytest.raises(_lib.MolKGNNLibraryError, match="prepare_state"):
            opt.step()
    assert "_packed" not in opt.state[ps[0]]
    opt.prepare_state()
    st = opt.state[ps[0]]
    assert st["_packed"].numel() == A.state_floats(1025) + V.average_floats(1025)
    assert st["param_avg"].shape == ps[0].shape and _same(st["param_avg"], ps[0]) and st["param_avg"].data_ptr() != ps[0].data_ptr()
    assert st["n_averaged"].dim() == 0 and float(st["n_averaged"]) == 0.0 and not bool(st["_packed"][A.state_floats(1025) + 1025:].any())
    assert [id(p) for p in opt.averaged_parameters()] == [id(ps[0])] and opt.averaged_parameters()[ps[0]].data_ptr() == st["param_avg"].data_ptr()
    opt.step()
    torch.cuda.synchronize()
    assert float(st["n_averaged"]) == 1.0 and _same(st["param_avg"], ps[0])
    # without averaging the packed state has the size it had
    qs, plain = _fused(dev, [torch.arange(1025.0)], [0], [A.group()])
    plain.prepare_state()
    assert plain.state[qs[0]]["_packed"].numel() == A.state_floats(1025) and "param_avg" not in plain.state[qs[0]]


# ---------------------------------------------------------------------------------------------------- 5: swap --
SWAP_SIZES = (1, 255, 1024, 1025, 4097)


class _Pairs:
    """121 pairs (two launches) cut out of two buffers with ``GUARD`` sentinels around every tensor."""

    def __init__(self, dev):
        from molkgnn_amd import _lib
        self._lib, self.lib, self.dev = _lib, _lib.load(), dev
        self.sizes = [SWAP_SIZES[i % len(SWAP_SIZES)] for i in range(121)]
        self.offs, o = [], 0
        for n in self.sizes:
            self.offs.append(o + GUARD)
            o += GUARD + n + GUARD
        g = torch.Generator().manual_seed(61)
        A0, B0 = torch.full((o,), SENTINEL), torch.full((o,), SENTINEL)
        self.inside = torch.zeros(o, dtype=torch.bool)
        for off, n in zip(self.offs, self.sizes):
            A0[off:off + n] = torch.randn(n, generator=g)
            B0[off:off + n] = torch.randn(n, generator=g) * 1e-3
            self.inside[off:off + n] = True
        A0[self.offs[0]] = math.nan                            # bits, not values, are exchanged
        self.A0, self.B0 = A0, B0
        self.A, self.B = A0.to(dev), B0.to(dev)
        self.items = (_lib.SwapItem * 121)()
        for e, off, n in zip(self.items, self.offs, self.sizes):
            e.a, e.b, e.numel = self.A.data_ptr() + 4 * off, self.B.data_ptr() + 4 * off, n

    def swap(self):
        with torch.cuda.device(self.dev):
            rc = self.lib.mkgnn_flat_swap(self.items, 121, self._lib.stream_ptr(self.dev))
        assert rc == 0, self.lib.mkgnn_last_error()

    def state(self):
        """0: as at the start; 1: exchanged inside every tensor, sentinels intact; None: anything else."""
        torch.cuda.synchronize()
        a, b = self.A.cpu(), self.B.cpu()
        if _same(a, self.A0) and _same(b, self.B0):
            return 0
        k = self.inside
        if _same(a[k], self.B0[k]) and _same(b[k], self.A0[k]) and _same(a[~k], self.A0[~k]) and _same(b[~k], self.B0[~k]):
            return 1
        return None


def test_swap_exchanges_bits_and_is_an_involution():
    d = _Pairs(_dev())
    assert d.state() == 0
    d.swap()
    assert d.state() == 1
    d.swap()
    assert d.state() == 0
    graph = torch.cuda.CUDAGraph()                             # (the kernel's first launch was an eager one)
    with torch.cuda.graph(graph):
        d.swap()
    assert d.state() == 0, "capturing must not swap"
    graph.replay()
    assert d.state() == 1
    graph.replay()
    assert d.state() == 0


def test_averaged_weights_swaps_back_and_refuses_a_step():
    dev = _dev()
    sizes = [1025, 3, 1]
    params0, grads = A.make_params(sizes, seed=71), A.make_grads(sizes, 2, seed=72)
    ps, opt = _fused(dev, params0, [0, 0, 0], [A.group(lr=1e-2)], average="ema", average_decay=0.5, average_warmup=False)
    for row in grads:
        for p, g in zip(ps, row):
            p.grad = g.to(dev)
        opt.step()
    live = [p.detach().clone() for p in ps]
    avgs = [opt.state[p]["param_avg"].clone() for p in ps]
    assert not any(_same(a, b) for a, b in zip(live, avgs))
    ptrs = [p.data_ptr() for p in ps]
    with opt.averaged_weights():
        assert all(_same(p, a) for p, a in zip(ps, avgs)) and all(_same(opt.state[p]["param_avg"], l) for p, l in zip(ps, live))
        with pytest.raises(RuntimeError, match="averaged_weights"):
            opt.step()
    assert all(_same(p, l) for p, l in zip(ps, live)) and all(_same(opt.state[p]["param_avg"], a) for p, a in zip(ps, avgs))
    with pytest.raises(KeyError, match="the body raised"):
        with opt.averaged_weights():
            raise KeyError("the body raised")
    assert all(_same(p, l) for p, l in zip(ps, live)) and all(_same(opt.state[p]["param_avg"], a) for p, a in zip(ps, avgs))
    assert [p.data_ptr() for p in ps] == ptrs
    opt.step()                                                 # ... and the optimiser steps again afterwards
    opt.swap_averaged()
    opt.swap_averaged()
    torch.cuda.synchronize()
    assert all(float(opt.state[p]["n_averaged"]) == 3.0 for p in ps)


# ---------------------------------------------------------------------------------------------- 6: state dict --
def test_state_dict_round_trip_continues_the_average():
    """Three steps, ``state_dict()`` into a fresh optimiser over fresh parameters, three more: bit-equal to six uninterrupted steps,
    averages and counts included.  A state without the two entries starts a fresh average."""
    dev = _dev()
    sizes, group_of, groups = [1025, 3, 2049, 1, 5], [0, 0, 1, 1, 1], A.FOUR_GROUPS[:2]
    params0, grads = A.make_params(sizes, seed=81), A.make_grads(sizes, 6, seed=82)
    kw = dict(max_grad_norm=MAX_NORM, skip_nonfinite=True, average="ema", average_decay=0.9, average_warmup=True, average_start=1)

    def steps(ps, opt, rows):
        for row in rows:
            for p, g in zip(ps, row):
                p.grad = g.to(dev)
            opt.step()
    ps, whole = _fused(dev, params0, group_of, groups, **kw)
    steps(ps, whole, grads)
    qs, first = _fused(dev, params0, group_of, groups, **kw)
    steps(qs, first, grads[:3])
    sd = copy.deepcopy(first.state_dict())
    assert all(set(v) == {"step", "exp_avg", "exp_avg_sq", "param_avg", "n_averaged"} for v in sd["state"].values())
    assert all(float(v["n_averaged"]) == 2.0 and v["param_avg"].shape == v["exp_avg"].shape for v in sd["state"].values())
    rs, second = _fused(dev, [q.detach().cpu() for q in qs], group_of, groups, **kw)
    second.load_state_dict(sd)
    steps(rs, second, grads[3:])
    assert _fused_equal(ps, whole, rs, second)
    assert all(float(whole.state[p]["n_averaged"]) == 5.0 for p in ps)
    # a state saved without averaging: a fresh average -- a copy of the parameter, count 0 -- and the moments as saved
    us, plain = _fused(dev, params0, group_of, groups)
    steps(us, plain, grads[:3])
    vs, fresh = _fused(dev, [u.detach().cpu() for u in us], group_of, groups, **kw)
    fresh.load_state_dict(copy.deepcopy(plain.state_dict()))
    torch.cuda.synchronize()
    for u, v in zip(us, vs):
        st = fresh.state[v]
        assert float(st["n_averaged"]) == 0.0 and _same(st["param_avg"], v) and float(st["step"]) == 3.0
        assert _same(st["exp_avg"], plain.state[u]["exp_avg"]) and not bool(st["_packed"][A.state_floats(v.numel()) + v.numel():].any())
    # ... and an averaging state loaded into an optimiser without averaging drops the two entries
    ws, off = _fused(dev, params0, group_of, groups)
    off.load_state_dict(copy.deepcopy(sd))
    assert all("param_avg" not in off.state[w] and off.state[w]["_packed"].numel() == A.state_floats(w.numel()) for w in ws)


# --------------------------------------------------------------------------------------------------- 7: model --
def test_model_evaluates_with_the_averaged_weights():
    """``GNNModel(num_layers=2)`` on 16 molecules, clipped, guarded, EMA 0.9, a few visits through ``CapturedSteps``.  Inside
    ``train.averaged_weights`` the prediction equals in bits that of a deep copy loaded with ``train.averaged_state_dict``; after
    the block the parameters are bit-equal to before; further replays give the trajectory of a twin that never swapped."""
    from molkgnn_amd import train
    from molkgnn_amd.synthetic import make_batch
    dev = _dev()
    torch.manual_seed(7)
    model = train.GNNModel(num_layers=2, ffn_dropout_rate=0.0).to(dev).train()
    twin = copy.deepcopy(model)
    batch = make_batch(16, seed=33).to(dev)
    kw = dict(lr=1e-3, average="ema", average_decay=0.9, max_grad_norm=1.0, skip_nonfinite=True)
    opt, opt_twin = train.configure_optimizer(model, **kw), train.configure_optimizer(twin, **kw)
    assert opt.average == "ema" and opt.average_decay == 0.9 and opt.average_warmup and opt.clipping
    steps, steps_twin = train.CapturedSteps(model, opt, warmup=1), train.CapturedSteps(twin, opt_twin, warmup=1)
    for _ in range(3):
        steps(batch)
        steps_twin(batch)
    torch.cuda.synchronize()
    assert len(steps._graphs) == 1 and len(steps_twin._graphs) == 1
    live = {n: p.detach().clone() for n, p in model.named_parameters()}
    assert all(_same(p, q) for p, q in zip(model.parameters(), twin.parameters()))
    sd = train.averaged_state_dict(model, opt)
    assert set(sd) == set(model.state_dict())
    changed = [n for n, p in model.named_parameters() if p.numel() > 1 and not _same(sd[n], p)]
    # the averages are not the last iterate -- where the weights moved: a bank of a degree the batch does not contain has no
    # gradient, is never stepped, and its average is the parameter itself
    moved = [n for n, p in model.named_parameters() if float(opt.state[p]["step"]) == 3.0]
    assert changed and set(changed) <= set(moved) and "ffn.weight" in changed
    assert all(_same(sd[n], p) for n, p in model.named_parameters() if float(opt.state[p]["step"]) == 0.0)
    assert all(torch.equal(sd[n], b) for n, b in model.named_buffers() if n in sd)        # buffers as they stand
    loaded = copy.deepcopy(model).eval()
    loaded.load_state_dict(sd)
    want = loaded.predict(batch)[0].clone()
    with train.evaluation_mode(model):
        plain = model.predict(batch)[0].clone()
        with train.averaged_weights(model, opt) as m:
            assert m is model
            got = model.predict(batch)[0].clone()
            with pytest.raises(RuntimeError, match="averaged_weights"):
                opt.step()
        again = model.predict(batch)[0].clone()
    torch.cuda.synchronize()
    assert got.shape == (16, 1) and _same(got, want) and not _same(got, plain) and _same(again, plain)
    assert model.training and all(_same(p, live[n]) for n, p in model.named_parameters())
    for _ in range(2):
        a, b = steps(batch), steps_twin(batch)
        torch.cuda.synchronize()
        assert _same(a, b)
    assert all(_same(p, q) for p, q in zip(model.parameters(), twin.parameters()))
    assert all(_same(opt.state[p]["_packed"], opt_twin.state[q]["_packed"]) for p, q in zip(model.parameters(), twin.parameters()) if p in opt.state)
    assert float(opt.skipped_steps) == 0.0 and all(float(st["n_averaged"]) == 5.0 for st in opt.state.values() if float(st["step"]) == 5.0)
