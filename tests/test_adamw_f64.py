"""``mkgnn_adamw_step`` (``adamw_step_kernel``, csrc/kgnn_optim.hip) against float64 at every edge of its tables: a tensor's end
around the 256-lane passes and the 1024-element blocks, tables around the 80 tensors of one launch, four groups interleaved over
two launches, the hyper-parameter edges, a state resumed at a million steps, tensors skipped by device flags and by ``None``
gradients, and a captured step replayed.  Driven through ``optim.FusedAdamW`` and, where the table's order or its surroundings
matter, through the C ABI directly.  ``pytest -m gpu``.

Bound, reference, yardstick and inputs: ``tests/_adamw_f64.py``.  Held exactly beside the bound: every step count -- the canonical
one and each of the ``ceil(n / 1024)`` per-block copies --, the guards around every buffer of a direct call, a skipped tensor's bits.
"""
import pytest
import torch

from tests import _adamw_f64 as A

pytestmark = pytest.mark.gpu

GUARD = 1024
SENTINEL = 1234567.0


def _dev():
    assert torch.cuda.is_available(), "pytest -m gpu needs the MI355X"
    return torch.device("cuda:0")


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _hold(tag, params, states, f32, f64, names=None):
    """The build's parameters and moments to the bound; its step counts to the reference's, exactly."""
    n = A.check(A.quantities(params, states), A.quantities(*f32), A.quantities(*f64), tag, names)
    assert [st.step for st in states] == [st.step for st in f64[1]], tag
    return n


# ------------------------------------------------------------------------------------------ the two drivers --
class _Direct:
    """A tensor table handed to ``mkgnn_adamw_step`` as it stands: param, grad and packed state of every tensor cut out of three
    larger buffers, ``GUARD`` sentinel floats on each side of each."""

    def __init__(self, dev, params0, group_of, active=False):
        from molkgnn_amd import _lib
        self.lib, self.dev, self.group_of = _lib.load(), dev, list(group_of)
        self.sizes = [p.numel() for p in params0]
        self.slens = [A.state_floats(n) for n in self.sizes]
        assert all(self.lib.mkgnn_adamw_state_floats(n) == s for n, s in zip(self.sizes, self.slens))

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
        torch.cuda.synchronize()

    def step(self, groups, grads, lr_device=None):
        """``groups``: group dicts (float32 values); ``lr_device``: a device float read for group 0's learning rate."""
        from molkgnn_amd import _lib
        for g, off, n in zip(grads, self.poff, self.sizes):
            self._G_host[off:off + n] = g
        self.G.copy_(self._G_host)
        arr = (_lib.AdamWGroup * len(groups))()
        for k, (e, G) in enumerate(zip(arr, groups)):
            dev_lr = lr_device is not None and k == 0
            e.lr_device, e.lr = (lr_device.data_ptr() if dev_lr else None), (0.0 if dev_lr else G["lr"])
            e.beta1, e.beta2, e.eps, e.weight_decay = G["betas"][0], G["betas"][1], G["eps"], G["weight_decay"]
            e.maximize, e.grad_scale = int(G["maximize"]), G["grad_scale"]
        with torch.cuda.device(self.dev):
            rc = self.lib.mkgnn_adamw_step(self.table, len(self.sizes), arr, len(groups), _lib.stream_ptr(self.dev))
        torch.cuda.synchronize()
        return rc

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
        """The sentinels around every param, grad and state slot, and the two reserved floats of every state (zero as handed over)."""
        want = _bits(torch.tensor([SENTINEL]))[0].item()
        S = self.S.cpu()
        reserved = all(S[so + 2 * n + 1:so + 2 * n + 3].tolist() == [0.0, 0.0] for so, n in zip(self.soff, self.sizes))
        return reserved and all(bool((_bits(buf)[mask] == want).all())
                                for buf, mask in ((self.P, self.pguard), (self.G, self.pguard), (self.S, self.sguard)))


def _fused(dev, params0, group_of, groups0, lr_device=None):
    """``FusedAdamW`` over device copies of ``params0``; the table's order is group by group, so ``group_of`` must not decrease for
    table position i to be tensor i."""
    from molkgnn_amd.optim import FusedAdamW
    assert list(group_of) == sorted(group_of)
    ps = [torch.nn.Parameter(p.to(dev)) for p in params0]
    pgs = [dict(params=[p for p, gi in zip(ps, group_of) if gi == k], lr=(lr_device if (k == 0 and lr_device is not None) else G["lr"]),
                betas=G["betas"], eps=G["eps"], weight_decay=G["weight_decay"], maximize=G["maximize"], grad_scale=G["grad_scale"])
           for k, G in enumerate(groups0)]
    return ps, FusedAdamW(pgs)


def _read_fused(ps, opt):
    torch.cuda.synchronize()
    params, states, blocks = [], [], []
    for p in ps:
        n, buf = p.numel(), opt.state[p]["_packed"].cpu()
        assert buf.numel() == A.state_floats(n)
        params.append(p.detach().cpu().reshape(-1))
        states.append(A.State((n,), buf[:n], buf[n:2 * n], int(buf[2 * n])))
        blocks.append(buf[2 * n + 3:].tolist())
        assert float(buf[2 * n]) == float(opt.state[p]["step"])
    return params, states, blocks


def _blocks_agree(states, blocks, sizes, tag):
    for i, (st, b, n) in enumerate(zip(states, blocks, sizes)):
        assert len(b) == (n + A.CHUNK - 1) // A.CHUNK and all(c == float(st.step) for c in b), (tag, i, n, st.step, b)


def _run_fused(dev, params0, group_of, groups, grads, state0=None):
    """Eager steps through FusedAdamW; ``groups`` unrounded (a list, or ``step -> list`` whose group 0 lr goes through a device
    tensor); ``state0``: ``(exp_avg, exp_avg_sq, step)`` per tensor, loaded as a state dict."""
    moving = callable(groups)
    g0 = groups(0) if moving else groups
    lr_t = torch.tensor(float(g0[0]["lr"]), device=dev) if moving else None
    ps, opt = _fused(dev, params0, group_of, g0, lr_t)
    if state0 is not None:
        sd = opt.state_dict()
        sd["state"] = {i: dict(step=torch.tensor(float(t)), exp_avg=m.clone(), exp_avg_sq=v.clone()) for i, (m, v, t) in enumerate(state0)}
        opt.load_state_dict(sd)
    for s, row in enumerate(grads):
        if moving:
            lr_t.fill_(float(groups(s)[0]["lr"]))
        for p, g in zip(ps, row):
            p.grad = None if g is None else g.to(dev)
        opt.step()
    return (ps, opt) + _read_fused(ps, opt)


def _cpu_legs(params0, group_of, groups, grads, active=None, state0=None):
    L = A.launched(groups)
    return A.run_torch(params0, group_of, L, grads, active, state0), A.run_f64(params0, group_of, L, grads, active, state0)


# ------------------------------------------------------------------------------------------------- block edges --
@pytest.fixture(scope="module")
def block_edge_run():
    """Eleven tensors, one per size around the 256-lane passes and the 1024-element blocks, two groups, twelve steps of a direct call."""
    dev = _dev()
    sizes = list(A.BLOCK_SIZES)
    group_of = [i % 2 for i in range(len(sizes))]
    groups = [A.group(lr=2e-3, weight_decay=0.02), A.group(lr=1e-3, betas=(0.8, 0.99), eps=1e-6, weight_decay=0.0, maximize=True)]
    params0, grads = A.make_params(sizes, seed=31), A.make_grads(sizes, 12, seed=32)
    d = _Direct(dev, params0, group_of)
    L = A.launched(groups)
    counts = []
    for row in grads:
        assert d.step(L, row) == 0
        counts.append(d.read()[2])
    return dict(d=d, sizes=sizes, counts=counts, legs=_cpu_legs(params0, group_of, groups, grads))


def test_block_edges_values(block_edge_run):
    r = block_edge_run
    params, states, _ = r["d"].read()
    assert _hold("block edges", params, states, *r["legs"]) == 3 * len(r["sizes"])


def test_block_edges_guards_and_state_length(block_edge_run):
    """Nothing outside ``[0, n)`` of a parameter and ``[0, mkgnn_adamw_state_floats(n))`` of its state is written, and the gradient
    buffer is not written at all."""
    d = block_edge_run["d"]
    assert d.guards_intact()
    assert torch.equal(d.G.cpu(), d._G_host)


def test_block_edges_every_block_counts_every_step(block_edge_run):
    r = block_edge_run
    for s, blocks in enumerate(r["counts"]):
        for n, b in zip(r["sizes"], blocks):
            assert b == [float(s + 1)] * ((n + 1023) // 1024), (s, n, b)
    _, states, blocks = r["d"].read()
    _blocks_agree(states, blocks, r["sizes"], "block edges")
    assert all(st.step == 12 for st in states)


# ------------------------------------------------------------------------------------------------- table edges --
@pytest.mark.parametrize("n_tensors", [1, 79, 80, 81, 160, 161])
def test_table_edges(n_tensors):
    """Tables around one and two launches' worth of tensors, a multi-block tensor on both sides of each boundary."""
    dev = _dev()
    sizes = A.table_sizes(n_tensors)
    group_of = [0] * n_tensors
    groups = [A.group(lr=2e-3, weight_decay=0.02)]
    params0, grads = A.make_params(sizes, seed=40 + n_tensors), A.make_grads(sizes, 6, seed=41 + n_tensors)
    _, _, params, states, blocks = _run_fused(dev, params0, group_of, groups, grads)
    assert _hold(f"table {n_tensors}", params, states, *_cpu_legs(params0, group_of, groups, grads)) == 3 * n_tensors
    _blocks_agree(states, blocks, sizes, n_tensors)
    assert all(st.step == 6 for st in states)


# ------------------------------------------------------------------------------------------------------ groups --
def test_four_interleaved_groups_over_two_launches():
    """81 tensors, and 84, tensor i in group i % 4 (a direct call: FusedAdamW's own table is group by group): the first launch indexes
    all four groups, the second one a three-block tensor of group 0 -- and, of 84, all four again; group 0's learning rate is a device
    float refilled before every step."""
    dev = _dev()
    sizes = A.table_sizes(81)
    group_of = [i % 4 for i in range(81)]
    assert {group_of[i] for i in range(80)} == {0, 1, 2, 3} and group_of[80] == 0 and sizes[80] == 2049
    # the second launch holds one tensor: a second table of 84 puts all four groups into it as well
    for n_tensors in (81, 84):
        sz, go = A.table_sizes(n_tensors), [i % 4 for i in range(n_tensors)]
        params0, grads = A.make_params(sz, seed=50), A.make_grads(sz, 12, seed=51)
        d = _Direct(dev, params0, go)
        lr_t = torch.zeros((), device=dev)
        for s, row in enumerate(grads):
            L = A.launched(A.four_groups_at)(s)
            lr_t.fill_(L[0]["lr"])
            assert d.step(L, row, lr_device=lr_t) == 0
        params, states, blocks = d.read()
        assert _hold(f"four groups {n_tensors}", params, states, *_cpu_legs(params0, go, A.four_groups_at, grads)) == 3 * n_tensors
        _blocks_agree(states, blocks, sz, n_tensors)
        assert d.guards_intact()


def test_a_fifth_group_is_refused():
    from molkgnn_amd import _lib
    from molkgnn_amd.optim import FusedAdamW
    dev = _dev()
    params0 = A.make_params([3, 5], seed=52)
    d = _Direct(dev, params0, [0, 4])
    before = d.P.clone()
    rc = d.step([A.as_launched(A.group())] * 5, A.make_grads([3, 5], 1, seed=53)[0])
    assert rc != 0 and b"5 groups" in _lib.load().mkgnn_last_error()
    assert torch.equal(_bits(d.P), _bits(before)) and d.read()[1][0].step == 0
    with pytest.raises(ValueError):
        FusedAdamW([dict(params=[torch.nn.Parameter(torch.zeros(1, device=dev))]) for _ in range(5)])


# ------------------------------------------------------------------------------------------- hyper-parameter edges --
HYPER_SIZES = [3, 1025, 1, 5, 257, 2]


@pytest.mark.parametrize("edge", sorted(A.HYPER_EDGES))
def test_hyper_parameter_edges(edge):
    dev = _dev()
    groups = [A.HYPER_EDGES[edge]]
    group_of = [0] * len(HYPER_SIZES)
    params0, grads = A.make_params(HYPER_SIZES, seed=60), A.make_grads(HYPER_SIZES, 12, seed=61)
    _, _, params, states, blocks = _run_fused(dev, params0, group_of, groups, grads)
    assert _hold(edge, params, states, *_cpu_legs(params0, group_of, groups, grads)) == 3 * len(HYPER_SIZES)
    _blocks_agree(states, blocks, HYPER_SIZES, edge)
    assert all(st.step == 12 for st in states)
    if edge == "lr_0_weight_decay_0":
        assert all(torch.equal(_bits(p), _bits(q)) for p, q in zip(params, params0))
        assert all(float(st.exp_avg.abs().max()) > 0.0 and float(st.exp_avg_sq.abs().max()) > 0.0 for st in states)


# ---------------------------------------------------------------------------------------------------- resumed state --
def test_state_resumed_at_a_million_steps():
    dev = _dev()
    sizes = [3, 2049, 1, 1025]
    group_of = [0] * len(sizes)
    groups = [A.group(lr=2e-3, weight_decay=0.02)]
    state0 = [(m, v, 1_000_000) for m, v in A.make_moments(sizes, seed=70)]
    params0, grads = A.make_params(sizes, seed=71), A.make_grads(sizes, 2, seed=72)
    assert A.bias_corrections_fp32(A.as_launched(groups[0])["betas"], 1_000_001) == (1.0, 1.0)
    _, _, params, states, blocks = _run_fused(dev, params0, group_of, groups, grads, state0=state0)
    assert _hold("resumed", params, states, *_cpu_legs(params0, group_of, groups, grads, state0=state0)) == 3 * len(sizes)
    assert all(st.step == 1_000_002 for st in states)
    _blocks_agree(states, blocks, sizes, "resumed")
    assert blocks[1] == [1_000_002.0] * 3 and blocks[3] == [1_000_002.0] * 2


# --------------------------------------------------------------------------------------------------------- skipping --
def test_skipped_tensors_stand_still_in_both_launches():
    """81 tensors; device flags on tensor 79 (2049 elements, the first launch's last) and tensor 80 (1025 elements, the second launch);
    each reads 0 on some steps, on others some tensors have no gradient."""
    dev = _dev()
    sizes = A.table_sizes(81, big_even=False)
    assert sizes[79] == 2049 and sizes[80] == 1025
    steps, T = 8, 81
    group_of, groups = [0] * T, [A.group(lr=2e-3, weight_decay=0.02)]
    params0, grads = A.make_params(sizes, seed=80), A.make_grads(sizes, steps, seed=81)
    active = [[1.0] * T for _ in range(steps)]
    for s, i in ((0, 80), (2, 79), (3, 79), (3, 80), (6, 80)):
        active[s][i] = 0.0
    for s, i in ((1, 5), (1, 40), (5, 0), (5, 60)):
        grads[s][i] = None
    ps, opt = _fused(dev, params0, group_of, groups)
    flags = torch.ones(2, device=dev)
    opt.set_grad_active({ps[79]: flags[0], ps[80]: flags[1]})
    f64_snaps = A.run_f64(params0, group_of, A.launched(groups), grads, active, snapshots=True)
    for s, row in enumerate(grads):
        flags.copy_(torch.tensor([active[s][79], active[s][80]]))
        for p, g in zip(ps, row):
            p.grad = None if g is None else g.to(dev)
        before = {i: (ps[i].detach().clone(), opt.state[ps[i]]["_packed"].clone()) for i in (79, 80)}
        opt.step()
        torch.cuda.synchronize()
        for i in (79, 80):
            same = torch.equal(_bits(before[i][0]), _bits(ps[i])) and torch.equal(_bits(before[i][1]), _bits(opt.state[ps[i]]["_packed"]))
            assert same == (active[s][i] == 0.0), (s, i)
        params, states, blocks = _read_fused([ps[79], ps[80]], opt)
        assert [st.step for st in states] == [f64_snaps[s][1][79].step, f64_snaps[s][1][80].step], s
        _blocks_agree(states, blocks, [2049, 1025], ("skipping", s))
        if s == 4:                                       # the active step that follows both tensors' skipped one
            f32 = A.run_torch(params0, group_of, A.launched(groups), grads[:5], active)
            assert _hold("skipping, the step after", *_read_fused(ps, opt)[:2], f32, f64_snaps[4]) == 3 * T
    params, states, blocks = _read_fused(ps, opt)
    f32 = A.run_torch(params0, group_of, A.launched(groups), grads, active)
    assert _hold("skipping", params, states, f32, f64_snaps[-1]) == 3 * T
    _blocks_agree(states, blocks, sizes, "skipping")
    assert states[79].step == 6 and states[80].step == 5 and states[5].step == 7 and states[0].step == 7


# ---------------------------------------------------------------------------------------------------- under capture --
def test_captured_step_replayed_over_four_groups():
    """81 tensors in four groups (group by group: 20, 20, 20, 21), state prepared, ONE step captured on one stream and replayed five times;
    between replays the static gradients, group 0's device learning rate and the flag of tensor 80 are refilled."""
    dev = _dev()
    T, replays = 81, 5
    sizes = A.table_sizes(T)
    group_of = [min(i // 20, 3) for i in range(T)]
    params0, grads = A.make_params(sizes, seed=90), A.make_grads(sizes, replays, seed=91)
    active = [[1.0] * T for _ in range(replays)]
    active[1][80] = 0.0
    active[3][80] = 0.0
    lr_t = torch.zeros((), device=dev)
    ps, opt = _fused(dev, params0, group_of, A.four_groups_at(0), lr_t)
    flag = torch.ones(1, device=dev)
    opt.set_grad_active({ps[80]: flag[0]})
    opt.prepare_state()
    for p in ps:
        p.grad = torch.zeros_like(p)
    scratch, warm = _fused(dev, [torch.ones(3)], [0], [A.group()])      # the kernel's first launch ever is not a captured one
    scratch[0].grad = torch.ones(3, device=dev)
    warm.step()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt.step()
    torch.cuda.synchronize()
    assert all(torch.equal(_bits(p.detach().cpu().reshape(-1)), _bits(q)) for p, q in zip(ps, params0)), "capturing must not step"
    for s in range(replays):
        for p, g in zip(ps, grads[s]):
            p.grad.copy_(g)
        lr_t.fill_(A.four_groups_at(s)[0]["lr"])
        flag.fill_(active[s][80])
        graph.replay()
    params, states, blocks = _read_fused(ps, opt)
    assert _hold("captured", params, states, *_cpu_legs(params0, group_of, A.four_groups_at, grads, active)) == 3 * T
    _blocks_agree(states, blocks, sizes, "captured")
    assert states[80].step == 3 and states[79].step == 5
