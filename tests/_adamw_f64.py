"""The float64 leg of the optimiser checks: AdamW written from its definition on the CPU in float64, the float32 yardstick
(``torch.optim.AdamW(foreach=False, fused=False)`` on the same inputs), the seeded inputs, and the bound the build's parameters and
moments are held to.  Nothing here imports the package under test; ``tests/test_adamw_reference_cpu.py`` pins the reference to
``torch.optim.AdamW`` run in float64.

The update of one tensor with gradient ``g`` in a group ``(lr, beta1, beta2, eps, weight_decay, maximize, grad_scale)``::

    g <- grad_scale * g;  g <- -g if maximize            (the scale comes before anything else)
    t <- t + 1
    p <- p - lr * weight_decay * p                        (decoupled: the decay never enters the moments)
    m <- beta1 m + (1 - beta1) g
    v <- beta2 v + (1 - beta2) g g
    p <- p - lr * (m / (1 - beta1^t)) / (sqrt(v / (1 - beta2^t)) + eps)

A tensor is skipped when its gradient is ``None`` or its active flag is 0: ``t`` does not advance and ``m``, ``v`` do not decay.

Per tensor and quantity (parameter, ``exp_avg``, ``exp_avg_sq``): ``max|build - f64| <= C * max|fp32 torch - f64| + R * max(max|f64|,
FLOOR)`` -- the form of ``tests/_f64.check``.  ``C`` and ``R`` are this module's own: at least twice the worst need of an
``MKGNN_F64_RECORD`` run of ``tests/test_adamw_f64.py`` on the MI355X (DESIGN.md lists the measurements) and no larger than
``_f64``'s.  With ``MKGNN_F64_RECORD=<file>`` every comparison is appended to that file as one JSON line before it is asserted.

Hyper-parameters: ``mkgnn_adamw_group`` carries them as float32, so the update the launch can be held to is the one with the
float32 values.  ``as_launched`` rounds a group; all three legs are then given the same numbers and the comparison measures the
arithmetic alone.  (What the rounding itself costs -- ``1 - fp32(0.999)`` is 1.3e-5 away from 0.001, relatively -- is pinned by the
CPU module and described in DESIGN.md.)
"""
from __future__ import annotations

import json
import math
import os

import torch

C = 4.0             # worst need 0.96 (exp_avg of a one-element tensor whose float32 torch value is one ulp off as well)
R = 2.0 ** -19      # worst need 2.8e-7 (exp_avg of a one-element tensor that float32 torch happens to get almost exactly)
FLOOR = 1e-3       # R * FLOOR: the absolute part, for a quantity that is zero in exact arithmetic (a moment of zero gradients)

QUANTITIES = ("param", "exp_avg", "exp_avg_sq")
CHUNK = 1024        # elements per block of the launch: a tensor has ceil(n / CHUNK) per-block step counts
BLOCK_SIZES = (1, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 4097)


def state_floats(n: int) -> int:
    """[exp_avg | exp_avg_sq | step | 2 reserved | one step count per block]."""
    return 2 * n + 3 + (n + CHUNK - 1) // CHUNK


def fp32(x) -> float:
    """``x`` as a float32 carries it, as a Python float."""
    return float(torch.tensor(float(x), dtype=torch.float32))


def group(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, maximize=False, grad_scale=1.0) -> dict:
    return dict(lr=lr, betas=(betas[0], betas[1]), eps=eps, weight_decay=weight_decay, maximize=bool(maximize), grad_scale=grad_scale)


def as_launched(g: dict) -> dict:
    return group(fp32(g["lr"]), (fp32(g["betas"][0]), fp32(g["betas"][1])), fp32(g["eps"]), fp32(g["weight_decay"]), g["maximize"],
                 fp32(g["grad_scale"]))


class State:
    """exp_avg, exp_avg_sq (float64, the parameter's shape) and the step count of one tensor."""

    def __init__(self, shape, exp_avg=None, exp_avg_sq=None, step=0):
        self.exp_avg = torch.zeros(shape, dtype=torch.float64) if exp_avg is None else exp_avg.detach().cpu().double().clone()
        self.exp_avg_sq = torch.zeros(shape, dtype=torch.float64) if exp_avg_sq is None else exp_avg_sq.detach().cpu().double().clone()
        self.step = int(step)


def step(entries, groups, states, active=None) -> None:
    """One AdamW step in float64, in place.  ``entries``: ``(param, grad or None, group index)`` per tensor, ``param`` a float64
    tensor; ``groups``: list of ``group()`` dicts; ``states``: one ``State`` per entry; ``active``: None or one number per entry."""
    for i, (p, g, gi) in enumerate(entries):
        if g is None or (active is not None and float(active[i]) == 0.0):
            continue
        G, st = groups[gi], states[i]
        lr, (b1, b2) = float(G["lr"]), G["betas"]
        g = g.detach().double() * float(G["grad_scale"])
        if G["maximize"]:
            g = -g
        st.step += 1
        t = st.step
        p.sub_(p * (lr * float(G["weight_decay"])))
        st.exp_avg.mul_(b1).add_(g * (1.0 - b1))
        st.exp_avg_sq.mul_(b2).add_(g * g * (1.0 - b2))
        m_hat = st.exp_avg / (1.0 - b1 ** t)
        v_hat = st.exp_avg_sq / (1.0 - b2 ** t)
        p.sub_(lr * m_hat / (v_hat.sqrt() + float(G["eps"])))


# -------------------------------------------------------------------------------------- hyper-parameters --
# the edges, each run on a small table with one 1025-element tensor (weight decay 0.5 at lr 1e-2 halves nothing: 0.5 % per step)
HYPER_EDGES = {
    "beta1_0": group(lr=2e-3, betas=(0.0, 0.999)),
    "beta2_0": group(lr=2e-3, betas=(0.9, 0.0)),
    "weight_decay_0": group(lr=2e-3, weight_decay=0.0),
    "weight_decay_half": group(lr=1e-2, weight_decay=0.5),
    "grad_scale_third": group(lr=2e-3, grad_scale=1.0 / 3.0),
    "eps_1e-3": group(lr=2e-3, eps=1e-3),
    "lr_0_weight_decay_0": group(lr=0.0, weight_decay=0.0),
}
# four groups, pairwise different in every field (the first one's lr is the one a test holds in a device tensor and refills)
FOUR_GROUPS = [
    group(lr=3e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, maximize=False, grad_scale=1.0),
    group(lr=1e-3, betas=(0.8, 0.99), eps=1e-6, weight_decay=0.05, maximize=True, grad_scale=0.5),
    group(lr=5e-4, betas=(0.5, 0.9), eps=1e-4, weight_decay=0.2, maximize=False, grad_scale=1.0 / 3.0),
    group(lr=2e-2, betas=(0.95, 0.95), eps=1e-5, weight_decay=0.01, maximize=True, grad_scale=0.1),
]
DEVICE_LR = (3e-3, 3e-3, 2e-3, 2e-3, 1e-3, 5e-4, 5e-4, 0.0, 4e-3, 4e-3, 1e-3, 1e-3)      # group 0's lr, step by step


def four_groups_at(s: int):
    """FOUR_GROUPS with group 0's learning rate of step ``s`` (the scheduler's refill)."""
    return [dict(FOUR_GROUPS[0], lr=DEVICE_LR[s % len(DEVICE_LR)])] + FOUR_GROUPS[1:]


def launched(groups):
    """``groups`` (a list or ``step -> list``) with every group rounded as the launch carries it."""
    if callable(groups):
        return lambda s: [as_launched(G) for G in groups(s)]
    return [as_launched(G) for G in groups]


def table_sizes(n_tensors: int, big_even: bool = True):
    """A table of ``n_tensors`` tensors of 1 .. 5 elements, with a multi-block tensor at each of positions 0, 79, 80, 159, 160 that
    exists: 2049 (three blocks) at the even ones, 1025 (two) at the odd ones -- uneven block counts on both sides of a launch boundary
    (``big_even=False``: the other way round)."""
    sizes = [1 + (7 * i) % 5 for i in range(n_tensors)]
    for pos in (0, 79, 80, 159, 160):
        if pos < n_tensors:
            sizes[pos] = 2049 if (pos % 2 == 0) == big_even else 1025
    return sizes


# ------------------------------------------------------------------------------------------------ inputs --
def make_params(sizes, seed):
    """float32 CPU tensors of ``sizes`` elements, N(0, 1); every fifth tensor a thousand times smaller."""
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(n, generator=g) * (1e-3 if i % 5 == 4 else 1.0) for i, n in enumerate(sizes)]


def make_grads(sizes, steps, seed):
    """``[step][tensor]`` float32 gradients: N(0, 1) times 10^e, e cycling through -6 .. 3 over steps and tensors; the middle element of
    a tensor of three or more is zero on every step (both moments stay zero: the update is 0 / eps), the first one of two or more on
    every other step."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for s in range(steps):
        row = []
        for i, n in enumerate(sizes):
            t = torch.randn(n, generator=g) * (10.0 ** ((3 * s + i) % 10 - 6))
            if n >= 3:
                t[n // 2] = 0.0
            if s % 2 and n >= 2:
                t[0] = 0.0
            row.append(t)
        out.append(row)
    return out


def make_moments(sizes, seed):
    """Non-trivial moments of a resumed state: exp_avg N(0, 1e-2), exp_avg_sq its square-scale, positive."""
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(n, generator=g) * 1e-2, torch.rand(n, generator=g) * 1e-3 + 1e-6) for n in sizes]


# -------------------------------------------------------------------------------------------- trajectories --
def _groups_at(groups, s):
    return groups(s) if callable(groups) else groups


def run_f64(params0, group_of, groups, grads, active=None, state0=None, snapshots=False):
    """The float64 trajectory.  ``groups``: a list of group dicts or ``step -> list``; ``grads``: ``[step][tensor]``, None allowed;
    ``active``: None or ``[step][tensor]``; ``state0``: None or ``(exp_avg, exp_avg_sq, step)`` per tensor.  Returns ``(params,
    states)``, or with ``snapshots`` the list of ``(params, states)`` copies after every step."""
    ps = [p.detach().cpu().double().clone() for p in params0]
    sts = [State(p.shape) if state0 is None else State(p.shape, *state0[i]) for i, p in enumerate(ps)]
    snaps = []
    for s, row in enumerate(grads):
        step([(p, g, gi) for p, g, gi in zip(ps, row, group_of)], _groups_at(groups, s), sts, None if active is None else active[s])
        if snapshots:
            snaps.append(([p.clone() for p in ps], [State(p.shape, st.exp_avg, st.exp_avg_sq, st.step) for p, st in zip(ps, sts)]))
    return snaps if snapshots else (ps, sts)


def run_torch(params0, group_of, groups, grads, active=None, state0=None, dtype=torch.float32):
    """The same trajectory through ``torch.optim.AdamW(foreach=False, fused=False)`` on CPU tensors of ``dtype``; the gradient scale
    is applied to the gradient it is handed (in ``dtype``), a skipped tensor's gradient is None.  Returns ``(params, states)``."""
    ps = [torch.nn.Parameter(p.detach().cpu().to(dtype).clone()) for p in params0]
    g0 = _groups_at(groups, 0)
    opt = torch.optim.AdamW([dict(params=[p for p, gi in zip(ps, group_of) if gi == k], lr=float(G["lr"]), betas=G["betas"], eps=G["eps"],
                                  weight_decay=G["weight_decay"], maximize=G["maximize"]) for k, G in enumerate(g0)],
                            foreach=False, fused=False)
    if state0 is not None:
        for p, (m, v, t) in zip(ps, state0):
            opt.state[p] = dict(step=torch.tensor(float(t)), exp_avg=m.detach().cpu().to(dtype).clone().view_as(p),
                                exp_avg_sq=v.detach().cpu().to(dtype).clone().view_as(p))
    for s, row in enumerate(grads):
        Gs = _groups_at(groups, s)
        for k, G in enumerate(Gs):
            opt.param_groups[k]["lr"] = float(G["lr"])
        for i, (p, g, gi) in enumerate(zip(ps, row, group_of)):
            skip = g is None or (active is not None and float(active[s][i]) == 0.0)
            p.grad = None if skip else g.detach().cpu().to(dtype) * float(Gs[gi]["grad_scale"])
        opt.step()
    sts = []
    for p in ps:
        st = opt.state.get(p)
        sts.append(State(p.shape) if not st else State(p.shape, st["exp_avg"], st["exp_avg_sq"], int(st["step"])))
    return [p.detach() for p in ps], sts


def quantities(params, states) -> dict:
    """``{"param[i:n]": tensor, "exp_avg[i:n]": ..., "exp_avg_sq[i:n]": ...}`` of a CPU trajectory, the names ``check`` compares by."""
    out = {}
    for i, (p, st) in enumerate(zip(params, states)):
        n = p.numel()
        out[f"param[{i}:{n}]"], out[f"exp_avg[{i}:{n}]"], out[f"exp_avg_sq[{i}:{n}]"] = p, st.exp_avg, st.exp_avg_sq
    return out


def check(got, f32, f64, tag, names=None):
    """Every tensor of ``got`` (name -> build tensor) against the bound above; returns the number checked."""
    rows = []
    for nm in (names if names is not None else list(got)):
        ref = f64[nm].detach().cpu().double().reshape(-1)
        g = got[nm].detach().cpu().double().reshape(-1)
        assert g.shape == ref.shape and bool(torch.isfinite(g).all()), (tag, nm)
        e_b = float((g - ref).abs().max())
        e_32 = float((f32[nm].detach().cpu().double().reshape(-1) - ref).abs().max())
        rows.append((nm, e_b, e_32, float(ref.abs().max())))
    path = os.environ.get("MKGNN_F64_RECORD")
    if path:
        with open(path, "a") as f:
            for nm, e_b, e_32, m in rows:
                f.write(json.dumps({"tag": tag, "name": nm, "build": e_b, "fp32": e_32, "max": m}) + "\n")
    bad = [(nm, e_b, e_32, m) for nm, e_b, e_32, m in rows if not e_b <= C * e_32 + R * max(m, FLOOR)]
    assert not bad, (tag, len(bad), bad[:6])
    return len(rows)


def bias_corrections_fp32(betas, t):
    """(1 - beta1^t, 1 - beta2^t) rounded to float32: both are exactly 1 once beta^t < 2^-25."""
    return fp32(1.0 - math.pow(betas[0], t)), fp32(1.0 - math.pow(betas[1], t))
