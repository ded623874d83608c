"""The float64 leg of the clipped optimiser step (``mkgnn_adamw_step_clipped``): the global norm, ``clip_grad_norm_``'s coefficient
and the skip rule written from their definition on the CPU, on top of ``tests/_adamw_f64.py`` (which is used as it stands), and the
float32 yardstick ``clip_grad_norm_(foreach=False)`` + ``torch.optim.AdamW(foreach=False, fused=False)``.  Nothing here imports the
package under test; ``tests/test_clip_cpu.py`` pins this module to ``torch.nn.utils.clip_grad_norm_`` run in float64.

A tensor is *stepped* when its gradient is not ``None`` and its active flag is not 0.  For a stepped tensor::

    gg   = fl32(+-g * grad_scale)                  element by element: maximize's sign, then the group's scale, in float32
    S    = sum gg^2                                over all elements of all stepped tensors of the whole table, in float64
    norm = sqrt(S)                                 non-finite if and only if some gg is
    coef = fl32(min(1, max_norm / (norm + 1e-6)))  evaluated in double, a NaN kept: clip_grad_norm_'s formula

and the update is ``_adamw_f64.step`` on the gradients ``g * coef``.  With ``skip_nonfinite`` a step whose norm is not finite does
not happen: nothing changes, no step count advances, the skip count goes up by one.  Without it a non-finite norm does what torch
does: ``inf`` gives ``coef = 0`` (an ``inf`` element times 0 is NaN, every other one 0), NaN gives ``coef = NaN``.

``max_norm`` travels as a float32, like the hyper-parameters of a group (``_adamw_f64.as_launched``): callers pass ``A.fp32(m)``.
"""
from __future__ import annotations

import math

import torch

from tests import _adamw_f64 as A


def _stepped(row, active_row):
    return [g is not None and (active_row is None or float(active_row[i]) != 0.0) for i, g in enumerate(row)]


def scaled_fp32(g, G) -> torch.Tensor:
    """``gg``: the float32 value the launch forms from a float32 gradient -- the sign of ``maximize``, then ``grad_scale``."""
    g = g.detach().cpu().float()
    return (-g if G["maximize"] else g) * torch.tensor(A.fp32(G["grad_scale"]), dtype=torch.float32)


def sum_of_squares(row, group_of, groups, active_row=None) -> float:
    """``S`` of one step, in float64.  A non-finite ``gg`` makes it non-finite (``inf`` or NaN)."""
    S = 0.0
    for on, g, gi in zip(_stepped(row, active_row), row, group_of):
        if on:
            S += float(scaled_fp32(g, groups[gi]).double().square().sum())
    return S


def norm_and_coef(row, group_of, groups, max_norm, active_row=None):
    """``(norm, coef)`` as Python floats: ``norm`` in double, ``coef`` rounded to float32."""
    S = sum_of_squares(row, group_of, groups, active_row)
    norm = math.sqrt(S)
    r = float(max_norm) / (norm + 1e-6)                    # (inf / inf is NaN, as in torch)
    coef = r if (r != r or r < 1.0) else 1.0              # min(1, r) that keeps a NaN
    return norm, A.fp32(coef)


def is_skipped(norm: float, skip_nonfinite: bool) -> bool:
    return bool(skip_nonfinite) and not math.isfinite(norm)


def clipped_row(row, coef: float):
    """The gradients of one step times ``coef`` (float64; ``None`` stays ``None``).  ``inf * 0`` and anything times NaN are NaN."""
    return [None if g is None else g.detach().cpu().double() * coef for g in row]


def run_f64(params0, group_of, groups, grads, max_norm, skip_nonfinite=False, active=None, state0=None, snapshots=False):
    """The float64 trajectory of the clipped step.  Arguments as ``_adamw_f64.run_f64``, ``groups`` as launched (float32 values).
    Returns ``(params, states, stats)`` with ``stats`` a list of ``(norm, coef, skipped so far)`` per step; with ``snapshots`` the
    list of ``(params, states)`` copies after every step comes fourth."""
    ps = [p.detach().cpu().double().clone() for p in params0]
    sts = [A.State(p.shape) if state0 is None else A.State(p.shape, *state0[i]) for i, p in enumerate(ps)]
    stats, snaps, skipped = [], [], 0
    for s, row in enumerate(grads):
        Gs = groups(s) if callable(groups) else groups
        act = None if active is None else active[s]
        norm, coef = norm_and_coef(row, group_of, Gs, max_norm, act)
        if is_skipped(norm, skip_nonfinite):
            skipped += 1
        else:
            A.step([(p, g, gi) for p, g, gi in zip(ps, clipped_row(row, coef), group_of)], Gs, sts, act)
        stats.append((norm, coef, skipped))
        if snapshots:
            snaps.append(([p.clone() for p in ps], [A.State(p.shape, st.exp_avg, st.exp_avg_sq, st.step) for p, st in zip(ps, sts)]))
    return (ps, sts, stats, snaps) if snapshots else (ps, sts, stats)


def run_torch(params0, group_of, groups, grads, max_norm, skip_nonfinite=False, active=None, state0=None, dtype=torch.float32):
    """The yardstick: per step the scaled, signed gradients are handed to ``clip_grad_norm_(foreach=False)`` and then to
    ``torch.optim.AdamW(foreach=False, fused=False)`` (whose ``maximize`` is therefore left off: the sign is already in), all in
    ``dtype`` on the CPU.  A skipped step is simply not made.  Returns ``(params, states, norms)``, ``norms`` what
    ``clip_grad_norm_`` returned per step."""
    ps = [torch.nn.Parameter(p.detach().cpu().to(dtype).clone()) for p in params0]
    g0 = groups(0) if callable(groups) else groups
    opt = torch.optim.AdamW([dict(params=[p for p, gi in zip(ps, group_of) if gi == k], lr=float(G["lr"]), betas=G["betas"], eps=G["eps"],
                                  weight_decay=G["weight_decay"], maximize=False) for k, G in enumerate(g0)], foreach=False, fused=False)
    if state0 is not None:
        for p, (m, v, t) in zip(ps, state0):
            opt.state[p] = dict(step=torch.tensor(float(t)), exp_avg=m.detach().cpu().to(dtype).clone().view_as(p),
                                exp_avg_sq=v.detach().cpu().to(dtype).clone().view_as(p))
    norms = []
    for s, row in enumerate(grads):
        Gs = groups(s) if callable(groups) else groups
        for k, G in enumerate(Gs):
            opt.param_groups[k]["lr"] = float(G["lr"])
        on = _stepped(row, None if active is None else active[s])
        for p, g, gi, o in zip(ps, row, group_of, on):
            if not o:
                p.grad = None
            else:
                gg = g.detach().cpu().to(dtype) * float(Gs[gi]["grad_scale"])
                p.grad = -gg if Gs[gi]["maximize"] else gg
        norm = torch.nn.utils.clip_grad_norm_([p for p in ps if p.grad is not None], float(max_norm), foreach=False)
        norms.append(float(norm))
        if not is_skipped(float(norm), skip_nonfinite):
            opt.step()
    sts = []
    for p in ps:
        st = opt.state.get(p)
        sts.append(A.State(p.shape) if not st else A.State(p.shape, st["exp_avg"], st["exp_avg_sq"], int(st["step"])))
    return [p.detach() for p in ps], sts, norms


def ulps_apart(a: float, b: float) -> int:
    """How many float32 values lie between the float32 roundings of ``a`` and ``b`` (0: equal; both NaN: 0)."""
    ta, tb = torch.tensor(float(a), dtype=torch.float32), torch.tensor(float(b), dtype=torch.float32)
    if bool(torch.isnan(ta)) or bool(torch.isnan(tb)):
        return 0 if bool(torch.isnan(ta)) and bool(torch.isnan(tb)) else 1 << 30
    ia, ib = int(ta.view(torch.int32)), int(tb.view(torch.int32))
    ia = ia if ia >= 0 else -(ia & 0x7FFFFFFF)
    ib = ib if ib >= 0 else -(ib & 0x7FFFFFFF)
    return abs(ia - ib)
