"""The average of the weights kept by the fused AdamW step (``mkgnn_adamw_step_averaged``), restated from its definition on the CPU:
a float32 leg of separate torch operators that the launch is held to bit for bit, and a float64 leg that
``tests/test_weight_average_cpu.py`` pins to ``torch.optim.swa_utils.AveragedModel`` run in float64.  Nothing here imports the
package under test; ``tests/_adamw_f64.py`` and ``tests/_clip_f64.py`` are used as they stand.

Per tensor: an average ``avg`` (the parameter's shape) and a count ``n`` (``n_averaged``), starting at the parameter and 0.  A step
of the tensor is *taken* when the optimiser steps it at all -- gradient present, active flag not 0, step not skipped by the
guard -- which is when its step count ``t`` advances.  After a taken step that produced ``p_new``::

    t <= start              avg = p_new (a bit copy), n stays 0
    t >  start, n == 0      avg = p_new,              n = 1           (AveragedModel's first update)
    t >  start, n >= 1      avg = avg + fl(w * fl(p_new - avg)), n = n + 1      three rounded operations, no fused multiply-add
                            (w == 1: avg = p_new instead)

    mean:  w = 1 / (n + 1)
    ema:   w = 1 - d,  d = decay,  or with warmup  d = min(decay, (1 + n) / (10 + n))

``w`` is formed in double and, in the float32 leg, rounded once to float32.  ``decay`` travels as a float32: callers pass
``A.fp32(decay)``.  A step that is not taken changes neither ``avg`` nor ``n``.
"""
from __future__ import annotations

import torch

from tests import _adamw_f64 as A

CHUNK = A.CHUNK
MODES = ("ema", "mean")


def average_floats(n: int) -> int:
    """[avg | canonical n_averaged | one n_averaged per block]."""
    return n + 1 + (n + CHUNK - 1) // CHUNK if n >= 1 else 0


def decay_at(decay: float, warmup: bool, n: int) -> float:
    """``d`` of the EMA at count ``n`` (a double)."""
    d = float(decay)
    if warmup:
        d = min(d, (1.0 + n) / (10.0 + n))
    return d


def weight(mode: str, decay: float, warmup: bool, n: int, rounded: bool = True) -> float:
    """``w`` at count ``n >= 1``: in double, and with ``rounded`` as the float32 the launch carries."""
    assert mode in MODES and n >= 1
    w = 1.0 / (n + 1.0) if mode == "mean" else 1.0 - decay_at(decay, warmup, n)
    return A.fp32(w) if rounded else w


def update(avg: torch.Tensor, n: int, p_new: torch.Tensor, t: int, mode: str, decay: float, warmup: bool = False, start: int = 0):
    """One taken step: ``(avg, n)`` after it.  ``avg``'s dtype decides the leg: float32 rounds ``w`` and every operation to float32
    (three separate torch operators), float64 keeps ``w`` as the double it is."""
    p_new = p_new.detach().cpu().to(avg.dtype)
    if t <= start:
        return p_new.clone(), n
    if n == 0:
        return p_new.clone(), 1
    w = weight(mode, decay, warmup, n, rounded=avg.dtype == torch.float32)
    if w == 1.0:
        return p_new.clone(), n + 1
    d = torch.sub(p_new, avg)
    wd = torch.mul(d, torch.tensor(w, dtype=avg.dtype))
    return torch.add(avg, wd), n + 1


def run(params0, snaps, counts, mode: str, decay: float, warmup: bool = False, start: int = 0, dtype=torch.float32):
    """The averages of a trajectory.  ``params0``: the initial parameters; ``snaps[s][i]``: tensor ``i`` after step ``s``;
    ``counts[s][i]``: its step count after step ``s`` (a step was taken when the count advanced).  Returns ``(avgs, ns, history)``,
    ``history[s]`` the ``(avgs, ns)`` after step ``s``."""
    avgs = [p.detach().cpu().to(dtype).clone() for p in params0]
    ns, prev, history = [0] * len(avgs), [0] * len(avgs), []
    for row, cnt in zip(snaps, counts):
        for i, (p, t) in enumerate(zip(row, cnt)):
            t = int(t)
            assert t in (prev[i], prev[i] + 1), (i, t, prev[i])
            if t > prev[i]:
                avgs[i], ns[i] = update(avgs[i], ns[i], p, t, mode, decay, warmup, start)
                prev[i] = t
        history.append(([a.clone() for a in avgs], list(ns)))
    return avgs, ns, history
