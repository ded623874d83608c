"""Inputs, case table and references of the task-indexed head (``readout.task_head_loss`` -> ``mkgnn_task_head_*``,
csrc/kgnn_task_head.hip).  No GPU in this file: everything is seeded and evaluated on the CPU.

The reference is ``readout.task_head_reference`` -- the definition, plain torch -- evaluated in float64 (the truth) and in float32
(the yardstick of ``tests/_f64.check``) on the same float32-drawn inputs, once per (case, loss kind, scale), shared and never
written to.  One row of cases per edge, not the full product: B around the 16-row block and past the final kernel's 256 threads,
H around the 32 lanes of a row and at the limit, T at 1, 2, 9 (the nine-assay panel) and the limit, every task pattern, and the
hazards (padding rows behind sentinels, a padded row stride, no bias, no input gradient, dropout, the ``row_ids`` indirection).
"""
from __future__ import annotations

import zlib
from dataclasses import dataclass
from functools import lru_cache
from typing import Dict, List

import torch

from tests import _philox

HEAD_ROWS = 16            # kgnn_head_terms.h: `constexpr int HEAD_ROWS = 16`
FINAL_THREADS = 256       # task_head_final_kernel: `for (int bk = t; bk < nb; bk += 256)`
MAX_TASKS, MAX_H = 32, 64 # MKGNN_TASK_HEAD_MAX_TASKS; kgnn_task_head.hip `TH_MAX_H`
SEED = 1234               # generator seed of the dropout rows (offset 0): the mask is _philox.head_mask(SEED, 0, B, H, p)
SCALE = 1.7               # a grad_loss that is not 1
SENTINEL = 2 ** 30        # task / row id of the padding rows: never read
KINDS = ("bce", "mse", "mse_sum")
PATTERNS = ("all_one", "round_robin", "sorted", "one_absent", "quarter_unlabelled", "all_unlabelled", "out_of_range")


def task_pattern(pattern: str, B: int, T: int) -> torch.Tensor:
    """int32 ``[B]``: the task of every row."""
    i = torch.arange(B)
    if pattern == "all_one":
        t = torch.full((B,), T - 1)
    elif pattern == "round_robin":
        t = i % T
    elif pattern == "sorted":
        t = torch.sort(i % T).values
    elif pattern == "one_absent":                        # task T // 2 has no row
        t = i % (T - 1)
        t = t + (t >= T // 2).long()
    elif pattern == "quarter_unlabelled":
        t = torch.where(i % 4 == 1, torch.full((B,), -1), i % T)
    elif pattern == "all_unlabelled":
        t = torch.full((B,), -1)
    elif pattern == "out_of_range":                      # T, T + 5 and -7 must behave as -1
        bad = torch.tensor([T, T + 5, -7])[(i // 3) % 3]
        t = torch.where(i % 3 == 0, bad, i % T)
    else:
        raise ValueError(pattern)
    return t.to(torch.int32)


@dataclass(frozen=True)
class Case:
    name: str
    B: int
    H: int
    T: int
    pattern: str
    bias: bool = True
    emb_grad: bool = True
    p: float = 0.0
    n_pad: int = 0
    stride_pad: int = 0       # emb rows of H + stride_pad floats
    row_ids: bool = False     # the task through task_table[row_ids]


def _rows() -> List[Case]:
    t = [  # (B, H, T, pattern, then keyword hazards)
        (1, 1, 1, "all_one", {}),
        (15, 5, 2, "round_robin", dict(bias=False, p=0.25, n_pad=3)),
        (16, 31, 9, "sorted", dict(emb_grad=False)),
        (17, 32, 32, "round_robin", dict(p=0.25)),
        (33, 33, 9, "one_absent", {}),
        (577, 64, 9, "quarter_unlabelled", dict(p=0.25, stride_pad=3)),
        (4097, 32, 9, "round_robin", {}),
        (4097, 64, 32, "quarter_unlabelled", dict(p=0.25, n_pad=3)),
        (17, 5, 2, "all_unlabelled", dict(n_pad=3)),
        (33, 31, 9, "out_of_range", {}),
        (577, 33, 2, "all_one", dict(bias=False, emb_grad=False)),
        (16, 64, 1, "all_one", dict(p=0.25)),
        (15, 32, 32, "sorted", {}),
        (1, 64, 9, "all_one", dict(n_pad=3, stride_pad=3)),
        (33, 1, 32, "quarter_unlabelled", {}),
        (17, 33, 1, "round_robin", dict(stride_pad=3, p=0.25)),
        (577, 5, 32, "one_absent", dict(p=0.25, n_pad=3)),
        (16, 1, 2, "out_of_range", dict(bias=False)),
        (4097, 33, 2, "sorted", dict(emb_grad=False)),
        (33, 32, 9, "round_robin", dict(row_ids=True, p=0.25, stride_pad=3, n_pad=3)),
        (577, 31, 9, "out_of_range", dict(row_ids=True)),
    ]
    return [Case(f"B{B}xH{H}xT{T}_{pat}", B, H, T, pat, **kw) for B, H, T, pat, kw in t]


CASES_LIST: List[Case] = _rows()
CASES: Dict[str, Case] = {c.name: c for c in CASES_LIST}

# BCE at saturated logits: rows 0 .. 5 are task 1 rows whose embedding is +-e_0 or 0; W[1, 0] = 90 and there is no bias, so their
# logits are exactly +90, -90 and 0 (each with target 0 and 1); expf(-x) overflows at x = -90 and 1 / (1 + inf) must come out 0
SATURATED = Case("bce_pm90", 21, 5, 3, "round_robin", bias=False)
SATURATED_LOGITS = (90.0, 90.0, -90.0, -90.0, 0.0, 0.0)
SATURATED_TARGETS = (0.0, 1.0, 0.0, 1.0, 0.0, 1.0)
SATURATED_TASK = 1


def case(name: str) -> Case:
    return SATURATED if name == SATURATED.name else CASES[name]


def _seed(*parts) -> int:
    return zlib.crc32(repr(parts).encode()) & 0x7FFFFFFF


@lru_cache(maxsize=None)
def inputs(name: str, kind: str) -> Dict[str, object]:
    """float32 CPU inputs of a case.  ``emb`` holds ``B + n_pad`` rows; ``y`` is NaN at every unlabelled row and at the padding
    rows; ``task`` (and ``row_ids``) hold ``SENTINEL`` at the padding rows.  With ``row_ids`` the task of row i is
    ``task_table[row_ids[i]]``: a permuted table of 2 B entries read through repeated ids; ``task`` is the same thing directly."""
    c = case(name)
    g = torch.Generator().manual_seed(_seed("task_head", name, kind))
    n = c.B + c.n_pad
    emb = torch.randn(n, c.H, generator=g) * 2
    w = torch.randn(c.T, c.H, generator=g) * c.H ** -0.5
    b = torch.randn(c.T, generator=g) if c.bias else None
    y = (torch.rand(c.B, generator=g) < 0.3).float() if kind == "bce" else torch.randn(c.B, generator=g) * 1.5 - 8.0
    task = task_pattern(c.pattern, c.B, c.T)
    if name == SATURATED.name:
        w[SATURATED_TASK, 0] = 90.0
        for r, x in enumerate(SATURATED_LOGITS):
            emb[r] = 0.0
            emb[r, 0] = x / 90.0
            y[r] = SATURATED_TARGETS[r]
            task[r] = SATURATED_TASK
    lab = (task >= 0) & (task < c.T)
    y = torch.where(lab, y, torch.full((), float("nan")))
    pad_i = torch.full((c.n_pad,), SENTINEL, dtype=torch.int32)
    out = dict(emb=emb, w=w, b=b, y=torch.cat([y, torch.full((c.n_pad,), float("nan"))]), task=torch.cat([task, pad_i]),
               lab=lab, keep=torch.from_numpy(_philox.head_mask(SEED, 0, c.B, c.H, c.p)) if c.p > 0.0 else None,
               task_table=None, row_ids=None)
    if c.row_ids:
        M = 2 * c.B
        perm = torch.randperm(M, generator=g)
        ids = perm[torch.arange(c.B) // 2 * 2]               # every id twice (B odd: the last one once)
        table = torch.full((M,), -1, dtype=torch.int32)
        # an id that repeats must name one task: give the table the task of the FIRST row that uses the id, and make `task` follow
        for r in range(c.B - 1, -1, -1):
            table[ids[r]] = task[r]
        task = table[ids]
        lab = (task >= 0) & (task < c.T)
        yy = (torch.rand(c.B, generator=g) < 0.3).float() if kind == "bce" else torch.randn(c.B, generator=g) * 1.5 - 8.0
        out.update(task=torch.cat([task, pad_i]), lab=lab, task_table=table, row_ids=torch.cat([ids.to(torch.int32), pad_i]),
                   y=torch.cat([torch.where(lab, yy, torch.full((), float("nan"))), torch.full((c.n_pad,), float("nan"))]))
    return out


def _evaluate(i, c: Case, kind: str, scale: float, dtype) -> Dict[str, torch.Tensor]:
    from molkgnn_amd.readout import task_head_reference
    cast = lambda t: None if t is None else t.detach().clone().to(dtype)
    emb, w, b = cast(i["emb"]).requires_grad_(True), cast(i["w"]).requires_grad_(True), cast(i["b"])
    if b is not None:
        b.requires_grad_(True)
    loss, pred = task_head_reference(emb, w, b, cast(i["y"]), i["task"], kind, cast(i["keep"]), c.B)
    (loss * scale).backward()
    res = {"pred": pred.detach(), "loss": loss.detach(), "emb": emb.grad, "w": w.grad.reshape(-1)}
    if b is not None:
        res["b"] = b.grad
    return res


@lru_cache(maxsize=None)
def reference(name: str, kind: str, scale: float = 1.0):
    """(float32 leg, float64 leg): pred [B], loss, and the gradients emb [B + n_pad, H], w [T * H], b [T] of ``scale * loss``."""
    c, i = case(name), inputs(name, kind)
    return _evaluate(i, c, kind, scale, torch.float32), _evaluate(i, c, kind, scale, torch.float64)
