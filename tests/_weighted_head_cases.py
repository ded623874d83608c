"""Inputs, case table and references of the WEIGHTED task-indexed head (``readout.task_head_loss`` / ``readout.head_loss`` with
``sample_weight`` / ``weight_table`` / ``pos_weight`` -> ``mkgnn_task_head_weighted_*``, csrc/kgnn_task_head.hip).  No GPU in this
file: everything is seeded and evaluated on the CPU.

The reference is ``readout.task_head_reference`` with the weight keywords -- the definition, plain torch -- evaluated in float64
(the truth) and in float32 (the yardstick of ``tests/_f64.check``) on the same float32-drawn inputs, once per (case, loss kind,
scale), shared and never written to.  One row of cases per edge, not the product: B around the 16-row block and past the final
kernel's 256 threads, H around the 32 lanes of a row and at the limit, T = 1 without a task vector (``T=None`` below: the
single-task use of the kernels) and 1, 2, 9, 32 with one, the three weight forms (none; per row with exact zeros and one row at
1e3; a permuted table of 2 B entries read through repeated and out-of-range ids), with and without positive weights, and the
hazards (padding rows behind NaN weights and sentinel ids, a padded row stride, no bias, no input gradient, dropout, a
``grad_loss`` that is not 1, a task whose rows all weigh zero, a task whose positive weight is exactly 1).
"""
from __future__ import annotations

import zlib
from dataclasses import dataclass
from functools import lru_cache
from typing import Dict, List, Optional

import torch

from tests import _philox
from tests._task_head_cases import HEAD_ROWS, KINDS, SCALE, SEED, SENTINEL, task_pattern   # noqa: F401  (shared with the unweighted cases)

WEIGHTS = ("none", "row", "table")
BIG = 1e3                 # the one large sample weight of the "row" form
POS_RANGE = (0.5, 40.0)   # positive weights are drawn in here


@dataclass(frozen=True)
class Case:
    name: str
    B: int
    H: int
    T: Optional[int]          # None: no task vector at all (every row has task 0, a one-output head)
    pattern: str
    weights: str = "none"     # one of WEIGHTS
    pos: bool = False         # a positive weight per task ("bce" only)
    pos_one: Optional[int] = None     # this task's positive weight is exactly 1.0
    zero_task: Optional[int] = None   # every row of this task has the sample weight 0
    task_table: bool = False  # the task through task_table[row_ids] too (the SAME ids as the weight table's)
    bias: bool = True
    emb_grad: bool = True
    p: float = 0.0
    n_pad: int = 0
    stride_pad: int = 0       # emb rows of H + stride_pad floats
    scale: bool = False       # also run with grad_loss = SCALE

    @property
    def tasks(self) -> int:
        return 1 if self.T is None else self.T

    @property
    def kinds(self):
        return ("bce",) if self.pos else KINDS


def _rows() -> List[Case]:
    t = [  # (B, H, T, pattern, weights, pos, then keyword hazards)
        (1, 1, None, "all_one", "row", True, {}),
        (15, 5, 2, "round_robin", "row", True, dict(bias=False, p=0.25, n_pad=3, zero_task=1)),
        (16, 31, 9, "sorted", "table", True, dict(emb_grad=False)),
        (17, 32, 32, "round_robin", "row", True, dict(p=0.25)),
        (33, 33, 9, "one_absent", "none", True, dict(pos_one=3)),
        (577, 64, 9, "quarter_unlabelled", "table", True, dict(p=0.25, stride_pad=3, task_table=True, scale=True)),
        (4097, 32, 9, "round_robin", "row", False, {}),
        (4097, 64, None, "all_one", "table", True, dict(p=0.25, n_pad=3)),
        (17, 5, 1, "all_one", "row", False, dict(n_pad=3)),
        (33, 31, 9, "out_of_range", "row", True, dict(zero_task=4)),
        (577, 33, 2, "all_one", "table", False, dict(bias=False, emb_grad=False, scale=True)),
        (16, 64, None, "all_one", "none", True, dict(p=0.25)),
        (15, 32, 32, "sorted", "row", True, dict(stride_pad=3)),
        (33, 1, 32, "quarter_unlabelled", "table", True, dict(n_pad=3)),
        (17, 33, None, "all_one", "row", False, {}),
        (577, 5, 32, "one_absent", "row", False, dict(p=0.25, n_pad=3)),
    ]
    return [Case(f"B{B}xH{H}xT{'none' if T is None else T}_{pat}_{wf}{'_pos' if pos else ''}", B, H, T, pat, wf, pos, **kw)
            for B, H, T, pat, wf, pos, kw in t]


CASES_LIST: List[Case] = _rows()
CASES: Dict[str, Case] = {c.name: c for c in CASES_LIST}
PAIRS = [(c.name, k) for c in CASES_LIST for k in c.kinds]

# BCE with a positive weight at saturated logits: rows 0 .. 5 are task 1 rows whose embedding is +-e_0 or 0; W[1, 0] = 90 and there
# is no bias, so their logits are exactly +90, -90 and 0 (each with target 0 and 1); p_1 = 37.5.  The term at x = -90, y = 1 is
# exactly 90 * 37.5 = 3375, and every gradient is finite
SATURATED = Case("bce_pos_pm90", 21, 5, 3, "round_robin", "none", True, bias=False)
SATURATED_LOGITS = (90.0, 90.0, -90.0, -90.0, 0.0, 0.0)
SATURATED_TARGETS = (0.0, 1.0, 0.0, 1.0, 0.0, 1.0)
SATURATED_TASK = 1
SATURATED_POS = 37.5
SATURATED_ROW = 3             # x = -90, y = 1
SATURATED_TERM = 3375.0


def case(name: str) -> Case:
    return SATURATED if name == SATURATED.name else CASES[name]


def _seed(*parts) -> int:
    return zlib.crc32(repr(parts).encode()) & 0x7FFFFFFF


@lru_cache(maxsize=None)
def inputs(name: str, kind: str) -> Dict[str, object]:
    """float32 CPU inputs of a case.  ``emb`` holds ``B + n_pad`` rows; ``y`` is NaN at every unlabelled row and at the padding
    rows; ``task`` and ``row_ids`` hold ``SENTINEL`` and ``s`` NaN at the padding rows.  ``s``: the per-row weights (None for the
    "none" and the "table" form); ``weight_table`` / ``row_ids``: the table form; ``s_eff [B]``: the weight every row ends up
    with, whatever the form (1 for "none"); ``task_direct``: the task of every row as a vector, also where it is passed through
    ``task_table``."""
    c = case(name)
    g = torch.Generator().manual_seed(_seed("weighted_head", name, kind))
    n, T = c.B + c.n_pad, c.tasks
    emb = torch.randn(n, c.H, generator=g) * 2
    w = torch.randn(T, c.H, generator=g) * c.H ** -0.5
    b = torch.randn(T, generator=g) if c.bias else None
    y = (torch.rand(c.B, generator=g) < 0.3).float() if kind == "bce" else torch.randn(c.B, generator=g) * 1.5 - 8.0
    task = torch.zeros(c.B, dtype=torch.int32) if c.T is None else task_pattern(c.pattern, c.B, T)
    pos = None
    if c.pos:
        pos = POS_RANGE[0] + (POS_RANGE[1] - POS_RANGE[0]) * torch.rand(T, generator=g)
        if c.pos_one is not None:
            pos[c.pos_one] = 1.0
    if name == SATURATED.name:
        w[SATURATED_TASK, 0] = 90.0
        pos[SATURATED_TASK] = SATURATED_POS
        for r, x in enumerate(SATURATED_LOGITS):
            emb[r] = 0.0
            emb[r, 0] = x / 90.0
            y[r] = SATURATED_TARGETS[r]
            task[r] = SATURATED_TASK
    # the weight every row is meant to have: in (0.1, 3), exact zeros, one row at BIG, a whole task at zero
    s_row = 0.1 + 2.9 * torch.rand(c.B, generator=g)
    s_row[torch.arange(c.B) % 5 == 2] = 0.0
    s_row[c.B // 2] = BIG
    if c.zero_task is not None:
        s_row[task == c.zero_task] = 0.0
    pad_i = torch.full((c.n_pad,), SENTINEL, dtype=torch.int32)
    pad_f = torch.full((c.n_pad,), float("nan"))
    s = table = ids = task_table = None
    s_eff = torch.ones(c.B)
    if c.weights == "row":
        s, s_eff = torch.cat([s_row, pad_f]), s_row
    elif c.weights == "table":
        M = 2 * c.B
        perm = torch.randperm(M, generator=g)
        ids = perm[torch.arange(c.B) // 2 * 2].to(torch.int32)    # every id twice (B odd: the last one once)
        table = torch.full((M,), float("nan"))                      # (an entry no id names is never read)
        task_table = torch.full((M,), -1, dtype=torch.int32)
        for r in range(c.B - 1, -1, -1):                            # an id that repeats names one weight and one task: the first row's
            table[ids[r]] = s_row[r]
            task_table[ids[r]] = task[r]
        if c.B >= 8:                                                # ids outside the table: weight +0.0 (and, through a task table, no label)
            ids[3::11] = M + 5
            ids[7::13] = -3
        inside = (ids >= 0) & (ids < M)
        s_eff = torch.where(inside, table[ids.long().clamp(0, M - 1)], torch.zeros(()))
        if c.task_table:
            task = torch.where(inside, task_table[ids.long().clamp(0, M - 1)], torch.full((), -1, dtype=torch.int32))
        ids = torch.cat([ids, pad_i])
    lab = (task >= 0) & (task < T)
    y = torch.where(lab, y, torch.full((), float("nan")))
    return dict(emb=emb, w=w, b=b, y=torch.cat([y, pad_f]), lab=lab, task_direct=torch.cat([task, pad_i]),
                task=None if (c.T is None or c.task_table) else torch.cat([task, pad_i]),
                task_table=task_table if c.task_table else None, row_ids=ids, s=s, weight_table=table, pos=pos, s_eff=s_eff,
                keep=torch.from_numpy(_philox.head_mask(SEED, 0, c.B, c.H, c.p)) if c.p > 0.0 else None)


def weight_keywords(i: Dict[str, object], cast=lambda t: t) -> Dict[str, object]:
    """The weight keywords of ``task_head_reference`` / ``task_head_loss`` for the inputs ``i``."""
    return dict(sample_weight=None if i["s"] is None else cast(i["s"]), pos_weight=None if i["pos"] is None else cast(i["pos"]),
                weight_table=None if i["weight_table"] is None else cast(i["weight_table"]))


def _evaluate(i, c: Case, kind: str, scale: float, dtype) -> Dict[str, torch.Tensor]:
    from molkgnn_amd.readout import task_head_reference
    cast = lambda t: None if t is None else t.detach().clone().to(dtype)
    emb, w, b = cast(i["emb"]).requires_grad_(True), cast(i["w"]).requires_grad_(True), cast(i["b"])
    if b is not None:
        b.requires_grad_(True)
    loss, pred = task_head_reference(emb, w, b, cast(i["y"]), i["task"], kind, cast(i["keep"]), c.B, i["task_table"], i["row_ids"],
                                     **weight_keywords(i, cast))
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
