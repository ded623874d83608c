"""Inputs, case table and references of the label-matrix head (``readout.label_head_loss`` -> ``mkgnn_label_head_*``,
csrc/kgnn_label_head.hip).  No GPU in this file: everything is seeded and evaluated on the CPU.

The reference is ``readout.label_head_reference`` -- the definition, plain torch -- evaluated in float64 (the truth) and in float32
(the yardstick of ``tests/_f64.check``) on the same float32-drawn inputs, once per (case, loss kind, scale), shared and never
written to.  One row of cases per edge, not the full product: B around the 16-row block and past the final kernel's 256 threads,
H around the 32 lanes of a row and at the limit, T at 1, 2, 9 (the nine-assay panel), 12 (Tox21) and the limit, every label
pattern, and the hazards (padding rows behind NaN labels / sentinel ids and inf / NaN embeddings, padded row strides of ``emb``,
``labels`` and ``pred``, no bias, no input gradient, dropout, the ``row_ids`` table with repeated and out-of-table ids,
``pos_weight``, sample weights direct and through a table, NaN sample weights on label-less rows).
"""
from __future__ import annotations

import zlib
from dataclasses import dataclass
from functools import lru_cache
from typing import Dict, List

import torch

from tests import _philox

HEAD_ROWS = 16            # kgnn_head_terms.h: `constexpr int HEAD_ROWS = 16`
MAX_TASKS, MAX_H = 32, 64 # MKGNN_TASK_HEAD_MAX_TASKS; kgnn_task_head_final.h `TH_MAX_H`
SEED = 1234               # generator seed of the dropout rows (offset 0): the mask is _philox.head_mask(SEED, 0, B, H, p)
SCALE = 1.7               # a grad_loss that is not 1
SENTINEL = 2 ** 30        # row id of the padding rows: never read
KINDS = ("bce", "mse", "mse_sum")
PATTERNS = ("dense", "one_per_row", "quarter_missing", "task_absent", "row_absent", "all_missing", "single_entry")
NAN = float("nan")


def label_mask(pattern: str, B: int, T: int) -> torch.Tensor:
    """bool ``[B, T]``: which entries are labelled."""
    i, t = torch.arange(B)[:, None], torch.arange(T)[None, :]
    if pattern == "dense":
        m = torch.ones(B, T, dtype=torch.bool)
    elif pattern == "one_per_row":
        m = t == i % T
    elif pattern == "quarter_missing":
        m = (i * 7 + t * 3) % 4 != 1
    elif pattern == "task_absent":                       # column T // 2 is all NaN; the rest three quarters present
        m = ((i * 5 + t) % 4 != 2) & (t != T // 2)
    elif pattern == "row_absent":                        # every fourth row is all NaN
        m = ((i + t) % 3 != 0) & (i % 4 != 1)
    elif pattern == "all_missing":
        m = torch.zeros(B, T, dtype=torch.bool)
    elif pattern == "single_entry":                      # one labelled entry in the whole call: in the last row
        m = (i == B - 1) & (t == T - 1)
    else:
        raise ValueError(pattern)
    return m.expand(B, T).clone()


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
    stride_pad: int = 0       # emb rows of H + stride_pad floats, label and pred rows of T + stride_pad
    row_ids: bool = False     # the labels through label_table[row_ids] (and the sample weights through weight_table[row_ids])
    pos_weight: bool = False  # (bce only: ignored for the squared-error kinds)
    sample_weight: bool = False


def _rows() -> List[Case]:
    t = [  # (B, H, T, pattern, then keyword hazards)
        (1, 1, 1, "dense", {}),
        (15, 5, 2, "quarter_missing", dict(bias=False, p=0.25, n_pad=3)),
        (16, 31, 9, "one_per_row", dict(emb_grad=False)),
        (17, 32, 32, "quarter_missing", dict(p=0.25, pos_weight=True)),
        (33, 33, 9, "task_absent", dict(sample_weight=True)),
        (577, 64, 9, "row_absent", dict(p=0.25, stride_pad=3, sample_weight=True, pos_weight=True)),
        (4097, 32, 12, "quarter_missing", {}),
        (17, 5, 2, "all_missing", dict(n_pad=3, sample_weight=True)),
        (33, 31, 12, "single_entry", {}),
        (577, 33, 2, "dense", dict(bias=False, emb_grad=False)),
        (16, 64, 1, "dense", dict(p=0.25)),
        (15, 32, 32, "one_per_row", dict(stride_pad=3)),
        (1, 64, 9, "task_absent", dict(n_pad=3, stride_pad=3)),
        (33, 1, 32, "row_absent", dict(pos_weight=True)),
        (33, 32, 9, "quarter_missing", dict(row_ids=True, p=0.25, stride_pad=3, n_pad=3, sample_weight=True)),
        (577, 31, 9, "row_absent", dict(row_ids=True, pos_weight=True)),
        (4097, 64, 32, "task_absent", dict(p=0.25, n_pad=3)),
    ]
    return [Case(f"B{B}xH{H}xT{T}_{pat}", B, H, T, pat, **kw) for B, H, T, pat, kw in t]


CASES_LIST: List[Case] = _rows()
CASES: Dict[str, Case] = {c.name: c for c in CASES_LIST}

# BCE at saturated logits: rows 0 .. 5 have an embedding of +-e_0 or 0; W[1, 0] = 90 and there is no bias, so their task-1 logits
# are exactly +90, -90 and 0 (each with label 0 and 1); expf(-x) overflows at x = -90 and 1 / (1 + inf) must come out 0.  Those
# rows carry the task-1 label alone.
SATURATED = Case("bce_pm90", 21, 5, 3, "quarter_missing", bias=False)
SATURATED_LOGITS = (90.0, 90.0, -90.0, -90.0, 0.0, 0.0)
SATURATED_TARGETS = (0.0, 1.0, 0.0, 1.0, 0.0, 1.0)
SATURATED_TASK = 1


def case(name: str) -> Case:
    return SATURATED if name == SATURATED.name else CASES[name]


def _seed(*parts) -> int:
    return zlib.crc32(repr(parts).encode()) & 0x7FFFFFFF


@lru_cache(maxsize=None)
def inputs(name: str, kind: str) -> Dict[str, object]:
    """float32 CPU inputs of a case.  ``emb`` holds ``B + n_pad`` rows, the padding rows filled with inf / NaN; ``labels [B + n_pad,
    T]`` is NaN at every unlabelled entry and at the padding rows; ``sw [B + n_pad]`` (sample weights) is NaN at every row without a
    label and at the padding rows.  With ``row_ids`` the labels of row i are ``label_table[row_ids[i]]`` -- a permuted table of 2 B
    rows read through repeated ids, every eighth id outside the table (``-3`` or ``2 B + 5``: a row without labels), ``SENTINEL`` at
    the padding rows -- and ``weight_table`` holds the weights the same way; ``labels`` / ``sw`` are the same thing directly."""
    c = case(name)
    g = torch.Generator().manual_seed(_seed("label_head", name, kind))
    n = c.B + c.n_pad
    emb = torch.randn(n, c.H, generator=g) * 2
    w = torch.randn(c.T, c.H, generator=g) * c.H ** -0.5
    b = torch.randn(c.T, generator=g) if c.bias else None
    draw = lambda rows: (torch.rand(rows, c.T, generator=g) < 0.3).float() if kind == "bce" \
        else torch.randn(rows, c.T, generator=g) * 1.5 - 8.0
    y = draw(c.B)
    mask = label_mask(c.pattern, c.B, c.T)
    if name == SATURATED.name:
        w[SATURATED_TASK, 0] = 90.0
        for r, x in enumerate(SATURATED_LOGITS):
            emb[r] = 0.0
            emb[r, 0] = x / 90.0
            mask[r] = False
            mask[r, SATURATED_TASK] = True
            y[r, SATURATED_TASK] = SATURATED_TARGETS[r]
    sw = torch.rand(c.B, generator=g) * 1.5 + 0.25
    pw = (torch.rand(c.T, generator=g) * 3 + 0.5) if (c.pos_weight and kind == "bce") else None
    out = dict(w=w, b=b, pw=pw, keep=torch.from_numpy(_philox.head_mask(SEED, 0, c.B, c.H, c.p)) if c.p > 0.0 else None,
               label_table=None, weight_table=None, row_ids=None)
    if c.row_ids:
        M = 2 * c.B
        perm = torch.randperm(M, generator=g)
        ids = perm[torch.arange(c.B) // 2 * 2]               # every id twice (B odd: the last one once)
        outside = torch.arange(c.B) % 8 == 5
        ids = torch.where(outside, torch.where(torch.arange(c.B) % 16 == 5, torch.tensor(-3), torch.tensor(M + 5)), ids)
        full = torch.cat([mask, label_mask(c.pattern, c.B, c.T)])[torch.randperm(M, generator=g)]
        table = torch.where(full, draw(M), torch.full((), NAN))
        wtable = torch.where(full.any(dim=1), torch.rand(M, generator=g) * 1.5 + 0.25, torch.full((), NAN))
        inside = ~outside
        y = torch.where(inside[:, None], table[ids.clamp(0, M - 1)], torch.full((), NAN))
        mask = ~torch.isnan(y)
        sw = torch.where(inside, wtable[ids.clamp(0, M - 1)], torch.zeros(()))
        out.update(label_table=table, weight_table=wtable if c.sample_weight else None,
                   row_ids=torch.cat([ids.to(torch.int32), torch.full((c.n_pad,), SENTINEL, dtype=torch.int32)]))
    labels = torch.where(mask, y, torch.full((), NAN))
    sw = torch.where(mask.any(dim=1), sw, torch.full((), NAN))           # (the weight of a row without labels: never used)
    if c.n_pad:
        emb[c.B:] = torch.tensor([float("inf"), NAN, -float("inf")])[torch.arange(c.n_pad * c.H) % 3].reshape(c.n_pad, c.H)
    out.update(emb=emb, labels=torch.cat([labels, torch.full((c.n_pad, c.T), NAN)]), mask=mask,
               sw=torch.cat([sw, torch.full((c.n_pad,), NAN)]) if c.sample_weight else None)
    return out


def _evaluate(i, c: Case, kind: str, scale: float, dtype) -> Dict[str, torch.Tensor]:
    from molkgnn_amd.readout import label_head_reference
    cast = lambda t: None if t is None else t.detach().clone().to(dtype)
    emb, w, b = cast(i["emb"]).requires_grad_(True), cast(i["w"]).requires_grad_(True), cast(i["b"])
    if b is not None:
        b.requires_grad_(True)
    loss, pred = label_head_reference(emb, w, b, cast(i["labels"]), kind, cast(i["keep"]), c.B, sample_weight=cast(i["sw"]),
                                      pos_weight=cast(i["pw"]))
    (loss * scale).backward()
    res = {"pred": pred.detach(), "loss": loss.detach(), "emb": emb.grad[:c.B], "w": w.grad.reshape(-1)}
    if b is not None:
        res["b"] = b.grad
    return res


@lru_cache(maxsize=None)
def reference(name: str, kind: str, scale: float = 1.0):
    """(float32 leg, float64 leg): pred [B, T], loss, and the gradients emb [B, H], w [T * H], b [T] of ``scale * loss``."""
    c, i = case(name), inputs(name, kind)
    return _evaluate(i, c, kind, scale, torch.float32), _evaluate(i, c, kind, scale, torch.float64)
