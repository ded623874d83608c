"""The float64 leg of the kernel convolution: the per-element gradient bound (shared with tests/test_scale_parity.py) and the case
table, builder and runner of the any-shape kernels' tests (tests/test_conv_anyshape_cpu.py, tests/test_conv_anyshape_f64.py).

The any-shape kernels (csrc/kgnn_generic.hip: ``kc_forward_generic``, ``kc_backward_rows``, ``kc_backward_bank``,
``kc_backward_bank_reduce``, ``kc_backward_gather``; csrc/kgnn_prepare.h: ``bank_prepare_task``) branch on the row width F, the
bond width E, the kernel counts and the atoms per degree bucket.  ``CASES`` names one case per side of every such branch; each
carries a predicate over ``(F, E, counts, atoms per degree, last layer)`` that proves it reaches its edge, asserted by the CPU
module.  Nothing here needs a GPU: a case is built on the CPU (``build``), and ``run_build`` is what the GPU module calls.
"""
from __future__ import annotations

import copy
import functools
import json
import os
from dataclasses import dataclass
from types import SimpleNamespace
from typing import Callable, Optional, Tuple

import torch

from oracle import kgnn_oracle as O
from tests import _f64
from tests import _topologies as T

# unit roundoff of fp32 times a small constant: what separates summation / rounding noise from a wrong term when the
# tolerance of a gradient element is its own sum of absolute terms (oracle.kernelset_gradients_f64)
F64_BOUND = 32 * 2.0 ** -24


def _check_gradients_f64(gx, grads, oracle, tag, bound=F64_BOUND, expect=24):
    """Every gradient against the float64 closed-form oracle, element by element within ``bound * sum |terms|`` of it
    (+ a denormal-sized floor): no global absolute or relative slack.  ``expect``: how many parameter gradients the oracle
    has (4 degrees x (3 kernel tensors + 3 score weights); a degree without atoms or without kernels has none, and the
    build must not have one either)."""
    gx_o, grads_o, gx_abs, grads_abs = oracle
    lim = bound * gx_abs + 1e-30
    err = (gx.double() - gx_o).abs()
    assert bool((err <= lim).all()), (tag, "grad_x", float((err / lim).max()), float(err.max()))
    worst = float((err / lim).max())
    checked = 0
    for name, ref in grads_o.items():
        if ref is None:
            assert name not in grads or name.endswith("p_support"), name
            continue
        assert name in grads, name
        got = grads[name].double().reshape(ref.shape)
        lim = bound * grads_abs[name] + 1e-30
        err = (got - ref).abs()
        assert bool((err <= lim).all()), (tag, name, float((err / lim).max()), float(err.max()), float(ref.abs().max()))
        worst = max(worst, float((err / lim).max()))
        checked += 1
    assert checked == expect, checked
    return worst


def worst_by_group(gx, grads, oracle, bound=F64_BOUND):
    """Measurement only: the worst ``err / lim`` of the x-gradient (rows + gather kernels), of the kernel-row gradients (bank +
    reduce kernels) and of the score weights (the bank kernel's partials + the reduce's tree), as ``_check_gradients_f64`` forms it."""
    gx_o, grads_o, gx_abs, grads_abs = oracle
    out = {"grad_x": float(((gx.double() - gx_o).abs() / (bound * gx_abs + 1e-30)).max()) if gx.numel() else 0.0,
           "bank": 0.0, "score_weights": 0.0}
    for name, ref in grads_o.items():
        if ref is None or name not in grads:
            continue
        r = float(((grads[name].double().reshape(ref.shape) - ref).abs() / (bound * grads_abs[name] + 1e-30)).max())
        grp = "score_weights" if name.endswith("sc_weight") else "bank"
        out[grp] = max(out[grp], r)
    return out


def record(row: dict) -> None:
    """With ``MKGNN_F64_RECORD=<file>``: one JSON line per measurement (the file ``tests/_f64.check`` appends to)."""
    path = os.environ.get("MKGNN_F64_RECORD")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(row) + "\n")


# ------------------------------------------------------------------------------------------------ the case table --
# constants of the kernels the predicates mirror (csrc/kgnn_generic.hip, kgnn_prepare.h, kgnn_common.h, kgnn_launch.h)
WAVE = 64                   # columns / kernels / bond columns a wave takes per pass
BANK_THREADS = 128          # kc_backward_bank: threads over a row and over L; bank_prepare_task's register path; the gather's half row
STREAM_MAX_F = 160          # bank_pitch(F) == 0 above: no padded copy, no streamed kernel
PART_WIDTH = 256            # kc_backward_bank_reduce: part[8][256]
UNIT_BOND_MAX = 8           # the 8-float bond copy and the unit bond rows exist for E <= 8
BANK_CHUNKS = 256           # nchunk = min(n_d, 256)
GRID_WAVES = 4096 * 4       # grid_for_waves: at most 4096 blocks of 4 waves
CLAMP_MARGIN = 100.0        # a clamped row's norm is this factor away from the epsilon, on either side


def _base():
    """A handful of molecules with atoms of all four degrees (46 atoms)."""
    return [T.tree(14), T.chain(5), T.star(4), T.star(3), T.tree(9, ring=False), T.chain(3), T.pair()]


def _stars(k):
    return lambda: [T.star(4)] * k


def _base_and_stars():
    return _base() + [T.star(4)] * 3


def _grid():
    return [T.chain(300)] * 60 + [T.circulant(128)] * 129


@dataclass(frozen=True)
class Case:
    name: str
    edge: str
    F: int
    E: int
    counts: Tuple[int, int, int, int]
    proves: Callable                      # info -> bool: the case reaches its edge
    last: bool = False
    specs: Callable = _base
    tweak: Optional[str] = None           # "clamp" | "chirality"
    bound: float = F64_BOUND              # (a per-case constant would be recorded here, with its measured justification)
    oracle_on_cpu: bool = True            # False: too large for the CPU module; its oracle runs once, in the GPU test


def _all_degrees(i):
    return all(n > 0 for n in i.n)


def _width_proves(F):
    def proves(i):
        side = (F <= WAVE, F <= BANK_THREADS, F <= STREAM_MAX_F, F <= 3 * WAVE, F <= PART_WIDTH, F % 2 == 0)
        return (i.F == F and _all_degrees(i) and all(L > 0 for L in i.counts) and 1 <= F <= PART_WIDTH
                and side == WIDTH_SIDES[F])
    return proves


# which side of (one 64-column pass, the 128-wide register path / half row, bank_pitch, three passes, part[8][256], float2 loads)
# every width is on: written out, so that the table below is seen to hold both sides of each
WIDTH_SIDES = {
    1: (True, True, True, True, True, False), 2: (True, True, True, True, True, True), 3: (True, True, True, True, True, False),
    63: (True, True, True, True, True, False), 64: (True, True, True, True, True, True), 65: (False, True, True, True, True, False),
    127: (False, True, True, True, True, False), 128: (False, True, True, True, True, True),
    129: (False, False, True, True, True, False), 160: (False, False, True, True, True, True),
    161: (False, False, False, True, True, False), 191: (False, False, False, True, True, False),
    192: (False, False, False, True, True, True), 193: (False, False, False, False, True, False),
    255: (False, False, False, False, True, False), 256: (False, False, False, False, True, True),
}


def _cases():
    cs = []
    std = (3, 2, 4, 2)
    for F in WIDTH_SIDES:
        cs.append(Case(f"width_f{F}", "row width", F, 7, std, _width_proves(F)))
    for F in (20, 129):
        for E in (1, 8, 9, 63, 64):
            cs.append(Case(f"bond_e{E}_f{F}", "bond width", F, E, std,
                           (lambda E, F: lambda i: i.E == E and i.F == F and _all_degrees(i)
                            and (E <= UNIT_BOND_MAX) == (E in (1, 8)) and (E < WAVE) == (E != 64))(E, F)))
    for F in (5, 130):
        cs += [
            # l += 64: one pass short of / exactly / one past a wave of kernels, and a bank far below it
            Case(f"counts_63_64_65_6_f{F}", "kernel counts", F, 7, (63, 64, 65, 6),
                 lambda i: _all_degrees(i) and i.counts[0] < WAVE == i.counts[1] < i.counts[2] and i.counts[3] < WAVE),
            # the 128-thread score-weight sum takes a second round; a degree with atoms and no kernels between two that have both
            Case(f"counts_129_1_0_17_f{F}", "kernel counts", F, 7, (129, 1, 0, 17),
                 lambda i: _all_degrees(i) and i.counts[0] > BANK_THREADS and i.counts[2] == 0 and i.counts[1] == 1, last=True),
            # row_start with three empty degrees in front of the only bank
            Case(f"counts_0_0_0_5_f{F}", "kernel counts", F, 7, (0, 0, 0, 5),
                 lambda i: _all_degrees(i) and i.counts[:3] == (0, 0, 0) and i.counts[3] > 0, last=True),
            Case(f"counts_1_1_1_1_f{F}", "kernel counts", F, 7, (1, 1, 1, 1),
                 lambda i: _all_degrees(i) and i.counts == (1, 1, 1, 1)),
        ]
    for L4 in (5, 6, 16, 17):              # ceil(12 L4 / 64) = 1, 2, 3, 4 chirality-table tasks
        cs.append(Case(f"table_l4_{L4}", "kernel counts", 130, 7, (3, 2, 4, L4),
                       (lambda L4: lambda i: i.last and i.n[3] > 0 and i.counts[3] == L4
                        and (12 * L4 + WAVE - 1) // WAVE == {5: 1, 6: 2, 16: 3, 17: 4}[L4])(L4), last=True))
    for N4 in (1, 2, 255, 256, 257):       # nchunk = min(n, 256) and the ranges n c / nchunk; degrees 2 and 3: kernels, no atoms
        cs.append(Case(f"atoms_n4_{N4}", "atoms per bucket", 20, 7, std,
                       (lambda N4: lambda i: i.n == (4 * N4, 0, 0, N4) and all(L > 0 for L in i.counts)
                        and (N4 < BANK_CHUNKS, N4 == BANK_CHUNKS, N4 > BANK_CHUNKS)
                        == {1: (True, False, False), 2: (True, False, False), 255: (True, False, False),
                            256: (False, True, False), 257: (False, False, True)}[N4]
                        and (4 * N4 > BANK_CHUNKS) == (N4 >= 255))(N4),
                       specs=_stars(N4)))
    cs.append(Case("atoms_n4_257_f161", "atoms per bucket", 161, 7, std,
                   lambda i: i.n == (1028, 0, 0, 257) and i.F > STREAM_MAX_F, specs=_stars(257)))
    cs.append(Case("atoms_without_kernels", "atoms per bucket", 20, 7, (3, 0, 4, 2),
                   lambda i: _all_degrees(i) and i.counts[1] == 0 and i.counts[0] > 0 and i.counts[2] > 0))
    cs.append(Case("atoms_without_kernels_f161", "atoms per bucket", 161, 7, (3, 2, 0, 2),
                   lambda i: _all_degrees(i) and i.counts[2] == 0 and i.F > STREAM_MAX_F))
    for last in (False, True):             # more than 4096 x 4 atoms of degree 2 and of degree 4: the grid-stride loops' second round
        cs.append(Case(f"grid_stride_last{int(last)}", "the grid-stride loop", 5, 1, (3, 1, 7, 2),
                       (lambda last: lambda i: i.last == last and i.n[1] == 60 * 298 and i.n[3] == 129 * 128
                        and i.n[1] > GRID_WAVES and i.n[3] > GRID_WAVES and i.n[1] < 2 * GRID_WAVES)(last),
                       last=last, specs=_grid, oracle_on_cpu=False))
    for F in (129, 256):
        cs.append(Case(f"clamp_f{F}", "the clamp", F, 7, std,
                       lambda i: _all_degrees(i) and i.F > BANK_THREADS and i.clamp_ok, tweak="clamp"))
    for F, col in ((65, 64), (129, 128), (256, 128)):
        cs.append(Case(f"chirality_f{F}", "chirality at width", F, 7, (3, 2, 4, 6),
                       (lambda col: lambda i: i.last and i.chir_col >= col and i.chir_ok)(col),
                       last=True, specs=_base_and_stars, tweak="chirality"))
    return cs


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def register(cases):
    """Cases of another table (tests/_conv_families.py) that ``build`` serves too; ``CASES`` -- what the any-shape modules run --
    stays as it is."""
    for c in cases:
        assert BY_NAME.get(c.name, c) is c, c.name
        BY_NAME[c.name] = c


# Which kernels the automatic dispatch gives the cases above at F <= STREAM_MAX_F, as ``mkgnn_debug_conv_dispatch`` answers (read off
# plan_conv_forward / plan_conv_backward, csrc/kgnn_capi.hip; the letters: ``dispatch_string`` below): forward / backward per degree /
# bank_fused, rows_streamed, bank_streamed.  Rows of at most 160 floats, bonds of at most 8 and banks within the streamed kernels'
# tables (<= 64 kernels of degree 4, <= 8 column parts) take the streamed kernels; one degree outside them takes every degree's
# backward off the streamed pair, and past 112 floats (or at an odd width) round 1's kernels take nothing.
_ALL_STREAMED = "SSSS/SSSS/111"
_NOTHING_FAST = "gggg/gggg/000"
AUTO_DISPATCH = {
    **{f"width_f{F}": _ALL_STREAMED for F in (1, 2, 3, 63, 64, 65, 127, 128, 129, 160)},
    **{f"bond_e{E}_f{F}": _ALL_STREAMED for E in (1, 8) for F in (20, 129)},
    **{f"bond_e{E}_f{F}": _NOTHING_FAST for E in (9, 63, 64) for F in (20, 129)},
    # 65 kernels of degree 3 are three column parts: 4 + 2 + 3 + 1 = 10 groups
    "counts_63_64_65_6_f5": _ALL_STREAMED, "counts_63_64_65_6_f130": _ALL_STREAMED,
    # 129 kernels of degree 1: nine column parts, the streamed kernels hold eight; round 1's forward splits them over two waves
    # (five column tiles each); no backward but the any-shape one takes 129 (or an odd width, or 130 floats)
    "counts_129_1_0_17_f5": "LS-S/ggzg/000", "counts_129_1_0_17_f130": "gS-S/ggzg/000",
    "counts_0_0_0_5_f5": "---S/zzzS/111", "counts_0_0_0_5_f130": "---S/zzzS/111",
    "counts_1_1_1_1_f5": _ALL_STREAMED, "counts_1_1_1_1_f130": _ALL_STREAMED,
    **{f"table_l4_{L4}": _ALL_STREAMED for L4 in (5, 6, 16, 17)},
    **{f"atoms_n4_{N4}": "S--S/S--S/111" for N4 in (1, 2, 255, 256, 257)},
    "atoms_without_kernels": "S-SS/SzSS/111",
    "grid_stride_last0": "SS-S/SS-S/111", "grid_stride_last1": "SS-S/SS-S/111",        # (no atom of degree 3)
    "clamp_f129": _ALL_STREAMED, "chirality_f65": _ALL_STREAMED, "chirality_f129": _ALL_STREAMED,
}


def _star_centres(cpu):
    """Positions in the degree-4 bucket of the atoms whose four neighbours are all leaves (the centres of ``star(4)``)."""
    deg = T.degrees(cpu)
    nei = cpu.nei_index_deg4.reshape(-1, 4)
    return [k for k in range(nei.shape[0]) if bool((deg[nei[k]] == 1).all())]


def _tweak_clamp(case, cpu, layer, x, g):
    """SURVEY 8 a-6 at width: rows of norm zero as focal atoms (every one is somebody's neighbour as well), one row of norm
    ~1e-11, and a zero centre, support and bond-support row."""
    zero = [int(cpu.selected_index_deg1[0]), int(cpu.selected_index_deg2[0]), int(cpu.selected_index_deg3[0]),
            int(cpu.selected_index_deg4[0])]
    for r in zero:
        x[r] = 0.0
    tiny = int(cpu.selected_index_deg2[1])
    x[tiny] = 1e-12 * torch.randn(case.F, generator=g)
    with torch.no_grad():
        layer.trainable_kernelconv_set[2].x_center[0].zero_()
        layer.trainable_kernelconv_set[1].x_support[1, 1].zero_()
        layer.trainable_kernelconv_set[3].edge_attr_support[0, 2].zero_()
        # ... and one kernel row of each kind of norm 0.9e-10: clamped, but its unit row is not zero, so that the projection a clamped
        # row must NOT get has a value (a zero row's is zero either way: `clamped` forced false in the reduce went unseen on those)
        for row in (layer.trainable_kernelconv_set[0].x_center[1], layer.trainable_kernelconv_set[2].x_support[2, 0],
                    layer.trainable_kernelconv_set[1].edge_attr_support[0, 1]):
            v = torch.randn(row.shape, generator=g)
            row.copy_(v * (0.9e-10 / float(v.norm())))
    return dict(zero_rows=zero, tiny_row=tiny)


def _tweak_chirality(case, cpu, layer, x, g):
    """Three ``star(4)`` centres in the last layer.  A: neighbours 0 and 1 bit-identical, 2 and 3 differ from them in the last
    column only (an equal pair: sign +1 whatever the geometry).  B: all four rows differ, and only in column ``col`` -- a loop that
    stops short of it sees four equal rows and answers +1.  C: coplanar neighbours (every z equal; small integers, so the triple
    product is exactly zero in any precision and matches no kernel's sign)."""
    F = case.F
    col = {32: 20, 112: 100, 65: 64, 129: 128, 256: 200}[F]
    kA, kB, kC = _star_centres(cpu)[:3]
    nei = cpu.nei_index_deg4.reshape(-1, 4)
    r = torch.randn(F, generator=g)
    for j, dv in enumerate((0.0, 0.0, 1.0, -1.0)):
        x[nei[kA, j]] = r
        x[nei[kA, j], F - 1] += dv
    r = torch.randn(F, generator=g)
    for j, v in enumerate((3.0, -2.0, 1.5, -4.0)):
        x[nei[kB, j]] = r
        x[nei[kB, j], col] = v
    cpu.p_focal_deg4[kC] = torch.tensor([1.0, 2.0, 3.0])
    cpu.nei_p_deg4.reshape(-1, 4, 3)[kC] = torch.tensor([[2.0, 2.0, 3.0], [1.0, 4.0, 3.0], [0.0, 1.0, 3.0], [3.0, 3.0, 3.0]])
    return dict(kA=kA, kB=kB, kC=kC, chir_col=min(col, F - 1))


def _norm_classes(rows):
    """(rows clamped, rows not clamped, every row at least CLAMP_MARGIN away from the epsilon) by float64 norms."""
    nrm = rows.double().reshape(-1, rows.shape[-1]).norm(dim=-1)
    low, high = nrm <= O.EPS / CLAMP_MARGIN, nrm >= O.EPS * CLAMP_MARGIN
    return int(low.sum()), int(high.sum()), bool((low | high).all())


@functools.lru_cache(maxsize=None)
def build(name: str):
    """The case's batch, layer, input rows and cotangent on the CPU (built once per process and shared: nobody modifies them),
    and ``info``: what the case's predicate looks at."""
    from molkgnn_amd.kernels import KernelSetConv
    case = BY_NAME[name]
    seed = 1 + sum(ord(ch) for ch in name)
    cpu = T.batch_of(case.specs(), F=case.F, E=case.E, seed=seed)
    torch.manual_seed(seed)
    layer = KernelSetConv(*case.counts, D=3, node_attr_dim=case.F, edge_attr_dim=case.E)
    if case.E == 1:
        # one bond column: every bond cosine is exactly +-1, and a kernel whose supports differ in sign scores (1 - 1) / 2 = 0 on
        # every atom.  The first kernel of each degree gets supports of one sign, so that no degree's edge-score tensor is zero
        # throughout: tests/_f64.check measures a tensor against its own largest entry, and the half ulp a unit term is off by
        # would otherwise be held to the floor of a tensor that is zero in exact arithmetic (seen on the MI355X: 3e-8 to 6e-8)
        with torch.no_grad():
            for conv in layer.trainable_kernelconv_set:
                if conv.num_kernels:
                    conv.edge_attr_support[0].abs_()
    g = torch.Generator().manual_seed(seed + 7)
    x = cpu.x.clone()
    n = x.shape[0]
    marks = {}
    if case.tweak == "clamp":
        marks = _tweak_clamp(case, cpu, layer, x, g)
    elif case.tweak == "chirality":
        marks = _tweak_chirality(case, cpu, layer, x, g)
    cot = torch.randn(n, sum(case.counts), generator=g)
    state = {k: v.detach().clone() for k, v in layer.state_dict().items()}
    info = SimpleNamespace(F=case.F, E=case.E, counts=tuple(case.counts), last=case.last,
                           n=tuple(int(getattr(cpu, f"selected_index_deg{d}").numel()) for d in range(1, 5)), **marks)
    assert sum(info.n) == n, "an atom of degree 0 or above 4"
    # every row that is normalised anywhere: clamped by a wide margin, or not clamped by a wide margin -- the fp32 flag
    # (inv >= 1 / MKGNN_EPS) and the float64 oracle's (nrm >= EPS) then agree by construction
    rows = [x] + [state[k] for k in state if k.endswith(("x_center", "x_support", "edge_attr_support"))] + \
           [getattr(cpu, f"nei_edge_attr_deg{d}") for d in range(1, 5)]
    classes = [_norm_classes(r) for r in rows if r.numel()]
    info.clamped_rows = sum(c[0] for c in classes)
    info.margins_ok = all(c[2] for c in classes)
    if case.tweak == "clamp":
        per = O.kernelset_params(state)
        low = lambda d, k: _norm_classes(per[d - 1][k])[0]
        tiny_kernel_rows = [per[0]["x_center"][1], per[2]["x_support"][2, 0], per[1]["edge_attr_support"][0, 1]]
        info.clamp_ok = (info.margins_ok and _norm_classes(x)[0] == 5
                         and (low(3, "x_center"), low(1, "x_center"), low(2, "x_support"), low(3, "x_support"),
                              low(4, "edge_attr_support"), low(2, "edge_attr_support")) == (1, 1, 1, 1, 1, 1)
                         and all(5e-11 < float(r.double().norm()) <= O.EPS / CLAMP_MARGIN for r in tiny_kernel_rows)
                         and 1e-12 < float(x[marks["tiny_row"]].double().norm()) < 1e-10)
    if case.tweak == "chirality":
        nei = cpu.nei_index_deg4.reshape(-1, 4)
        xa, xb = x[nei[marks["kA"]]], x[nei[marks["kB"]]]
        differ_b = (xb.unsqueeze(0) != xb.unsqueeze(1)).any(0).any(0)                      # columns in which any two rows of B differ
        pairs_b = all(not torch.equal(xb[i], xb[j]) for i in range(4) for j in range(i + 1, 4))
        idx = oracle_choices(SimpleNamespace(case=case, cpu=cpu, state=state, x=x))
        p_rel = cpu.nei_p_deg4 - cpu.p_focal_deg4.unsqueeze(1)
        sign = O.chirality_sign_vectorised(p_rel.double(), x[cpu.nei_index_deg4].reshape(-1, 4, case.F).double(),
                                           state["trainable_kernelconv_set.3.p_support"].double(), idx[3])
        info.chir_ok = (torch.equal(xa[0], xa[1]) and not torch.equal(xa[0], xa[2]) and not torch.equal(xa[2], xa[3])
                        and torch.equal(xa[0, :case.F - 1], xa[2, :case.F - 1]) and torch.equal(xa[0, :case.F - 1], xa[3, :case.F - 1])
                        and pairs_b and torch.nonzero(differ_b).flatten().tolist() == [marks["chir_col"]]
                        and bool((sign[:, marks["kA"]] == 1).all()) and bool((sign[:, marks["kB"]] == -1).any())
                        and bool((sign[:, marks["kC"]] == -1).all()))
    return SimpleNamespace(case=case, cpu=cpu, layer=layer, state=state, x=x, cot=cot, info=info)


def oracle_choices(built):
    """The fp32 oracle's own permutation choices (argmax of the reference-faithful form), one entry per degree."""
    idx = []
    with torch.no_grad():
        O.kernelsetconv(O.kernelset_params(built.state), built.x, built.cpu, built.case.last, form="faithful", idx_out=idx)
    return idx


def expected_gradients(built) -> int:
    """Parameter gradients the reference has: 6 per degree with atoms and kernels."""
    return 6 * sum(1 for n, L in zip(built.info.n, built.info.counts) if n > 0 and L > 0)


def oracle_gradients_fp32(built, idx):
    """(grad x, {name: gradient}) of the fp32 oracle's autograd at the choices ``idx`` (None gradients left out, as the build's)."""
    _, gx, grads = O.kernelset_gradients(built.state, built.x, built.cpu, built.case.last, built.cot, forced_idx=idx, form="faithful")
    if gx is None:                                       # (no atom with kernels: nothing reaches x)
        gx = torch.zeros_like(built.x)
    return gx, {k: v for k, v in grads.items() if v is not None}


def oracle_gradients_f64(built, idx):
    return O.kernelset_gradients_f64(built.state, built.x, built.cpu, built.case.last, built.cot, idx)


def pair_scores(built, idx, dtype):
    """Per degree ``{"support", "centre", "edge"}: [L_d, N_d]`` (+ ``"chirality"`` in the last layer's degree 4) of the oracle
    evaluated in ``dtype`` at the permutation choices ``idx``: what the kernels keep for backward (``kernelsetconv_details``)."""
    cpu = _f64.batch_as(built.cpu, dtype)
    per = O.kernelset_params({k: v.to(dtype) if v.is_floating_point() else v for k, v in built.state.items()})
    x = built.x.to(dtype)
    out = []
    for d in range(1, 5):
        sel = getattr(cpu, f"selected_index_deg{d}")
        if sel.numel() == 0 or built.info.counts[d - 1] == 0:
            out.append(None)
            continue
        nei = getattr(cpu, f"nei_index_deg{d}")
        with torch.no_grad():
            _, _, _, parts = O.kernelconv_cosmat(per[d - 1], x[sel], getattr(cpu, f"p_focal_deg{d}"), x[nei].reshape(-1, d, x.shape[-1]),
                                                 getattr(cpu, f"nei_p_deg{d}"), getattr(cpu, f"nei_edge_attr_deg{d}"), built.case.last,
                                                 forced_idx=idx[d - 1].long())
        out.append({"support": parts["best"], "centre": parts["center"], "edge": parts["edge"], "chirality": parts["chirality"]})
    return out


# ------------------------------------------------------------------------------------------------------ the runner --
PATHS = (("generic", "generic"), ("auto", "fast"))


def streamed_launches():
    """How often the three streamed kernels (forward, rows gradient, bank gradient) have been launched so far
    (``mkgnn_debug_last_plans``, entries 9..11)."""
    import ctypes
    from molkgnn_amd import _lib
    out = (ctypes.c_int32 * 12)()
    assert _lib.load().mkgnn_debug_last_plans(out) == 0
    return tuple(out[9:12])


def run_build(built, dev, variant, bwd_variant, prepared=None):
    """``_run_build`` of tests/test_scale_parity.py for any (F, E, counts): one forward + backward of the case's layer through
    the C ABI on ``dev``.  Returns a namespace of CPU tensors: ``out``, per degree ``idx`` (permutation ids), ``scores``
    ([3, L_d, N_d]: support, centre, edge) and ``chir`` from ``kernelsetconv_details``, ``gx`` and ``grads`` {name: gradient};
    ``streamed``: by how much the three streamed launch counters advanced; ``backward``: the backward variant that ran
    (``"fast"`` refuses shapes the fast kernels do not cover -- by design; such a case runs ``"auto"``, which takes the same
    kernels wherever ``"fast"`` is allowed and the any-shape ones elsewhere)."""
    from molkgnn_amd import functional as Fn
    from molkgnn_amd.plan import plan_from_data
    case = built.case
    layer = copy.deepcopy(built.layer).to(dev)
    bd = built.cpu.to(dev)
    plan = plan_from_data(bd)
    n, F = built.x.shape
    store = torch.zeros(n, F + (-F) % 4, device=dev)
    store[:, :F] = built.x.to(dev)
    x = store[:, :F].detach().requires_grad_(True)
    params, E = layer._bank_params("train", x)
    if bwd_variant == "fast" and not fast_backward_covers(plan, params, x, E):
        bwd_variant = "auto"
    layer.variant, layer.backward_variant = variant, bwd_variant
    dispatch = dispatch_string(Fn.debug_conv_dispatch(x.detach(), plan, params, E, variant, bwd_variant))
    before = streamed_launches()
    out_d, saved = Fn.kernelsetconv_details(x.detach(), plan, case.last, params, E, variant)
    out = layer._run(x, plan, case.last, prepared=prepared)
    (out * built.cot.to(dev)).sum().backward()
    torch.cuda.synchronize()
    after = streamed_launches()
    grads = {nm: p_.grad.detach().cpu() for nm, p_ in layer.named_parameters() if p_.grad is not None}
    return SimpleNamespace(out=out.detach().cpu(), out_details=out_d.cpu(),
                           idx=[None if s[0] is None else s[0].cpu().long() for s in saved],
                           scores=[None if s[1] is None else s[1].cpu() for s in saved],
                           chir=[None if s[2] is None else s[2].cpu() for s in saved],
                           gx=x.grad.detach().cpu(), grads=grads, streamed=tuple(a - b for a, b in zip(after, before)),
                           backward=bwd_variant, dispatch=dispatch)


FWD_LETTERS = {"skip": "-", "generic": "g", "lds_bank": "L", "streamed": "S"}
BWD_LETTERS = {"skip": "-", "zero_fill": "z", "generic": "g", "lds_pair": "P", "mfma_lds": "M", "streamed": "S"}


def dispatch_string(answer) -> str:
    """``functional.debug_conv_dispatch``'s answer as ``"SSSS/SSSS/111"``: a letter per degree for the forward (``-`` skip, ``g`` the
    any-shape kernel, ``L`` round 1's LDS-bank kernel, ``S`` the streamed kernel) and for the backward (``-`` skip, ``z`` zero fill,
    ``g`` any-shape, ``P`` the per-degree LDS pair, ``M`` MFMA rows + LDS bank kernel, ``S`` the streamed pair), then
    ``bank_fused``, ``rows_streamed``, ``bank_streamed``."""
    fwd, bwd, flags = answer
    return "".join(FWD_LETTERS[f] for f in fwd) + "/" + "".join(BWD_LETTERS[b] for b in bwd) + "/" + "".join(str(int(v)) for v in flags)


def check_streamed_counters(dispatch: str, streamed, tag) -> None:
    """The three streamed launch counters against the dispatch's answer: the forward's advanced iff some degree is ``streamed``,
    the rows kernel's iff ``rows_streamed``, the bank kernel's iff ``bank_streamed``."""
    fwd, _, flags = dispatch.split("/")
    assert (streamed[0] > 0) == ("S" in fwd), (tag, dispatch, streamed)
    assert (streamed[1] > 0) == (flags[1] == "1"), (tag, dispatch, streamed)
    assert (streamed[2] > 0) == (flags[2] == "1"), (tag, dispatch, streamed)


def own_block_mask(built):
    """[N, K] bool: column k belongs to the degree block of atom n."""
    n, K = built.cot.shape
    own = torch.zeros(n, K, dtype=torch.bool)
    off = 0
    for d in range(1, 5):
        L = built.info.counts[d - 1]
        own[getattr(built.cpu, f"selected_index_deg{d}"), off:off + L] = True
        off += L
    return own


def check_against_float64(built, res, tag, oracle=None):
    """What one run of a case (``run_build``'s result) must satisfy, whatever kernels ran -- the body of
    tests/test_conv_anyshape_f64.py::test_case_against_float64, shared with tests/test_conv_families_gpu.py: nothing non-finite,
    both output storages equal, zeros outside an atom's own block, the tie-aware criterion at ``FWD_TOL``, the three scores kept
    for backward through ``tests/_f64.check`` at the build's permutation, chirality signs exactly, every gradient per element
    within ``case.bound * sum |terms|`` of the float64 closed form, no gradient for a degenerate degree, and a tweak's marks.
    ``oracle``: ``oracle_gradients_f64(built, res.idx)`` where the caller has it already.  Returns ``(worst err / lim, oracle)``."""
    from tests.test_scale_parity import FWD_TOL
    case, info = built.case, built.info
    # ---- forward
    assert torch.isfinite(res.out).all() and torch.isfinite(res.gx).all()
    assert torch.equal(res.out, res.out_details)          # (padded and contiguous output storage: the same scores)
    assert bool((res.out[~own_block_mask(built)] == 0).all())
    per_degree = O.kernelset_params(built.state)
    assert O.kernelset_tie_aware_mismatch(per_degree, built.x, built.cpu, case.last, res.out, res.idx, tol=FWD_TOL) == 0
    # ---- the scores kept for backward, at the build's permutation
    s32, s64 = pair_scores(built, res.idx, torch.float32), pair_scores(built, res.idx, torch.float64)
    checked = 0
    for d in range(4):
        active = info.n[d] > 0 and info.counts[d] > 0
        assert (res.scores[d] is not None) == active and (res.idx[d] is not None) == active, (tag, d)
        if not active:
            continue
        names = ("support", "centre", "edge")
        got = {f"deg{d + 1}.{nm}": res.scores[d][k] for k, nm in enumerate(names)}
        checked += _f64.check(got, {f"deg{d + 1}.{nm}": s32[d][nm] for nm in names}, {f"deg{d + 1}.{nm}": s64[d][nm] for nm in names},
                              list(tag) + ["pair scores"])
        if d == 3 and case.last:
            assert torch.equal(res.chir[3].double(), s64[3]["chirality"]), tag
        else:
            assert res.chir[d] is None
    assert checked == 3 * sum(1 for n, L in zip(info.n, info.counts) if n and L)
    if case.tweak == "chirality":
        ch = res.chir[3]
        assert bool((ch[:, info.kA] == 1).all()) and bool((ch[:, info.kB] == -1).any()) and bool((ch[:, info.kC] == -1).all()), tag
    # ---- gradients, per element
    if oracle is None:
        oracle = oracle_gradients_f64(built, res.idx)
    print(tag, "by group:", worst_by_group(res.gx, res.grads, oracle), "streamed launches:", res.streamed, "backward:", res.backward)
    worst = _check_gradients_f64(res.gx, res.grads, oracle, tag, bound=case.bound, expect=expected_gradients(built))
    # ---- degenerate buckets: a degree without atoms, or without kernels, has no gradient at all (not a zero one); atoms without
    # kernels get a row of zeros and an x-gradient from their neighbours only
    for d in range(4):
        if info.n[d] == 0 or info.counts[d] == 0:
            assert not any(k.startswith(f"trainable_kernelconv_set.{d}.") for k in res.grads), (tag, d, sorted(res.grads))
    return worst, oracle


def fast_backward_covers(plan, params, x, E) -> bool:
    """The library's own answer (``mkgnn_backward_streams``): the streamed backward pair covers every degree of this call."""
    from molkgnn_amd import _lib
    from molkgnn_amd import functional as Fn
    banks, _, keep = Fn._banks([p.detach() for p in params], x.shape[1], E)
    buckets = Fn._buckets(plan, E, False)
    with torch.cuda.device(x.device):
        return _lib.load().mkgnn_backward_streams(banks, buckets, x.data_ptr(), Fn._stride0(x), x.shape[0], x.shape[1], E) == 1
