"""The convolution's fallback kernel families under their switches: the case table, the settings and the expected dispatch of
tests/test_conv_families_cpu.py and tests/test_conv_families_gpu.py (child: tests/_conv_families_child.py).

Between the streamed kernels and the any-shape ones, ``plan_conv_forward`` / ``plan_conv_backward`` (csrc/kgnn_capi.hip) choose
among round 1's LDS-bank forward (``kc_forward_fused``, kgnn_mfma.hip), the MFMA rows kernel with the LDS bank kernel
(kgnn_bwd_mfma.hip, kgnn_bwd.hip) and the per-degree LDS pair (``kc_backward_rows_lds`` / ``kc_backward_bank_lds``, kgnn_bwd.hip).
They serve the shapes the streamed kernels refuse, and they are the other side of every A/B switch.  ``SETTINGS`` names one
environment per switch (one child process each: the library reads its switches once); ``CASES`` the smallest batches on both
sides of every limit those families have; ``EXPECTED`` what ``mkgnn_debug_conv_dispatch`` must answer for every (setting, case)
-- written down from the plan functions and the ``*_supported`` predicates, not recorded from the library.

Everything else is tests/_conv_f64.py's: ``Case``, ``build`` (the cases are registered there), ``run_build``, the oracles and the
bounds.  Nothing here needs a GPU.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Tuple

from tests import _conv_f64 as C
from tests import _topologies as T

# ---- constants of the kernels the predicates mirror (kernels per degree 1 / 2 / 3 / 4)
PADDED_WIDTHS = (32, 112)               # mfma_padded_width (kgnn_common.h): rows padded to 32 or 112 floats, nothing above 112
LDS_PAIR_MAX_L = (16, 24, 32, 56)       # lds_backward_supported (kgnn_bwd.hip): L <= 8 bank_li(d); even F only
MFMA_ROWS_MAX_L = (12, 20, 32, 52)      # mfma_backward_supported (kgnn_bwd_mfma.hip): L <= 4 bwd_lq(d)
BANK_TILE_ATOMS = (32, 32, 16, 16)      # bank_ta(d): atoms per tile of kc_backward_bank_lds
ROWS_TILE_ATOMS = 32                    # kc_backward_rows_lds: TA
FWD_TILE_ATOMS = 16                     # kc_forward_fused / the MFMA rows kernel: 16-atom tiles
COLUMN_TILE = 16                        # forward column tiles of <= 16 kernels: nct = ceil(L / 16), kpt = ceil(L / nct)
MAX_GROUPS = 16                         # FUSED_MAX_GROUPS (kgnn_launch.h): (degree, column part) groups of one launch
STREAM_TILES_PER_PART = (1, 2, 2, 2)    # stream_tiles_per_part(d): column tiles a streamed column part holds
STREAM_MAX_L4 = 64                      # stream_forward_supported: degree 4's sign table holds 64 kernels
FUSED_WAVES = (2, 2, 1, 1)              # fused_group_count: column tiles resident per block before the 60 KB LDS budget splits further
REF = (10, 20, 30, 50)                  # the reference's kernel counts
STD = (3, 2, 4, 2)

# ---- the settings: one environment each (MKGNN_* otherwise stripped)
SETTINGS = {
    "default": {},
    "fwd_stream0": {"MKGNN_FWD_STREAM": "0"},         # forward: round 1's LDS-bank kernel wherever it covers the shape
    "rows_stream0": {"MKGNN_ROWS_STREAM": "0"},       # backward: MFMA rows + LDS bank kernel per degree, the LDS pair past the MFMA limit
    "bank_stream0": {"MKGNN_BANK_STREAM": "0"},       # backward: the streamed rows launch with the all-degree LDS bank launch
    "no_mfma_bwd": {"MKGNN_NO_MFMA_BWD": "1"},        # backward: the per-degree LDS pair
    "bank_fused0": {"MKGNN_BANK_FUSED": "0"},         # backward: MFMA rows + one LDS bank launch per degree
    "split0": {"MKGNN_FWD_SPLIT": "0", "MKGNN_BWD_SPLIT": "0"},      # the streamed kernels' products in fp32: the same dispatch
}
SETTING_NAMES = tuple(SETTINGS)


def environment(setting: str, base) -> dict:
    """``base`` without any ``MKGNN_*`` entry, plus the setting's switches (as tests/test_dispatch_cpu.py's ``answers`` does)."""
    env = {k: v for k, v in base.items() if not k.startswith("MKGNN_")}
    env.update(SETTINGS[setting])
    return env


# ---- topologies
def cubic(n: int) -> T.Spec:
    """``n`` (even) atoms of degree 3: a ring with every atom bonded to the one opposite."""
    assert n % 2 == 0 and n >= 6
    return n, [(i, (i + 1) % n) for i in range(n)] + [(i, i + n // 2) for i in range(n // 2)]


def _small():
    """Every bucket below one 16-atom tile: 4 / 7 / 6 / 5 atoms of degree 1 / 2 / 3 / 4."""
    return [T.circulant(5), cubic(6), T.chain(6), T.chain(5)]


def _tiles_a():
    """32 / 33 / 16 / 17 atoms of degree 1 / 2 / 3 / 4: 16 chains (2 ends each; 15 x 2 + 3 inner atoms), a cubic ring, a circulant."""
    return [T.chain(4)] * 15 + [T.chain(5), cubic(16), T.circulant(17)]


def _tiles_b():
    """33 / 32 / 17 / 16: 15 chains (30 ends; 14 x 2 + 4 inner atoms), a cubic ring and star(3) (its 3 leaves), a circulant."""
    return [T.chain(4)] * 14 + [T.chain(6), cubic(16), T.star(3), T.circulant(16)]


@dataclass(frozen=True)
class FamilyCase(C.Case):
    no_unit: bool = False                 # the buckets answer no unit bond rows (a C caller that passes none): default setting only


def _all(i):
    return all(n > 0 for n in i.n)


def _padded(F):
    return 32 if F <= 32 else (112 if F <= 112 else 0)


def _width_proves(F):
    def proves(i):
        side = (F <= PADDED_WIDTHS[0], F <= PADDED_WIDTHS[1], F % 2 == 0, F == _padded(F))
        return i.F == F and i.E == 7 and i.counts == STD and _all(i) and side == WIDTH_SIDES[F]
    return proves


# which side of (the 32-float rows, the 112-float rows, even F -- the LDS pair's float2 loads --, no padding column at all) a width is on
WIDTH_SIDES = {
    2: (True, True, True, False), 30: (True, True, True, False), 32: (True, True, True, True), 34: (False, True, True, False),
    110: (False, True, True, False), 112: (False, True, True, True), 27: (True, True, False, False), 111: (False, True, False, False),
    114: (False, False, True, False),
}

# which side of (the MFMA rows limit, the LDS pair's limit) each degree's count is on: (<, ==, >) each
COUNT_SIDES = {
    (12, 20, 32, 52): ("====", "<<=<"), (13, 21, 32, 53): (">>=>", "<<=<"), (16, 24, 32, 56): (">>=>", "===="),
    (17, 25, 33, 57): (">>>>", ">>>>"), REF: ("<=<<", "<<<<"), (10, 0, 30, 50): ("<<<<", "<<<<"),
}


def _cmp(a, b):
    return "<" if a < b else ("=" if a == b else ">")


def _counts_proves(counts, F, last):
    def proves(i):
        return (i.F == F and i.counts == counts and i.last == last and _all(i) and F % 2 == 0 and 0 < _padded(F)
                and COUNT_SIDES[counts] == ("".join(_cmp(L, m) for L, m in zip(counts, MFMA_ROWS_MAX_L)),
                                            "".join(_cmp(L, m) for L, m in zip(counts, LDS_PAIR_MAX_L))))
    return proves


def column_tiles(L):
    """(nct, kpt) of the forward: column tiles of at most 16 kernels."""
    nct = (L + COLUMN_TILE - 1) // COLUMN_TILE
    return nct, (L + nct - 1) // nct


def stream_parts(counts):
    """(degree, column part) groups the streamed launches need: ceil(nct / stream_tiles_per_part(d)) per degree."""
    return [(column_tiles(L)[0] + t - 1) // t if L else 0 for L, t in zip(counts, STREAM_TILES_PER_PART)]


def fused_parts(counts):
    """... and round 1's LDS-bank launch, at widths whose banks fit the LDS budget unsplit: ceil(nct / (2, 2, 1, 1))."""
    return [(column_tiles(L)[0] + w - 1) // w if L else 0 for L, w in zip(counts, FUSED_WAVES)]


def _tile_sides(n):
    """Per degree: atoms against (one forward tile, the bank tile of the degree, the rows tile) as <, =, >."""
    return tuple(_cmp(n[d], FWD_TILE_ATOMS) + _cmp(n[d], BANK_TILE_ATOMS[d]) + _cmp(n[d], ROWS_TILE_ATOMS) for d in range(4))


def _cases():
    cs = []
    for F in WIDTH_SIDES:
        cs.append(FamilyCase(f"fam_width_f{F}", "padded width", F, 7, STD, _width_proves(F)))
    for F in (28, 110):
        for counts in ((12, 20, 32, 52), (13, 21, 32, 53), (16, 24, 32, 56), (17, 25, 33, 57)):
            cs.append(FamilyCase("fam_counts_" + "_".join(map(str, counts)) + f"_f{F}", "backward limits", F, 7, counts,
                                 _counts_proves(counts, F, False)))
        for last in (False, True):
            cs.append(FamilyCase(f"fam_counts_ref_last{int(last)}_f{F}", "backward limits", F, 7, REF, _counts_proves(REF, F, last),
                                 last=last))
        # a degree with atoms and no kernels: zero fill between degrees that run the family
        cs.append(FamilyCase(f"fam_counts_10_0_30_50_f{F}", "backward limits", F, 7, (10, 0, 30, 50),
                             (lambda F: lambda i: i.F == F and i.counts == (10, 0, 30, 50) and _all(i))(F)))
    cs += [
        FamilyCase("fam_tiles_16", "forward column tiles", 28, 7, (16,) * 4,
                   lambda i: _all(i) and all(column_tiles(L) == (1, 16) for L in i.counts)),
        FamilyCase("fam_tiles_17", "forward column tiles", 28, 7, (17,) * 4,
                   lambda i: _all(i) and all(column_tiles(L) == (2, 9) for L in i.counts)),
        # 65 kernels of degree 4: one past the streamed kernels' sign table, and past the LDS pair's 56
        FamilyCase("fam_tiles_l4_65", "forward column tiles", 28, 7, (3, 2, 4, 65),
                   lambda i: _all(i) and i.last and i.counts[3] == STREAM_MAX_L4 + 1 > LDS_PAIR_MAX_L[3] and column_tiles(65) == (5, 13),
                   last=True),
        # 17 streamed groups (7 + 4 + 4 + 2) and 19 of round 1's (4 + 4 + 7 + 4): the demotion rules
        FamilyCase("fam_tiles_17_groups", "forward column tiles", 28, 7, (100, 100, 100, 64),
                   lambda i: _all(i) and stream_parts(i.counts) == [7, 4, 4, 2] and sum(stream_parts(i.counts)) == MAX_GROUPS + 1
                   and fused_parts(i.counts) == [4, 4, 7, 4] and sum(fused_parts(i.counts)) - 7 <= MAX_GROUPS),
        FamilyCase("fam_atoms_small", "atoms per bucket", 28, 7, REF,
                   lambda i: i.n == (4, 7, 6, 5) and i.last and _tile_sides(i.n) == ("<<<",) * 4, last=True, specs=_small),
        FamilyCase("fam_atoms_tiles_a", "atoms per bucket", 28, 7, REF,
                   lambda i: i.n == (32, 33, 16, 17) and i.last and _tile_sides(i.n) == (">==", ">>>", "==<", ">><"),
                   last=True, specs=_tiles_a),
        FamilyCase("fam_atoms_tiles_b", "atoms per bucket", 28, 7, REF,
                   lambda i: i.n == (33, 32, 17, 16) and i.last and _tile_sides(i.n) == (">>>", ">==", ">><", "==<"),
                   last=True, specs=_tiles_b),
    ]
    for E in (1, 8):
        cs.append(FamilyCase(f"fam_bond_e{E}", "bond width", 32, E, STD,
                             (lambda E: lambda i: i.E == E and i.F == 32 and _all(i) and E <= C.UNIT_BOND_MAX)(E)))
    for F in PADDED_WIDTHS:
        cs.append(FamilyCase(f"fam_clamp_f{F}", "the clamp", F, 7, STD,
                             (lambda F: lambda i: _all(i) and i.F == F == _padded(F) and i.clamp_ok)(F), tweak="clamp"))
        # the only column in which the four rows differ lies in the last 16-float chunk of the padded row
        cs.append(FamilyCase(f"fam_chirality_f{F}", "chirality at width", F, 7, (3, 2, 4, 6),
                             (lambda F: lambda i: i.last and i.F == F and F - 16 <= i.chir_col < F and i.chir_ok)(F),
                             last=True, specs=C._base_and_stars, tweak="chirality"))
    for F in (28, 110):
        cs.append(FamilyCase(f"fam_no_unit_f{F}", "no unit bond rows", F, 7, REF,
                             (lambda F: lambda i: i.F == F and i.counts == REF and _all(i))(F), no_unit=True))
    return cs


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
C.register(CASES)
NAMES = tuple(c.name for c in CASES)


def cases_of(setting: str) -> Tuple[str, ...]:
    """The cases a setting's child runs: all of them, but the cases without unit bond rows in the default setting only."""
    return tuple(c.name for c in CASES if setting == "default" or not c.no_unit)


PAIRS = tuple((s, n) for s in SETTING_NAMES for n in cases_of(s))
# run a second time in every child (bit-identical): one per width class, one counts limit, one tweak, one with the LDS pair's tiles
TWICE = ("fam_width_f30", "fam_width_f110", "fam_width_f114", "fam_counts_13_21_32_53_f110", "fam_clamp_f112")

# ---- the expected dispatch.  Per case, in the order of SETTING_NAMES, ``mkgnn_debug_conv_dispatch``'s eleven answers in
# tests/_conv_f64.dispatch_string's letters -- forward per degree (- skip, g any-shape, L LDS bank, S streamed) / backward per degree
# (- skip, z zero fill, g any-shape, P LDS pair, M MFMA rows + LDS bank, S streamed pair) / bank_fused rows_streamed bank_streamed.
# How they follow from the plan functions:
#  * forward: S wherever stream_forward_supported (F <= 160, E <= 8, unit bond rows, <= 64 kernels of degree 4, <= 8 column parts);
#    MKGNN_FWD_STREAM=0, or a degree the streamed kernel refuses: L where mfma_forward_supported (F <= 112), else g.  More than 16 of
#    round 1's groups demote the widest degree to g even where the streamed kernel would take it (rule 2 of plan_conv_forward).
#  * backward, all four backward switches at their defaults and every degree within the streamed kernels: S, flags 111.
#  * otherwise per degree: g unless lds_backward_supported (even F <= 112, L <= 16/24/32/56); then M where mfma_backward_supported
#    (L <= 12/20/32/52) and MKGNN_NO_MFMA_BWD is unset, else P.  bank_fused only if every degree is M (and the switch allows);
#    rows_streamed = bank_fused and MKGNN_ROWS_STREAM; bank_streamed = bank_fused, MKGNN_BANK_STREAM and the streamed bank kernel's
#    own conditions.  MKGNN_FWD_SPLIT / MKGNN_BWD_SPLIT change no family.
_S = "SSSS/SSSS/111"


def _row(default, fwd_stream0, rows_stream0, bank_stream0, no_mfma_bwd, bank_fused0, split0=None):
    return dict(zip(SETTING_NAMES, (default, fwd_stream0, rows_stream0, bank_stream0, no_mfma_bwd, bank_fused0, split0 or default)))


def _even(F):      # an even width within the padded rows, counts within the MFMA rows limit
    return _row(_S, "LLLL/SSSS/111", "SSSS/MMMM/101", "SSSS/MMMM/110", "SSSS/PPPP/000", "SSSS/MMMM/000")


_ODD = _row(_S, "LLLL/SSSS/111", "SSSS/gggg/000", "SSSS/gggg/000", "SSSS/gggg/000", "SSSS/gggg/000")
EXPECTED = {
    **{f"fam_width_f{F}": _even(F) for F in (2, 30, 32, 34, 110, 112)},
    "fam_width_f27": _ODD, "fam_width_f111": _ODD,
    "fam_width_f114": _row(_S, "gggg/SSSS/111", "SSSS/gggg/000", "SSSS/gggg/000", "SSSS/gggg/000", "SSSS/gggg/000"),
}
for _F in (28, 110):
    EXPECTED.update({
        f"fam_counts_12_20_32_52_f{_F}": _even(_F),
        f"fam_counts_13_21_32_53_f{_F}": _row(_S, "LLLL/SSSS/111", "SSSS/PPMP/000", "SSSS/PPMP/000", "SSSS/PPPP/000", "SSSS/PPMP/000"),
        f"fam_counts_16_24_32_56_f{_F}": _row(_S, "LLLL/SSSS/111", "SSSS/PPMP/000", "SSSS/PPMP/000", "SSSS/PPPP/000", "SSSS/PPMP/000"),
        f"fam_counts_17_25_33_57_f{_F}": _row(_S, "LLLL/SSSS/111", "SSSS/gggg/000", "SSSS/gggg/000", "SSSS/gggg/000", "SSSS/gggg/000"),
        f"fam_counts_ref_last0_f{_F}": _even(_F), f"fam_counts_ref_last1_f{_F}": _even(_F),
        f"fam_counts_10_0_30_50_f{_F}": _row("S-SS/SzSS/111", "L-LL/SzSS/111", "S-SS/MzMM/101", "S-SS/MzMM/110", "S-SS/PzPP/000",
                                             "S-SS/MzMM/000"),
        # no unit bond rows: neither streamed bank kernel nor streamed forward, whatever the switches (default setting only)
        f"fam_no_unit_f{_F}": {"default": "LLLL/MMMM/110"},
    })
EXPECTED.update({
    "fam_tiles_16": _row(_S, "LLLL/SSSS/111", "SSSS/PMMM/000", "SSSS/PMMM/000", "SSSS/PPPP/000", "SSSS/PMMM/000"),
    "fam_tiles_17": _row(_S, "LLLL/SSSS/111", "SSSS/gMMM/000", "SSSS/gMMM/000", "SSSS/gPPP/000", "SSSS/gMMM/000"),
    # 65 kernels of degree 4: L in the forward whatever the switch; no streamed backward, and degree 4 past the LDS pair's 56
    "fam_tiles_l4_65": _row("SSSL/MMMg/000", "LLLL/MMMg/000", "SSSL/MMMg/000", "SSSL/MMMg/000", "SSSL/PPPg/000", "SSSL/MMMg/000"),
    # 19 of round 1's groups: degree 3 (7) goes to g; the other three are 13 streamed groups.  17 streamed groups: no streamed backward
    "fam_tiles_17_groups": _row("SSgS/gggg/000", "LLgL/gggg/000", "SSgS/gggg/000", "SSgS/gggg/000", "SSgS/gggg/000", "SSgS/gggg/000"),
    "fam_atoms_small": _even(28), "fam_atoms_tiles_a": _even(28), "fam_atoms_tiles_b": _even(28),
    "fam_bond_e1": _even(32), "fam_bond_e8": _even(32),
    "fam_clamp_f32": _even(32), "fam_clamp_f112": _even(112), "fam_chirality_f32": _even(32), "fam_chirality_f112": _even(112),
})
assert set(EXPECTED) == set(NAMES)
assert all(set(EXPECTED[n]) == {s for s in SETTING_NAMES if n in cases_of(s)} for n in NAMES)
