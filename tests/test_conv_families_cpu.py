"""The table of the fallback convolution families (tests/_conv_families.py), checked without a GPU: it holds both sides of every
limit those kernels have, every case reaches its edge, the yardstick passes its own test on every case -- the fp32 oracle within
the per-element bound of the float64 closed form -- and ``mkgnn_debug_conv_dispatch`` answers the table's expected families for
every (setting, case): one fresh child per setting, fake non-null integers for pointers (the query looks at shapes, null-ness and
alignment only, as tests/test_dispatch_cpu.py's do)."""
import json
import os
import subprocess
import sys

import pytest
import torch

from tests import _conv_f64 as C
from tests import _conv_families as Fam
from tests import _f64
from tests.test_dispatch_cpu import LIB


def test_the_table_holds_every_edge_of_the_issue():
    by_edge = {}
    for c in Fam.CASES:
        by_edge.setdefault(c.edge, []).append(c)
    # ---- padded width: both sides of 32 and of 112, widths with and without padding columns, odd widths in both classes
    widths = sorted(c.F for c in by_edge["padded width"])
    assert widths == [2, 27, 30, 32, 34, 110, 111, 112, 114]
    assert all(c.E == 7 and c.counts == Fam.STD for c in by_edge["padded width"])
    for k in range(4):
        assert {Fam.WIDTH_SIDES[F][k] for F in widths} == {True, False}, k
    assert {F for F in widths if F % 2} == {27, 111} and {Fam._padded(F) for F in (27, 111)} == {32, 112}
    # ---- kernel counts: at, past and below both backward limits for every degree, at both padded widths
    for F in (28, 110):
        counts = {c.counts: c for c in by_edge["backward limits"] if c.F == F}
        assert set(counts) == {(12, 20, 32, 52), (13, 21, 32, 53), (16, 24, 32, 56), (17, 25, 33, 57), Fam.REF, (10, 0, 30, 50)}
        assert (12, 20, 32, 52) == Fam.MFMA_ROWS_MAX_L and (16, 24, 32, 56) == Fam.LDS_PAIR_MAX_L
        for d in range(4):
            for limit in (Fam.MFMA_ROWS_MAX_L, Fam.LDS_PAIR_MAX_L):
                sides = {Fam._cmp(k[d], limit[d]) for k in counts if k[d]}
                # (degree 2 is never below the MFMA rows limit in these rows: the reference's 20 kernels ARE the limit; the
                # width cases' 2 kernels are below it)
                assert sides == {"<", "=", ">"} or (sides == {"=", ">"} and d == 1 and Fam.STD[d] < limit[d]), (F, d, limit)
        assert sorted(c.last for c in by_edge["backward limits"] if c.F == F and c.counts == Fam.REF) == [False, True]
    # ---- forward column tiles: one tile / two tiles, past the streamed sign table, past the group table
    tiles = {c.counts: c for c in by_edge["forward column tiles"]}
    assert set(tiles) == {(16,) * 4, (17,) * 4, (3, 2, 4, 65), (100, 100, 100, 64)} and all(c.F == 28 for c in tiles.values())
    assert Fam.column_tiles(16) == (1, 16) and Fam.column_tiles(17) == (2, 9) and tiles[(3, 2, 4, 65)].last
    assert sum(Fam.stream_parts((100, 100, 100, 64))) == 17 and sum(Fam.stream_parts((40, 70, 100, 64))) <= Fam.MAX_GROUPS
    # ---- atoms per bucket: below one tile; 16 / 17 for degrees 3 and 4 and 32 / 33 for degrees 1 and 2, both ways round
    atoms = [C.build(c.name).info.n for c in by_edge["atoms per bucket"]]
    assert all(c.counts == Fam.REF and c.F == 28 and c.last for c in by_edge["atoms per bucket"])
    assert any(max(n) < 16 for n in atoms)
    exact = [n for n in atoms if sorted(n) == [16, 17, 32, 33]]
    assert len(exact) == 2
    for d in (0, 1):
        assert {n[d] for n in exact} == {32, 33}
    for d in (2, 3):
        assert {n[d] for n in exact} == {16, 17}
    # ---- bond width, tweaks, no unit bond rows
    assert sorted((c.E, c.F) for c in by_edge["bond width"]) == [(1, 32), (8, 32)]
    assert sorted(c.F for c in by_edge["the clamp"]) == [32, 112] and all(c.tweak == "clamp" for c in by_edge["the clamp"])
    assert sorted(c.F for c in by_edge["chirality at width"]) == [32, 112]
    assert all(c.tweak == "chirality" and c.last for c in by_edge["chirality at width"])
    assert sorted(c.F for c in by_edge["no unit bond rows"]) == [28, 110]
    assert all(c.no_unit and c.counts == Fam.REF for c in by_edge["no unit bond rows"])
    assert [c.name for c in Fam.CASES if c.no_unit] == [c.name for c in by_edge["no unit bond rows"]]
    assert all(Fam.cases_of(s) == tuple(c.name for c in Fam.CASES if not c.no_unit) for s in Fam.SETTING_NAMES if s != "default")
    assert Fam.cases_of("default") == Fam.NAMES
    # ---- settings and bounds
    assert [Fam.SETTINGS[s] for s in Fam.SETTING_NAMES] == [
        {}, {"MKGNN_FWD_STREAM": "0"}, {"MKGNN_ROWS_STREAM": "0"}, {"MKGNN_BANK_STREAM": "0"}, {"MKGNN_NO_MFMA_BWD": "1"},
        {"MKGNN_BANK_FUSED": "0"}, {"MKGNN_FWD_SPLIT": "0", "MKGNN_BWD_SPLIT": "0"}]
    assert all(c.bound == C.F64_BOUND for c in Fam.CASES)          # (no case has a constant of its own)
    assert len(Fam.TWICE) == 5 and set(Fam.TWICE) <= set(Fam.cases_of("split0"))
    # every family is expected somewhere, in the forward and in the backward
    fwd = {ch for row in Fam.EXPECTED.values() for a in row.values() for ch in a.split("/")[0]}
    bwd = {ch for row in Fam.EXPECTED.values() for a in row.values() for ch in a.split("/")[1]}
    assert fwd == set("-gLS") and bwd == set("zgPMS")


@pytest.mark.parametrize("name", Fam.NAMES)
def test_case_reaches_its_edge(name):
    built = C.build(name)
    info = built.info
    assert built.case is Fam.BY_NAME[name] and built.case.proves(info), (name, vars(info))
    assert built.x.shape == (sum(info.n), built.case.F) and built.cot.shape == (sum(info.n), sum(built.case.counts))
    for d in range(1, 5):
        assert getattr(built.cpu, f"nei_edge_attr_deg{d}").numel() == info.n[d - 1] * d * built.case.E
    assert info.margins_ok, name
    assert (info.clamped_rows > 0) == (built.case.tweak == "clamp"), (name, info.clamped_rows)
    assert sum(info.n) <= 200


@pytest.mark.parametrize("name", Fam.NAMES)
def test_fp32_oracle_is_within_the_bound_of_the_float64_oracle(name):
    """The fallback families compute in fp32 (fmaf chains, v_mfma_f32_16x16x4_f32): the bound they are held to is the one the fp32
    oracle itself passes on every case."""
    built = C.build(name)
    idx = C.oracle_choices(built)
    gx, grads = C.oracle_gradients_fp32(built, idx)
    oracle = C.oracle_gradients_f64(built, idx)
    assert torch.isfinite(oracle[0]).all() and torch.isfinite(gx).all()
    worst = C._check_gradients_f64(gx, grads, oracle, name, bound=built.case.bound, expect=C.expected_gradients(built))
    print(f"{name}: fp32 oracle worst err / lim = {worst:.3f}")
    s32, s64 = C.pair_scores(built, idx, torch.float32), C.pair_scores(built, idx, torch.float64)
    names = ("support", "centre", "edge")
    for d in range(4):
        has = built.info.n[d] > 0 and built.info.counts[d] > 0
        assert (s64[d] is not None) == has and (s32[d] is not None) == has
        if not has:
            continue
        f32 = {f"deg{d + 1}.{nm}": s32[d][nm] for nm in names}
        assert _f64.check(f32, f32, {f"deg{d + 1}.{nm}": s64[d][nm] for nm in names}, [name, "fp32 oracle", "pair scores"]) == 3
        if built.case.last and d == 3:
            assert torch.equal(s32[d]["chirality"].double(), s64[d]["chirality"])


_WORKER = r"""
import ctypes, json, sys
lib = ctypes.CDLL(sys.argv[1])
P = ctypes.c_void_p
class Bank(ctypes.Structure):
    _fields_ = [("num_kernels", ctypes.c_int32), ("reserved", ctypes.c_int32)] + [("p%d" % k, P) for k in range(7)]
class Bucket(ctypes.Structure):
    _fields_ = [("count", ctypes.c_int64)] + [("p%d" % k, P) for k in range(5)] + [("nei_edge_unit", P)]
I32, I64 = ctypes.c_int32, ctypes.c_int64
lib.mkgnn_debug_conv_dispatch.argtypes = [P, P, P, I64, I64, I64, I32, I32, I32, I32, I32, P, I64, P]
want = json.loads(sys.argv[2])
for name, value in want["env"].items():
    import os
    assert os.environ.get(name) == value, name
got = []
for ks, atoms, F, E, unit in want["rows"]:
    banks, buckets = (Bank * 4)(), (Bucket * 4)()
    for i in range(4):
        banks[i].num_kernels = ks[i]
        for k in range(7): setattr(banks[i], "p%d" % k, 0x1000)
        buckets[i].count = atoms[i]
        for k in range(5): setattr(buckets[i], "p%d" % k, 0x2000)
        buckets[i].nei_edge_unit = 0x3000 if unit else None
    F4, K4 = (F + 3) // 4 * 4, (sum(ks) + 3) // 4 * 4
    out = (I32 * 11)()
    rc = lib.mkgnn_debug_conv_dispatch(ctypes.addressof(banks), ctypes.addressof(buckets), 0x10000, F4, K4, sum(atoms), F, E, 0, 0, 1,
                                       0x20000, F4, ctypes.addressof(out))
    assert rc == 0
    got.append(list(out))
print(json.dumps(got))
"""


def test_the_query_answers_the_expected_families_for_every_setting_and_case():
    wrong = []
    for setting in Fam.SETTING_NAMES:
        names = Fam.cases_of(setting)
        rows = []
        for name in names:
            case, info = Fam.BY_NAME[name], C.build(name).info
            rows.append([list(case.counts), list(info.n), case.F, case.E, 0 if case.no_unit else 1])
        res = subprocess.run([sys.executable, "-c", _WORKER, LIB, json.dumps({"env": Fam.SETTINGS[setting], "rows": rows})],
                             env=Fam.environment(setting, os.environ), check=True, capture_output=True, text=True)
        fwd_names, bwd_names = ("skip", "generic", "lds_bank", "streamed"), ("skip", "zero_fill", "generic", "lds_pair", "mfma_lds", "streamed")
        for name, out in zip(names, json.loads(res.stdout)):
            got = C.dispatch_string(([fwd_names[v] for v in out[:4]], [bwd_names[v] for v in out[4:8]], out[8:11]))
            if got != Fam.EXPECTED[name][setting]:
                wrong.append((setting, name, got, Fam.EXPECTED[name][setting]))
    assert not wrong, wrong
