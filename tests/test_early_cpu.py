"""The early-recognition metrics without a GPU: ``evaluation.early_reference`` against a brute force that shares none of its closed
forms (explicit resampling, distinct thresholds, exact rationals, a loop of ``exp`` over every position), scikit-learn's average
precision where it imports, BEDROC's and the enrichment factor's known values, the point functions, the names, the additive C ABI
surface of ``mkgnn_bootstrap_early`` with its refusals, and the Python layers on CPU tensors."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from tests import _bootstrap_cases as BC
from tests import _early_cases as EC

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ("distinct", "grid8", "grid1", "equal", "actives_last")


@pytest.mark.parametrize("n", [1, 2, 3, 8, 65, 300])
@pytest.mark.parametrize("stratified", [False, True])
def test_definition_against_the_brute_force(n, stratified):
    from molkgnn_amd import evaluation as E
    B, seed, offset = 6, 7, (1 << 33) + 2
    cuts = EC.cuts_for(n, tile=8)
    for kind in (KINDS if n >= 2 else ("equal",)):
        y, s = BC.case(kind, n)
        got = E.early_reference(y, s, B, cuts, EC.ALPHAS, seed, offset, stratified)
        ap, hits, rie, n_pos = EC.brute_force(y, s, B, cuts, EC.ALPHAS, seed, offset, stratified)
        assert got["ap"].shape == (B,) and got["hits"].shape == (B, len(cuts)) and got["rie"].shape == (B, len(EC.ALPHAS))
        assert got["n_pos"].dtype == np.int32 and np.array_equal(got["n_pos"], n_pos), kind
        assert got["n_undefined"] == int(((n_pos == 0) | (n_pos == n)).sum())
        errs = EC.relative_error(got["ap"], ap), EC.relative_error(got["hits"], hits), EC.relative_error(got["rie"], rie)
        print(f"n={n} {kind} stratified={stratified}: ap {errs[0]:.3g} hits {errs[1]:.3g} rie {errs[2]:.3g}")
        assert errs[0] <= EC.HOST_TOL and errs[1] <= EC.HITS_TOL and errs[2] <= EC.HOST_TOL, (kind, errs)
        # the whole list holds every drawn active; the first row holds at most one
        assert np.array_equal(got["hits"][:, cuts.index(n)], n_pos.astype(np.float64))
        assert (got["hits"][:, 0] <= 1.0).all()
        if stratified and n >= 2:
            assert (got["n_pos"] == int((y == 1).sum())).all()


def test_average_precision_is_sklearns_with_sample_weights():
    sk = pytest.importorskip("sklearn.metrics")
    from molkgnn_amd import evaluation as E
    for kind in ("distinct", "grid8", "grid1"):
        y, s = BC.case(kind, 300)
        got = E.early_reference(y, s, 8, (), (), seed=2, offset=5)
        for b in range(8):
            c = np.bincount(BC.draws(300, 300, 2, 5 + b), minlength=300)
            want = sk.average_precision_score(y, s, sample_weight=c)
            assert abs(got["ap"][b] - want) <= EC.HOST_TOL * want, (kind, b)
        assert abs(E.calculate_average_precision(y, s) - sk.average_precision_score(y, s)) <= EC.HOST_TOL


def test_known_values_of_bedroc_and_the_enrichment_factor():
    from molkgnn_amd import evaluation as E
    for n, T in ((1000, 10), (200, 8), (65, 1)):
        assert math.ceil(T / n * n) == T                      # (sizes at which the float product T / n * n does not round past T)
        y = np.zeros(n, dtype=np.int64)
        y[:T] = 1
        s = -np.arange(n, dtype=np.float64)
        for alpha in (20.0, 160.9, 0.5):
            assert abs(E.calculate_bedroc(y, s, alpha) - 1.0) <= 1e-9, (n, T, alpha)             # a perfect ranking
            assert abs(E.calculate_bedroc(y[::-1].copy(), s, alpha)) <= 1e-9, (n, T, alpha)     # the worst one
        assert abs(E.calculate_enrichment_factor(y, s, T / n) - n / T) <= 1e-12 * n / T          # (two divisions' rounding)
        assert E.calculate_average_precision(y, s) == 1.0
    # all scores equal: every active takes the mean over all positions, strictly inside (0, 1), and nothing is enriched
    y, s = BC.case("equal", 300)
    assert 0.0 < E.calculate_bedroc(y, s, 20.0) < 1.0
    assert abs(E.calculate_enrichment_factor(y, s, 0.1) - 1.0) <= 1e-12
    # a class is absent: -1, as the existing metrics answer
    for fn in (E.calculate_average_precision, E.calculate_enrichment_factor, E.calculate_bedroc):
        assert fn(np.zeros(5), np.arange(5.0)) == -1 and fn(np.ones(5), np.arange(5.0)) == -1
    for bad in (0.0, -1.0, 1.5, float("nan")):
        with pytest.raises(ValueError, match="fraction"):
            E.calculate_enrichment_factor(y, s, bad)
    for bad in (0.0, -2.0, 500.5, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="alpha"):
            E.calculate_bedroc(y, s, bad)


@pytest.mark.parametrize("kind", KINDS)
def test_point_functions_are_the_definition_with_unit_multiplicities(kind):
    """The definition's replicate with ``c = 1`` everywhere (``_replicate_early``), derived by the shared function."""
    from molkgnn_amd import evaluation as E
    n = 300
    y, s = BC.case(kind, n)
    rank, ys, gl, _ = BC.sorted_inputs(y, s)
    gid = np.concatenate([[0], np.cumsum(gl[:-1] != 0)]).astype(np.int64)
    cuts, alphas = [E.early_cut(0.01, n), E.early_cut(0.1, n)], [20.0, 160.9]
    ap, hits, rie, T = E._replicate_early(np.ones(n, dtype=np.int64), ys.astype(np.int64), gid, int(gid[-1]) + 1, cuts, alphas)
    want = E.early_derived(np.array([ap]), hits[None], rie[None], np.array([T]), n, cuts, alphas)
    assert abs(E.calculate_average_precision(y, s) - float(want["AP"][0])) <= EC.HOST_TOL
    for j, x in enumerate((0.01, 0.1)):
        assert abs(E.calculate_enrichment_factor(y, s, x) - float(want["EF"][0, j])) <= EC.HOST_TOL * float(want["EF"][0, j]) + 1e-300
    for a, alpha in enumerate(alphas):
        assert abs(E.calculate_bedroc(y, s, alpha) - float(want["BEDROC"][0, a])) <= EC.HOST_TOL
    # torch tensors and float32 scores go the same way
    assert E.calculate_average_precision(torch.from_numpy(y), torch.from_numpy(s)) == E.calculate_average_precision(y, s)


def test_derived_metrics_are_nan_for_a_one_class_replicate():
    from molkgnn_amd import evaluation as E
    got = E.early_reference(BC.UNDEFINED_Y, BC.UNDEFINED_S, BC.UNDEFINED_BOOT, (1, 4), (20.0,), seed=BC.UNDEFINED_SEED)
    empty = got["n_pos"] == 0
    assert 0 < int(empty.sum()) == got["n_undefined"] < BC.UNDEFINED_BOOT
    assert (got["ap"][empty] == 0.0).all() and (got["hits"][empty] == 0.0).all() and (got["rie"][empty] == 0.0).all()
    d = E.early_derived(got["ap"], got["hits"], got["rie"], got["n_pos"], 8, (1, 4), (20.0,))
    for key in ("AP", "EF", "BEDROC"):
        assert np.array_equal(np.isnan(d[key].numpy()).reshape(BC.UNDEFINED_BOOT, -1).all(axis=1), empty), key
        assert np.array_equal(np.isnan(d[key].numpy()).reshape(BC.UNDEFINED_BOOT, -1).any(axis=1), empty), key
    # cuts and alphas outside their ranges: NaN columns, the others untouched
    bad = E.early_reference(BC.UNDEFINED_Y, BC.UNDEFINED_S, 4, (0, 1, 9, 4), (20.0, 0.0, float("nan"), 501.0), seed=BC.UNDEFINED_SEED)
    assert np.isnan(bad["hits"][:, [0, 2]]).all() and np.isnan(bad["rie"][:, 1:]).all()
    assert np.array_equal(bad["hits"][:, [1, 3]], got["hits"][:4]) and np.array_equal(bad["rie"][:, :1], got["rie"][:4])


def test_names():
    from molkgnn_amd import evaluation as E
    from molkgnn_amd.train import _check_metrics
    assert E.parse_early_name("AP") == ("AP", None) and E.parse_early_name("EF_0.01") == ("EF", 0.01)
    assert E.parse_early_name("BEDROC_20") == ("BEDROC", 20.0) and E.parse_early_name("BEDROC_160.9") == ("BEDROC", 160.9)
    assert E.parse_early_name("EF_1") == ("EF", 1.0) and E.parse_early_name("BEDROC_500") == ("BEDROC", 500.0)
    for bad in ("ap", "EF", "EF_", "EF_x", "EF_0", "EF_1.5", "EF_-0.1", "EF_nan", "BEDROC_", "BEDROC_0", "BEDROC_501", "BEDROC_inf",
                "BEDROC_nan", "AUC", "PRAUC", 3, None):
        with pytest.raises(ValueError):
            E.parse_early_name(bad)
    spec = E.EarlySpec(("EF_0.01", "AP", "BEDROC_20", "EF_0.010", "EF_0.1"))
    assert spec.fractions == [0.01, 0.1] and spec.alphas == [20.0] and spec.cuts(4097) == [41, 410] and spec.cuts(5) == [1, 1]
    assert spec.where == {"EF_0.01": ("EF", 0), "AP": ("AP", None), "BEDROC_20": ("BEDROC", 0), "EF_0.010": ("EF", 0), "EF_0.1": ("EF", 1)}
    assert E.early_cut(0.001, 1 << 20) == 1049 and E.early_cut(1.0, 7) == 7 and E.early_cut(1e-9, 7) == 1
    E.EarlySpec(tuple(f"EF_0.0{i}" for i in range(1, 9)) + tuple(f"BEDROC_{a}" for a in (5, 10, 20, 40)))       # 8 and 4: the limits
    y, s = (torch.from_numpy(v) for v in BC.case("grid8", 65))
    nine = tuple(f"EF_0.0{i}" for i in range(1, 10))
    five = tuple(f"BEDROC_{a}" for a in (5, 10, 20, 40, 80))
    for fn in (lambda **kw: E.bootstrap_metrics(y, s, n_boot=2, **kw), lambda **kw: E.bootstrap_compare(y, s, s, n_boot=2, **kw),
               lambda **kw: E.bootstrap_per_task(y, s, torch.zeros(65, dtype=torch.int64), 1, n_boot=2, **kw)):
        for early, text in ((nine, "distinct enrichment fractions"), (five, "distinct BEDROC alphas"), (("EF_2",), "fraction"),
                            (("nope",), "unknown early-recognition"), ("AP", "not one string"), (("BEDROC_x",), "BEDROC_<number>")):
            with pytest.raises(ValueError, match=text):
                fn(early=early)
    # the evaluate family's metric table
    table = _check_metrics(("AUC", "AP", "EF_0.05", "BEDROC_20"))
    yn, sn = BC.case("grid8", 300)
    assert table["AP"](yn, sn) == E.calculate_average_precision(yn, sn)
    assert table["EF_0.05"](yn, sn) == E.calculate_enrichment_factor(yn, sn, 0.05)
    assert table["BEDROC_20"](yn, sn) == E.calculate_bedroc(yn, sn, 20.0)
    assert set(_check_metrics(("AUC",))) == set(_check_metrics(()))                 # naming none adds none
    for bad, text in ((("EF_3",), "fraction"), (("BEDROC_0",), "alpha"), (("EF_0.01", "oops"), "unknown metric"), (nine, "distinct")):
        with pytest.raises(ValueError, match=text):
            _check_metrics(bad)


def test_entry_point_is_declared_typed_and_additive_to_abi_8():
    from molkgnn_amd import _lib
    with open(os.path.join(REPO, "include", "molkgnn_hip.h")) as f:
        h = f.read()
    assert re.search(r"\bint mkgnn_bootstrap_early\(const int32_t\* rank, const uint8_t\* y_sorted, const uint8_t\* group_last, int64_t n, "
                     r"int64_t split, int32_t B,\s+uint64_t seed, uint64_t offset, double lower, double upper, const int32_t\* cuts, "
                     r"int32_t J,\s+const double\* alphas, int32_t A, double\* auc, double\* logauc, int64_t\* two_u, int32_t\* n_pos, "
                     r"double\* ap,\s+double\* hits, double\* rie, void\* workspace, size_t workspace_bytes, void\* stream\);", h)
    m = re.search(r"#define\s+MKGNN_ABI_VERSION\s+(\d+)", h)
    assert m and int(m.group(1)) == 8 and _lib.ABI_VERSION == 8
    for name, value in (("MAX_CUTS", _lib.BOOTSTRAP_MAX_CUTS), ("MAX_ALPHAS", _lib.BOOTSTRAP_MAX_ALPHAS)):
        d = re.search(r"#define\s+MKGNN_BOOTSTRAP_%s\s+(\d+)" % name, h)
        assert d and int(d.group(1)) == value, name
    from molkgnn_amd import evaluation as E
    assert (_lib.BOOTSTRAP_MAX_CUTS, _lib.BOOTSTRAP_MAX_ALPHAS) == (8, 4) == (E.BOOTSTRAP_MAX_CUTS, E.BOOTSTRAP_MAX_ALPHAS)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    raw.mkgnn_abi_version.restype = ctypes.c_int
    assert raw.mkgnn_abi_version() == 8 and hasattr(raw, "mkgnn_bootstrap_early")
    assert "mkgnn_bootstrap_early" in _lib.EXPORTS and len(set(_lib.EXPORTS)) == len(_lib.EXPORTS)
    lib = _lib.load()
    P, I32 = ctypes.c_void_p, ctypes.c_int32
    assert lib.mkgnn_bootstrap_early.argtypes == [P, P, P, ctypes.c_int64, ctypes.c_int64, I32, ctypes.c_uint64, ctypes.c_uint64,
                                                  ctypes.c_double, ctypes.c_double, P, I32, P, I32, P, P, P, P, P, P, P, P,
                                                  ctypes.c_size_t, P]
    assert lib.mkgnn_bootstrap_early.restype is ctypes.c_int


def test_rejections_before_a_launch_at_the_c_entry():
    """Checked before anything is launched: no device needed (no pointer is read)."""
    from molkgnn_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_uint64 * 128)()
    p = ctypes.addressof(buf)
    ok = dict(rank=p, ys=p + 64, gl=p + 128, n=8, split=8, B=2, seed=1, offset=0, lower=0.001, upper=0.1, cuts=p + 448, J=2,
              alphas=p + 512, A=2, auc=p + 192, logauc=p + 256, two_u=p + 320, n_pos=p + 384, ap=p + 576, hits=p + 640, rie=p + 704,
              ws=None, wsb=0, stream=None)

    def call(**kw):
        a = dict(ok, **kw)
        rc = lib.mkgnn_bootstrap_early(a["rank"], a["ys"], a["gl"], a["n"], a["split"], a["B"], a["seed"], a["offset"], a["lower"],
                                       a["upper"], a["cuts"], a["J"], a["alphas"], a["A"], a["auc"], a["logauc"], a["two_u"],
                                       a["n_pos"], a["ap"], a["hits"], a["rie"], a["ws"], a["wsb"], a["stream"])
        return rc, lib.mkgnn_last_error().decode()
    for kw, text in ((dict(n=0), "rows outside"), (dict(n=(1 << 22) + 1), "rows outside"), (dict(B=0), "replicates outside"),
                     (dict(B=4097), "replicates outside"), (dict(split=9), "split"), (dict(lower=0.0), "FPR window"),
                     (dict(upper=1.5), "FPR window"), (dict(rank=None), "null pointer"), (dict(n_pos=None), "null pointer"),
                     (dict(J=-1), "cuts outside"), (dict(J=9), "cuts outside"), (dict(A=-1), "alphas outside"), (dict(A=5), "alphas outside"),
                     (dict(ap=None), "null pointer"), (dict(cuts=None), "null pointer"), (dict(hits=None), "null pointer"),
                     (dict(alphas=None), "null pointer"), (dict(rie=None), "null pointer"),
                     (dict(ap=None, J=0, A=0, cuts=None, hits=None, alphas=None, rie=None), "null pointer"),
                     (dict(auc=p + 196), "misaligned"), (dict(ap=p + 580), "misaligned"), (dict(hits=p + 644), "misaligned"),
                     (dict(rie=p + 708), "misaligned"), (dict(alphas=p + 516), "misaligned"), (dict(cuts=p + 450), "misaligned"),
                     (dict(auc=p), "aliases rank"), (dict(logauc=p + 192), "alias each other"),
                     (dict(ap=p), "aliases rank"), (dict(hits=p + 64), "aliases rank"), (dict(rie=p + 128), "aliases rank"),
                     (dict(ap=p + 448), "cuts or alphas"), (dict(hits=p + 512), "cuts or alphas"), (dict(rie=p + 448), "cuts or alphas"),
                     (dict(auc=p + 512), "cuts or alphas"), (dict(ap=p + 192), "alias each other"), (dict(hits=p + 576), "alias each other"),
                     (dict(rie=p + 640), "alias each other"), (dict(rie=p + 384), "alias each other"),
                     (dict(n=8193), "null workspace"), (dict(n=8193, ws=p + 768, wsb=64), "workspace of 64 bytes"),
                     (dict(n=8193, ws=p + 772, wsb=1 << 20), "16-byte aligned")):
        rc, msg = call(**kw)
        assert rc != 0 and text in msg and "mkgnn_bootstrap_early" in msg, (kw, rc, msg)


def test_default_early_changes_nothing():
    from molkgnn_amd import evaluation as E
    y, s = (torch.from_numpy(v) for v in BC.case("grid8", 300))
    kw = dict(n_boot=16, FPR_range=(0.001, 1.0), confidence=0.9, seed=5, offset=9, stratified=True)

    def same(a, b):
        if torch.is_tensor(a):
            return torch.is_tensor(b) and a.dtype == b.dtype and torch.equal(a.view(torch.int64) if a.dtype == torch.float64 else a,
                                                                             b.view(torch.int64) if b.dtype == torch.float64 else b)
        if isinstance(a, dict):
            return isinstance(b, dict) and list(a) == list(b) and all(same(a[k], b[k]) for k in a)
        if isinstance(a, (tuple, list)):
            return type(a) is type(b) and len(a) == len(b) and all(same(x, z) for x, z in zip(a, b))
        return type(a) is type(b) and (a == b or (a != a and b != b))
    plain = E.bootstrap_metrics(y, s, **kw)
    assert same(plain, E.bootstrap_metrics(y, s, early=(), **kw))
    assert list(plain) == ["point", "replicates", "AUC", "logAUC", "n_undefined", "n_pos", "seed", "offset", "n_boot", "confidence",
                           "FPR_range", "stratified"]
    assert same(E.bootstrap_compare(y, s, s * 0.5, n_boot=8), E.bootstrap_compare(y, s, s * 0.5, n_boot=8, early=()))
    task = torch.arange(300) % 2
    assert same(E.bootstrap_per_task(y, s, task, 2, n_boot=8), E.bootstrap_per_task(y, s, task, 2, n_boot=8, early=()))
    # with names: the keys of before, unchanged, and per name what AUC has
    names = ("AP", "EF_0.01", "BEDROC_20")
    full = E.bootstrap_metrics(y, s, early=names, **kw)
    assert set(full) == set(plain) | set(names) | {"cuts"} and full["cuts"] == {"EF_0.01": 3}
    for key in plain:
        if key not in ("point", "replicates"):
            assert same(full[key], plain[key]), key
    for block in ("point", "replicates"):
        assert set(full[block]) == set(plain[block]) | set(names)
        assert all(same(full[block][k], plain[block][k]) for k in plain[block])
    ref = E.early_reference(y, s, 16, [3], [20.0], seed=5, offset=9, stratified=True)
    d = E.early_derived(ref["ap"], ref["hits"], ref["rie"], ref["n_pos"], 300, [3], [20.0])
    assert torch.equal(full["replicates"]["AP"], d["AP"]) and torch.equal(full["replicates"]["EF_0.01"], d["EF"][:, 0])
    assert torch.equal(full["replicates"]["BEDROC_20"], d["BEDROC"][:, 0])
    for name, fn in (("AP", E.calculate_average_precision), ("EF_0.01", lambda a, b: E.calculate_enrichment_factor(a, b, 0.01)),
                     ("BEDROC_20", lambda a, b: E.calculate_bedroc(a, b, 20.0))):
        assert full["point"][name] == fn(y, s), name
        assert set(full[name]) == {"mean", "std", "ci"} and full[name]["ci"][0] <= full[name]["mean"] <= full[name]["ci"][1]
    cmp_ = E.bootstrap_compare(y, s, s.clone(), n_boot=8, early=names)
    assert all(bool((cmp_[k]["diff"] == 0).all()) and cmp_["point"]["diff"][k] == 0 for k in names) and cmp_["cuts"] == {"EF_0.01": 3}
    per = E.bootstrap_per_task(y, s, task, 2, n_boot=8, early=("EF_0.1",))
    assert all(r["cuts"] == {"EF_0.1": 15} and r["replicates"]["EF_0.1"].shape == (8,) for r in per)
    assert not math.isnan(per[0]["EF_0.1"]["mean"])
