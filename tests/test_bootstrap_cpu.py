"""The bootstrap of AUC and logAUC without a GPU: the additive C ABI surface of ``mkgnn_bootstrap_roc``, its host-side sizing and
rejections, ``evaluation.bootstrap_reference`` against the brute-force counterpart (explicit resampling, then the existing
``evaluation`` functions), and the Python layers on CPU tensors."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from tests import _bootstrap_cases as BC

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header() -> str:
    with open(os.path.join(REPO, "include", "molkgnn_hip.h")) as f:
        return f.read()


def test_entry_points_are_declared_typed_and_additive_to_abi_8():
    from molkgnn_amd import _lib
    h = _header()
    assert re.search(r"\bsize_t mkgnn_bootstrap_roc_workspace_bytes\(int64_t n, int32_t replicates_per_pass\);", h)
    assert re.search(r"\bint mkgnn_bootstrap_roc\(const int32_t\* rank, const uint8_t\* y_sorted, const uint8_t\* group_last, int64_t n, "
                     r"int64_t split, int32_t B,\s+uint64_t seed, uint64_t offset, double lower, double upper, double\* auc, "
                     r"double\* logauc, int64_t\* two_u,\s+int32_t\* n_pos, void\* workspace, size_t workspace_bytes, void\* stream\);", h)
    m = re.search(r"#define\s+MKGNN_ABI_VERSION\s+(\d+)", h)
    assert m and int(m.group(1)) == 8 and _lib.ABI_VERSION == 8
    for name, value in (("MAX_ROWS", _lib.BOOTSTRAP_MAX_ROWS), ("MAX_REPLICATES", _lib.BOOTSTRAP_MAX_REPLICATES),
                        ("WORKSPACE_CAP", _lib.BOOTSTRAP_WORKSPACE_CAP)):
        d = re.search(r"#define\s+MKGNN_BOOTSTRAP_%s\s+(\d+)" % name, h)
        assert d and int(d.group(1)) == value, name
    assert _lib.BOOTSTRAP_MAX_ROWS == 1 << 22 and _lib.BOOTSTRAP_MAX_REPLICATES == 4096
    raw = ctypes.CDLL(_lib.LIB_PATH)
    raw.mkgnn_abi_version.restype = ctypes.c_int
    assert raw.mkgnn_abi_version() == 8
    for name in ("mkgnn_bootstrap_roc", "mkgnn_bootstrap_roc_workspace_bytes"):
        assert hasattr(raw, name), name
        assert name in _lib.EXPORTS, name
    assert len(set(_lib.EXPORTS)) == len(_lib.EXPORTS)
    lib = _lib.load()
    P = ctypes.c_void_p
    assert lib.mkgnn_bootstrap_roc.argtypes == [P, P, P, ctypes.c_int64, ctypes.c_int64, ctypes.c_int32, ctypes.c_uint64, ctypes.c_uint64,
                                                ctypes.c_double, ctypes.c_double, P, P, P, P, P, ctypes.c_size_t, P]
    assert lib.mkgnn_bootstrap_roc.restype is ctypes.c_int
    assert lib.mkgnn_bootstrap_roc_workspace_bytes.argtypes == [ctypes.c_int64, ctypes.c_int32]
    assert lib.mkgnn_bootstrap_roc_workspace_bytes.restype is ctypes.c_size_t
    # the tiling the GPU tests place their shapes around is the kernel file's
    with open(os.path.join(REPO, "molkgnn_amd", "csrc", "kgnn_bootstrap.hip")) as f:
        src = f.read()
    assert "BS_THREADS = 256" in src and "BS_PER = 4" in src and "BS_TILE = BS_THREADS * BS_PER" in src
    assert "BS_DRAW_ROWS = BS_THREADS * BS_PER" in src and "BS_LDS_MAX_N = %d" % _lib.BOOTSTRAP_LDS_MAX_N in src
    assert _lib.BOOTSTRAP_TILE == 1024 and _lib.BOOTSTRAP_DRAW_ROWS == 1024


def test_workspace_sizing_on_the_host():
    from molkgnn_amd import _lib
    from molkgnn_amd.readout import bootstrap_roc_replicates_per_pass as per_pass
    size = _lib.load().mkgnn_bootstrap_roc_workspace_bytes
    edge = _lib.BOOTSTRAP_LDS_MAX_N
    assert size(1, 1) == 16 and size(edge, 4096) == 16                       # the LDS form: no scratch, and not the rejected 0
    assert size(edge + 1, 1) == 4 * (edge + 4) and size(edge + 1, 7) == 7 * 4 * (edge + 4)
    assert size(edge + 4, 3) == 3 * 4 * (edge + 4) and size(edge + 5, 3) == 3 * 4 * (edge + 8)
    assert size(1 << 22, 16) == 1 << 28 and size(1 << 22, 4096) == 4096 << 24       # (size_t: beyond 2^32)
    for n, reps in ((0, 1), (-1, 1), ((1 << 22) + 1, 1), (100, 0), (100, -3), (100, 4097), (1 << 40, 1)):
        assert size(n, reps) == 0, (n, reps)
    # the wrapper's own scratch stays under the cap, with at least one replicate in flight
    cap = _lib.BOOTSTRAP_WORKSPACE_CAP
    assert per_pass(edge + 1, 1000) == 1000 and per_pass(1 << 20, 1000) == 256 and per_pass(1 << 22, 1000) == 64
    assert per_pass(1 << 22, 3) == 3
    for n in (edge + 1, 65536, (1 << 20) + 1, 1 << 22):
        assert 16 <= size(n, per_pass(n, 4096)) <= cap


def test_rejections_before_a_launch_at_the_c_entry():
    """Checked before anything is launched: no device needed (no pointer is read)."""
    from molkgnn_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_uint64 * 64)()
    p = ctypes.addressof(buf)
    ok = dict(rank=p, ys=p + 64, gl=p + 128, n=8, split=8, B=2, seed=1, offset=0, lower=0.001, upper=0.1, auc=p + 192, logauc=p + 256,
              two_u=p + 320, n_pos=p + 384, ws=None, wsb=0, stream=None)

    def call(**kw):
        a = dict(ok, **kw)
        rc = lib.mkgnn_bootstrap_roc(a["rank"], a["ys"], a["gl"], a["n"], a["split"], a["B"], a["seed"], a["offset"], a["lower"],
                                     a["upper"], a["auc"], a["logauc"], a["two_u"], a["n_pos"], a["ws"], a["wsb"], a["stream"])
        return rc, lib.mkgnn_last_error().decode()
    for kw, text in ((dict(n=0), "rows outside"), (dict(n=(1 << 22) + 1), "rows outside"), (dict(B=0), "replicates outside"),
                     (dict(B=4097), "replicates outside"), (dict(split=-1), "split"), (dict(split=9), "split"),
                     (dict(lower=0.0), "FPR window"), (dict(lower=-0.1), "FPR window"), (dict(upper=1.5), "FPR window"),
                     (dict(lower=0.2, upper=0.1), "FPR window"), (dict(lower=float("nan")), "FPR window"),
                     (dict(rank=None), "null pointer"), (dict(n_pos=None), "null pointer"), (dict(auc=p + 196), "misaligned"),
                     (dict(auc=p), "aliases rank"), (dict(logauc=p + 192), "alias each other"),
                     (dict(n=8193), "null workspace"), (dict(n=8193, ws=p + 448, wsb=64), "workspace of 64 bytes"),
                     (dict(n=8193, ws=p + 452, wsb=1 << 20), "16-byte aligned")):
        rc, msg = call(**kw)
        assert rc != 0 and text in msg, (kw, rc, msg)


@pytest.mark.parametrize("n", [2, 3, 40, 257, 1500])
@pytest.mark.parametrize("stratified", [False, True])
def test_reference_against_explicit_resampling(n, stratified):
    from molkgnn_amd import evaluation as E
    B = 6
    for kind in BC.KINDS:
        y, s = BC.case(kind, n)
        for window in BC.WINDOWS:
            got = E.bootstrap_reference(y, s, B, window, seed=7, offset=(1 << 33) + 2, stratified=stratified)
            auc, logauc, n_pos = BC.brute_force(y, s, B, window, 7, (1 << 33) + 2, stratified)
            assert got["AUC"].dtype == np.float64 and got["two_u"].dtype == np.int64 and got["n_pos"].dtype == np.int32
            assert np.array_equal(got["n_pos"], n_pos), (kind, window)
            assert np.array_equal(np.isnan(got["AUC"]), np.isnan(auc)) and np.array_equal(np.isnan(got["logAUC"]), np.isnan(auc))
            assert got["n_undefined"] == int(np.isnan(auc).sum())
            live = ~np.isnan(auc)
            err_auc = np.abs(got["AUC"][live] - auc[live]).max(initial=0.0)
            err_log = np.abs(got["logAUC"][live] - logauc[live]).max(initial=0.0)
            print(f"n={n} {kind} window={window} stratified={stratified}: |dAUC|={err_auc:.3g} |dlogAUC|={err_log:.3g}")
            assert err_auc <= BC.AUC_TOL, (kind, window, err_auc)
            assert err_log <= BC.LOGAUC_TOL, (kind, window, err_log)
            if kind == "equal":
                assert (got["AUC"][live] == 0.5).all()
            T = got["n_pos"][live].astype(np.int64)
            assert np.array_equal(got["AUC"][live], got["two_u"][live].astype(np.float64) / (2 * T * (n - T)).astype(np.float64))
            if stratified:
                assert (got["n_pos"] == int((y == 1).sum())).all() and got["n_undefined"] == 0


def test_negative_zero_ties_with_positive_zero():
    from molkgnn_amd import evaluation as E
    y = np.array([1, 0, 1, 0, 0, 1])
    a = E.bootstrap_reference(y, np.array([0.0, -0.0, 0.0, -0.0, -1.0, 1.0]), 16, (0.001, 1.0), seed=3)
    b = E.bootstrap_reference(y, np.array([0.0, 0.0, 0.0, 0.0, -1.0, 1.0]), 16, (0.001, 1.0), seed=3)
    for k in ("AUC", "logAUC", "two_u", "n_pos"):
        assert np.array_equal(a[k], b[k], equal_nan=k in ("AUC", "logAUC")), k


def test_one_active_in_eight_rows_gives_undefined_replicates():
    from molkgnn_amd import evaluation as E
    got = E.bootstrap_reference(BC.UNDEFINED_Y, BC.UNDEFINED_S, BC.UNDEFINED_BOOT, seed=BC.UNDEFINED_SEED)
    _, _, n_pos = BC.brute_force(BC.UNDEFINED_Y, BC.UNDEFINED_S, BC.UNDEFINED_BOOT, (0.001, 0.1), BC.UNDEFINED_SEED, 0, False)
    one_class = (n_pos == 0) | (n_pos == 8)
    assert one_class.any() and not one_class.all()                          # the fixture's seed gives both
    assert np.array_equal(np.isnan(got["AUC"]), one_class) and np.array_equal(np.isnan(got["logAUC"]), one_class)
    assert got["n_undefined"] == int(one_class.sum())
    m = E.bootstrap_metrics(BC.UNDEFINED_Y, BC.UNDEFINED_S, n_boot=BC.UNDEFINED_BOOT, seed=BC.UNDEFINED_SEED)
    assert m["n_undefined"] == int(one_class.sum()) and np.array_equal(torch.isnan(m["replicates"]["AUC"]).numpy(), one_class)
    defined = got["AUC"][~one_class]
    assert m["AUC"]["mean"] == pytest.approx(defined.mean(), abs=1e-15)
    assert m["AUC"]["std"] == pytest.approx(defined.std(ddof=1), abs=1e-15)


def test_two_score_vectors_see_the_same_resamples():
    from molkgnn_amd import evaluation as E
    y, s = BC.case("grid8", 257)
    other = BC.scores("distinct", 257, 77)
    for stratified in (False, True):
        a = E.bootstrap_reference(y, s, 32, seed=5, offset=9, stratified=stratified)
        b = E.bootstrap_reference(y, other, 32, seed=5, offset=9, stratified=stratified)
        assert np.array_equal(a["n_pos"], b["n_pos"])
        assert not np.array_equal(a["two_u"], b["two_u"])
    # and the offsets a call consumes are offset .. offset + B - 1
    head, tail = E.bootstrap_reference(y, s, 5, seed=5, offset=9), E.bootstrap_reference(y, s, 3, seed=5, offset=11)
    assert np.array_equal(head["AUC"][2:], tail["AUC"], equal_nan=True) and np.array_equal(head["n_pos"][2:], tail["n_pos"])


def test_compare_of_a_vector_with_itself_is_all_zero():
    from molkgnn_amd import evaluation as E
    y, s = BC.case("grid8", 257)
    r = E.bootstrap_compare(y, s, s.copy(), n_boot=40, seed=2)
    for name in ("AUC", "logAUC"):
        assert r[name]["diff"].shape == (40,) and bool((r[name]["diff"] == 0).all())
        assert r[name]["ci"] == (0.0, 0.0) and r[name]["p_a_better"] == 0.0 and r[name]["mean"] == 0.0
    assert r["point"]["diff"] == {"AUC": 0.0, "logAUC": 0.0} and r["n_undefined"] == 0
    # a better vector is better in most replicates
    better = np.where(y == 1, s + 1.0, s)
    r = E.bootstrap_compare(y, better, s, n_boot=40, seed=2)
    assert r["AUC"]["p_a_better"] > 0.9 and r["AUC"]["ci"][0] > 0.0 and r["point"]["diff"]["AUC"] > 0.0


def test_the_quantile_rule_on_a_planted_vector():
    from molkgnn_amd import evaluation as E
    v = torch.tensor([float("nan"), 4.0, 0.0, 1.0, float("nan"), 3.0, 2.0], dtype=torch.float64)       # defined: 0 .. 4
    r = E._interval(v, 0.5)                                    # the 0.25 and 0.75 quantiles by the linear rule: positions 1 and 3
    assert r["ci"] == (1.0, 3.0) and r["mean"] == 2.0 and r["std"] == pytest.approx(math.sqrt(2.5), abs=1e-15)
    r = E._interval(v, 0.9)                                    # 0.05 and 0.95: positions 0.2 and 3.8
    assert r["ci"][0] == pytest.approx(0.2, abs=1e-15) and r["ci"][1] == pytest.approx(3.8, abs=1e-15)
    nothing = E._interval(torch.full((3,), float("nan"), dtype=torch.float64), 0.95)
    assert all(math.isnan(x) for x in (nothing["mean"], nothing["std"]) + nothing["ci"])


def test_metrics_layout_on_cpu_tensors():
    from molkgnn_amd import evaluation as E
    y, s = BC.case("grid8", 257)
    r = E.bootstrap_metrics(torch.from_numpy(y), torch.from_numpy(s), n_boot=50, FPR_range=(0.001, 1.0), confidence=0.9, seed=4,
                            offset=6, stratified=True)
    assert r["point"] == {"AUC": E.calculate_auc(y, s), "logAUC": E.calculate_logAUC(y, s, (0.001, 1.0))}
    ref = E.bootstrap_reference(y, s, 50, (0.001, 1.0), 4, 6, True)
    assert np.array_equal(r["replicates"]["AUC"].numpy(), ref["AUC"]) and np.array_equal(r["replicates"]["logAUC"].numpy(), ref["logAUC"])
    assert np.array_equal(r["n_pos"].numpy(), ref["n_pos"]) and r["n_pos"].dtype == torch.int32
    assert (r["seed"], r["offset"], r["n_boot"], r["n_undefined"]) == (4, 6, 50, 0)
    for name in ("AUC", "logAUC"):
        lo, hi = r[name]["ci"]
        q = np.quantile(ref[name], [0.05, 0.95])
        assert lo == pytest.approx(q[0], abs=1e-15) and hi == pytest.approx(q[1], abs=1e-15) and lo <= r[name]["mean"] <= hi


def test_per_task_offsets_and_empty_tasks():
    from molkgnn_amd import evaluation as E
    y, s = BC.case("grid8", 257)
    task = np.arange(257) % 4
    task[task == 2] = -1                                       # task 2 has no row; task 3 gets one class only
    y = y.copy()
    y[task == 3] = 0
    got = E.bootstrap_per_task(y, s, task, 4, n_boot=12, seed=8, offset=100)
    assert got[2] is None and got[3] is None
    for t in (0, 1):
        want = E.bootstrap_metrics(y[task == t], s[task == t], n_boot=12, seed=8, offset=100 + 12 * t)
        assert got[t]["offset"] == 100 + 12 * t
        assert torch.equal(got[t]["replicates"]["logAUC"], want["replicates"]["logAUC"]) and got[t]["AUC"] == want["AUC"]


def test_rejections_in_python():
    from molkgnn_amd import evaluation as E
    from molkgnn_amd import readout
    y, s = BC.case("grid8", 40)
    bad = s.copy()
    bad[3] = float("nan")
    for fn in (lambda: E.bootstrap_reference(y, bad, 4), lambda: E.bootstrap_metrics(y, bad, n_boot=4)):
        with pytest.raises(ValueError, match="NaN or an infinite"):
            fn()
    bad[3] = float("inf")
    with pytest.raises(ValueError, match="NaN or an infinite"):
        E.bootstrap_reference(y, bad, 4)
    for window in ((0.0, 0.1), (-1.0, 0.1), (0.001, 1.5), (0.1, 0.1), (0.2, 0.1)):
        for fn in (E.bootstrap_reference, lambda *a: E.bootstrap_metrics(a[0], a[1], n_boot=a[2], FPR_range=a[3])):
            with pytest.raises(ValueError, match="0 < lower < upper <= 1"):
                fn(y, s, 4, window)
    for labels in (np.zeros(40), np.ones(40)):
        with pytest.raises(ValueError, match="both classes"):
            E.bootstrap_metrics(labels, s, n_boot=4)
        with pytest.raises(ValueError, match="both classes"):
            E.bootstrap_compare(labels, s, s, n_boot=4)
    with pytest.raises(ValueError, match="at least one replicate"):
        E.bootstrap_reference(y, s, 0)
    with pytest.raises(ValueError, match="confidence"):
        E.bootstrap_metrics(y, s, n_boot=4, confidence=1.0)
    rank, ys, gl, split = (torch.from_numpy(a) if isinstance(a, np.ndarray) else a for a in BC.sorted_inputs(y, s))
    with pytest.raises(ValueError, match="evaluation.bootstrap_reference"):
        readout.bootstrap_roc(rank, ys, gl, split, 4, 0, 0, 0.001, 0.1)                 # CPU tensors at the raw operator
    with pytest.raises(ValueError, match="int32"):
        readout.bootstrap_roc(rank.long(), ys, gl, split, 4, 0, 0, 0.001, 0.1)


class _Batch:
    def __init__(self, y):
        self.y = y


class _Stub(torch.nn.Module):
    def __init__(self, preds):
        super().__init__()
        self.preds, self.loss_func, self.calls = list(preds), torch.nn.BCEWithLogitsLoss(), 0

    def predict(self, batch):
        i, self.calls = self.calls, self.calls + 1
        return self.preds[i].view(-1, 1), None


def test_evaluate_without_bootstrap_returns_todays_keys_only():
    from molkgnn_amd import evaluation as E
    from molkgnn_amd.train import evaluate
    y, s = BC.case("grid8", 40)
    ys = [torch.from_numpy(y[:25]), torch.from_numpy(y[25:])]
    preds = [torch.from_numpy(s[:25]).float(), torch.from_numpy(s[25:]).float()]
    plain = evaluate(_Stub(preds), [_Batch(v) for v in ys], metrics=("AUC",))
    none = evaluate(_Stub(preds), [_Batch(v) for v in ys], metrics=("AUC",), bootstrap=None)
    assert set(plain) == set(none) == {"loss", "AUC", "pred_y", "true_y"} and plain["AUC"] == none["AUC"]
    got = evaluate(_Stub(preds), [_Batch(v) for v in ys], metrics=("AUC",), bootstrap=16)
    assert set(got) == set(plain) | {"bootstrap"} and got["AUC"] == plain["AUC"]
    want = E.bootstrap_metrics(torch.cat(ys), torch.cat(preds), n_boot=16)
    assert torch.equal(got["bootstrap"]["replicates"]["logAUC"], want["replicates"]["logAUC"]) and got["bootstrap"]["AUC"] == want["AUC"]
    for bad in (0, -1, 2.5, True, "64"):
        model = _Stub(preds)
        with pytest.raises(ValueError, match="bootstrap"):
            evaluate(model, [_Batch(v) for v in ys], bootstrap=bad)
        assert model.calls == 0                                # refused before a batch is run
