"""The regression bootstrap on the host: ``evaluation.regression_reference`` + ``regression_derived`` against explicit resampling
followed by numpy and scipy (integers EQUAL, Spearman within 1e-14, the moment-derived metrics within 1e-12), the top-k hits
against the intersection of explicit sets of copies, the draw, the degenerate folds, the names, the refusals (the C entry's too:
they come before any launch and read no pointer), and ``train.evaluate`` with stub models."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from tests import _bootstrap_cases as BC
from tests import _regression_cases as RC

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
METRICS = ("RMSE", "MAE", "R2", "pearson", "spearman")


def _derived(ref, cuts):
    from molkgnn_amd import evaluation as E
    return {k: v.numpy() for k, v in E.regression_derived(ref["mom"], ref["rank_sums"], ref["hits"], ref["n_drawn"], cuts).items()}


@pytest.mark.parametrize("block", range(4))
def test_definition_against_explicit_resampling(block):
    from molkgnn_amd import evaluation as E
    worst = dict.fromkeys(METRICS, 0.0)
    for case in range(block * 25, block * 25 + 25):
        t, p, lower = RC.small_fold(case)
        n, B = t.size, 6
        cuts = (1, max(1, n // 3), n)
        ref = E.regression_reference(t, p, B, cuts, seed=3, offset=case, lower_is_better=lower)
        want = RC.brute_force(t, p, B, cuts, 3, case, lower)
        assert ref["hits"].dtype == np.int64 and ref["rank_sums"].dtype == np.int64 and ref["n_drawn"].dtype == np.int32
        assert np.array_equal(ref["hits"], want["hits"]), case             # the closed form = the intersection of the copy sets
        assert (ref["n_drawn"] == n).all()
        got = _derived(ref, cuts)
        for name in METRICS:
            assert np.array_equal(np.isnan(got[name]), np.isnan(want[name])), (case, name)
            live = ~np.isnan(want[name])
            err = float(np.abs(got[name][live] - want[name][live]).max(initial=0.0))
            worst[name] = max(worst[name], err)
            assert err <= (RC.SPEARMAN_TOL if name == "spearman" else RC.MOMENT_TOL), (case, name, err)
        assert np.array_equal(got["top"], want["hits"] / np.array(cuts, dtype=np.float64))
        # sum c a = sum c b = 0 holds identically; here through Cauchy-Schwarz on the exact integers
        xy, xx, yy = (ref["rank_sums"][:, k].astype(object) for k in range(3))
        assert all(a * a <= b * c for a, b, c in zip(xy, xx, yy))
    print(f"block {block}: largest |definition - explicit| {worst}")


def test_the_draw_is_the_classification_bootstraps():
    from molkgnn_amd import evaluation as E
    for n in (1, 2, 5, 257, 1030):
        for offset in (0, 9, 1 << 40):
            assert np.array_equal(E.bootstrap_draw(n, n, 7, offset), RC.draws(n, 7, offset))
    # a regression fold and a classification fold with the same (seed, offset, n) see the same rows
    y, s = BC.case("grid8", 300)
    t, p = RC.case("grid", 300)
    roc = E.bootstrap_reference(y, s, 5, seed=7, offset=2)
    reg = E.regression_reference(t, p, 5, (), seed=7, offset=2)
    for b in range(5):
        idx = E.bootstrap_draw(300, 300, 7, 2 + b)
        assert roc["n_pos"][b] == int(y[idx].sum())
        assert abs(reg["mom"][b, 5] - np.abs(p[idx] - t[idx]).sum()) <= 1e-10


def test_degenerate_folds():
    from molkgnn_amd import evaluation as E
    t = np.array([0.5, -1.0, 2.0, 0.25, 3.0])
    for name, tt, pp, const_p, const_t in (("constant p", t, np.full(5, 1.5), True, False), ("constant t", np.full(5, -2.0), t, False, True),
                                           ("n = 1", np.array([2.0]), np.array([3.0]), True, True)):
        ref = E.regression_reference(tt, pp, 8, (1,), seed=1)
        xy, xx, yy = ref["rank_sums"].T
        assert (xy == 0).all(), name
        assert (xx == 0).all() if const_p else (xx > 0).any(), name
        assert (yy == 0).all() if const_t else (yy > 0).any(), name
        d = _derived(ref, (1,))
        assert np.isnan(d["spearman"]).all() and np.isnan(d["pearson"]).all(), name
        assert np.isnan(d["R2"]).all() == const_t, name
        assert not np.isnan(d["RMSE"]).any() and not np.isnan(d["MAE"]).any() and not np.isnan(d["top"]).any(), name
        point = E.regression_points(tt, pp, (0.5,))
        assert math.isnan(point["spearman"]) and math.isnan(point["pearson"]) and math.isnan(point["R2"]) == const_t, name
    assert E.regression_points([2.0], [3.0])["RMSE"] == 1.0 and E.calculate_mae([2.0, 4.0], [3.0, 2.0]) == 1.5
    # a replicate that happens to be constant is NaN by its exact rank sum, not by the sign of a rounded variance
    ref = E.regression_reference(np.array([0.1, 0.7]), np.array([0.3, 0.2]), 32, (), seed=0)
    d = _derived(ref, ())
    constant = ref["rank_sums"][:, 1] == 0
    assert constant.any() and not constant.all()
    assert np.array_equal(np.isnan(d["pearson"]), constant) and np.array_equal(np.isnan(d["spearman"]), constant)


def test_point_estimates_against_scipy():
    from scipy import stats
    from molkgnn_amd import evaluation as E
    for kind, n, lower in (("distinct", 300, True), ("grid", 300, False), ("grid", 1025, True)):
        t, p = RC.case(kind, n)
        assert abs(E.calculate_spearman(t, p) - stats.spearmanr(p, t)[0]) <= RC.SPEARMAN_TOL
        assert abs(E.calculate_pearson(t, p) - stats.pearsonr(p, t)[0]) <= RC.MOMENT_TOL
        assert abs(E.calculate_mae(t, p) - np.abs(p - t).mean()) <= RC.MOMENT_TOL
        assert abs(E.calculate_r2(t, p) - (1.0 - np.sum((p - t) ** 2) / np.sum((t - t.mean()) ** 2))) <= RC.MOMENT_TOL
        assert abs(E.regression_points(t, p)["RMSE"] - E.calculate_rmse(t, p)) <= RC.MOMENT_TOL
        k = E.early_cut(0.05, n)
        sign = 1.0 if lower else -1.0
        best_p = set(sorted(range(n), key=lambda i: (sign * p[i], i))[:k])
        best_t = set(sorted(range(n), key=lambda i: (sign * t[i], i))[:k])
        assert E.calculate_top_recall(t, p, 0.05, lower) == len(best_p & best_t) / k
        # float32 predictions on torch tensors: the same numbers as their float64 copies
        p32 = torch.from_numpy(p).float()
        assert E.calculate_spearman(torch.from_numpy(t), p32) == E.calculate_spearman(t, p32.double().numpy())


def test_cuts_and_names():
    from molkgnn_amd import evaluation as E
    from molkgnn_amd.train import _check_metrics
    assert E.top_name(0.01) == "top_0.01" and E.top_name(1) == "top_1.0" and E.parse_top_name("top_0.010") == 0.01
    assert E.is_top_name("top_0.5") and not E.is_top_name("EF_0.5") and not E.is_top_name("topmost") and not E.is_top_name(3)
    for bad in ("top_", "top_x", "top_0", "top_1.5", "top_-0.1", "top_nan", "TOP_0.1", "top", None):
        with pytest.raises(ValueError):
            E.parse_top_name(bad)
    t, p = (torch.from_numpy(v) for v in RC.case("grid", 300))
    r = E.bootstrap_regression(t, p, n_boot=4, top=(0.01, 0.1, 0.010, 1.0))
    assert r["cuts"] == {"top_0.01": E.early_cut(0.01, 300), "top_0.1": E.early_cut(0.1, 300), "top_1.0": 300}
    assert r["cuts"]["top_0.01"] == 3
    assert bool((r["replicates"]["top_1.0"] == 1.0).all()) and r["point"]["top_1.0"] == 1.0
    nine = tuple(0.01 * i for i in range(1, 10))
    for kw, text in ((dict(top=nine), "distinct fractions"), (dict(top=(2.0,)), "fraction"), (dict(top=0.01), "tuple of fractions"),
                     (dict(n_boot=0), "at least one replicate"), (dict(confidence=1.0), "confidence"), (dict(seed=-1), "64-bit")):
        for fn in (lambda **k: E.bootstrap_regression(t, p, **k), lambda **k: E.bootstrap_regression_compare(t, p, p, **k)):
            with pytest.raises(ValueError, match=text):
                fn(**dict(dict(n_boot=2), **kw))
    for bad in (float("nan"), float("inf")):
        q = p.clone()
        q[7] = bad
        for args in ((t, q), (q, p)):
            with pytest.raises(ValueError, match="NaN or an infinite"):
                E.bootstrap_regression(*args, n_boot=2)
    with pytest.raises(ValueError, match="differ in length"):
        E.bootstrap_regression(t[:-1], p, n_boot=2)
    with pytest.raises(ValueError, match="rows"):
        E.bootstrap_regression(t[:0], p[:0], n_boot=2)
    with pytest.raises(ValueError, match="rows"):
        E._check_regression_sizes((1 << 20) + 1, 1, 0, 0)
    E._check_regression_sizes(1 << 20, 1, 0, 0)
    # the evaluate family's metric table
    table = _check_metrics(("RMSE", "MAE", "R2", "pearson", "spearman", "top_0.05"), lower_is_better=False)
    tn, pn = RC.case("grid", 300)
    assert table["MAE"](tn, pn) == E.calculate_mae(tn, pn) and table["R2"](tn, pn) == E.calculate_r2(tn, pn)
    assert table["pearson"](tn, pn) == E.calculate_pearson(tn, pn) and table["spearman"](tn, pn) == E.calculate_spearman(tn, pn)
    assert table["top_0.05"](tn, pn) == E.calculate_top_recall(tn, pn, 0.05, False) != E.calculate_top_recall(tn, pn, 0.05, True)
    assert set(_check_metrics(("AUC",))) == set(_check_metrics(()))                 # naming none adds none
    for bad, text in ((("top_3",), "fraction"), (("top_x",), "top_<number>"), (("MAE", "oops"), "unknown metric"),
                      (tuple(f"top_0.0{i}" for i in range(1, 10)), "distinct top fractions")):
        with pytest.raises(ValueError, match=text):
            _check_metrics(bad)


def test_bootstrap_regression_and_compare_on_the_host():
    from molkgnn_amd import evaluation as E
    t, p = (torch.from_numpy(v) for v in RC.case("grid", 300))
    r = E.bootstrap_regression(t, p, n_boot=32, confidence=0.9, seed=5, offset=9, top=(0.05,), lower_is_better=False)
    names = METRICS + ("top_0.05",)
    assert list(r) == ["point", "replicates", "n_undefined", "cuts", "n_drawn", "seed", "offset", "n_boot", "confidence",
                       "lower_is_better"] + list(names)
    assert (r["seed"], r["offset"], r["n_boot"], r["confidence"], r["lower_is_better"]) == (5, 9, 32, 0.9, False)
    assert r["n_undefined"] == dict.fromkeys(names, 0) and set(r["point"]) == set(names) == set(r["replicates"])
    k = E.early_cut(0.05, 300)
    assert r["cuts"] == {"top_0.05": k}
    ref = E.regression_reference(t, p, 32, (k,), seed=5, offset=9, lower_is_better=False)
    d = E.regression_derived(ref["mom"], ref["rank_sums"], ref["hits"], ref["n_drawn"], (k,))
    assert all(torch.equal(r["replicates"][k], d[k]) for k in METRICS) and torch.equal(r["replicates"]["top_0.05"], d["top"][:, 0])
    for name in names:
        assert set(r[name]) == {"mean", "std", "ci"} and r[name]["ci"][0] <= r[name]["mean"] <= r[name]["ci"][1], name
        assert r[name]["ci"][0] <= r["point"][name] + 0.2 and r["point"][name] - 0.2 <= r[name]["ci"][1], name
    assert r["point"]["RMSE"] == pytest.approx(E.calculate_rmse(t, p), abs=1e-12)
    # the paired form: antisymmetric, a - a = 0, and a worse model is seen as worse
    worse = p + torch.from_numpy(np.random.default_rng(1).normal(size=300))
    ab = E.bootstrap_regression_compare(t, p, worse, n_boot=32, seed=5, top=(0.05,))
    ba = E.bootstrap_regression_compare(t, worse, p, n_boot=32, seed=5, top=(0.05,))
    for name in names:
        assert torch.equal(ab[name]["diff"], -ba[name]["diff"]), name
        assert ab["point"]["diff"][name] == -ba["point"]["diff"][name]
        ties = float((ab[name]["diff"] == 0).double().mean())
        assert ab[name]["p_a_better"] + ba[name]["p_a_better"] == pytest.approx(1.0 - ties), name
        assert ab[name]["ci"][0] == pytest.approx(-ba[name]["ci"][1]) and ab[name]["mean"] == pytest.approx(-ba[name]["mean"])
    assert ab["RMSE"]["p_a_better"] == 1.0 and ab["MAE"]["p_a_better"] == 1.0 and bool((ab["RMSE"]["diff"] < 0).all())
    assert ab["spearman"]["p_a_better"] == 1.0 and ab["R2"]["p_a_better"] == 1.0 and ab["cuts"] == {"top_0.05": k}
    same = E.bootstrap_regression_compare(t, p, p.clone(), n_boot=8)
    assert all(bool((same[k]["diff"] == 0).all()) and same[k]["p_a_better"] == 0.0 for k in METRICS)


def test_entry_points_are_declared_typed_and_additive_to_abi_8():
    from molkgnn_amd import _lib
    from molkgnn_amd import evaluation as E
    with open(os.path.join(REPO, "include", "molkgnn_hip.h")) as f:
        h = f.read()
    assert re.search(r"\bsize_t mkgnn_bootstrap_regression_workspace_bytes\(int64_t n, int32_t replicates_per_pass\);", h)
    assert re.search(r"\bint mkgnn_bootstrap_regression\(const int32_t\* rank_p, const int32_t\* first_p, const int32_t\* last_p, "
                     r"const int32_t\* cross,\s+const int32_t\* first_t, const int32_t\* last_t, const double\* p_sorted, "
                     r"const double\* t_by_prank,\s+const double\* centre, const int32_t\* cuts, int32_t J, int64_t n, int32_t B, "
                     r"uint64_t seed,\s+uint64_t offset, double\* mom, int64_t\* rank_sums, int64_t\* hits, int32_t\* n_drawn, "
                     r"void\* workspace,\s+size_t workspace_bytes, void\* stream\);", h)
    m = re.search(r"#define\s+MKGNN_ABI_VERSION\s+(\d+)", h)
    assert m and int(m.group(1)) == 8 and _lib.ABI_VERSION == 8
    d = re.search(r"#define\s+MKGNN_BOOTSTRAP_REG_MAX_ROWS\s+(\d+)", h)
    assert d and int(d.group(1)) == _lib.BOOTSTRAP_REG_MAX_ROWS == E.BOOTSTRAP_REG_MAX_ROWS == 1 << 20
    assert (1 << 20) * ((1 << 20) - 1) ** 2 < 1 << 63 <= (1 << 22) * ((1 << 22) - 1) ** 2       # why the limit is where it is
    for name in ("mkgnn_bootstrap_regression", "mkgnn_bootstrap_regression_workspace_bytes"):
        assert name in _lib.EXPORTS
    assert len(set(_lib.EXPORTS)) == len(_lib.EXPORTS)
    lib = _lib.load()
    P, I32, I64, U64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_uint64
    assert lib.mkgnn_bootstrap_regression.argtypes == [P] * 10 + [I32, I64, I32, U64, U64, P, P, P, P, P, ctypes.c_size_t, P]
    assert lib.mkgnn_bootstrap_regression.restype is ctypes.c_int
    size = lib.mkgnn_bootstrap_regression_workspace_bytes
    assert size(1, 1) == 32 and size(5, 3) == 3 * 64 and size(1 << 20, 2) == 2 * 8 * (1 << 20) and size(8193, 1) == 8 * 8196
    assert size(0, 1) == 0 and size((1 << 20) + 1, 1) == 0 and size(8, 0) == 0 and size(8, 4097) == 0


def test_rejections_before_a_launch_at_the_c_entry():
    """Checked before anything is launched: no device needed (no pointer is read)."""
    from molkgnn_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_uint64 * 256)()
    p = ctypes.addressof(buf)
    p += -p % 16
    ok = dict(rank_p=p, first_p=p + 32, last_p=p + 64, cross=p + 96, first_t=p + 128, last_t=p + 160, p_sorted=p + 192, t_by_prank=p + 256,
              centre=p + 320, cuts=p + 336, J=2, n=8, B=2, seed=1, offset=0, mom=p + 352, rank_sums=p + 464, hits=p + 512, n_drawn=p + 544,
              ws=p + 560, wsb=128, stream=None)
    order = ("rank_p", "first_p", "last_p", "cross", "first_t", "last_t", "p_sorted", "t_by_prank", "centre", "cuts", "J", "n", "B", "seed",
             "offset", "mom", "rank_sums", "hits", "n_drawn", "ws", "wsb", "stream")

    def call(**kw):
        a = dict(ok, **kw)
        rc = lib.mkgnn_bootstrap_regression(*(a[k] for k in order))
        return rc, lib.mkgnn_last_error().decode()
    cells = [(dict(n=0), "rows outside"), (dict(n=(1 << 20) + 1), "rows outside"), (dict(B=0), "replicates outside"),
             (dict(B=4097), "replicates outside"), (dict(J=-1), "cuts outside"), (dict(J=9), "cuts outside"),
             (dict(cuts=None), "null pointer"), (dict(hits=None), "null pointer"), (dict(ws=None), "null workspace"),
             (dict(ws=p + 564), "16-byte aligned"), (dict(wsb=63), "workspace of 63 bytes, 64 needed"), (dict(wsb=0), "workspace of 0 bytes"),
             (dict(mom=p), "aliases an input"), (dict(hits=p + 320), "aliases an input"), (dict(n_drawn=p + 336), "aliases an input"),
             (dict(ws=p + 192), "aliases an input"), (dict(rank_sums=p + 352), "alias each other"), (dict(ws=p + 544), "alias each other"),
             (dict(hits=p + 464), "alias each other")]
    cells += [({k: None}, "null pointer") for k in order[:9] + ("mom", "rank_sums", "n_drawn")]
    cells += [({k: ok[k] + 2}, "misaligned") for k in order[:6] + ("cuts", "n_drawn")]
    cells += [({k: ok[k] + 4}, "misaligned") for k in ("p_sorted", "t_by_prank", "centre", "mom", "rank_sums", "hits")]
    for kw, text in cells:
        rc, msg = call(**kw)
        assert rc != 0 and text in msg and "mkgnn_bootstrap_regression" in msg, (kw, rc, msg)


class _Stub(torch.nn.Module):
    """What ``train.evaluate`` asks of a model: ``predict``, ``loss_func``, ``_loss_kind`` and the training flag."""

    def __init__(self, loss_func, kind):
        super().__init__()
        self.loss_func, self._kind = loss_func, kind

    def _loss_kind(self):
        return self._kind

    def predict(self, batch):
        return batch.pred, None


class _Batch:
    def __init__(self, pred, y):
        self.pred, self.y = pred, y


def test_evaluate_with_stub_models():
    from molkgnn_amd import evaluation as E
    from molkgnn_amd.train import evaluate
    t, p = (torch.from_numpy(v).float() for v in RC.case("grid", 300))
    batches = [_Batch(p[:128], t[:128]), _Batch(p[128:], t[128:])]
    names = ("RMSE", "MAE", "R2", "pearson", "spearman", "top_0.05", "top_0.2")
    for kind, loss in (("mse", torch.nn.MSELoss()), ("mse_sum", torch.nn.MSELoss(reduction="sum"))):
        model = _Stub(loss, kind).train()
        got = evaluate(model, batches, names, bootstrap=16, lower_is_better=False)
        assert model.training
        want = E.bootstrap_regression(t, p, n_boot=16, top=(0.05, 0.2), lower_is_better=False)
        assert list(got["bootstrap"]) == list(want) and got["bootstrap"]["cuts"] == {"top_0.05": E.early_cut(0.05, 300), "top_0.2": E.early_cut(0.2, 300)}
        for name in names:
            assert torch.equal(got["bootstrap"]["replicates"][name], want["replicates"][name]), name
            assert got[name] == want["point"][name] == got["bootstrap"]["point"][name], name
            assert got["bootstrap"][name] == want[name]
        assert got["top_0.05"] == E.calculate_top_recall(t, p, 0.05, False)
        plain = evaluate(model, batches, ("RMSE",))
        assert "bootstrap" not in plain and set(plain) == {"loss", "RMSE", "pred_y", "true_y"} and plain["RMSE"] == got["RMSE"]
        assert list(evaluate(model, batches, ("RMSE",), bootstrap=4)["bootstrap"]["cuts"]) == []       # no 'top_' named: none handed on
    # a BCE model: today's result, bit for bit, whatever lower_is_better says; the new names are metrics like any other
    y = (t > 0).float()
    bce = _Stub(torch.nn.BCEWithLogitsLoss(), "bce")
    cls_batches = [_Batch(p[:128], y[:128]), _Batch(p[128:], y[128:])]
    got = evaluate(bce, cls_batches, ("AUC", "EF_0.05"), bootstrap=16, lower_is_better=False)
    want = E.bootstrap_metrics(y, p, n_boot=16, early=("EF_0.05",))
    assert list(got) == ["loss", "AUC", "EF_0.05", "bootstrap", "pred_y", "true_y"] and list(got["bootstrap"]) == list(want)
    assert got["AUC"] == E.calculate_auc(y, p) and float(got["loss"]) == float(torch.nn.BCEWithLogitsLoss()(p, y))
    for key in ("AUC", "logAUC", "EF_0.05"):
        assert torch.equal(got["bootstrap"]["replicates"][key].view(torch.int64), want["replicates"][key].view(torch.int64)), key
        assert got["bootstrap"][key] == want[key] and got["bootstrap"]["point"][key] == want["point"][key]
    assert torch.equal(got["bootstrap"]["n_pos"], want["n_pos"])
    assert evaluate(bce, cls_batches, ("AUC", "MAE"))["MAE"] == E.calculate_mae(y, p)
    with pytest.raises(ValueError, match="unknown metric"):
        evaluate(bce, cls_batches, ("top",))
