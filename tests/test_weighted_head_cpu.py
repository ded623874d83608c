"""The weighted losses of the HIP head and fused tail, everything that needs no GPU: the torch definition
(``readout.task_head_reference`` with ``sample_weight`` / ``weight_table`` / ``pos_weight``) against PyTorch's own weighted
losses, the C ABI's declarations and exports, the argument checks of the raw entry points, ``GNNModel``'s loss selectors,
``sampling.pos_weights``, the resident shard's weights and the refusals."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import _weighted_head_cases as WC

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("mkgnn_task_head_weighted_forward", "mkgnn_task_head_weighted_backward", "mkgnn_task_head_weighted_fused",
           "mkgnn_tail_fused_weighted")


def _leaves(i, dtype=torch.float64):
    d = lambda t: None if t is None else t.detach().clone().to(dtype)
    emb, w = d(i["emb"]).requires_grad_(True), d(i["w"]).requires_grad_(True)
    b = None if i["b"] is None else d(i["b"]).requires_grad_(True)
    return emb, w, b, d


def _close(got, want, tol=1e-12):
    assert float((got - want).abs().max()) <= tol * max(1.0, float(want.abs().max())), (float((got - want).abs().max()),)


# ------------------------------------------------------------------------------------------ the definition --
def test_definition_is_torchs_weighted_bce_for_one_task():
    """T = 1, n = 577, zeros among the weights, p = 37.5, float64: value and gradients of
    ``binary_cross_entropy_with_logits(x, y, weight=s, pos_weight=p)`` (mean over the rows, not over the sum of the weights)."""
    from molkgnn_amd.readout import task_head_reference
    g = torch.Generator().manual_seed(11)
    n, H = 577, 5
    emb = torch.randn(n, H, generator=g, dtype=torch.float64).requires_grad_(True)
    w = torch.randn(1, H, generator=g, dtype=torch.float64).requires_grad_(True)
    b = torch.randn(1, generator=g, dtype=torch.float64).requires_grad_(True)
    y = (torch.rand(n, generator=g) < 0.3).double()
    s = torch.rand(n, generator=g, dtype=torch.float64) * 3
    s[::7] = 0.0
    p = torch.tensor([37.5], dtype=torch.float64)
    for kw, tkw in ((dict(sample_weight=s, pos_weight=p), dict(weight=s, pos_weight=p)), (dict(pos_weight=p), dict(pos_weight=p)),
                    (dict(sample_weight=s), dict(weight=s))):
        loss, pred = task_head_reference(emb, w, b, y, None, "bce", **kw)
        got = torch.autograd.grad(loss, [emb, w, b])
        x = (emb @ w.T + b).view(-1)
        want_loss = F.binary_cross_entropy_with_logits(x, y, **tkw)
        want = torch.autograd.grad(want_loss, [emb, w, b])
        _close(pred.detach(), x.detach(), 1e-14)
        _close(loss.detach(), want_loss.detach(), 1e-14)
        for a, c in zip(got, want):
            _close(a, c, 1e-14)


def test_definition_is_torchs_weighted_bce_column_by_column():
    """T = 9 with masked rows: per task the SUM form of torch's loss over that task's rows, added up and divided by the number
    of labelled rows."""
    from molkgnn_amd.readout import task_head_reference
    name = "B577xH64xT9_quarter_unlabelled_table_pos"
    c, i = WC.CASES[name], WC.inputs(name, "bce")
    legs = []
    for how in ("reference", "torch"):
        emb, w, b, d = _leaves(i)
        if how == "reference":
            loss, _ = task_head_reference(emb, w, b, d(i["y"]), i["task"], "bce", d(i["keep"]), c.B, i["task_table"], i["row_ids"],
                                          **WC.weight_keywords(i, d))
        else:
            task, lab = i["task_direct"][:c.B].long(), i["lab"]
            out = F.linear(emb[:c.B] * d(i["keep"]), w, b)
            total = 0.0
            for t in range(c.T):
                rows = lab & (task == t)
                if bool(rows.any()):
                    total = total + F.binary_cross_entropy_with_logits(out[rows, t], d(i["y"][:c.B])[rows], weight=d(i["s_eff"])[rows],
                                                                        pos_weight=d(i["pos"])[t], reduction="sum")
            loss = total / int(lab.sum())
        loss.backward()
        legs.append([loss.detach(), emb.grad, w.grad, b.grad])
    assert int((~i["lab"]).sum()) > 0 and int((i["s_eff"] == 0).sum()) > 0
    for got, want in zip(*legs):
        _close(got, want)


@pytest.mark.parametrize("kind", ["mse", "mse_sum"])
def test_definition_is_the_weighted_squared_error(kind):
    from molkgnn_amd.readout import task_head_reference
    name = "B17xH5xT1_all_one_row"
    c, i = WC.CASES[name], WC.inputs(name, kind)
    emb, w, b, d = _leaves(i)
    loss, pred = task_head_reference(emb, w, b, d(i["y"]), i["task"], kind, None, c.B, **WC.weight_keywords(i, d))
    x = (emb[:c.B] @ w.T + b).view(-1)
    s, y = d(i["s_eff"]), d(i["y"][:c.B])
    want = (s * (x - y) ** 2).sum()
    if kind == "mse":
        want = want / c.B
    _close(loss.detach(), want.detach())
    for a, e in zip(torch.autograd.grad(loss, [emb, w, b]), torch.autograd.grad(want, [emb, w, b])):
        _close(a, e)


@pytest.mark.parametrize("name,kind", [p for p in WC.PAIRS if WC.CASES[p[0]].B <= 577])
def test_all_ones_weights_are_no_weights(name, kind):
    """Weights of exactly 1 (per row, and as a table) and no weights: ``torch.equal`` loss, pred and gradients, in float32."""
    from molkgnn_amd.readout import task_head_reference
    c, i = WC.CASES[name], WC.inputs(name, kind)
    pos = i["pos"]
    legs = []
    # (grad W and grad b are index_put accumulations, whose order -- and so whose bits -- is only fixed on one thread)
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        _all_ones_legs(c, i, kind, pos, legs)
    finally:
        torch.set_num_threads(threads)
    for other in legs[1:]:
        for a, e in zip(legs[0], other):
            assert torch.equal(a, e), (name, kind)


def _all_ones_legs(c, i, kind, pos, legs):
    from molkgnn_amd.readout import task_head_reference
    for how in ("none", "row", "table"):
        emb, w, b, d = _leaves(i, torch.float32)
        kw = dict(pos_weight=pos)
        ids = i["row_ids"] if i["task_table"] is not None else None
        if how == "row":
            kw["sample_weight"] = torch.ones(c.B + c.n_pad)
        elif how == "table":
            if i["task_table"] is not None:
                continue                                   # (its ids leave the table on purpose: those rows would weigh 0)
            kw["weight_table"], ids = torch.ones(4), torch.arange(c.B + c.n_pad, dtype=torch.int32) % 4
        loss, pred = task_head_reference(emb, w, b, i["y"], i["task"], kind, i["keep"], c.B, i["task_table"], ids, **kw)
        loss.backward()
        legs.append([loss.detach(), pred.detach(), emb.grad, w.grad] + ([] if b is None else [b.grad]))


@pytest.mark.parametrize("name,kind", [p for p in WC.PAIRS if WC.CASES[p[0]].B <= 577])
def test_reference_keeps_the_zero_and_nan_rules(name, kind):
    """Nothing NaN although y, the weights and the ids are NaN / sentinels wherever they must not be used; rows with the weight 0,
    unlabelled rows and rows >= n_rows have an all-zero grad_emb row; tasks whose rows all weigh 0 have zero grad rows."""
    c, i = WC.CASES[name], WC.inputs(name, kind)
    task = i["task_direct"][:c.B]
    for leg in WC.reference(name, kind):
        for nm, v in leg.items():
            assert bool(torch.isfinite(v).all()), (name, nm)
        dead = ~i["lab"] | (i["s_eff"] == 0)
        assert float(leg["emb"][c.B:].abs().sum()) == 0.0
        if bool(dead.any()):
            assert float(leg["emb"][:c.B][dead].abs().sum()) == 0.0
        silent = torch.tensor([not bool(((task == t) & ~dead).any()) for t in range(c.tasks)])
        if bool(silent.any()):
            assert float(leg["w"].reshape(c.tasks, c.H)[silent].abs().sum()) == 0.0
            if c.bias:
                assert float(leg["b"][silent].abs().sum()) == 0.0
    if c.zero_task is not None:
        assert bool(silent[c.zero_task]) and bool((i["lab"] & (task == c.zero_task)).any())


def test_a_nan_weight_on_a_labelled_row_propagates():
    from molkgnn_amd.readout import task_head_reference
    i = WC.inputs("B17xH5xT1_all_one_row", "bce")
    s = i["s"].clone()
    s[4] = float("nan")
    loss, _ = task_head_reference(i["emb"], i["w"], i["b"], i["y"], i["task"], "bce", None, 17, sample_weight=s)
    assert bool(torch.isnan(loss))


def test_saturated_logits_with_a_positive_weight():
    """x = -90, y = 1, p = 37.5: the term is exactly 3375 (one-hot sample weights single it out); every gradient is finite."""
    from molkgnn_amd.readout import task_head_reference
    c, i = WC.SATURATED, WC.inputs(WC.SATURATED.name, "bce")
    for f32, f64 in (WC.reference(c.name, "bce"),):
        for leg in (f32, f64):
            assert leg["pred"][:6].tolist() == list(WC.SATURATED_LOGITS)
            for nm, v in leg.items():
                assert bool(torch.isfinite(v).all()), nm
    onehot = torch.zeros(c.B)
    onehot[WC.SATURATED_ROW] = 1.0
    for dt in (torch.float32, torch.float64):
        d = lambda t: None if t is None else t.to(dt)
        loss, _ = task_head_reference(d(i["emb"]), d(i["w"]), None, d(i["y"]), i["task"], "bce", None, c.B, sample_weight=d(onehot),
                                      pos_weight=d(i["pos"]))
        assert float(loss) == float(torch.tensor(WC.SATURATED_TERM, dtype=dt) / c.B)
    # d term / d x at the six rows: (1 - y) - L sigmoid(-x), L = 1 + 36.5 y
    sig_neg = {90.0: 0.0, -90.0: 1.0, 0.0: 0.5}
    want = torch.tensor([(1 - y) - (1 + (WC.SATURATED_POS - 1) * y) * sig_neg[x] for x, y in zip(WC.SATURATED_LOGITS, WC.SATURATED_TARGETS)],
                        dtype=torch.float64)
    _, f64 = WC.reference(c.name, "bce")
    got = f64["emb"][:6, 0] * c.B / 90.0                     # d loss / d emb[r, 0] = d term / d x * W[1, 0] / n_lab
    _close(got, want, 1e-13)


def test_weights_are_read_through_a_table():
    from molkgnn_amd.readout import task_head_reference
    name = "B16xH31xT9_sorted_table_pos"
    i = WC.inputs(name, "bce")
    a = task_head_reference(i["emb"], i["w"], i["b"], i["y"], i["task"], "bce", None, 16, row_ids=i["row_ids"], weight_table=i["weight_table"],
                            pos_weight=i["pos"])
    b = task_head_reference(i["emb"], i["w"], i["b"], i["y"], i["task"], "bce", None, 16, sample_weight=i["s_eff"], pos_weight=i["pos"])
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    ids = i["row_ids"][:16]
    assert len(set(ids.tolist())) < 16 and bool(((ids < 0) | (ids >= 32)).any()) and float(i["s_eff"][3]) == 0.0


# ------------------------------------------------------------------------------------------------ the ABI --
def test_header_declares_the_entry_points_and_abi_stays_8():
    text = open(os.path.join(REPO, "include", "molkgnn_hip.h")).read()
    for name in ENTRIES:
        assert re.search(r"\bint " + name + r"\(", text), name
    assert re.search(r"typedef struct mkgnn_loss_weights \{[^}]*sample_weight;[^}]*weight_ids;[^}]*n_sample_weight;[^}]*pos_weight;[^}]*\}",
                     text)
    assert re.search(r"#define MKGNN_ABI_VERSION 8\b", text)


def test_library_exports_the_entry_points():
    from molkgnn_amd import _lib
    assert _lib.ABI_VERSION == 8
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRIES:
        assert name in _lib.EXPORTS, name
        assert hasattr(raw, name), name
    assert _lib.load().mkgnn_abi_version() == 8
    assert [f[0] for f in _lib.LossWeights._fields_] == ["sample_weight", "weight_ids", "n_sample_weight", "pos_weight"]
    assert ctypes.sizeof(_lib.LossWeights) == 32


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """No GPU is touched: every argument check comes before a launch.  An unknown kind, ``pos_weight`` with a squared-error kind, a
    null task with T != 1 (or with row_ids), ``n_sample_weight`` < 1 (ids) or < n_rows (no ids), and the unweighted limits."""
    from molkgnn_amd import _lib
    lib = _lib.load()
    buf = np.zeros(1 << 16, dtype=np.uint8)
    p = buf.ctypes.data

    def weights(sw=None, ids=None, n=0, pw=None):
        lw = _lib.LossWeights()
        lw.sample_weight, lw.weight_ids, lw.n_sample_weight, lw.pos_weight = sw, ids, n, pw
        return lw

    ok = dict(kind=0, H=4, T=1, task=None, ids=None, n_task=0, lw=weights(sw=p, n=8))
    bad = (dict(kind=7), dict(kind=-1), dict(kind=1, lw=weights(pw=p)), dict(kind=2, lw=weights(pw=p)), dict(T=2), dict(ids=p),
           dict(lw=weights(sw=p, n=7)), dict(lw=weights(sw=p, ids=p, n=0)), dict(T=33, task=p, n_task=8), dict(H=65), dict(H=0),
           dict(task=p, n_task=7))
    for change in bad:
        a = dict(ok, **change)
        es = 4 if a["H"] <= 4 else a["H"]
        lw = ctypes.byref(a["lw"])
        rc = lib.mkgnn_task_head_weighted_forward(a["kind"], p, es, 8, a["H"], a["T"], p, p, p, a["task"], a["ids"], a["n_task"], 0.0, None,
                                                  None, p, p, lw, p, buf.nbytes, None)
        assert rc != 0 and lib.mkgnn_last_error(), change
        rc = lib.mkgnn_task_head_weighted_fused(a["kind"], p, es, 8, a["H"], a["T"], p, p, p, a["task"], a["ids"], a["n_task"], 0.0, None,
                                                None, p, p, p, 4, p, p, lw, p, buf.nbytes, None)
        assert rc != 0 and lib.mkgnn_last_error(), change
        rc = lib.mkgnn_task_head_weighted_backward(a["kind"], p, es, 8, a["H"], a["T"], p, p, a["task"], a["ids"], a["n_task"], p, p, 0.0,
                                                   None, p, 4, p, p, lw, p, buf.nbytes, None)
        assert rc != 0 and lib.mkgnn_last_error(), change
    # n_rows == 0: as the unweighted entry
    rc = lib.mkgnn_task_head_weighted_forward(0, p, 4, 0, 4, 1, p, p, p, None, None, 0, 0.0, None, None, p, p, None, p, buf.nbytes, None)
    assert rc != 0 and rc == lib.mkgnn_task_head_forward(0, p, 4, 0, 4, 1, p, p, p, p, None, 8, 0.0, None, None, p, p, p, buf.nbytes, None)


# -------------------------------------------------------------------------------------------- the refusals --
def test_python_refusals():
    from molkgnn_amd.readout import task_head_reference
    i = WC.inputs("B17xH5xT1_all_one_row", "bce")
    args = (i["emb"], i["w"], i["b"], i["y"], i["task"])
    with pytest.raises(ValueError, match="gradient"):
        task_head_reference(*args, "bce", None, 17, sample_weight=i["s"].clone().requires_grad_(True))
    with pytest.raises(ValueError, match="gradient"):
        task_head_reference(*args, "bce", None, 17, pos_weight=torch.ones(1, requires_grad=True))
    with pytest.raises(ValueError, match="gradient"):
        task_head_reference(*args, "bce", None, 17, weight_table=torch.ones(4, requires_grad=True), row_ids=torch.zeros(17, dtype=torch.int32))
    for kind in ("mse", "mse_sum"):
        with pytest.raises(ValueError, match="pos_weight"):
            task_head_reference(*args, kind, None, 17, pos_weight=torch.ones(1))
    with pytest.raises(ValueError, match="pos_weight"):
        task_head_reference(*args, "bce", None, 17, pos_weight=torch.ones(2))
    with pytest.raises(ValueError):
        task_head_reference(*args, "bce", None, 17, weight_table=torch.ones(4))             # (no ids)
    with pytest.raises(ValueError):
        task_head_reference(*args, "bce", None, 17, sample_weight=torch.ones(16))           # (too short)
    i9 = WC.inputs("B33xH33xT9_one_absent_none_pos", "bce")
    with pytest.raises(ValueError):
        task_head_reference(i9["emb"], i9["w"], i9["b"], i9["y"], None, "bce", None, 33, pos_weight=i9["pos"])   # (no task, nine outputs)


# ------------------------------------------------------------------------------------------------ the model --
def test_loss_selectors():
    """``_loss_kind`` is what it was (None for a ``pos_weight`` loss); ``_weighted_loss`` names the weighted route."""
    from types import SimpleNamespace
    from torch.nn import BCEWithLogitsLoss, MSELoss
    from molkgnn_amd.train import GNNModel
    x = torch.zeros(3, 28)
    plain = SimpleNamespace(x=x)
    m = GNNModel(loss_func=BCEWithLogitsLoss(pos_weight=torch.tensor([7.])))
    assert m._loss_kind() is None
    kind, pw, sw, table, rows = m._weighted_loss(plain)
    assert kind == "bce" and torch.equal(pw, torch.tensor([7.])) and sw is None and table is None and rows is None
    assert "loss_func.pos_weight" in dict(m.named_buffers())               # (model.to(device) moves it)
    # one element for nine tasks: broadcast once, kept by identity and version
    m9 = GNNModel(task_dim=9, loss_func=BCEWithLogitsLoss(pos_weight=torch.tensor([3.])))
    assert m9._weighted_loss(plain) is None                                # (nine outputs, no task: today's route)
    tasked = SimpleNamespace(x=x, task=torch.zeros(3, dtype=torch.int32))
    a, b = m9._weighted_loss(tasked)[1], m9._weighted_loss(tasked)[1]
    assert a is b and a.tolist() == [3.] * 9
    m9.loss_func.pos_weight.mul_(2)
    assert m9._weighted_loss(tasked)[1].tolist() == [6.] * 9
    nine = torch.arange(1., 10.)
    assert torch.equal(GNNModel(task_dim=9, loss_func=BCEWithLogitsLoss(pos_weight=nine))._weighted_loss(tasked)[1], nine)
    # not recognised: a wrong length, a dtype other than float32, reduction or torch's fixed weight
    for lf in (BCEWithLogitsLoss(pos_weight=torch.ones(4)), BCEWithLogitsLoss(pos_weight=torch.ones(9, dtype=torch.float64)),
               BCEWithLogitsLoss(pos_weight=torch.ones(9), reduction="sum"), BCEWithLogitsLoss(pos_weight=torch.ones(9), weight=torch.ones(9))):
        assert GNNModel(task_dim=9, loss_func=lf)._weighted_loss(tasked) is None
    # sample weights: with every kind _loss_kind knows
    w = torch.ones(3)
    for lf, want in ((BCEWithLogitsLoss(), "bce"), (MSELoss(), "mse"), (MSELoss(reduction="sum"), "mse_sum")):
        mm = GNNModel(loss_func=lf)
        assert mm._weighted_loss(plain) is None and mm._loss_kind() == want
        kind, pw, sw, table, rows = mm._weighted_loss(SimpleNamespace(x=x, weight=w))
        assert kind == want and pw is None and sw is w and table is None
        kind, pw, sw, table, rows = mm._weighted_loss(SimpleNamespace(x=x, weight_table=w, weight_rows=torch.zeros(3, dtype=torch.int32)))
        assert sw is None and table is w and rows is not None
    assert GNNModel(loss_func=torch.nn.L1Loss())._weighted_loss(SimpleNamespace(x=x, weight=w)) is None
    with pytest.raises(ValueError, match="float32"):
        GNNModel()._weighted_loss(SimpleNamespace(x=x, weight=w.double()))


def test_pos_weights():
    from molkgnn_amd.sampling import pos_weights
    #                        task 0: 1 active, 3 inactive | task 1: 2 active, 1 inactive | task 2: inactive only | unlabelled | task 3: none
    tasks = torch.tensor([0, 0, 0, 0, 1, 1, 1, 2, 2, -1, -1])
    labels = torch.tensor([1, 0, 0, 0, 1, 1, 0, 0, 0, 1, 0])
    w = pos_weights(labels, tasks, 4)
    assert w.dtype == torch.float32 and torch.equal(w, torch.tensor([3., .5, 1., 1.]))
    y = (torch.arange(1000) % 13 == 0).long()
    assert torch.equal(pos_weights(y), torch.tensor([(1000 - 77) / 77], dtype=torch.float32))
    with pytest.raises(ValueError):
        pos_weights(labels, tasks[:-1], 4)


def test_resident_shard_keeps_the_weight_of_every_molecule(tmp_path):
    from molkgnn_amd import shards as S
    from molkgnn_amd.synthetic import make_batch
    whole = make_batch(16, seed=12, with_receptive_fields=False)
    path = str(tmp_path / "w.mkgs")
    S.write_shard(path, whole)
    w = np.linspace(0.0, 3.0, 16)
    res = S.ResidentShard(S.Shard(path), device="cpu", weights=w)
    assert res.weight.dtype == torch.float32 and torch.equal(res.weight, torch.from_numpy(w).float()) and "weight" not in res.tensors
    assert torch.equal(S.ResidentShard(S.Shard(path), device="cpu", weights=torch.from_numpy(w)).weight, res.weight)
    assert S.ResidentShard(S.Shard(path), device="cpu").weight is None
    with pytest.raises(ValueError):
        S.ResidentShard(S.Shard(path), device="cpu", weights=w[:-1])
