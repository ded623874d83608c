"""The label-matrix head, everything that needs no GPU: the C ABI's declarations and exports, the torch definition
``readout.label_head_reference`` against PyTorch's own losses over the labelled entries, against the task-indexed head's
definition and against its contract's zero rules; the operator's and ``GNNModel.loss``'s refusals; the resident shard's label
table and its hand-over by ``gather``; ``sampling.label_pos_weights``; ``train.evaluate_labels``."""
import os
import re
import types

import pytest
import torch

from tests import _label_head_cases as LC

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("mkgnn_label_head_workspace_bytes", "mkgnn_label_head_forward", "mkgnn_label_head_backward", "mkgnn_label_head_fused")
F = torch.nn.functional


def test_header_declares_the_entry_points_and_abi_stays_8():
    text = open(os.path.join(REPO, "include", "molkgnn_hip.h")).read()
    for name in ENTRIES:
        assert re.search(r"\b(size_t|int) " + name + r"\(", text), name
    assert re.search(r"#define MKGNN_ABI_VERSION 8\b", text)


def test_library_exports_the_entry_points_and_lib_types_them():
    import ctypes
    from molkgnn_amd import _lib
    assert _lib.ABI_VERSION == 8
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRIES:
        assert name in _lib.EXPORTS, name
        assert hasattr(raw, name), name
    lib = _lib.load()
    assert lib.mkgnn_abi_version() == 8
    for name in ENTRIES[1:]:
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and ctypes.POINTER(_lib.LossWeights) in fn.argtypes, name
    assert lib.mkgnn_label_head_workspace_bytes.restype is ctypes.c_size_t
    # the workspace is the task head's: 16 bytes + per 16-row block a [T][H + 1] partial and {loss, labelled entries}
    assert lib.mkgnn_label_head_workspace_bytes(17, 5, 3) == 16 + 2 * (3 * 6 + 2) * 4 == lib.mkgnn_task_head_workspace_bytes(17, 5, 3)
    # 0 outside the limits; n_rows * T < 2^31
    for n, H, T in ((0, 5, 3), (17, 0, 3), (17, 65, 3), (17, 5, 0), (17, 5, 33), (2 ** 31 // 32, 5, 32), (2 ** 31, 5, 1)):
        assert lib.mkgnn_label_head_workspace_bytes(n, H, T) == 0, (n, H, T)
    assert lib.mkgnn_label_head_workspace_bytes(2 ** 31 // 32 - 1, 5, 32) > 0
    assert _lib.load().mkgnn_label_head_workspace_bytes(2 ** 31 - 1, 5, 1) > 0


def _c_calls(lib, p, nbytes, a, weights=None):
    """The three entries on host pointers with the arguments ``a``: nothing may be launched (every call must be refused)."""
    es = max(a["H"], 4) if "es" not in a else a["es"]
    yield lib.mkgnn_label_head_forward(a["kind"], p, es, a["n"], a["H"], a["T"], p, p, p, a["ls"], a["ids"], a["rows"], a["p"],
                                       a["rng"], a["rng"], p, a["ps"], p, weights, a["ws"], nbytes, None)
    yield lib.mkgnn_label_head_fused(a["kind"], p, es, a["n"], a["H"], a["T"], p, p, p, a["ls"], a["ids"], a["rows"], a["p"],
                                     a["rng"], a["rng"], p, a["ps"], p, p, a["ges"], p, p, weights, a["ws"], nbytes, None)
    yield lib.mkgnn_label_head_backward(a["kind"], p, es, a["n"], a["H"], a["T"], p, p, a["ls"], a["ids"], a["rows"], p, a["ps"], p,
                                        a["p"], a["rng"], p, a["ges"], p, p, weights, a["ws"], nbytes, None)


def test_entry_points_refuse_what_is_outside_their_limits():
    """No GPU is touched: every argument check comes before a launch, and the buffers (a canary) stay as they were."""
    import ctypes
    import numpy as np
    from molkgnn_amd import _lib
    lib = _lib.load()
    buf = np.full(1 << 16, 0xA5, dtype=np.uint8)
    p = buf.ctypes.data
    ok = dict(kind=0, n=8, H=4, T=3, ls=3, ps=3, ids=None, rows=8, p=0.0, rng=None, ges=4, ws=p)
    bad = (dict(T=33), dict(T=0), dict(H=65), dict(H=0), dict(n=0), dict(rows=7), dict(ids=p, rows=0), dict(ls=2), dict(ps=2),
           dict(kind=3), dict(p=1.0), dict(p=-0.5), dict(p=0.25), dict(es=3), dict(ws=None), dict(n=2 ** 31 // 3 + 1, rows=2 ** 31))
    for change in bad:
        for which, rc in enumerate(_c_calls(lib, p, buf.nbytes, dict(ok, **change))):
            assert rc != 0 and lib.mkgnn_last_error(), (change, which)
    rc = lib.mkgnn_label_head_fused(0, p, 4, 8, 4, 3, p, p, p, 3, None, 8, 0.0, None, None, p, 3, p, p, 3, p, p, None, p, buf.nbytes, None)
    assert rc != 0 and b"grad_emb" in lib.mkgnn_last_error()
    # the weights: pos_weight with a squared-error kind, a short sample_weight (direct and through ids)
    for kind, lw in ((1, dict(pos_weight=p)), (2, dict(pos_weight=p)), (0, dict(sample_weight=p, n_sample_weight=7)),
                     (0, dict(sample_weight=p, weight_ids=p, n_sample_weight=0))):
        w = _lib.LossWeights()
        for k, v in lw.items():
            setattr(w, k, v)
        for which, rc in enumerate(_c_calls(lib, p, buf.nbytes, dict(ok, kind=kind), ctypes.byref(w))):
            assert rc != 0 and lib.mkgnn_last_error(), (kind, lw, which)
    assert bool((buf == 0xA5).all())


# ------------------------------------------------------------------------------------------- the definition --
def _torch_formulation(i, c, kind, dtype=torch.float64):
    """PyTorch's own loss over the labelled entries, in float64."""
    cast = lambda t: None if t is None else t.to(dtype)
    e = cast(i["emb"])[:c.B]
    if i["keep"] is not None:
        e = e * cast(i["keep"])
    x = F.linear(e, cast(i["w"]), cast(i["b"]))
    m = i["mask"]
    y = cast(i["labels"])[:c.B]
    n = max(int(m.sum()), 1)
    s = None if i["sw"] is None else cast(i["sw"])[:c.B, None].expand(c.B, c.T)[m]
    if not bool(m.any()):
        return torch.zeros((), dtype=dtype)
    if kind == "bce":
        pw = None if i["pw"] is None else cast(i["pw"])[None, :].expand(c.B, c.T)[m]
        return F.binary_cross_entropy_with_logits(x[m], y[m], weight=s, pos_weight=pw, reduction="sum") / n
    sq = (x[m] - y[m]) ** 2
    total = (sq if s is None else s * sq).sum()
    return total if kind == "mse_sum" else total / n


@pytest.mark.parametrize("name,kind", [(c.name, k) for c in LC.CASES_LIST if c.B <= 577 for k in LC.KINDS]
                         + [(LC.SATURATED.name, "bce")])
def test_reference_is_pytorchs_loss_over_the_labelled_entries(name, kind):
    c, i = LC.case(name), LC.inputs(name, kind)
    _, f64 = LC.reference(name, kind, 1.0)
    want = _torch_formulation(i, c, kind)
    assert abs(float(f64["loss"]) - float(want)) <= 1e-12 * max(abs(float(want)), 1e-300), (float(f64["loss"]), float(want))
    assert f64["pred"].shape == (c.B, c.T) and bool(torch.isfinite(f64["pred"]).all())
    # the row_ids table gives what the direct labels give
    if c.row_ids:
        from molkgnn_amd.readout import label_head_reference
        d = lambda t: None if t is None else t.double()
        via, pred = label_head_reference(d(i["emb"]), d(i["w"]), d(i["b"]), None, kind, d(i["keep"]), c.B,
                                         label_table=d(i["label_table"]), row_ids=i["row_ids"], pos_weight=d(i["pw"]),
                                         weight_table=d(i["weight_table"]))
        assert float(via) == float(f64["loss"]) and torch.equal(pred, f64["pred"])


@pytest.mark.parametrize("kind", LC.KINDS)
@pytest.mark.parametrize("name", [c.name for c in LC.CASES_LIST if c.pattern == "one_per_row"])
def test_one_label_per_row_is_the_task_indexed_head(name, kind):
    from molkgnn_amd.readout import task_head_reference
    c, i = LC.case(name), LC.inputs(name, kind)
    _, f64 = LC.reference(name, kind, LC.SCALE)
    task = torch.arange(c.B) % c.T
    y = i["labels"][:c.B].double()[torch.arange(c.B), task]
    emb, w = i["emb"].double().requires_grad_(True), i["w"].double().requires_grad_(True)
    b = None if i["b"] is None else i["b"].double().requires_grad_(True)
    loss, pred = task_head_reference(emb, w, b, y, task, kind, None if i["keep"] is None else i["keep"].double(), c.B)
    (loss * LC.SCALE).backward()
    close = lambda a, r: float((a - r).abs().max()) <= 1e-12 * max(float(r.abs().max()), 1e-300)
    assert close(f64["loss"], loss.detach())
    assert close(f64["pred"][torch.arange(c.B), task], pred.detach())
    assert close(f64["emb"], emb.grad[:c.B]) and close(f64["w"], w.grad.reshape(-1))
    if b is not None:
        assert close(f64["b"], b.grad)


@pytest.mark.parametrize("kind", LC.KINDS)
def test_one_task_without_holes_is_the_single_task_definition(kind):
    name = "B16xH64xT1_dense"
    c, i = LC.case(name), LC.inputs(name, kind)
    _, f64 = LC.reference(name, kind, 1.0)
    x = F.linear(i["emb"].double() * i["keep"].double(), i["w"].double(), i["b"].double()).view(-1)
    y = i["labels"].double().view(-1)
    want = {"bce": F.binary_cross_entropy_with_logits, "mse": F.mse_loss,
            "mse_sum": lambda a, b: F.mse_loss(a, b, reduction="sum")}[kind](x, y)
    assert abs(float(f64["loss"]) - float(want)) <= 1e-12 * abs(float(want))


@pytest.mark.parametrize("kind", LC.KINDS)
@pytest.mark.parametrize("name", ["B17xH5xT2_all_missing", "B33xH33xT9_task_absent", "B577xH64xT9_row_absent", "B33xH31xT12_single_entry"])
def test_reference_keeps_the_zero_rules(name, kind):
    c, i = LC.case(name), LC.inputs(name, kind)
    for leg in LC.reference(name, kind, LC.SCALE):
        m = i["mask"]
        for nm in ("loss", "pred", "emb", "w"):
            assert bool(torch.isfinite(leg[nm]).all()), nm         # (NaN labels, NaN weights of label-less rows: reach nothing)
        absent, bare = ~m.any(dim=0), ~m.any(dim=1)
        if bool(absent.any()):
            assert float(leg["w"].reshape(c.T, c.H)[absent].abs().max()) == 0.0 and float(leg["b"][absent].abs().max()) == 0.0
        if bool(bare.any()):
            assert float(leg["emb"][bare].abs().max()) == 0.0
        if not bool(m.any()):
            assert float(leg["loss"]) == 0.0 and float(leg["w"].abs().max()) == 0.0 and float(leg["emb"].abs().max()) == 0.0


def test_what_stands_in_an_unlabelled_place_reaches_nothing():
    """The sample weight of a row without labels may be anything (NaN, inf, 7): value and gradients do not move by a bit; an
    infinite LABEL is a label (the loss is not finite)."""
    from molkgnn_amd.readout import label_head_reference
    name, kind = "B33xH33xT9_task_absent", "mse"
    c, i = LC.case(name), LC.inputs(name, kind)
    labels = i["labels"].clone()
    labels[4] = LC.NAN
    out = []
    for filler in (LC.NAN, float("inf"), 7.0):
        sw = i["sw"].clone()
        sw[4] = filler
        emb, w = i["emb"].double().requires_grad_(True), i["w"].double().requires_grad_(True)
        loss, _ = label_head_reference(emb, w, i["b"].double(), labels.double(), kind, None, c.B, sample_weight=sw.double())
        loss.backward()
        out.append((loss.detach(), emb.grad, w.grad))
        assert bool(torch.isfinite(loss)) and bool(torch.isfinite(emb.grad).all()) and float(emb.grad[4].abs().max()) == 0.0
    for o in out[1:]:
        assert all(torch.equal(a, b) for a, b in zip(o, out[0]))
    labels[5, 0] = float("inf")
    loss, _ = label_head_reference(i["emb"].double(), i["w"].double(), i["b"].double(), labels.double(), kind, None, c.B)
    assert not bool(torch.isfinite(loss))


def test_reference_refuses_a_weight_with_a_gradient():
    from molkgnn_amd.readout import label_head_reference
    emb, w, labels = torch.randn(4, 3), torch.randn(2, 3), torch.zeros(4, 2)
    for kw in (dict(sample_weight=torch.ones(4, requires_grad=True)), dict(pos_weight=torch.ones(2, requires_grad=True)),
               dict(weight_table=torch.ones(4, requires_grad=True), row_ids=torch.arange(4, dtype=torch.int32))):
        with pytest.raises(ValueError, match="must not require a gradient"):
            label_head_reference(emb, w, None, labels, "bce", **kw)


# ------------------------------------------------------------------------------------------------ refusals --
def test_the_operator_raises_value_errors(monkeypatch):
    from molkgnn_amd import _lib, readout as R
    monkeypatch.setattr(_lib, "require_gpu_tensor", lambda t, name: None)      # (the checks under test come before any launch)
    B, H, T = 6, 5, 3
    emb, ffn, labels = torch.randn(B, H), torch.nn.Linear(H, T), torch.zeros(B, T)
    ids = torch.zeros(B, dtype=torch.int32)
    bad = {
        "neither": dict(labels=None),
        "both": dict(label_table=torch.zeros(4, T), row_ids=ids),
        "table without ids": dict(labels=None, label_table=torch.zeros(4, T)),
        "empty table": dict(labels=None, label_table=torch.zeros(0, T), row_ids=ids),
        "wrong width": dict(labels=torch.zeros(B, T + 1)),
        "flat labels": dict(labels=torch.zeros(B * T)),
        "integer labels": dict(labels=torch.zeros(B, T, dtype=torch.int64)),
        "too few label rows": dict(labels=torch.zeros(B - 1, T)),
        "too few ids": dict(labels=None, label_table=torch.zeros(4, T), row_ids=ids[:-1]),
        "n_rows": dict(n_rows=B + 1),
        "no rows": dict(n_rows=0),
        "dropout": dict(dropout_p=1.0),
        "loss": dict(loss="l1"),
        "pos_weight with mse": dict(loss="mse", pos_weight=torch.ones(T)),
        "pos_weight length": dict(pos_weight=torch.ones(T + 1)),
        "both weights": dict(sample_weight=torch.ones(B), weight_table=torch.ones(4), row_ids=ids),
        "weight table without ids": dict(weight_table=torch.ones(4)),
        "short sample_weight": dict(sample_weight=torch.ones(B - 1)),
        "weight with a gradient": dict(sample_weight=torch.ones(B, requires_grad=True)),
    }
    for what, kw in bad.items():
        with pytest.raises(ValueError):
            R.label_head_loss(emb, ffn, **{"labels": labels, **kw})
            pytest.fail(what)
    with pytest.raises(ValueError):
        R.label_head_loss(emb, torch.nn.Linear(H + 1, T), labels)
    monkeypatch.undo()
    with pytest.raises(_lib.MolKGNNLibraryError):              # a tensor on the wrong device: the library's own error
        R.label_head_loss(emb, ffn, labels)
    assert R.label_head_supported(32, 64) and R.label_head_supported(1, 1)
    assert not R.label_head_supported(33, 8) and not R.label_head_supported(3, 65) and not R.label_head_supported(0, 8)


def test_model_loss_refuses_what_it_cannot_take():
    """Before the network runs (no GPU): tasks together with labels, and a loss that is none of the head's kinds."""
    from molkgnn_amd.synthetic import make_batch
    from molkgnn_amd.train import GNNModel
    b = make_batch(4, seed=1)
    b.labels = torch.zeros(4, 3)
    b.task = torch.zeros(4, dtype=torch.int32)
    with pytest.raises(ValueError, match="both tasks"):
        GNNModel(task_dim=3).train().loss(b)
    del b.task
    b.task_table, b.task_rows = torch.zeros(8, dtype=torch.int32), torch.zeros(4, dtype=torch.int32)
    with pytest.raises(ValueError, match="both tasks"):
        GNNModel(task_dim=3).train().loss(b)
    b.task_table = b.task_rows = None
    with pytest.raises(ValueError, match="label matrix"):
        GNNModel(task_dim=3, loss_func=torch.nn.L1Loss()).train().loss(b)
    with pytest.raises(ValueError, match="label matrix"):
        GNNModel(task_dim=3, loss_func=torch.nn.BCEWithLogitsLoss(reduction="sum")).train().loss(b)
    del b.labels
    b.label_table, b.label_rows = torch.zeros(8, 3), torch.zeros(4, dtype=torch.int32)
    with pytest.raises(ValueError, match="label matrix"):
        GNNModel(task_dim=3, loss_func=torch.nn.L1Loss()).train().loss(b)
    b.label_table = b.label_rows = None                      # (cleared, as gather leaves a shard without labels: the old route)
    from molkgnn_amd._lib import MolKGNNLibraryError
    with pytest.raises(MolKGNNLibraryError):
        GNNModel(task_dim=1).train().loss(b)


# ------------------------------------------------------------------------------------ data and evaluation --
def test_label_pos_weights_on_a_matrix_with_holes():
    from molkgnn_amd.sampling import label_pos_weights, pos_weights
    n = LC.NAN
    labels = torch.tensor([[1., 0., n, n, 0.],
                           [0., 0., n, 1., 0.],
                           [0., n, n, 1., 0.],
                           [n, 1., n, 0., 0.],
                           [0., 0., n, 1., n]])
    got = label_pos_weights(labels)
    assert got.dtype == torch.float32 and got.tolist() == [3.0, 3.0, 1.0, torch.tensor(1 / 3).item(), 1.0]
    for t in range(5):                                       # (column by column: pos_weights of the column's labelled entries)
        known = ~torch.isnan(labels[:, t])
        if bool(known.any()):
            assert got[t] == pos_weights(labels[known, t])[0]
    assert torch.equal(label_pos_weights(labels.numpy()), got)
    with pytest.raises(ValueError):
        label_pos_weights(torch.zeros(5))


def _label_matrix(n, T, seed, present=0.3):
    g = torch.Generator().manual_seed(seed)
    y = (torch.rand(n, T, generator=g) < 0.35).float()
    return torch.where(torch.rand(n, T, generator=g) < present, y, torch.full((), LC.NAN))


def test_resident_shard_keeps_the_label_matrix(tmp_path):
    from molkgnn_amd import shards as S
    from molkgnn_amd.synthetic import NINE_ASSAYS, make_batch
    whole = make_batch(24, seed=12, assay="all9", with_receptive_fields=False)
    path = str(tmp_path / "all9.mkgs")
    S.write_shard(path, whole)
    shard = S.Shard(path)
    L = _label_matrix(24, 9, 3)
    res = S.ResidentShard(shard, device="cpu", labels=L.double().numpy())
    assert res.labels.dtype == torch.float32 and res.labels.shape == (24, 9)
    assert torch.equal(torch.isnan(res.labels), torch.isnan(L)) and torch.equal(res.labels.nan_to_num(-1.0), L.nan_to_num(-1.0))
    assert "labels" not in res.tensors                       # (nothing is uploaded on the CPU)
    assert S.ResidentShard(shard, device="cpu").labels is None
    with pytest.raises(ValueError, match="exclude"):
        S.ResidentShard(shard, device="cpu", labels=L, assays=[int(a) for a in NINE_ASSAYS])
    for bad in (L[:-1], L.reshape(-1), torch.zeros(24, 0)):
        with pytest.raises(ValueError):
            S.ResidentShard(shard, device="cpu", labels=bad)


def test_gather_hands_over_and_clears_the_label_table(monkeypatch):
    """``CompactStaticBatch.gather``'s hand-over on stand-ins (the gather kernel itself is not run): a shard with labels gives
    the batch ``label_table`` / ``label_rows`` (its own static id buffer); a shard without them clears both."""
    from molkgnn_amd import _lib, padding as P
    dev = torch.device("cpu")
    lib = types.SimpleNamespace(mkgnn_gather_compact=lambda *a: 0, mkgnn_gather_compact_workspace_bytes=lambda n: 16)
    monkeypatch.setattr(_lib, "load", lambda: lib)
    monkeypatch.setattr(_lib, "stream_ptr", lambda d: None)
    monkeypatch.setattr(torch.cuda, "device", lambda d: __import__("contextlib").nullcontext())
    csb = P.CompactStaticBatch.__new__(P.CompactStaticBatch)
    csb.wire, csb.num_molecules, csb.ids, csb._gather_ws = torch.zeros(8, dtype=torch.uint8), 4, None, None
    csb.x_dim, csb.p_dim, csb.e_dim = 3, 3, 2
    csb.shape = dict(atoms=8, edges=8, n1=2, n2=2, n3=2, n4=2)
    csb.data = types.SimpleNamespace()
    table = torch.zeros(10, 9)
    with_labels = types.SimpleNamespace(view=object(), device=dev, x_dim=3, p_dim=3, e_dim=2, packed=False, tensors={"labels": table})
    without = types.SimpleNamespace(view=object(), device=dev, x_dim=3, p_dim=3, e_dim=2, packed=False, tensors={})
    csb.gather(with_labels)
    assert csb.data.label_table is table and csb.data.label_rows is csb.ids and csb.ids.dtype == torch.int32
    assert getattr(csb.data, "task_table", None) is None and getattr(csb.data, "weight_table", None) is None
    csb.gather(without)
    assert csb.data.label_table is None and csb.data.label_rows is None
    from molkgnn_amd.train import _has_labels
    assert not _has_labels(csb.data)


def test_evaluate_labels_is_per_task_on_the_flattened_triples():
    from molkgnn_amd import evaluation as E
    from molkgnn_amd.readout import label_head_reference
    from molkgnn_amd.train import GNNModel, evaluate_labels
    T, n = 4, 60
    g = torch.Generator().manual_seed(9)
    preds = [torch.randn(n, T, generator=g) for _ in range(2)]
    labels = [_label_matrix(n, T, 20 + k, present=0.6) for k in range(2)]
    labels[0][:, 2] = LC.NAN
    labels[1][:, 2] = LC.NAN                                  # (task 2 has no labelled entry)

    class Stub(GNNModel):
        def predict_tasks(self, data):
            self._needs_eval("predict_tasks")
            return data.pred, None

    model = Stub(num_layers=1, task_dim=T).train()
    batches = [types.SimpleNamespace(pred=p, labels=l) for p, l in zip(preds, labels)]
    res = evaluate_labels(model, batches, metrics=("AUC", "logAUC_0.001_0.1"))
    assert model.training
    P, L = torch.cat(preds), torch.cat(labels)
    lab = ~torch.isnan(L)
    row, task = lab.nonzero(as_tuple=True)
    assert torch.equal(res["task"], task) and torch.equal(res["true_y"], L[row, task]) and torch.equal(res["pred_y"], P[row, task])
    assert res["n_labelled"] == lab.sum(dim=0).tolist() and res["n_labelled"][2] == 0
    for m, fn in (("AUC", E.calculate_auc), ("logAUC_0.001_0.1", E.calculate_logAUC)):
        want = E.per_task(L[row, task], P[row, task], task, fn, T)
        for t in range(T):
            assert res[m][t] == want[t] or (want[t] != want[t] and res[m][t] != res[m][t]), (m, t)
            if t != 2:
                assert res[m][t] == fn(L[:, t][lab[:, t]], P[:, t][lab[:, t]])
        assert res[m][2] != res[m][2]
    # the loss: the definition on the predictions themselves (an identity head)
    want, _ = label_head_reference(P, torch.eye(T), None, L, "bce")
    assert abs(float(res["loss"]) - float(want)) <= 1e-6 * abs(float(want))
    with pytest.raises(ValueError, match="labels"):
        evaluate_labels(model, [types.SimpleNamespace(pred=preds[0])])
    with pytest.raises(ValueError):
        evaluate_labels(model, [])
