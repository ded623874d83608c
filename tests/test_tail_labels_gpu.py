"""The multi-output fused tail (csrc/kgnn_tail_labels.hip, ``readout.tail_labels_loss``, ``GNNModel.multi_output_tail``): the
label-matrix head's and the task-indexed head's definitions behind the tail's readout, forward and every gradient in the tail's
four launches plus a small count launch.  ``pytest -m gpu``.

Operator-level inputs as in tests/test_tail.py: random block rows with NaN outside each atom's block, ``make_batch``, K = 110,
H = 32, G = 32 (and 20).  The float64 reference is the dense formula of ``test_fused_tail_against_the_pytorch_formula`` followed by
``label_head_reference`` / ``task_head_reference`` in float64; the fp32 yardstick is the separate route (``readout_blocks`` +
``label_head_loss`` / ``task_head_loss``) from the same generator state; the bound is ``tests/_f64.check``'s."""
import numpy as np
import pytest
import torch

from tests import _f64 as F64
from tests import _label_head_cases as LC
from tests import _label_training_child as LT

pytestmark = pytest.mark.gpu

LS = (10, 20, 30, 50)
NAN = float("nan")
NAMES = ("lin1.weight", "lin1.bias", "lin2.weight", "lin2.bias", "ffn.weight", "ffn.bias")
_CACHE = {}


def _dev():
    assert torch.cuda.is_available(), "pytest -m gpu needs the MI355X"
    return torch.device("cuda:0")


def _setup(mols, T, G=32, seed=41):
    """Batch, plan, segments, modules and block rows: made once per shape and shared, never modified."""
    key = (mols, T, G, seed)
    if key not in _CACHE:
        from molkgnn_amd import readout as R
        from molkgnn_amd.plan import plan_from_data
        from molkgnn_amd.synthetic import make_batch
        from tests.test_tail import _block_rows
        dev = _dev()
        b = make_batch(mols, seed=seed).to(dev)
        plan = plan_from_data(b)
        seg = R.molecule_segments(b.batch, mols)
        assert R.tail_supported(110, 32, G, LS) and R._tail_limits_ok(seg, plan)
        torch.manual_seed(5)
        mods = (torch.nn.Linear(110, 32).to(dev), torch.nn.Linear(32, G).to(dev), torch.nn.Linear(G, T).to(dev))
        sim0, inblock = _block_rows(b, plan, LS, dev, 3)
        _CACHE[key] = (dev, b, plan, seg, mods, sim0, inblock)
    return _CACHE[key]


def _params(mods):
    return [p for m in mods for p in m.parameters()]


def _labels(pattern, n, T, kind, seed=0):
    """float32 [n, T] on the CPU: values for the loss kind, NaN where ``label_mask`` says unlabelled."""
    g = torch.Generator().manual_seed(100 + seed)
    y = (torch.rand(n, T, generator=g) < 0.35).float() if kind == "bce" else torch.randn(n, T, generator=g) * 2 - 1
    return torch.where(LC.label_mask(pattern, n, T), y, torch.full((), NAN))


def _tail(s, src, kind="bce", p_head=0.0, p_ro=0.0, n_rows=None, seed=1234, deferred=False, **w):
    """One forward + backward of ``tail_labels_loss``: loss, pred, block-row grad_sim, the six gradients, generator state."""
    from molkgnn_amd import readout as R
    from molkgnn_amd.train import backward
    dev, b, plan, seg, mods, sim0, inblock = s
    R.reset_head_rng(dev, seed=seed)
    for p in _params(mods):
        p.grad = None
    sim = sim0.detach().requires_grad_(True)
    call = lambda: R.tail_labels_loss(sim, plan, LS, *mods, seg, loss=kind, dropout_p=p_head, n_rows=n_rows,
                                      readout_dropout_p=p_ro, **src, **w)
    if deferred:
        with R.deferred_tail_reduce(dev):
            out = call()
            pred = out.grad_fn.pred
            backward(out)
    else:
        out = call()
        pred = out.grad_fn.pred
        out.backward()
    torch.cuda.synchronize()
    res = {"loss": out.detach().clone(), "pred": pred.clone(), "grad_sim": torch.where(inblock, sim.grad, torch.zeros((), device=dev))}
    res.update({n: p.grad.clone() for n, p in zip(NAMES, _params(mods))})
    res["state"] = R.head_rng_state(dev).clone()
    return res


def _separate(s, src, kind="bce", p_head=0.0, p_ro=0.0, n_rows=None, seed=1234, **w):
    """The route that exists today from the same generator state: ``readout_blocks`` (its mask handed over) + the head operator."""
    from molkgnn_amd import readout as R
    dev, b, plan, seg, mods, sim0, inblock = s
    lin1, lin2, ffn = mods
    R.reset_head_rng(dev, seed=seed)
    for p in _params(mods):
        p.grad = None
    sim = sim0.detach().requires_grad_(True)
    keep = R.readout_dropout_mask(R.head_rng_state(dev).clone(), sim.shape[0], 32, p_ro) if p_ro > 0 else None
    emb = R._ReadoutBlocksFn.apply(sim, lin1.weight, lin1.bias, lin2.weight, lin2.bias, keep, seg, plan, LS)
    n = seg.size if n_rows is None else n_rows
    if "task" in src or "task_table" in src:
        out = R.task_head_loss(emb, ffn, src["target"], src.get("task"), kind, dropout_p=p_head, n_rows=n_rows,
                               task_table=src.get("task_table"), row_ids=src.get("row_ids") if "task_table" in src else w.get("row_ids"),
                               **{k: v for k, v in w.items() if k != "row_ids"})
        pred = None
    else:
        out, pred = R.label_head_loss(emb, ffn, src.get("labels"), kind, dropout_p=p_head, n_rows=n_rows,
                                      label_table=src.get("label_table"), row_ids=src.get("row_ids"), return_pred=True, **w)
        if p_head == 0.0:                                    # (the yardstick the logits are held to: task_scores of that embedding)
            with torch.no_grad():
                pred = R.task_scores(emb.detach(), ffn, n_rows=n)
    out.backward()
    torch.cuda.synchronize()
    res = {"loss": out.detach().clone(), "pred": pred, "grad_sim": torch.where(inblock, sim.grad, torch.zeros((), device=dev))}
    res.update({n_: p.grad.clone() for n_, p in zip(NAMES, _params(mods))})
    return res


def _formula64(s, src, kind="bce", p_head=0.0, p_ro=0.0, n_rows=None, seed=1234, **w):
    """The dense formula in float64 (tests/test_tail.py) with the call's two masks, then the head's definition in float64."""
    from molkgnn_amd import readout as R
    from tests import _philox as PH
    dev, b, plan, seg, mods, sim0, inblock = s
    mols, G = seg.size, mods[1].out_features
    n = mols if n_rows is None else n_rows
    dense = torch.where(inblock, sim0, torch.zeros((), device=dev)).double().requires_grad_(True)
    p64 = [p.detach().double().requires_grad_(True) for p in _params(mods)]
    w1, b1, w2, b2, wh, bh = p64
    src_, dst = b.edge_index[0], b.edge_index[1]
    h = torch.zeros_like(dense).index_add_(0, dst, dense[src_])
    z = h @ w1.t() + b1
    z = z * torch.sigmoid(z)
    if p_ro > 0:
        z = z * torch.from_numpy(PH.readout_mask(seed, 0, sim0.shape[0], 32, p_ro)).to(dev).double()
    z = z @ w2.t() + b2
    emb = torch.zeros(mols, G, dtype=torch.float64, device=dev).index_add_(0, b.batch, z)
    keep = torch.from_numpy(PH.head_mask(seed, 0, n, G, p_head)).to(dev).double() if p_head > 0 else None
    d = lambda t: None if t is None else (t.double() if t.is_floating_point() else t)
    ww = {k: d(v) for k, v in w.items()}
    if "task" in src or "task_table" in src:
        rid = src.get("row_ids") if "task_table" in src else ww.pop("row_ids", None)
        ww.pop("row_ids", None)
        loss, pred = R.task_head_reference(emb, wh, bh, src["target"].double(), src.get("task"), kind, keep, n, src.get("task_table"),
                                           rid, **ww)
        pred = None
    else:
        loss, pred = R.label_head_reference(emb, wh, bh, d(src.get("labels")), kind, keep, n, d(src.get("label_table")),
                                            src.get("row_ids"), **ww)
    grads = torch.autograd.grad(loss, [dense] + p64)
    res = {"loss": loss.detach(), "pred": None if pred is None else pred.detach(),
           "grad_sim": torch.where(inblock, grads[0], torch.zeros((), device=dev, dtype=torch.float64))}
    res.update({n_: g for n_, g in zip(NAMES, grads[1:])})
    return res


# (mols, T, G, kind, pattern, p_head, p_ro, n_pad, extras) -- not the full product: every value of every axis at least once, the
# small shapes carrying most of it.  40: one group per workgroup; 300 with 7 padding molecules: groups wrap round; 1 600: three
# molecules per group; 4 096 at T = 9: groups of six, several chunks per group.
F64_CASES = [
    (40, 9, 32, "bce", "quarter_missing", 0.0, 0.0, 0, ""),
    (40, 1, 32, "mse", "one_per_row", 0.25, 0.0, 0, ""),
    (40, 2, 32, "mse_sum", "task_absent", 0.0, 0.2, 0, ""),
    (40, 32, 32, "bce", "row_absent", 0.25, 0.2, 0, "pos,sw"),
    (40, 9, 20, "bce", "single_entry", 0.0, 0.0, 0, ""),
    (40, 9, 32, "mse", "quarter_missing", 0.0, 0.0, 0, "sw"),
    (40, 9, 32, "bce", "task", 0.25, 0.0, 0, ""),
    (300, 9, 32, "bce", "quarter_missing", 0.25, 0.2, 7, "pos"),
    (300, 32, 20, "mse", "row_absent", 0.0, 0.0, 7, ""),
    (300, 9, 32, "mse_sum", "task", 0.0, 0.2, 7, "sw"),
    (1600, 2, 32, "bce", "task_absent", 0.0, 0.0, 0, ""),
    (1600, 32, 32, "mse", "one_per_row", 0.25, 0.0, 0, ""),
    (4096, 9, 32, "bce", "quarter_missing", 0.0, 0.0, 0, ""),
]


def _source(pattern, n, T, kind, dev, seed=0):
    if pattern == "task":                                     # the task-indexed source, some molecules without a task
        task = (torch.arange(n) * 7 % (T + 2) - 1).clamp(max=T - 1).to(torch.int32)
        g = torch.Generator().manual_seed(7 + seed)
        y = (torch.rand(n, generator=g) < 0.4).float() if kind == "bce" else torch.randn(n, generator=g)
        assert int((task < 0).sum()) > 0
        return dict(task=task.to(dev), target=y.to(dev))
    return dict(labels=_labels(pattern, n, T, kind, seed).to(dev))


@pytest.mark.parametrize("mols,T,G,kind,pattern,p_head,p_ro,n_pad,extras", F64_CASES)
def test_against_float64(mols, T, G, kind, pattern, p_head, p_ro, n_pad, extras):
    s = _setup(mols, T, G)
    dev = s[0]
    n = mols - n_pad
    src = _source(pattern, n, T, kind, dev)
    w = {}
    if "sw" in extras:
        w["sample_weight"] = (torch.rand(n, generator=torch.Generator().manual_seed(3)) + 0.5).to(dev)
    if "pos" in extras:
        w["pos_weight"] = (torch.rand(T, generator=torch.Generator().manual_seed(4)) * 3 + 0.5).to(dev)
    kw = dict(kind=kind, p_head=p_head, p_ro=p_ro, n_rows=n if n_pad else None, **w)
    got, f32, f64 = _tail(s, src, **kw), _separate(s, src, **kw), _formula64(s, src, **kw)
    assert got["pred"].shape == (n, T) and bool(torch.isfinite(got["pred"]).all()) and bool(torch.isfinite(got["loss"]))
    assert got["state"].tolist() == [1234, 1 if (p_head > 0 or p_ro > 0) else 0]
    names = ["loss", "grad_sim", *NAMES] + (["pred"] if f64["pred"] is not None else [])
    print({nm: (float((got[nm].double().cpu() - f64[nm].cpu()).abs().max()), float((f32[nm].double().cpu() - f64[nm].cpu()).abs().max()))
           for nm in names})
    assert F64.check(got, f32, f64, f"tail_labels:{mols}:{T}:{G}:{kind}:{pattern}:{p_head}:{p_ro}:{extras}", names) == len(names)


def _same(a, b, what=("loss", "pred", "grad_sim", *NAMES)):
    for k in what:
        assert torch.equal(a[k], b[k]), (k, float((a[k] - b[k]).abs().max()))


@pytest.mark.parametrize("mols", [40, 300, 1600])
@pytest.mark.parametrize("kind", ["bce", "mse", "mse_sum"])
@pytest.mark.parametrize("p_head,p_ro", [(0.0, 0.0), (0.25, 0.2)])
def test_one_dense_task_is_the_single_task_tail(mols, kind, p_head, p_ro):
    """T = 1 with a dense label column: loss, pred, grad_sim, all six gradients and the generator state of ``tail_loss``."""
    from molkgnn_amd import readout as R
    s = _setup(mols, 1)
    dev, b, plan, seg, mods, sim0, inblock = s
    y = _labels("dense", mols, 1, kind).to(dev)
    got = _tail(s, dict(labels=y), kind=kind, p_head=p_head, p_ro=p_ro)
    R.reset_head_rng(dev, seed=1234)
    for p in _params(mods):
        p.grad = None
    sim = sim0.detach().requires_grad_(True)
    out = R.tail_loss(sim, plan, LS, *mods, y.reshape(-1), seg, p_head, None, loss=kind, readout_dropout_p=p_ro)
    pred = out.grad_fn.pred
    out.backward()
    torch.cuda.synchronize()
    want = {"loss": out.detach(), "pred": pred.reshape(-1, 1), "grad_sim": torch.where(inblock, sim.grad, torch.zeros((), device=dev))}
    want.update({n: p.grad.reshape(got[n].shape) for n, p in zip(NAMES, _params(mods))})
    _same(got, want)
    assert torch.equal(got["state"], R.head_rng_state(dev))


@pytest.mark.parametrize("kind", ["bce", "mse", "mse_sum"])
def test_weights_of_exactly_one_give_the_unweighted_bits(kind):
    s = _setup(300, 9)
    dev = s[0]
    src = dict(labels=_labels("quarter_missing", 300, 9, kind).to(dev))
    base = _tail(s, src, kind=kind, p_head=0.25, p_ro=0.2)
    forms = [dict(sample_weight=torch.ones(300, device=dev)),
             dict(weight_table=torch.ones(5, device=dev), row_ids=(torch.arange(300, device=dev) % 5).to(torch.int32))]
    if kind == "bce":
        forms += [dict(pos_weight=torch.ones(9, device=dev)), dict(pos_weight=torch.ones(9, device=dev), sample_weight=torch.ones(300, device=dev))]
    for w in forms:
        _same(_tail(s, src, kind=kind, p_head=0.25, p_ro=0.2, **w), base)


@pytest.mark.parametrize("source", ["labels", "task"])
def test_the_table_route_equals_the_direct_route(source):
    """``label_table`` / ``task_table`` + ``row_ids`` (ids in shuffled order, one id outside the table) against the same rows given
    directly (the row of the outside id: no label)."""
    s = _setup(300, 9)
    dev = s[0]
    n, M = 300, 500
    ids = torch.randperm(M, generator=torch.Generator().manual_seed(5))[:n].to(torch.int32)
    ids[17] = M + 3                                           # outside the table
    safe = ids.long().clamp(max=M - 1)
    if source == "labels":
        table = _labels("quarter_missing", M, 9, "bce")
        direct = table[safe].clone()
        direct[17] = NAN
        a = _tail(s, dict(label_table=table.to(dev), row_ids=ids.to(dev)), p_head=0.25)
        c = _tail(s, dict(labels=direct.to(dev)), p_head=0.25)
    else:
        table = (torch.arange(M) * 7 % 11 - 1).clamp(max=8).to(torch.int32)
        direct = table[safe].clone()
        direct[17] = -1
        y = (torch.rand(n, generator=torch.Generator().manual_seed(6)) < 0.4).float().to(dev)
        a = _tail(s, dict(task_table=table.to(dev), row_ids=ids.to(dev), target=y), p_head=0.25)
        c = _tail(s, dict(task=direct.to(dev), target=y), p_head=0.25)
    _same(a, c)
    assert float(a["loss"]) > 0 and float(a["grad_sim"].abs().max()) > 0


def test_missing_entries_give_exact_zeros():
    s = _setup(40, 9)
    dev, b = s[0], s[1]
    # all_missing: loss exactly 0.0, every gradient exactly zero, nothing NaN
    got = _tail(s, dict(labels=_labels("all_missing", 40, 9, "bce").to(dev)), p_head=0.25, p_ro=0.2)
    assert float(got["loss"]) == 0.0 and bool(torch.isfinite(got["pred"]).all())
    for k in ("grad_sim", *NAMES):
        assert float(got[k].abs().max()) == 0.0 and not bool(torch.isnan(got[k]).any()), k
    # a row with no labelled entry: its atoms' grad_sim rows exactly zero; a task with none: zero rows of the head's gradient
    for pattern, kind in (("row_absent", "bce"), ("task_absent", "mse")):
        y = _labels(pattern, 40, 9, kind)
        got = _tail(s, dict(labels=y.to(dev)), kind=kind)
        lab = ~torch.isnan(y)
        empty_rows, empty_tasks = ~lab.any(dim=1), ~lab.any(dim=0)
        atoms = empty_rows.to(dev)[b.batch]
        assert float(got["grad_sim"][atoms].abs().max() if bool(atoms.any()) else 0.0) == 0.0
        assert float(got["grad_sim"][~atoms].abs().max()) > 0.0
        if bool(empty_tasks.any()):
            assert float(got["ffn.weight"][empty_tasks.to(dev)].abs().max()) == 0.0
            assert float(got["ffn.bias"][empty_tasks.to(dev)].abs().max()) == 0.0
        assert float(got["ffn.weight"][~empty_tasks.to(dev)].abs().max()) > 0.0
        assert (pattern == "row_absent") == bool(empty_rows.any()) and (pattern == "task_absent") == bool(empty_tasks.any())


def test_n_rows_equals_trailing_rows_of_nan():
    """``n_rows = 33`` of 40 against all 40 rows with the trailing seven set to NaN.  pred and grad_sim are per-molecule results
    and equal for any pair of sizes; the loss and the parameter gradients are sums over workgroup slabs in block order, cut
    into eight runs of ceil(blocks / 8) slabs -- 33 and 40 blocks are cut alike, so these are the same sums too."""
    s = _setup(40, 9)
    dev = s[0]
    y = _labels("quarter_missing", 40, 9, "bce")
    trimmed = y.clone()
    trimmed[33:] = NAN
    a = _tail(s, dict(labels=y.to(dev)), p_head=0.25, n_rows=33)
    c = _tail(s, dict(labels=trimmed.to(dev)), p_head=0.25)
    assert a["pred"].shape == (33, 9)
    c["pred"] = c["pred"][:33]
    _same(a, c)


def test_the_padded_batch_equals_the_unpadded_one(monkeypatch):
    """``padding.pad_batch`` with 64 padding molecules through ``GNNModel.loss`` with the attribute on: the loss bit for bit."""
    from molkgnn_amd import _lib, padding as P
    from molkgnn_amd.receptive_field import attach_receptive_fields
    from molkgnn_amd.synthetic import make_batch
    from molkgnn_amd.train import GNNModel
    dev = _dev()
    torch.manual_seed(3)
    model = GNNModel(num_layers=2, task_dim=9, dropout_ratio=0.0, ffn_dropout_rate=0.0).to(dev).train()
    model.multi_output_tail = True
    B = 300
    raw = make_batch(B, seed=4100, with_receptive_fields=False)
    other = make_batch(B, seed=4101, with_receptive_fields=False)
    shape = P.fixed_shape([P.degree_histogram(raw), P.degree_histogram(other)])
    labels = _labels("quarter_missing", B, 9, "bce")
    calls = []
    real = _lib.check
    monkeypatch.setattr(_lib, "check", lambda rc, what: (calls.append(what), real(rc, what))[1])
    res = []
    padded = P.pad_batch(raw, shape, B)
    for batch, lab in ((attach_receptive_fields(raw.to(dev)), labels),
                       (attach_receptive_fields(padded.to(dev), sizes=[shape[f"n{d}"] for d in range(1, 5)]), labels)):
        batch.labels = lab.to(dev)
        model.zero_grad(set_to_none=True)
        loss = model.loss(batch)
        loss.backward()
        torch.cuda.synchronize()
        res.append((loss.detach().clone(), {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}))
    assert calls.count("mkgnn_tail_fused_labels") == 2 and not [c for c in calls if "label_head" in c], calls
    assert torch.equal(res[0][0], res[1][0]), (float(res[0][0]), float(res[1][0]))
    for n in ("ffn.weight", "ffn.bias", "gnn_model.graph_embedding_lin2.weight", "gnn_model.graph_embedding_lin2.bias",
              "gnn_model.graph_embedding_lin1.bias"):
        assert torch.equal(res[0][1][n], res[1][1][n]), n


def test_oversize_molecule_is_refused_by_the_host_and_loud_in_the_kernel():
    from molkgnn_amd import readout as R
    from molkgnn_amd.plan import plan_from_data
    from molkgnn_amd.synthetic import make_batch
    from tests.test_tail import _block_rows
    dev = _dev()
    b = make_batch(40, seed=51).to(dev)
    plan = plan_from_data(b)
    batch = b.batch.clone()
    assert int((batch < 9).sum()) > 128
    merged = torch.where(batch < 9, torch.zeros_like(batch), batch - 8)
    seg = R.MoleculeSegments(merged, int(merged.max()) + 1)
    assert not R._tail_limits_ok(seg, plan)                   # the host's check says no: the model falls back (below, at model level)
    mods = _setup(40, 9)[4]
    sim0, _ = _block_rows(b, plan, LS, dev, 2)
    y = _labels("quarter_missing", seg.size, 9, "bce").to(dev)
    loss = R.tail_labels_loss(sim0.detach().requires_grad_(True), plan, LS, *mods, seg, labels=y)
    assert torch.isnan(loss) and loss.grad_fn.pred.shape == (seg.size, 9)
    seg_ok = R.molecule_segments(b.batch, 40)
    loss = R.tail_labels_loss(sim0.detach().requires_grad_(True), plan, LS, *mods, seg_ok, labels=_labels("dense", 40, 9, "bce").to(dev))
    assert torch.isfinite(loss)


# ------------------------------------------------------------------------------------------------ the model --
def _spy(monkeypatch):
    from molkgnn_amd import _lib
    calls = []
    real = _lib.check
    monkeypatch.setattr(_lib, "check", lambda rc, what: (calls.append(what), real(rc, what))[1])
    return calls


def _model_batches(dev):
    from molkgnn_amd.sampling import task_index
    from molkgnn_amd.synthetic import NINE_ASSAYS, make_batch
    model, lab = LT.model_and_batch(dev)
    tb = make_batch(40, seed=7, assay="all9")
    tb.task = task_index(tb.assay_id, [int(a) for a in NINE_ASSAYS])
    return model, {"labels": lab.to(dev), "task": tb.to(dev)}


@pytest.mark.parametrize("which", ["labels", "task"])
def test_model_loss_takes_the_multi_output_tail_on_request(which, monkeypatch):
    from molkgnn_amd import readout as R
    from molkgnn_amd.train import backward
    dev = _dev()
    model, batches = _model_batches(dev)
    bd = batches[which]
    calls = _spy(monkeypatch)

    def step(on):
        model.multi_output_tail = on
        del calls[:]
        R.reset_head_rng(dev, seed=99)
        model.zero_grad(set_to_none=True)
        loss = model.loss(bd)
        backward(loss)
        torch.cuda.synchronize()
        return float(loss.detach()), {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}, list(calls)

    l1, g1, c1 = step(True)
    assert "mkgnn_tail_fused_labels" in c1 and not [c for c in c1 if "label_head" in c or "task_head" in c or "readout_blocks" in c], c1
    l0, g0, c0 = step(None)                                   # unset: today's calls
    today = "mkgnn_label_head_fused" if which == "labels" else "mkgnn_task_head_fused"
    assert today in c0 and "mkgnn_tail_fused_labels" not in c0, c0
    assert abs(l0 - l1) <= 2e-6 * max(1.0, abs(l0)), (l0, l1)
    assert set(g0) == set(g1) and len(g0) > 20
    for n in g0:
        assert float((g0[n] - g1[n]).abs().max()) <= 5e-5 * max(float(g0[n].abs().max()), 1e-6), n


def test_model_falls_back_where_the_tail_does_not_apply(monkeypatch):
    """More than 32 outputs and head dropout p >= 1: exactly today's calls with the attribute on."""
    from molkgnn_amd.train import GNNModel
    dev = _dev()
    _, batches = _model_batches(dev)
    calls = _spy(monkeypatch)
    for kw in (dict(task_dim=9, ffn_dropout_rate=1.0), dict(task_dim=33, ffn_dropout_rate=0.0)):
        torch.manual_seed(0)
        model = GNNModel(num_layers=2, dropout_ratio=0.0, **kw).to(dev).train()
        bd = batches["labels"]
        bd.labels = _labels("quarter_missing", 40, kw["task_dim"], "bce").to(dev)
        seen = []
        for on in (True, None):
            model.multi_output_tail = on
            del calls[:]
            model.loss(bd)
            torch.cuda.synchronize()
            seen.append([c for c in calls if "head" in c or "tail" in c or "molecule" in c or "readout" in c])
        assert seen[0] == seen[1] and "mkgnn_tail_fused_labels" not in seen[0], seen


@pytest.mark.parametrize("which", ["labels", "task"])
def test_training_step_defers_and_gives_the_same_parameters(which):
    """``train.training_step`` (deferred reduction and projection) against the undeferred calls: the same parameters after one
    ``FusedAdamW`` step, bit for bit."""
    from molkgnn_amd import readout as R
    from molkgnn_amd.train import backward, configure_optimizer, training_step
    dev = _dev()
    out = []
    for unit in (False, True):
        model, batches = _model_batches(dev)
        model.multi_output_tail = True
        opt = configure_optimizer(model, lr=1e-3, capturable=True)
        R.reset_head_rng(dev, seed=99)
        if unit:
            loss = training_step(model, batches[which], opt)
        else:
            model.zero_grad(set_to_none=True)
            loss = model.loss(batches[which])
            backward(loss)
            opt.step()
        torch.cuda.synchronize()
        out.append((loss.detach().clone(), {n: p.detach().clone() for n, p in model.named_parameters()}))
    assert torch.equal(out[0][0], out[1][0])
    for n in out[0][1]:
        assert torch.equal(out[0][1][n], out[1][1][n]), n


def test_one_captured_graph_serves_batches_with_different_divisors(tmp_path):
    """``train.CapturedSteps`` over a ``ResidentShard(labels=...)`` with the attribute on: one graph, id rows whose hole patterns (and
    so whose divisors) differ, each replay's loss the eager call's bits; ``predict_tasks`` right after sees flushed results."""
    from molkgnn_amd import padding as P, shards as S
    from molkgnn_amd.receptive_field import attach_receptive_fields
    from molkgnn_amd.synthetic import make_batch
    from molkgnn_amd.train import CapturedSteps, GNNModel, configure_optimizer, training_step
    dev = _dev()
    whole = make_batch(48, seed=12, assay="all9", with_receptive_fields=False)
    path = str(tmp_path / "all9.mkgs")
    S.write_shard(path, whole)
    labels = LT.label_matrix(48, 21)
    labels[:16] = torch.where(torch.arange(16)[:, None] % 2 == 0, labels[:16], torch.full((), NAN))     # (fewer labels in these rows)
    res = S.ResidentShard(S.Shard(path), dev, labels=labels)
    rows = np.concatenate([np.arange(0, 16), np.arange(16, 32), np.arange(32, 48)])
    loader = S.ResidentLoader(res, 16, rows, dev)
    batches = list(loader)
    counts = [int((~torch.isnan(labels[r * 16:(r + 1) * 16])).sum()) for r in range(3)]
    assert len(set(counts)) == 3, counts
    csb = P.CompactStaticBatch(loader.shape, 16, res.x_dim, res.p_dim, res.e_dim, dev, max_mol_atoms=loader.max_mol_atoms,
                               max_mol_edges=loader.max_mol_edges)

    def fresh():
        torch.manual_seed(1)
        model = GNNModel(num_layers=2, task_dim=LT.T, dropout_ratio=0.0, ffn_dropout_rate=0.0).to(dev).train()
        model.multi_output_tail = True
        return model, configure_optimizer(model, lr=1e-3, capturable=True)

    def feed(k):
        """The molecules of id row 0, gathered once (a captured step is recognised by its batch and its x); the LABELS of id row k:
        the ids the label table is read through are refilled in place, as a captured loop refills them."""
        if not fed:
            csb.gather(res, batches[0])
            csb.expand()
            attach_receptive_fields(csb.data, sizes=csb.data.bucket_sizes, overlap=True)
            assert csb.data.label_table is res.tensors["labels"] and csb.data.label_rows is csb.ids
            fed.append(1)
        csb.ids.copy_(batches[k])
        return csb.data

    fed = []

    from molkgnn_amd import _lib
    seen = []
    real = _lib.check
    _lib.check = lambda rc, what: (seen.append(what), real(rc, what))[1]
    try:
        model, opt = fresh()
        want = []
        for k in (0, 1, 2, 1):
            want.append(training_step(model, feed(k), opt).detach().clone())
        torch.cuda.synchronize()
        assert "mkgnn_tail_fused_labels" in seen and not [c for c in seen if "label_head" in c], seen
    finally:
        _lib.check = real
    model, opt = fresh()
    steps = CapturedSteps(model, opt, warmup=1, max_graphs=1)
    got = []
    for k in (0, 1, 2, 1):
        got.append(steps(feed(k)).detach().clone())
    torch.cuda.synchronize()
    assert len(steps._graphs) == 1                            # one graph: the first visit eager, three replays
    for k in range(4):
        assert torch.equal(got[k], want[k]), (k, float(got[k]), float(want[k]))
    assert len({float(x) for x in got[:3]}) == 3
    model.eval()
    with torch.no_grad():
        scores = model.predict_tasks(feed(2))[0]
    assert bool(torch.isfinite(scores).all()) and bool(all(torch.isfinite(p).all() for p in model.parameters()))
    # ... right after a deferred step: the step's results are flushed before the forward-only pass reads the parameters
    model2, opt2 = fresh()
    training_step(model2, feed(2), opt2)
    model2.eval()
    with torch.no_grad():
        after = model2.predict_tasks(feed(2))[0].clone()
    torch.cuda.synchronize()
    with torch.no_grad():
        again = model2.predict_tasks(feed(2))[0]
    assert torch.equal(after, again) and bool(torch.isfinite(after).all())
