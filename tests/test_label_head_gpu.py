"""The label-matrix head on the GPU (``readout.label_head_loss`` -> ``_LabelHeadFn``; ``mkgnn_label_head_*``,
csrc/kgnn_label_head.hip): against float64 at the edges of its kernels (cases and references: ``tests/_label_head_cases.py``).
``pytest -m gpu``.

Bound: ``tests/_f64.check``, constants as they stand; the float32 leg is ``readout.label_head_reference`` in float32, the exact
leg the same function in float64.  Per case: ``pred``, ``loss``, each gradient of ``loss`` and of ``1.7 * loss``; the exact-zero
rules by ``== 0.0``; ``pred`` bit for bit against ``task_scores`` / the task-indexed head; fused against the forward + backward
pair, run against run and the table route against the direct one by ``torch.equal``.
"""
import ctypes

import pytest
import torch

from tests import _f64 as F64
from tests import _label_head_cases as LC

pytestmark = pytest.mark.gpu
CANARY = -12345.5


def _dev():
    assert torch.cuda.is_available(), "pytest -m gpu needs the MI355X"
    return torch.device("cuda:0")


def _ffn(i, c, dev):
    ffn = torch.nn.Linear(c.H, c.T, bias=c.bias)
    with torch.no_grad():
        ffn.weight.copy_(i["w"])
        if c.bias:
            ffn.bias.copy_(i["b"])
    return ffn.to(dev)


def _to(t, dev):
    return None if t is None else t.to(dev)


def _runner(c, kind, monkeypatch):
    """``run(split, scale, emb_grad=True, direct=False, ones=False, weights=True)`` -> loss, pred, the gradients and the generator
    state of one forward + backward of the case on the GPU; ``scale`` None: seeded by train.backward's registered 1."""
    from molkgnn_amd import readout as R
    from molkgnn_amd.train import backward
    dev = _dev()
    i = LC.inputs(c.name, kind)
    ffn = _ffn(i, c, dev)
    n = c.B + c.n_pad
    store = torch.zeros(n, c.H + c.stride_pad, device=dev)
    store[:, :c.H] = i["emb"].to(dev)
    labels, sw, pw = i["labels"].to(dev), _to(i["sw"], dev), _to(i["pw"], dev)
    table, wtable, ids = _to(i["label_table"], dev), _to(i["weight_table"], dev), _to(i["row_ids"], dev)

    def run(split, scale, emb_grad=True, direct=False, ones=False, weights=True):
        monkeypatch.setattr(R, "_SPLIT_HEAD", split)
        R.reset_head_rng(dev, seed=LC.SEED)
        leaf = store.clone().requires_grad_(emb_grad)
        emb = leaf[:, :c.H]                                   # (row stride H + stride_pad)
        assert emb.stride(0) == c.H + c.stride_pad
        ffn.zero_grad(set_to_none=True)
        kw = dict(pos_weight=pw) if weights else {}
        if ones:
            kw["sample_weight"] = torch.ones(n, device=dev)
        if table is not None and not direct:
            loss, pred = R.label_head_loss(emb, ffn, None, kind, dropout_p=c.p, n_rows=c.B, label_table=table, row_ids=ids,
                                           weight_table=wtable if (weights and not ones) else None, return_pred=True, **kw)
        else:
            if weights and not ones:
                kw["sample_weight"] = sw
            loss, pred = R.label_head_loss(emb, ffn, labels, kind, dropout_p=c.p, n_rows=c.B, return_pred=True, **kw)
        assert not pred.requires_grad and pred.shape == (c.B, c.T)
        if scale is None:
            backward(loss)
        else:
            (loss * scale).backward()
        torch.cuda.synchronize()
        rng = R.head_rng_state(dev).clone() if c.p > 0.0 else None
        return dict(loss=loss.detach().clone(), pred=pred.clone(), emb=None if leaf.grad is None else leaf.grad[:, :c.H].clone(),
                    w=ffn.weight.grad.clone().reshape(-1), b=None if not c.bias else ffn.bias.grad.clone(), rng=rng)

    return run, i


def _check_zero_rules(r, c, i, tag):
    m = i["mask"].to(r["pred"].device)
    for nm in ("loss", "pred", "emb", "w", "b"):
        if r[nm] is not None:
            assert bool(torch.isfinite(r[nm]).all()), (tag, nm)
    bare, absent = ~m.any(dim=1), ~m.any(dim=0)
    if r["emb"] is not None:
        assert r["emb"].shape == (c.B + c.n_pad, c.H)
        if c.n_pad:
            assert float(r["emb"][c.B:].abs().max()) == 0.0, (tag, "padding rows")
        if bool(bare.any()):
            assert float(r["emb"][:c.B][bare].abs().max()) == 0.0, (tag, "rows without a label")
    if bool(absent.any()):
        assert float(r["w"].reshape(c.T, c.H)[absent].abs().max()) == 0.0, (tag, "absent tasks: grad W")
        if c.bias:
            assert float(r["b"][absent].abs().max()) == 0.0, (tag, "absent tasks: grad b")
    if not bool(m.any()):
        assert float(r["loss"]) == 0.0 and float(r["w"].abs().max()) == 0.0, (tag, "no labelled entry")
        assert r["emb"] is None or float(r["emb"].abs().max()) == 0.0, (tag, "no labelled entry")
        assert r["b"] is None or float(r["b"].abs().max()) == 0.0, (tag, "no labelled entry")
    if c.p > 0.0:
        assert r["rng"].tolist() == [LC.SEED, 1], (tag, "one draw per forward")


def _task_head_pred(c, i, kind, dev):
    """``pred [B, T]`` by T calls of the task-indexed head's forward entry, every row labelled with task t, each from the
    generator state ``{SEED, 0}``."""
    from molkgnn_amd import _lib, readout as R
    lib, p = _lib.load(), _lib.ptr
    emb, w, b = i["emb"][:c.B].to(dev).contiguous(), i["w"].to(dev).contiguous(), _to(i["b"], dev)
    y, loss = torch.zeros(c.B, device=dev), torch.zeros(1, device=dev)
    ws = torch.zeros(int(lib.mkgnn_task_head_workspace_bytes(c.B, c.H, c.T)), dtype=torch.uint8, device=dev)
    used = torch.zeros(2, dtype=torch.int64, device=dev)
    out = torch.empty(c.T, c.B, device=dev)
    for t in range(c.T):
        rng = torch.tensor([LC.SEED, 0], dtype=torch.int64, device=dev)
        task = torch.full((c.B,), t, dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            _lib.check(lib.mkgnn_task_head_forward(R.loss_kind(kind), p(emb), c.H, c.B, c.H, c.T, p(w), p(b), p(y), p(task), None, c.B,
                                                   float(c.p), p(rng), p(used), p(out[t]), p(loss), p(ws), ws.numel(),
                                                   _lib.stream_ptr(dev)), "mkgnn_task_head_forward")
        torch.cuda.synchronize()
    return out.t().contiguous()


def _run_case(c, kind, monkeypatch):
    from molkgnn_amd import readout as R
    run, i = _runner(c, kind, monkeypatch)
    runs = {"fused": run(False, None), "split": run(True, None), "split*scale": run(True, LC.SCALE), "fused*scale": run(False, LC.SCALE)}
    B = c.B
    checked = 0
    for how, r in runs.items():
        tag = f"label_head:{c.name}:{kind}:{how}"
        _check_zero_rules(r, c, i, tag)
        f32, f64 = LC.reference(c.name, kind, LC.SCALE if how.endswith("scale") else 1.0)
        last = slice(LC.HEAD_ROWS * ((B - 1) // LC.HEAD_ROWS), B)
        legs = [{"pred": r["pred"], "loss": r["loss"], "emb": r["emb"], "w": r["w"], "b": r["b"]}, dict(f32), dict(f64)]
        for d in legs:
            d["emb"] = d["emb"][:B]
            d["emb[last block]"], d["emb[first block]"] = d["emb"][last], d["emb"][:LC.HEAD_ROWS]
            d["pred[last block]"], d["pred[first block]"] = d["pred"][last], d["pred"][:LC.HEAD_ROWS]
        n = F64.check(*legs, tag)
        assert n >= 8 - (0 if c.bias else 1)
        checked += n
    print(f"F64.check {c.name} {kind}: {checked} tensors")
    # the fused entry against the forward + backward pair at grad_loss = 1: the same kernels' arithmetic, to the bit
    a, s = runs["fused"], runs["split"]
    assert abs(float(a["loss"]) - float(s["loss"])) <= 1e-6 * abs(float(s["loss"])), (c.name, kind)   # (two instantiations of the terms)
    for nm in ("pred", "emb", "w", "b"):
        if a[nm] is not None:
            assert torch.equal(a[nm], s[nm]), (c.name, kind, nm, "fused and split differ")
    # two identical calls: the same bits
    again = run(False, None)
    for nm in ("loss", "pred", "emb", "w", "b"):
        if a[nm] is not None:
            assert torch.equal(again[nm], a[nm]), (c.name, kind, nm, "not reproducible")
    # pred: bit for bit task_scores at dropout 0, and the task-indexed head's pred of every (row, task) under dropout
    dev = a["pred"].device
    if c.p == 0.0:
        with torch.no_grad():
            want = R.task_scores(i["emb"][:B].to(dev), _ffn(i, c, dev), n_rows=B)
        assert torch.equal(a["pred"], want), (c.name, kind, "pred differs from task_scores")
    if B <= 33:
        assert torch.equal(a["pred"], _task_head_pred(c, i, kind, dev)), (c.name, kind, "pred differs from the task head's")
    # an embedding that needs no gradient: the parameter gradients, pred and loss to the bit
    if not c.emb_grad:
        for split in (False, True):
            full, none = runs["split" if split else "fused"], run(split, None, emb_grad=False)
            assert none["emb"] is None
            for nm in ("loss", "pred", "w", "b"):
                if full[nm] is not None:
                    assert torch.equal(none[nm], full[nm]), (c.name, kind, split, nm, "changes when emb needs no gradient")
    # the label_table + row_ids route (a permuted table, repeated and out-of-table ids) against the same labels passed directly
    if c.row_ids:
        for split in (False, True):
            via, direct = runs["split" if split else "fused"], run(split, None, direct=True)
            for nm in ("loss", "pred", "emb", "w", "b"):
                if via[nm] is not None:
                    assert torch.equal(via[nm], direct[nm]), (c.name, kind, split, nm, "row_ids and labels differ")
    # sample weights that are all exactly 1 against no sample weights at all
    if not c.sample_weight:
        for split in (False, True):
            plain, ones = runs["split" if split else "fused"], run(split, None, ones=True)
            for nm in ("loss", "pred", "emb", "w", "b"):
                if plain[nm] is not None:
                    assert torch.equal(plain[nm], ones[nm]), (c.name, kind, split, nm, "weights of 1 change the bits")
    return runs


@pytest.mark.parametrize("kind", LC.KINDS)
@pytest.mark.parametrize("name", [c.name for c in LC.CASES_LIST])
def test_label_head_edges(name, kind, monkeypatch):
    _run_case(LC.CASES[name], kind, monkeypatch)


def test_bce_at_saturated_logits(monkeypatch):
    """Task-1 logits of exactly +90, -90 and 0 for both labels: finite everywhere, and d loss / d emb of those rows (their only
    label) is (sigmoid - y) W[1] / n_lab within the bound; where the sigmoid saturates onto the label it is exactly zero."""
    c = LC.SATURATED
    runs = _run_case(c, "bce", monkeypatch)
    i = LC.inputs(c.name, "bce")
    n_lab = int(i["mask"].sum())
    w64 = i["w"][LC.SATURATED_TASK].double()
    sig = {90.0: 1.0, -90.0: 0.0, 0.0: 0.5}
    want = torch.stack([(sig[x] - t) * w64 / n_lab for x, t in zip(LC.SATURATED_LOGITS, LC.SATURATED_TARGETS)])
    _, f64 = LC.reference(c.name, "bce", 1.0)
    assert float((f64["emb"][:6] - want).abs().max()) <= 1e-15 * float(want.abs().max())      # (the reference itself)
    for how in ("fused", "split"):
        r = runs[how]
        assert r["pred"][:6, LC.SATURATED_TASK].tolist() == list(LC.SATURATED_LOGITS), how
        got = {f"emb[row {k}]": r["emb"][k] for k in range(6)}
        F64.check(got, {k: want[n].float() for n, k in enumerate(got)}, {k: want[n] for n, k in enumerate(got)},
                  f"label_head:{c.name}:bce:{how}:rows")
        assert float(r["emb"][1].abs().max()) == 0.0 and float(r["emb"][2].abs().max()) == 0.0, how


def test_the_generator_advances_once_per_forward_with_dropout_only(monkeypatch):
    from molkgnn_amd import readout as R
    dev = _dev()
    c = LC.CASES["B15xH5xT2_quarter_missing"]
    i = LC.inputs(c.name, "bce")
    ffn, emb, labels = _ffn(i, c, dev), i["emb"][:c.B].to(dev), i["labels"][:c.B].to(dev)
    for split in (False, True):
        monkeypatch.setattr(R, "_SPLIT_HEAD", split)
        R.reset_head_rng(dev, seed=LC.SEED)
        state = R.head_rng_state(dev)
        for k, (p, grad) in enumerate(((0.25, True), (0.25, False), (0.0, True), (0.5, True))):
            e = emb.clone().requires_grad_(grad)
            loss = R.label_head_loss(e, ffn, labels, "bce", dropout_p=p)
            if grad:
                loss.backward()                                   # (the backward draws nothing: it reads the forward's rng_used)
            torch.cuda.synchronize()
            assert state.tolist() == [LC.SEED, (1, 2, 2, 3)[k]], (split, k)


# ---------------------------------------------------------------------------------------------- the C ABI --
def _c_buffers(c, kind, dev, pad):
    """Device buffers of a case with every row stride padded by ``pad`` and the outputs pre-filled with the canary."""
    i = LC.inputs(c.name, kind)
    n = c.B + c.n_pad
    f = lambda rows, cols, src=None: (torch.full((rows, cols + pad), CANARY, device=dev) if src is None else
                                      torch.cat([src.to(dev), torch.full((rows, pad), LC.NAN, device=dev)], dim=1).contiguous())
    b = dict(emb=f(n, c.H, i["emb"]), labels=f(n, c.T, i["labels"]), pred=f(n, c.T), gemb=f(n, c.H),
             w=i["w"].to(dev).contiguous(), b=_to(i["b"], dev), gw=torch.full((c.T, c.H), CANARY, device=dev),
             gb=torch.full((c.T,), CANARY, device=dev), loss=torch.full((1,), CANARY, device=dev),
             sw=_to(i["sw"], dev), pw=_to(i["pw"], dev), rng=torch.tensor([LC.SEED, 0], dtype=torch.int64, device=dev),
             used=torch.zeros(2, dtype=torch.int64, device=dev), ws=torch.zeros(1 << 22, dtype=torch.uint8, device=dev))
    return i, b


def _weights(b):
    from molkgnn_amd import _lib
    lw = _lib.LossWeights()
    lw.sample_weight, lw.pos_weight = _lib.ptr(b["sw"]), _lib.ptr(b["pw"])
    lw.n_sample_weight = 0 if b["sw"] is None else b["sw"].numel()
    return lw


@pytest.mark.parametrize("kind", ["bce", "mse"])
@pytest.mark.parametrize("name", ["B577xH64xT9_row_absent", "B1xH64xT9_task_absent", "B15xH32xT32_one_per_row",
                                  "B15xH5xT2_quarter_missing"])
def test_c_entries_with_padded_strides_leave_the_rest_untouched(name, kind, monkeypatch):
    """The three entries called directly with padded row strides of emb, labels, pred and grad_emb: the operator's bits, and
    rows >= n_rows of grad_emb and pred, and the elements between the strides, keep their canary."""
    from molkgnn_amd import _lib
    lib, dev = _lib.load(), _dev()
    c = LC.CASES[name]
    pad = 3
    i, b = _c_buffers(c, kind, dev, pad)
    lw = _weights(b)
    B, H, T = c.B, c.H, c.T
    lk = {"bce": 0, "mse": 1}[kind]
    p = _lib.ptr
    args = (lk, p(b["emb"]), H + pad, B, H, T, p(b["w"]), p(b["b"]), p(b["labels"]), T + pad, None, b["labels"].shape[0],
            float(c.p), p(b["rng"]), p(b["used"]), p(b["pred"]), T + pad, p(b["loss"]))
    with torch.cuda.device(dev):
        rc = lib.mkgnn_label_head_fused(*args, p(b["gemb"]), H + pad, p(b["gw"]), p(b["gb"]), ctypes.byref(lw), p(b["ws"]),
                                        b["ws"].numel(), _lib.stream_ptr(dev))
    assert rc == 0, lib.mkgnn_last_error()
    torch.cuda.synchronize()
    fused = {k: b[k].clone() for k in ("pred", "gemb", "gw", "gb", "loss")}
    for nm in ("pred", "gemb"):
        width = T if nm == "pred" else H
        assert bool((fused[nm][B:] == CANARY).all()) and bool((fused[nm][:, width:] == CANARY).all()), (nm, "canary")
        assert bool(torch.isfinite(fused[nm][:B, :width]).all()), nm
    # the operator on the same inputs: the same bits
    run, _ = _runner(c, kind, monkeypatch)
    r = run(False, None)
    assert torch.equal(fused["pred"][:B, :T], r["pred"]) and torch.equal(fused["loss"][0], r["loss"])
    assert torch.equal(fused["gemb"][:B, :H], r["emb"][:B]) and torch.equal(fused["gw"].reshape(-1), r["w"])
    if c.bias:
        assert torch.equal(fused["gb"], r["b"])
    if c.p > 0.0:
        assert b["rng"].tolist() == [LC.SEED, 1] and b["used"].tolist() == [LC.SEED, 0]
    # forward, then backward with grad_loss = 1 from the device: pred and loss of the forward, the fused entry's gradients
    for k in ("pred", "gemb", "gw", "gb", "loss"):
        b[k].fill_(CANARY)
    b["rng"].copy_(torch.tensor([LC.SEED, 0]))
    one = torch.ones(1, device=dev)
    with torch.cuda.device(dev):
        rc = lib.mkgnn_label_head_forward(*args, ctypes.byref(lw), p(b["ws"]), b["ws"].numel(), _lib.stream_ptr(dev))
        assert rc == 0, lib.mkgnn_last_error()
        rc = lib.mkgnn_label_head_backward(lk, p(b["emb"]), H + pad, B, H, T, p(b["w"]), p(b["labels"]), T + pad, None,
                                           b["labels"].shape[0], p(b["pred"]), T + pad, p(one), float(c.p), p(b["used"]),
                                           p(b["gemb"]), H + pad, p(b["gw"]), p(b["gb"]), ctypes.byref(lw), p(b["ws"]),
                                           b["ws"].numel(), _lib.stream_ptr(dev))
        assert rc == 0, lib.mkgnn_last_error()
    torch.cuda.synchronize()
    for k in ("pred", "gemb", "gw", "gb"):
        assert torch.equal(b[k], fused[k]), (k, "forward + backward differ from fused")
    assert abs(float(b["loss"]) - float(fused["loss"])) <= 1e-6 * abs(float(fused["loss"]))
    # grad_emb may be null: the parameter gradients are the same bits
    b["gw"].fill_(CANARY)
    with torch.cuda.device(dev):
        rc = lib.mkgnn_label_head_backward(lk, p(b["emb"]), H + pad, B, H, T, p(b["w"]), p(b["labels"]), T + pad, None,
                                           b["labels"].shape[0], p(b["pred"]), T + pad, p(one), float(c.p), p(b["used"]),
                                           None, 0, p(b["gw"]), None, ctypes.byref(lw), p(b["ws"]), b["ws"].numel(),
                                           _lib.stream_ptr(dev))
    assert rc == 0, lib.mkgnn_last_error()
    torch.cuda.synchronize()
    assert torch.equal(b["gw"], fused["gw"])


def test_c_entries_reject_bad_arguments_before_any_launch():
    from molkgnn_amd import _lib
    lib, dev = _lib.load(), _dev()
    c = LC.CASES["B15xH5xT2_quarter_missing"]
    i, b = _c_buffers(c, "bce", dev, 0)
    B, H, T = c.B, c.H, c.T
    p = _lib.ptr
    ok = dict(kind=0, es=H, n=B, H=H, T=T, ls=T, ids=None, rows=B + c.n_pad, p=0.25, ps=T, ges=H, emb=p(b["emb"]), ws=p(b["ws"]),
              rng=p(b["rng"]), lw=None)
    short = _lib.LossWeights()
    short.sample_weight, short.n_sample_weight = p(b["sw"]) if b["sw"] is not None else p(b["w"]), B - 1
    posw = _lib.LossWeights()
    posw.pos_weight = p(b["w"])
    bad = (dict(T=33), dict(T=0), dict(H=65), dict(H=0), dict(n=0), dict(n=-1), dict(es=H - 1), dict(ls=T - 1), dict(ps=T - 1),
           dict(rows=B - 1), dict(ids=p(b["rng"]), rows=0), dict(kind=7), dict(p=1.0), dict(p=float("nan")), dict(rng=None),
           dict(emb=None), dict(ws=None), dict(ges=H - 1), dict(lw=ctypes.byref(short)), dict(kind=1, lw=ctypes.byref(posw)))
    for change in bad:
        a = dict(ok, **change)
        rc = lib.mkgnn_label_head_fused(a["kind"], a["emb"], a["es"], a["n"], a["H"], a["T"], p(b["w"]), p(b["b"]), p(b["labels"]),
                                        a["ls"], a["ids"], a["rows"], a["p"], a["rng"], p(b["used"]), p(b["pred"]), a["ps"],
                                        p(b["loss"]), p(b["gemb"]), a["ges"], p(b["gw"]), p(b["gb"]), a["lw"], a["ws"],
                                        b["ws"].numel(), _lib.stream_ptr(dev))
        assert rc != 0 and lib.mkgnn_last_error(), change
    torch.cuda.synchronize()
    for k in ("pred", "gemb", "gw", "gb", "loss"):
        assert bool((b[k] == CANARY).all()), k
    assert b["rng"].tolist() == [LC.SEED, 0]


# ------------------------------------------------------------------------------------------ the torch route --
@pytest.mark.parametrize("T,H,switch", [(33, 8, True), (3, 65, True), (9, 32, False)])
def test_outside_the_limits_or_switched_off_takes_the_torch_route(T, H, switch, monkeypatch):
    """More than 32 tasks, an embedding wider than 64, or ``MKGNN_LABEL_HEAD=0``: ``label_head_reference`` on the GPU, no call
    into the library."""
    from molkgnn_amd import _lib, readout as R
    dev = _dev()
    monkeypatch.setattr(R, "_LABEL_HEAD", switch)
    g = torch.Generator().manual_seed(T * 100 + H)
    B = 40
    emb = torch.randn(B, H, generator=g).to(dev).requires_grad_(True)
    ffn = torch.nn.Linear(H, T).to(dev)
    mask = LC.label_mask("row_absent", B, T)
    labels = torch.where(mask, (torch.rand(B, T, generator=g) < 0.3).float(), torch.full((), LC.NAN)).to(dev)
    calls = []
    real = _lib.check
    monkeypatch.setattr(_lib, "check", lambda rc, what: (calls.append(what), real(rc, what))[1])
    loss, pred = R.label_head_loss(emb, ffn, labels, "bce", return_pred=True)
    loss.backward()
    torch.cuda.synchronize()
    assert calls == [] and pred.shape == (B, T) and not pred.requires_grad, calls
    want, _ = R.label_head_reference(emb.detach().cpu().double(), ffn.weight.detach().cpu().double(), ffn.bias.detach().cpu().double(),
                                     labels.cpu().double(), "bce")
    assert abs(float(loss.detach()) - float(want)) <= 1e-5 * abs(float(want))
    assert bool(torch.isfinite(emb.grad).all()) and float(emb.grad[~mask.any(dim=1).to(dev)].abs().max()) == 0.0
