"""The weighted task-indexed head on the GPU (``readout.task_head_loss`` / ``readout.head_loss`` with weights ->
``_WeightedTaskHeadFn``; ``mkgnn_task_head_weighted_*``, csrc/kgnn_task_head.hip): against float64 at the edges of its kernels
(cases and references: ``tests/_weighted_head_cases.py``), the bit links to the unweighted entry points, the exact-zero rules and
the raw ABI's refusals.  ``pytest -m gpu``.

Bound: ``tests/_f64.check``, constants as they stand; the float32 leg is ``readout.task_head_reference`` in float32, the exact
leg the same function in float64.  Per case: ``pred``, ``loss``, each gradient, and the rows of the first and of the last
(partial) 16-row block of ``pred`` and ``grad_emb`` on their own; the exact-zero rules by ``== 0.0``.
"""
import ctypes

import pytest
import torch

from tests import _f64 as F64
from tests import _weighted_head_cases as WC

pytestmark = pytest.mark.gpu


def _dev():
    assert torch.cuda.is_available(), "pytest -m gpu needs the MI355X"
    return torch.device("cuda:0")


def _ffn(i, c, dev):
    ffn = torch.nn.Linear(c.H, c.tasks, bias=c.bias)
    with torch.no_grad():
        ffn.weight.copy_(i["w"])
        if c.bias:
            ffn.bias.copy_(i["b"])
    return ffn.to(dev)


def _runner(c, kind, monkeypatch, override=None):
    """``run(split, scale, emb_grad=True)`` -> loss, pred, the gradients and the generator state of one forward + backward of the
    case on the GPU; ``scale`` None: seeded by train.backward's registered 1.  ``override``: replaces weight keywords."""
    from molkgnn_amd import readout as R
    from molkgnn_amd.train import backward
    dev = _dev()
    i = WC.inputs(c.name, kind)
    ffn = _ffn(i, c, dev)
    n = c.B + c.n_pad
    store = torch.zeros(n, c.H + c.stride_pad, device=dev)
    store[:, :c.H] = i["emb"].to(dev)
    on = lambda t: None if t is None else t.to(dev)
    y, task, table, ids = on(i["y"]), on(i["task"]), on(i["task_table"]), on(i["row_ids"])
    kw = WC.weight_keywords(i, on)
    if override is not None:
        kw.update(override)

    def run(split, scale, emb_grad=True, task_vector=None, single=False):
        monkeypatch.setattr(R, "_SPLIT_HEAD", split)
        R.reset_head_rng(dev, seed=WC.SEED)
        leaf = store.clone().requires_grad_(emb_grad)
        emb = leaf[:, :c.H]                                   # (row stride H + stride_pad)
        assert emb.stride(0) == c.H + c.stride_pad
        ffn.zero_grad(set_to_none=True)
        if single:                                            # the single-task entry: head_loss, no task at all
            loss = R.head_loss(emb, ffn, y, kind, dropout_p=c.p, n_rows=c.B, row_ids=ids, **kw)
        else:
            loss = R.task_head_loss(emb, ffn, y, task if task_vector is None else task_vector, kind, dropout_p=c.p, n_rows=c.B,
                                    task_table=table, row_ids=ids, **kw)
        assert type(loss.grad_fn).__name__ == "_WeightedTaskHeadFnBackward"
        pred = loss.grad_fn.saved_tensors[3].clone()
        if scale is None:
            backward(loss)
        else:
            (loss * scale).backward()
        torch.cuda.synchronize()
        rng = R.head_rng_state(dev).clone() if c.p > 0.0 else None
        return dict(loss=loss.detach().clone(), pred=pred, emb=None if leaf.grad is None else leaf.grad[:, :c.H].clone(),
                    w=ffn.weight.grad.clone().reshape(-1), b=None if not c.bias else ffn.bias.grad.clone(), rng=rng)

    return run, i


def _check_zero_rules(r, c, i, tag):
    dev = r["pred"].device
    lab, s_eff, task = i["lab"].to(dev), i["s_eff"].to(dev), i["task_direct"][:c.B].to(dev)
    for nm in ("loss", "pred", "emb", "w", "b"):
        if r[nm] is not None:
            assert bool(torch.isfinite(r[nm]).all()), (tag, nm)
    dead = ~lab | (s_eff == 0)
    if r["emb"] is not None:
        assert r["emb"].shape == (c.B + c.n_pad, c.H)
        if c.n_pad:
            assert float(r["emb"][c.B:].abs().max()) == 0.0, (tag, "padding rows")
        if bool(dead.any()):
            assert float(r["emb"][:c.B][dead].abs().max()) == 0.0, (tag, "unlabelled rows and rows of weight 0")
    if bool((~lab).any()):
        assert float(r["pred"][~lab].abs().max()) == 0.0 and not bool(torch.signbit(r["pred"][~lab]).any()), (tag, "pred of unlabelled rows")
    silent = torch.tensor([not bool(((task == t) & ~dead).any()) for t in range(c.tasks)], device=dev)
    if bool(silent.any()):
        assert float(r["w"].reshape(c.tasks, c.H)[silent].abs().max()) == 0.0, (tag, "tasks without a weighing row: grad W")
        if c.bias:
            assert float(r["b"][silent].abs().max()) == 0.0, (tag, "tasks without a weighing row: grad b")
    if c.p > 0.0:
        assert r["rng"].tolist() == [WC.SEED, 1], (tag, "one draw per forward, as the unweighted call")


def _run_case(c, kind, monkeypatch):
    run, i = _runner(c, kind, monkeypatch)
    runs = {"fused": run(False, None), "split": run(True, None)}
    if c.scale:
        runs.update({"split*scale": run(True, WC.SCALE), "fused*scale": run(False, WC.SCALE)})
    B = c.B
    checked = 0
    for how, r in runs.items():
        tag = f"weighted_head:{c.name}:{kind}:{how}"
        _check_zero_rules(r, c, i, tag)
        f32, f64 = WC.reference(c.name, kind, WC.SCALE if how.endswith("scale") else 1.0)
        last = slice(WC.HEAD_ROWS * ((B - 1) // WC.HEAD_ROWS), B)
        legs = [{"pred": r["pred"], "loss": r["loss"], "emb": r["emb"], "w": r["w"], "b": r["b"]}, dict(f32), dict(f64)]
        for d in legs:
            d["emb"] = d["emb"][:B]
            d["emb[last block]"], d["emb[first block]"] = d["emb"][last], d["emb"][:WC.HEAD_ROWS]
            d["pred[last block]"], d["pred[first block]"] = d["pred"][last], d["pred"][:WC.HEAD_ROWS]
        n = F64.check(*legs, tag)
        assert n >= 8 - (0 if c.bias else 1)
        checked += n
    print(f"F64.check {c.name} {kind}: {checked} tensors")
    # (c) the fused form against forward + backward where they must agree to the bit: seeded by the registered unit gradient
    a, s = runs["fused"], runs["split"]
    assert abs(float(a["loss"]) - float(s["loss"])) <= 1e-6 * abs(float(s["loss"])), (c.name, kind)   # (two fixed orders of the partials)
    assert torch.equal(a["pred"], s["pred"])
    for nm in ("emb", "w", "b"):
        if a[nm] is not None:
            assert torch.equal(a[nm], s[nm]), (c.name, kind, nm, "fused and split differ")
    # (d) two identical calls: the same bits
    again = run(False, None)
    for nm in ("loss", "pred", "emb", "w", "b"):
        if a[nm] is not None:
            assert torch.equal(again[nm], a[nm]), (c.name, kind, nm, "not reproducible")
    # an embedding that needs no gradient: the parameter gradients, pred and loss to the bit
    if not c.emb_grad:
        for split in (False, True):
            full, none = runs["split" if split else "fused"], run(split, None, emb_grad=False)
            assert none["emb"] is None
            for nm in ("loss", "pred", "w", "b"):
                if full[nm] is not None:
                    assert torch.equal(none[nm], full[nm]), (c.name, kind, split, nm, "changes when emb needs no gradient")
    # (e) no task vector at a one-output head: the bits of an all-zero task vector, and of head_loss
    if c.T is None:
        zeros = torch.zeros(c.B + c.n_pad, dtype=torch.int32, device=_dev())
        for split in (False, True):
            base = runs["split" if split else "fused"]
            for other in (run(split, None, task_vector=zeros), run(split, None, single=True)):
                for nm in ("loss", "pred", "emb", "w", "b"):
                    if base[nm] is not None:
                        assert torch.equal(other[nm], base[nm]), (c.name, kind, split, nm, "task=None differs from an all-zero task")
    return runs


@pytest.mark.parametrize("name,kind", WC.PAIRS)
def test_weighted_head_edges(name, kind, monkeypatch):
    _run_case(WC.CASES[name], kind, monkeypatch)


def test_bce_with_a_positive_weight_at_saturated_logits(monkeypatch):
    """Logits of exactly +90, -90 and 0 on task-1 rows for both targets with p = 37.5: finite everywhere, within the bound, and the
    term at x = -90, y = 1 -- singled out by one-hot sample weights -- is exactly 3375."""
    from molkgnn_amd import readout as R
    c = WC.SATURATED
    runs = _run_case(c, "bce", monkeypatch)
    for how in ("fused", "split"):
        assert runs[how]["pred"][:6].tolist() == list(WC.SATURATED_LOGITS), how
    onehot = torch.zeros(c.B, device=_dev())
    onehot[WC.SATURATED_ROW] = 1.0
    run, _ = _runner(c, "bce", monkeypatch, override=dict(sample_weight=onehot))
    want = float(torch.tensor(WC.SATURATED_TERM) / c.B)
    for split in (False, True):
        r = run(split, None)
        assert float(r["loss"]) == want, (split, float(r["loss"]))
        # d term / d x = (1 - y) - L sigmoid(-x) = -37.5 there, and exactly 0 at every other row
        assert float(r["emb"][WC.SATURATED_ROW, 0]) == float(torch.tensor(-WC.SATURATED_POS * 90.0) * (torch.tensor(1.0) / c.B))
        others = torch.arange(c.B, device=_dev()) != WC.SATURATED_ROW
        assert float(r["emb"][others].abs().max()) == 0.0


# --------------------------------------------------------------------------------- links to the unweighted head --
@pytest.mark.parametrize("kind", WC.KINDS)
@pytest.mark.parametrize("name", ["B577xH64xT9_quarter_unlabelled_table_pos", "B15xH5xT2_round_robin_row_pos", "B17xH33xTnone_all_one_row"])
def test_all_ones_weights_give_the_unweighted_bits(name, kind, monkeypatch):
    """(b) Sample weights of exactly 1.0 (per row, and as a table) without ``pos_weight``: loss, pred, every gradient and the
    generator state of ``task_head_loss`` without keywords, for all three kinds, fused and split, at ``grad_loss`` 1 and 1.7."""
    from molkgnn_amd import readout as R
    from molkgnn_amd.train import backward
    dev = _dev()
    c = WC.CASES[name]
    i = WC.inputs(name, "bce" if c.pos else kind)
    ffn = _ffn(i, c, dev)
    n = c.B + c.n_pad
    emb0, y = i["emb"].to(dev), i["y"].to(dev)
    if kind != "bce":
        y = y * 3 - 8
    task = i["task_direct"].to(dev)
    forms = {"none": {}, "row": dict(sample_weight=torch.ones(n, device=dev)),
             "table": dict(weight_table=torch.ones(5, device=dev), row_ids=(torch.arange(n, device=dev) % 5).to(torch.int32))}
    for split in (False, True):
        monkeypatch.setattr(R, "_SPLIT_HEAD", split)
        for scale in (None, WC.SCALE):
            out = {}
            for how, kw in forms.items():
                R.reset_head_rng(dev, seed=WC.SEED)
                emb = emb0.clone().requires_grad_(True)
                ffn.zero_grad(set_to_none=True)
                loss = R.task_head_loss(emb, ffn, y, task, kind, dropout_p=c.p, n_rows=c.B, **kw)
                assert type(loss.grad_fn).__name__ == ("_TaskHeadFnBackward" if how == "none" else "_WeightedTaskHeadFnBackward")
                pred = loss.grad_fn.saved_tensors[3].clone()
                backward(loss) if scale is None else (loss * scale).backward()
                out[how] = [loss.detach().clone(), pred, emb.grad.clone(), ffn.weight.grad.clone()] + \
                    ([ffn.bias.grad.clone()] if c.bias else []) + ([R.head_rng_state(dev).clone()] if c.p > 0 else [])
            torch.cuda.synchronize()
            for how in ("row", "table"):
                for k, (a, e) in enumerate(zip(out[how], out["none"])):
                    assert torch.equal(a, e), (name, kind, split, scale, how, k)


def _raw_buffers(B, H, T, dev, seed=5):
    g = torch.Generator().manual_seed(seed)
    t = lambda *s: torch.randn(*s, generator=g).to(dev)
    return dict(emb=t(B, H), w=t(T, H), b=t(T), y=(torch.rand(B, generator=g) < 0.3).float().to(dev),
                task=WC.task_pattern("quarter_unlabelled", B, T).to(dev), gl=torch.tensor([WC.SCALE], device=dev))


def _raw_call(lib, entry, weighted, lw, x, B, H, T, p, ws, kind=0, task="task"):
    """One raw call of (mkgnn_task_head_[weighted_]<entry>) on fresh outputs filled with a sentinel -> (rc, outputs, generator)."""
    dev = x["emb"].device
    fill = lambda *s: torch.full(s, -7.25, device=dev)
    pred, loss, gemb, gw, gb = fill(B), fill(1), fill(B, H), fill(T, H), fill(T)
    rng = torch.tensor([WC.SEED, 0], dtype=torch.int64, device=dev)
    used = torch.tensor([WC.SEED, 0], dtype=torch.int64, device=dev)
    tk = None if task is None else x[task].data_ptr()
    head = (kind, x["emb"].data_ptr(), H, B, H, T, x["w"].data_ptr())
    extra = () if not weighted else (None if lw is None else ctypes.byref(lw),)
    tail = (*extra, ws.data_ptr(), ws.numel(), None)
    fn = getattr(lib, ("mkgnn_task_head_weighted_" if weighted else "mkgnn_task_head_") + entry)
    if entry == "forward":
        rc = fn(*head, x["b"].data_ptr(), x["y"].data_ptr(), tk, None, B, p, rng.data_ptr(), used.data_ptr(), pred.data_ptr(),
                loss.data_ptr(), *tail)
    elif entry == "fused":
        rc = fn(*head, x["b"].data_ptr(), x["y"].data_ptr(), tk, None, B, p, rng.data_ptr(), used.data_ptr(), pred.data_ptr(),
                loss.data_ptr(), gemb.data_ptr(), H, gw.data_ptr(), gb.data_ptr(), *tail)
    else:
        pred = x["pred"].clone()
        rc = fn(*head, x["y"].data_ptr(), tk, None, B, pred.data_ptr(), x["gl"].data_ptr(), p, used.data_ptr(), gemb.data_ptr(), H,
                gw.data_ptr(), gb.data_ptr(), *tail)
    torch.cuda.synchronize()
    return rc, [pred, loss, gemb, gw, gb], rng


@pytest.mark.parametrize("kind", [0, 1, 2])
def test_null_weights_are_the_unweighted_entry_points(kind):
    """(a), (f) ``weights == NULL``, and a struct whose pointers are all NULL, with a task vector: every output and the generator
    state of ``mkgnn_task_head_forward`` / ``_backward`` / ``_fused``, bit for bit."""
    from molkgnn_amd import _lib
    lib = _lib.load()
    dev = _dev()
    B, H, T, p = 577, 33, 9, 0.25
    x = _raw_buffers(B, H, T, dev)
    ws = torch.zeros(int(lib.mkgnn_task_head_workspace_bytes(B, H, T)), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        rc, fwd, _ = _raw_call(lib, "forward", False, None, x, B, H, T, p, ws, kind)
        assert rc == 0
        x["pred"] = fwd[0]
        for entry in ("forward", "backward", "fused"):
            rc, want, rng_want = _raw_call(lib, entry, False, None, x, B, H, T, p, ws, kind)
            assert rc == 0, lib.mkgnn_last_error()
            for lw in (None, _lib.LossWeights()):
                rc, got, rng = _raw_call(lib, entry, True, lw, x, B, H, T, p, ws, kind)
                assert rc == 0, lib.mkgnn_last_error()
                assert torch.equal(rng, rng_want) and rng.tolist() == [WC.SEED, 0 if entry == "backward" else 1]
                for k, (a, e) in enumerate(zip(got, want)):
                    assert torch.equal(a, e), (entry, kind, k)


def test_raw_entry_points_refuse_and_launch_nothing():
    """Device pointers, bad arguments: non-zero, ``mkgnn_last_error`` set, and every output still holds its sentinel."""
    from molkgnn_amd import _lib
    lib = _lib.load()
    dev = _dev()
    B, H, p = 40, 8, 0.0
    ws = torch.zeros(1 << 20, dtype=torch.uint8, device=dev)
    one = torch.ones(B, device=dev)

    def weights(sw=None, ids=None, n=0, pw=None):
        lw = _lib.LossWeights()
        lw.sample_weight, lw.weight_ids, lw.n_sample_weight, lw.pos_weight = _lib.ptr(sw), _lib.ptr(ids), n, _lib.ptr(pw)
        return lw

    ids = torch.zeros(B, dtype=torch.int32, device=dev)
    bad = [dict(T=1, kind=9, lw=weights(sw=one, n=B)), dict(T=1, kind=1, lw=weights(pw=one)), dict(T=1, kind=2, lw=weights(pw=one)),
           dict(T=3, kind=0, lw=weights(sw=one, n=B), task=None), dict(T=1, kind=0, lw=weights(sw=one, n=B - 1)),
           dict(T=1, kind=0, lw=weights(sw=one, ids=ids, n=0)), dict(T=33, kind=0, lw=weights(sw=one, n=B))]
    with torch.cuda.device(dev):
        for a in bad:
            T = a["T"]
            x = _raw_buffers(B, H, T, dev)
            x["pred"] = torch.zeros(B, device=dev)
            for entry in ("forward", "backward", "fused"):
                rc, outs, rng = _raw_call(lib, entry, True, a["lw"], x, B, H, T, p, ws, a["kind"], task=a.get("task", "task"))
                assert rc != 0 and lib.mkgnn_last_error(), (a, entry)
                for k, o in enumerate(outs):
                    if not (entry == "backward" and k == 0):
                        assert bool((o == -7.25).all()), (a, entry, k, "something was launched")
                assert rng.tolist() == [WC.SEED, 0]


# ------------------------------------------------------------------------------------------ the torch routes --
@pytest.mark.parametrize("how", ["beyond the limits", "MKGNN_WEIGHTED_LOSS=0"])
def test_the_definition_runs_in_torch_operators_where_the_kernels_do_not(how, monkeypatch):
    from molkgnn_amd import _lib, readout as R
    dev = _dev()
    T, H, B = (3, 65, 40) if how == "beyond the limits" else (3, 8, 40)
    if how != "beyond the limits":
        monkeypatch.setattr(R, "_WEIGHTED_LOSS", False)
    g = torch.Generator().manual_seed(T * 100 + H)
    emb = torch.randn(B, H, generator=g).to(dev).requires_grad_(True)
    ffn = torch.nn.Linear(H, T).to(dev)
    y = (torch.rand(B, generator=g) < 0.3).float().to(dev)
    task = WC.task_pattern("quarter_unlabelled", B, T).to(dev)
    s = torch.rand(B, generator=g).to(dev)
    s[::4] = 0.0
    pw = torch.tensor([2.0, 37.5, 0.5], device=dev)
    calls = []
    real = _lib.check
    monkeypatch.setattr(_lib, "check", lambda rc, what: (calls.append(what), real(rc, what))[1])
    loss = R.task_head_loss(emb, ffn, y, task, "bce", sample_weight=s, pos_weight=pw)
    loss.backward()
    torch.cuda.synchronize()
    assert calls == [], calls
    want, _ = R.task_head_reference(emb.detach().cpu().double(), ffn.weight.detach().cpu().double(), ffn.bias.detach().cpu().double(),
                                    y.cpu().double(), task.cpu(), "bce", sample_weight=s.cpu().double(), pos_weight=pw.cpu().double())
    assert abs(float(loss.detach()) - float(want)) <= 1e-5 * abs(float(want))
    assert bool(torch.isfinite(emb.grad).all()) and float(emb.grad[(task < 0) | (s == 0)].abs().max()) == 0.0
