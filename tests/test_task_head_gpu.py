"""The task-indexed head with masked labels on the GPU (``readout.task_head_loss`` -> ``_TaskHeadFn``; ``mkgnn_task_head_*``,
csrc/kgnn_task_head.hip): against float64 at the edges of its kernels (cases and references: ``tests/_task_head_cases.py``),
through ``GNNModel.loss`` and through one captured step fed from a resident shard.  ``pytest -m gpu``.

Bound: ``tests/_f64.check``, constants as they stand; the float32 leg is ``readout.task_head_reference`` in float32, the exact
leg the same function in float64.  Per case: ``pred``, ``loss``, each gradient, and the rows of the first and of the last
(partial) 16-row block of ``pred`` and ``grad_emb`` on their own; the exact-zero rules by ``== 0.0``.
"""
import copy

import numpy as np
import pytest
import torch

from tests import _f64 as F64
from tests import _philox
from tests import _readout_f64 as RF
from tests import _task_head_cases as TC

pytestmark = pytest.mark.gpu


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


def _runner(c, kind, monkeypatch):
    """``run(split, scale, emb_grad=True, direct=False)`` -> loss, pred, the gradients and the generator state of one forward +
    backward of the case on the GPU; ``scale`` None: seeded by train.backward's registered 1."""
    from molkgnn_amd import readout as R
    from molkgnn_amd.train import backward
    dev = _dev()
    i = TC.inputs(c.name, kind)
    ffn = _ffn(i, c, dev)
    n = c.B + c.n_pad
    store = torch.zeros(n, c.H + c.stride_pad, device=dev)
    store[:, :c.H] = i["emb"].to(dev)
    y, task = i["y"].to(dev), i["task"].to(dev)
    table = None if i["task_table"] is None else i["task_table"].to(dev)
    ids = None if i["row_ids"] is None else i["row_ids"].to(dev)

    def run(split, scale, emb_grad=True, direct=False):
        monkeypatch.setattr(R, "_SPLIT_HEAD", split)
        R.reset_head_rng(dev, seed=TC.SEED)
        leaf = store.clone().requires_grad_(emb_grad)
        emb = leaf[:, :c.H]                                   # (row stride H + stride_pad)
        assert emb.stride(0) == c.H + c.stride_pad
        ffn.zero_grad(set_to_none=True)
        if table is not None and not direct:
            loss = R.task_head_loss(emb, ffn, y, None, kind, dropout_p=c.p, n_rows=c.B, task_table=table, row_ids=ids)
        else:
            loss = R.task_head_loss(emb, ffn, y, task, kind, dropout_p=c.p, n_rows=c.B)
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
    lab = i["lab"].to(r["pred"].device)
    task = i["task"][:c.B].to(lab.device)
    for nm in ("loss", "pred", "emb", "w", "b"):
        if r[nm] is not None:
            assert bool(torch.isfinite(r[nm]).all()), (tag, nm)
    if r["emb"] is not None:
        assert r["emb"].shape == (c.B + c.n_pad, c.H)
        if c.n_pad:
            assert float(r["emb"][c.B:].abs().max()) == 0.0, (tag, "padding rows")
        if bool((~lab).any()):
            assert float(r["emb"][:c.B][~lab].abs().max()) == 0.0, (tag, "unlabelled rows")
    if bool((~lab).any()):
        assert float(r["pred"][~lab].abs().max()) == 0.0 and not bool(torch.signbit(r["pred"][~lab]).any()), (tag, "pred of unlabelled rows")
    absent = torch.tensor([not bool((task[lab] == t).any()) for t in range(c.T)], device=lab.device)
    if bool(absent.any()):
        assert float(r["w"].reshape(c.T, c.H)[absent].abs().max()) == 0.0, (tag, "absent tasks: grad W")
        if c.bias:
            assert float(r["b"][absent].abs().max()) == 0.0, (tag, "absent tasks: grad b")
    if not bool(lab.any()):
        assert float(r["loss"]) == 0.0 and float(r["w"].abs().max()) == 0.0, (tag, "no labelled row")
    if c.p > 0.0:
        assert r["rng"].tolist() == [TC.SEED, 1], (tag, "one draw per forward")


def _run_case(c, kind, monkeypatch):
    run, i = _runner(c, kind, monkeypatch)
    runs = {"fused": run(False, None), "split": run(True, None), "split*scale": run(True, TC.SCALE), "fused*scale": run(False, TC.SCALE)}
    B = c.B
    checked = 0
    for how, r in runs.items():
        tag = f"task_head:{c.name}:{kind}:{how}"
        _check_zero_rules(r, c, i, tag)
        f32, f64 = TC.reference(c.name, kind, TC.SCALE if how.endswith("scale") else 1.0)
        last = slice(TC.HEAD_ROWS * ((B - 1) // TC.HEAD_ROWS), B)
        legs = [{"pred": r["pred"], "loss": r["loss"], "emb": r["emb"], "w": r["w"], "b": r["b"]}, dict(f32), dict(f64)]
        for d in legs:
            d["emb"] = d["emb"][:B]
            d["emb[last block]"], d["emb[first block]"] = d["emb"][last], d["emb"][:TC.HEAD_ROWS]
            d["pred[last block]"], d["pred[first block]"] = d["pred"][last], d["pred"][:TC.HEAD_ROWS]
        n = F64.check(*legs, tag)
        assert n >= 8 - (0 if c.bias else 1)
        checked += n
    print(f"F64.check {c.name} {kind}: {checked} tensors")
    # the fused form against the split one where they must agree to the bit: gradients seeded by the registered unit gradient
    a, s = runs["fused"], runs["split"]
    assert abs(float(a["loss"]) - float(s["loss"])) <= 1e-6 * abs(float(s["loss"])), (c.name, kind)   # (two fixed orders of the partials)
    assert torch.equal(a["pred"], s["pred"])
    for nm in ("emb", "w", "b"):
        if a[nm] is not None:
            assert torch.equal(a[nm], s[nm]), (c.name, kind, nm, "fused and split differ")
    # two identical calls: the same bits
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
    # the row_ids indirection (a permuted table, repeated ids) against the same tasks passed directly
    if c.row_ids:
        for split in (False, True):
            via, direct = runs["split" if split else "fused"], run(split, None, direct=True)
            for nm in ("loss", "pred", "emb", "w", "b"):
                if via[nm] is not None:
                    assert torch.equal(via[nm], direct[nm]), (c.name, kind, split, nm, "row_ids and task differ")
    return runs


@pytest.mark.parametrize("kind", TC.KINDS)
@pytest.mark.parametrize("name", [c.name for c in TC.CASES_LIST])
def test_task_head_edges(name, kind, monkeypatch):
    _run_case(TC.CASES[name], kind, monkeypatch)


@pytest.mark.parametrize("p", [0.0, 0.25])
@pytest.mark.parametrize("kind", TC.KINDS)
@pytest.mark.parametrize("B,H", [(17, 33), (577, 32)])
def test_one_task_gives_the_single_task_heads_pred_bit_for_bit(B, H, kind, p, monkeypatch):
    """T = 1, every row labelled: ``pred`` is the single-task head's (``readout.head_loss``) to the bit, the rest within the bound."""
    from molkgnn_amd import readout as R
    from molkgnn_amd.train import backward
    dev = _dev()
    g = torch.Generator().manual_seed(B * 100 + H)
    emb0, y = (torch.randn(B, H, generator=g) * 2).to(dev), (torch.rand(B, generator=g) < 0.3).float().to(dev)
    ffn = torch.nn.Linear(H, 1).to(dev)
    task = torch.zeros(B, dtype=torch.int32, device=dev)
    out = {}
    for split in (False, True):
        monkeypatch.setattr(R, "_SPLIT_HEAD", split)
        for how in ("single", "task"):
            R.reset_head_rng(dev, seed=TC.SEED)
            emb = emb0.clone().requires_grad_(True)
            ffn.zero_grad(set_to_none=True)
            loss = R.head_loss(emb, ffn, y, kind, dropout_p=p) if how == "single" else R.task_head_loss(emb, ffn, y, task, kind, dropout_p=p)
            pred = loss.grad_fn.saved_tensors[3].clone()
            backward(loss)
            out[how] = {"pred": pred, "loss": loss.detach().clone(), "emb": emb.grad.clone(), "w": ffn.weight.grad.clone().reshape(-1),
                        "b": ffn.bias.grad.clone()}
        assert torch.equal(out["task"]["pred"], out["single"]["pred"]), (split, "pred differs from the single-task head's")
        keep = None if p == 0.0 else torch.from_numpy(_philox.head_mask(TC.SEED, 0, B, H, p))
        f32, f64 = RF.both(lambda e, w, b, yy, k: RF.head(e, w, b, yy, kind, k), emb0.cpu(), ffn.weight.detach().cpu().reshape(-1),
                           ffn.bias.detach().cpu(), y.cpu(), keep)
        assert F64.check(out["task"], f32, f64, f"task_head:T1:B{B}xH{H}:{kind}:p{p}:split{split}") == 5


def test_bce_at_saturated_logits(monkeypatch):
    """Logits of exactly +90, -90 and 0 on task-1 rows for both targets: finite everywhere, and d loss / d emb of those rows is
    (sigmoid - y) W[1] / n_lab within the bound; where the sigmoid saturates onto the target the gradient is exactly zero."""
    c = TC.SATURATED
    runs = _run_case(c, "bce", monkeypatch)
    i = TC.inputs(c.name, "bce")
    n_lab = int(i["lab"].sum())
    assert n_lab == c.B
    w64 = i["w"][TC.SATURATED_TASK].double()
    sig = {90.0: 1.0, -90.0: 0.0, 0.0: 0.5}
    want = torch.stack([(sig[x] - t) * w64 / n_lab for x, t in zip(TC.SATURATED_LOGITS, TC.SATURATED_TARGETS)])
    _, f64 = TC.reference(c.name, "bce", 1.0)
    assert float((f64["emb"][:6] - want).abs().max()) <= 1e-15 * float(want.abs().max())      # (the reference itself)
    for how in ("fused", "split"):
        r = runs[how]
        assert r["pred"][:6].tolist() == list(TC.SATURATED_LOGITS), how
        got = {f"emb[row {k}]": r["emb"][k] for k in range(6)}
        F64.check(got, {k: want[n].float() for n, k in enumerate(got)}, {k: want[n] for n, k in enumerate(got)}, f"task_head:{c.name}:bce:{how}:rows")
        assert float(r["emb"][1].abs().max()) == 0.0 and float(r["emb"][2].abs().max()) == 0.0, how


@pytest.mark.parametrize("T,H", [(33, 8), (3, 65)])
def test_beyond_the_kernels_limits_takes_the_torch_route(T, H, monkeypatch):
    """More than 32 tasks or an embedding wider than 64: ``task_head_reference`` on the GPU, no call into the library."""
    from molkgnn_amd import _lib, readout as R
    dev = _dev()
    g = torch.Generator().manual_seed(T * 100 + H)
    B = 40
    emb = (torch.randn(B, H, generator=g)).to(dev).requires_grad_(True)
    ffn = torch.nn.Linear(H, T).to(dev)
    y = (torch.rand(B, generator=g) < 0.3).float().to(dev)
    task = TC.task_pattern("quarter_unlabelled", B, T).to(dev)
    calls = []
    real = _lib.check
    monkeypatch.setattr(_lib, "check", lambda rc, what: (calls.append(what), real(rc, what))[1])
    loss = R.task_head_loss(emb, ffn, y, task, "bce")
    loss.backward()
    torch.cuda.synchronize()
    assert calls == [], calls
    want, _ = R.task_head_reference(emb.detach().cpu().double(), ffn.weight.detach().cpu().double(), ffn.bias.detach().cpu().double(),
                                    y.cpu().double(), task.cpu(), "bce")
    assert abs(float(loss.detach()) - float(want)) <= 1e-5 * abs(float(want))
    assert bool(torch.isfinite(emb.grad).all()) and float(emb.grad[task < 0].abs().max()) == 0.0


def test_c_entry_refuses_33_tasks():
    from molkgnn_amd import _lib
    lib = _lib.load()
    dev = _dev()
    T, H, B = 33, 8, 16
    f = lambda *s: torch.zeros(*s, device=dev)
    emb, w, b, y, pred, loss = f(B, H), f(T, H), f(T), f(B), f(B), f(1)
    task = torch.zeros(B, dtype=torch.int32, device=dev)
    ws = torch.zeros(1 << 20, dtype=torch.uint8, device=dev)
    rc = lib.mkgnn_task_head_forward(0, emb.data_ptr(), H, B, H, T, w.data_ptr(), b.data_ptr(), y.data_ptr(), task.data_ptr(), None, B,
                                     0.0, None, None, pred.data_ptr(), loss.data_ptr(), ws.data_ptr(), ws.numel(), None)
    assert rc != 0 and b"tasks" in lib.mkgnn_last_error()
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ the model --
def _three_task_batch():
    from molkgnn_amd.sampling import task_index
    from molkgnn_amd.synthetic import NINE_ASSAYS, make_batch
    batch = make_batch(40, seed=7, assay="all9")
    three = [int(NINE_ASSAYS[k]) for k in (1, 4, 6)]        # 1798, 2258, 488997: the three largest assays of the panel
    batch.task = task_index(batch.assay_id, three)
    counts = [int((batch.task == t).sum()) for t in range(3)]
    assert sum(n > 0 for n in counts) >= 2 and int((batch.task < 0).sum()) > 0, counts
    return batch, counts


def _spy(monkeypatch):
    from molkgnn_amd import _lib
    calls = []
    real = _lib.check
    monkeypatch.setattr(_lib, "check", lambda rc, what: (calls.append(what), real(rc, what))[1])
    return calls


def test_model_loss_takes_the_task_head(monkeypatch):
    from molkgnn_amd import readout as R
    from molkgnn_amd.train import GNNModel, backward
    dev = _dev()
    batch, counts = _three_task_batch()
    bd = batch.to(dev)
    torch.manual_seed(0)
    model = GNNModel(num_layers=2, task_dim=3, dropout_ratio=0.0, ffn_dropout_rate=0.0).to(dev).train()
    want = R.task_head_loss(model.gnn_model(bd), model.ffn, bd.y, bd.task, "bce").detach().clone()
    calls = _spy(monkeypatch)
    model.zero_grad(set_to_none=True)
    loss = model.loss(bd)
    assert "mkgnn_task_head_fused" in calls and not [c for c in calls if "tail" in c or "molecule" in c], calls
    emb = loss.grad_fn.saved_tensors[0].detach().clone()
    backward(loss)
    torch.cuda.synchronize()
    assert torch.equal(loss.detach(), want), (float(loss), float(want))
    # the PyTorch formulation of the same loss: which parameters get a gradient at all
    ref = copy.deepcopy(model)
    ref.zero_grad(set_to_none=True)
    lab = bd.task >= 0
    out = ref.ffn(ref.gnn_model(bd)).gather(1, bd.task.clamp(min=0).long()[:, None]).view(-1)
    torch.nn.BCEWithLogitsLoss()(out[lab], bd.y.view(-1).float()[lab]).backward()
    for (n, p), (_, q) in zip(model.named_parameters(), ref.named_parameters()):
        if q.grad is not None:
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()), n
    # the head's own gradients and the loss against the definition on the detached fp32 embedding
    legs = []
    for dt in (torch.float32, torch.float64):
        w = model.ffn.weight.detach().cpu().to(dt).requires_grad_(True)
        b = model.ffn.bias.detach().cpu().to(dt).requires_grad_(True)
        l, _ = R.task_head_reference(emb.cpu().to(dt), w, b, batch.y.to(dt), batch.task, "bce")
        l.backward()
        legs.append({"loss": l.detach(), "ffn.weight": w.grad, "ffn.bias": b.grad})
    got = {"loss": loss.detach(), "ffn.weight": model.ffn.weight.grad, "ffn.bias": model.ffn.bias.grad}
    n = F64.check(got, *legs, "task_head:model")
    print(f"F64.check model: {n} tensors")
    assert n == 3
    for t in range(3):
        if counts[t] == 0:
            assert float(model.ffn.weight.grad[t].abs().max()) == 0.0 and float(model.ffn.bias.grad[t]) == 0.0


def test_a_batch_without_tasks_is_the_single_task_route(monkeypatch):
    from molkgnn_amd.train import GNNModel
    dev = _dev()
    batch, _ = _three_task_batch()
    del batch.task
    bd = batch.to(dev)
    torch.manual_seed(0)
    model = GNNModel(num_layers=2, task_dim=1, dropout_ratio=0.0, ffn_dropout_rate=0.0).to(dev).train()
    calls = _spy(monkeypatch)
    loss = model.loss(bd)
    torch.cuda.synchronize()
    assert not [c for c in calls if "task_head" in c], calls
    assert [c for c in calls if c in ("mkgnn_molecule_step", "mkgnn_tail_fused", "mkgnn_bce_head_fused")], calls
    with torch.no_grad():
        # the same loss through PyTorch's head on the separate operators (training mode, no dropout anywhere).  1e-4: two float32
        # evaluations of a two-layer network in different summation orders differ by a few units of 1e-7 x its depth
        pred, _ = model(bd)
        want = torch.nn.BCEWithLogitsLoss()(pred.view(-1), bd.y.view(-1).float())
    assert abs(float(loss.detach()) - float(want)) <= 1e-4 * abs(float(want))


def test_evaluate_tasks_scores_every_task(monkeypatch):
    from molkgnn_amd import evaluation as E
    from molkgnn_amd.train import GNNModel, evaluate_tasks
    dev = _dev()
    batch, counts = _three_task_batch()
    bd = batch.to(dev)
    torch.manual_seed(0)
    model = GNNModel(num_layers=2, task_dim=3, dropout_ratio=0.0, ffn_dropout_rate=0.0).to(dev).train()
    res = evaluate_tasks(model, [bd, bd], metrics=("AUC",))
    assert model.training
    pred, _ = model.eval().predict(bd)
    assert pred.shape == (40, 3)
    task = bd.task.long()
    for t in range(3):
        rows = task == t
        want = E.calculate_auc(bd.y.view(-1)[rows].repeat(2), pred[rows, t].repeat(2)) if counts[t] else float("nan")
        assert res["AUC"][t] == want or (want != want and res["AUC"][t] != res["AUC"][t]), t
    assert res["pred_y"].shape == (80,) and bool(torch.isnan(res["pred_y"][:40][task < 0]).all())
    assert torch.equal(res["task"][:40], task) and bool(torch.isfinite(res["loss"]))


# ------------------------------------------------------------------------------ the resident captured step --
def test_one_captured_graph_serves_mixed_assay_batches(tmp_path):
    """gather -> expand -> receptive fields -> model.loss -> backward captured ONCE on a resident all9 shard with a task table, and
    replayed on two id rows (one with a repeated id): each replay's loss and ffn.weight.grad equal, bit for bit, an eager run on
    the same ids with ``data.task = task_table[ids]`` set directly."""
    from molkgnn_amd import padding as P, shards as S
    from molkgnn_amd.receptive_field import attach_receptive_fields
    from molkgnn_amd.synthetic import NINE_ASSAYS, make_batch
    from molkgnn_amd.train import GNNModel, backward
    dev = _dev()
    whole = make_batch(64, seed=12, assay="all9", with_receptive_fields=False)
    path = str(tmp_path / "all9.mkgs")
    S.write_shard(path, whole)
    nine = [int(a) for a in NINE_ASSAYS]
    res = S.ResidentShard(S.Shard(path), dev, assays=nine)
    assert res.tensors["task"].dtype == torch.int32 and torch.equal(res.tensors["task"].cpu(), res.task) and int(res.task.min()) >= 0
    rows = np.random.default_rng(3).integers(0, 64, size=(3, 16))
    rows[2, 5] = rows[2, 11]                                  # (a repeated id)
    loader = S.ResidentLoader(res, 16, rows.reshape(-1), dev)
    batches = list(loader)
    torch.manual_seed(1)
    model = GNNModel(num_layers=2, task_dim=9, dropout_ratio=0.0, ffn_dropout_rate=0.0).to(dev).train()
    csb = P.CompactStaticBatch(loader.shape, 16, res.x_dim, res.p_dim, res.e_dim, dev, max_mol_atoms=loader.max_mol_atoms,
                               max_mol_edges=loader.max_mol_edges)

    def step():
        csb.gather(res)
        csb.expand()
        attach_receptive_fields(csb.data, sizes=csb.data.bucket_sizes, overlap=True)
        model.zero_grad(set_to_none=True)
        loss = model.loss(csb.data)
        backward(loss)
        return loss

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        csb.gather(res, batches[0])
        assert csb.data.task_table is res.tensors["task"] and csb.data.task_rows is csb.ids
        for _ in range(2):
            step()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            static_loss = step()
        got = []
        for k in (1, 2):
            csb.ids.copy_(batches[k])
            g.replay()
            got.append((static_loss.detach().clone(), model.ffn.weight.grad.detach().clone()))
        want = []
        for k in (1, 2):
            csb.ids.copy_(batches[k])
            csb.data.task = res.tensors["task"][csb.ids.long()]
            loss = step()
            want.append((loss.detach().clone(), model.ffn.weight.grad.detach().clone()))
            del csb.data.task
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for k in range(2):
        assert torch.equal(got[k][0], want[k][0]), (k, float(got[k][0]), float(want[k][0]))
        assert torch.equal(got[k][1], want[k][1]), k
    assert float(got[0][0]) != float(got[1][0]) and float(got[0][0]) > 0.0
    assert csb.gather_status() == 0
