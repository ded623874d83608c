"""The task-indexed head with masked labels, everything that needs no GPU: the C ABI's declarations and exports, the torch
definition ``readout.task_head_reference`` against PyTorch's own losses and against its contract's zero rules, the sampler's
task index and per-task oversampling weights, per-task evaluation and the resident shard's task table."""
import os
import re

import pytest
import torch

from tests import _readout_f64 as RF
from tests import _task_head_cases as TC

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("mkgnn_task_head_workspace_bytes", "mkgnn_task_head_forward", "mkgnn_task_head_backward", "mkgnn_task_head_fused")


def test_header_declares_the_entry_points_and_abi_stays_8():
    text = open(os.path.join(REPO, "include", "molkgnn_hip.h")).read()
    for name in ENTRIES:
        assert re.search(r"\b(size_t|int) " + name + r"\(", text), name
    assert re.search(r"#define MKGNN_TASK_HEAD_MAX_TASKS 32\b", text)
    assert re.search(r"#define MKGNN_ABI_VERSION 8\b", text)


def test_library_exports_the_entry_points():
    import ctypes
    from molkgnn_amd import _lib
    assert _lib.ABI_VERSION == 8 and _lib.TASK_HEAD_MAX_TASKS == TC.MAX_TASKS and _lib.TASK_HEAD_MAX_H == TC.MAX_H
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRIES:
        assert name in _lib.EXPORTS, name
        assert hasattr(raw, name), name
    lib = _lib.load()
    assert lib.mkgnn_abi_version() == 8
    # the workspace: 16 bytes + per 16-row block a [T][H + 1] partial and {loss, labelled rows}; 0 outside the limits
    assert lib.mkgnn_task_head_workspace_bytes(17, 5, 3) == 16 + 2 * (3 * 6 + 2) * 4
    for n, H, T in ((0, 5, 3), (17, 0, 3), (17, 65, 3), (17, 5, 0), (17, 5, 33)):
        assert lib.mkgnn_task_head_workspace_bytes(n, H, T) == 0, (n, H, T)


def test_entry_points_refuse_what_is_outside_their_limits():
    """No GPU is touched: every argument check comes before a launch.  T = 33, H = 65, an unknown loss kind, a short task vector."""
    import numpy as np
    from molkgnn_amd import _lib
    lib = _lib.load()
    buf = np.zeros(1 << 16, dtype=np.uint8)
    p = buf.ctypes.data
    ok = dict(kind=0, H=4, T=3, n_task=8)
    for change in (dict(T=33), dict(T=0), dict(H=65), dict(H=0), dict(n_task=7)):
        a = dict(ok, **change)
        rc = lib.mkgnn_task_head_forward(a["kind"], p, 4 if a["H"] <= 4 else a["H"], 8, a["H"], a["T"], p, p, p, p, None, a["n_task"],
                                         0.0, None, None, p, p, p, buf.nbytes, None)
        assert rc != 0, change
        rc = lib.mkgnn_task_head_fused(a["kind"], p, 4 if a["H"] <= 4 else a["H"], 8, a["H"], a["T"], p, p, p, p, None, a["n_task"],
                                       0.0, None, None, p, p, p, 4, p, p, p, buf.nbytes, None)
        assert rc != 0, change
        rc = lib.mkgnn_task_head_backward(a["kind"], p, 4 if a["H"] <= 4 else a["H"], 8, a["H"], a["T"], p, p, p, None, a["n_task"],
                                          p, p, 0.0, None, p, 4, p, p, p, buf.nbytes, None)
        assert rc != 0, change
        assert lib.mkgnn_last_error()


def _torch_formulation(emb, w, b, y, task, kind, keep, T):
    """``loss_func(ffn(e).gather(1, task)[lab], y[lab])`` with PyTorch's own modules."""
    lab = (task >= 0) & (task < T)
    e = emb if keep is None else emb * keep
    out = torch.nn.functional.linear(e, w, b)
    sel = out.gather(1, torch.where(lab, task, torch.zeros_like(task)).long()[:, None]).view(-1)[lab]
    fn = {"bce": torch.nn.BCEWithLogitsLoss(), "mse": torch.nn.MSELoss(), "mse_sum": torch.nn.MSELoss(reduction="sum")}[kind]
    return fn(sel, y[lab])


@pytest.mark.parametrize("kind", TC.KINDS)
@pytest.mark.parametrize("name", ["B15xH5xT2_round_robin", "B33xH33xT9_one_absent", "B577xH64xT9_quarter_unlabelled",
                                  "B33xH31xT9_out_of_range", "B17xH32xT32_round_robin"])
def test_reference_is_pytorchs_loss_of_the_selected_outputs(name, kind):
    """float64, to 1e-12: the loss and the autograd gradients of emb, W and b."""
    from molkgnn_amd.readout import task_head_reference
    c, i = TC.CASES[name], TC.inputs(name, kind)
    d = lambda t: None if t is None else t.double()
    legs = []
    for how in ("reference", "torch"):
        emb, w = d(i["emb"][:c.B]).requires_grad_(True), d(i["w"]).requires_grad_(True)
        b = None if i["b"] is None else d(i["b"]).requires_grad_(True)
        if how == "reference":
            loss, _ = task_head_reference(emb, w, b, d(i["y"]), i["task"], kind, d(i["keep"]), c.B)
        else:
            loss = _torch_formulation(emb, w, b, d(i["y"][:c.B]), i["task"][:c.B].long(), kind, d(i["keep"]), c.T)
        loss.backward()
        legs.append([loss.detach(), emb.grad, w.grad] + ([] if b is None else [b.grad]))
    for got, want in zip(*legs):
        assert float((got - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max())), name


@pytest.mark.parametrize("kind", TC.KINDS)
@pytest.mark.parametrize("name", [c.name for c in TC.CASES_LIST if c.B <= 577])
def test_reference_keeps_the_zero_rules(name, kind):
    """Unlabelled rows and rows >= n_rows of grad_emb, rows of grad_W / grad_b of tasks without a labelled row: exactly zero; pred
    of an unlabelled row +0.0; nothing NaN although y is NaN wherever it must not be used; no labelled row: all zero."""
    c, i = TC.CASES[name], TC.inputs(name, kind)
    for leg in TC.reference(name, kind):
        lab = i["lab"]
        for nm, v in leg.items():
            assert bool(torch.isfinite(v).all()), (name, nm)
        assert leg["emb"].shape == (c.B + c.n_pad, c.H)
        assert float(leg["emb"][c.B:].abs().sum()) == 0.0 and float(leg["emb"][:c.B][~lab].abs().sum()) == 0.0
        assert float(leg["pred"][~lab].abs().sum()) == 0.0 and not bool(torch.signbit(leg["pred"][~lab]).any())
        absent = torch.tensor([not bool((i["task"][:c.B][lab] == t).any()) for t in range(c.T)])
        assert float(leg["w"].reshape(c.T, c.H)[absent].abs().sum()) == 0.0
        if c.bias:
            assert float(leg["b"][absent].abs().sum()) == 0.0
        if not bool(lab.any()):
            assert float(leg["loss"]) == 0.0 and float(leg["w"].abs().sum()) == 0.0
    if c.pattern == "one_absent":
        assert bool(absent.any())


@pytest.mark.parametrize("kind", RF.HEAD_KINDS)
@pytest.mark.parametrize("name", ["B15xH31", "B17xH33", "B528xH64"])
def test_one_task_with_every_row_labelled_is_the_single_task_head(name, kind):
    from molkgnn_amd.readout import task_head_reference
    c, i = RF.HEAD_CASES[name], RF.head_inputs(name, kind)
    _, want = RF.head_reference(name, kind, 1.0)
    d = lambda t: None if t is None else t.double()
    emb, w = d(i["emb"]).requires_grad_(True), d(i["w"])[None, :].requires_grad_(True)
    b = None if i["b"] is None else d(i["b"]).requires_grad_(True)
    loss, pred = task_head_reference(emb, w, b, d(i["y"]), torch.zeros(c.B, dtype=torch.int32), kind, d(i["keep"]), c.B)
    loss.backward()
    got = {"pred": pred.detach(), "loss": loss.detach(), "emb": emb.grad[:c.B], "w": w.grad.reshape(-1)}
    if b is not None:
        got["b"] = b.grad
    for nm, v in got.items():
        assert float((v - want[nm]).abs().max()) <= 1e-12 * max(1.0, float(want[nm].abs().max())), (name, kind, nm)


def test_reference_reads_the_task_through_a_table():
    from molkgnn_amd.readout import task_head_reference
    i = TC.inputs("B33xH32xT9_round_robin", "bce")
    a = task_head_reference(i["emb"], i["w"], i["b"], i["y"], i["task"], "bce", i["keep"], 33)
    b = task_head_reference(i["emb"], i["w"], i["b"], i["y"], None, "bce", i["keep"], 33, task_table=i["task_table"], row_ids=i["row_ids"])
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert len(set(i["row_ids"][:33].tolist())) < 33           # (ids repeat)


def test_task_index():
    from molkgnn_amd.sampling import task_index
    from molkgnn_amd.synthetic import NINE_ASSAYS
    ids = torch.tensor([1798, 435008, 7, 2258, 1798, 485290])
    t = task_index(ids, (2258, 1798, 485290))
    assert t.dtype == torch.int32 and t.tolist() == [1, -1, -1, 0, 1, 2]
    assert task_index(ids, [int(a) for a in NINE_ASSAYS]).tolist() == [1, 0, -1, 4, 1, 8]
    assert task_index(ids.to(torch.int32), ["1798"]).tolist() == [0, -1, -1, -1, 0, -1]
    with pytest.raises(ValueError):
        task_index(ids, ())


def test_task_oversampling_weights():
    from molkgnn_amd.sampling import oversampling_weights, task_oversampling_weights
    #                        task 0: 1 active, 3 inactive | task 1: 2 active, 1 inactive | task 2: inactive only | unlabelled
    tasks = torch.tensor([0, 0, 0, 0, 1, 1, 1, 2, 2, -1, -1])
    labels = torch.tensor([1, 0, 0, 0, 1, 1, 0, 0, 0, 1, 0])
    w = task_oversampling_weights(labels, tasks)
    want = torch.tensor([1., 1 / 3, 1 / 3, 1 / 3, .5, .5, 1., .5, .5, 0., 0.])
    assert w.dtype == torch.float32 and torch.equal(w, want)
    y = (torch.arange(1000) % 13 == 0).long()
    assert torch.equal(task_oversampling_weights(y, torch.zeros(1000, dtype=torch.int32)), oversampling_weights(y))
    with pytest.raises(ValueError):
        task_oversampling_weights(labels, tasks[:-1])


def test_per_task_is_a_loop_over_the_tasks():
    from molkgnn_amd import evaluation as E
    g = torch.Generator().manual_seed(5)
    n = 600
    task = torch.randint(-1, 4, (n,), generator=g)            # task 4 of 5 has no row
    y = (torch.rand(n, generator=g) < 0.3).long()
    s = torch.randn(n, generator=g) + y
    for fn in (E.calculate_auc, E.calculate_logAUC):
        got = E.per_task(y, s, task, fn, 5)
        assert len(got) == 5 and got[4] != got[4]               # (nan)
        for t in range(4):
            assert got[t] == fn(y[task == t], s[task == t]), (fn.__name__, t)
    with pytest.raises(ValueError):
        E.per_task(y, s, task[:-1], E.calculate_auc, 5)


def test_resident_shard_keeps_the_task_of_every_molecule(tmp_path):
    from molkgnn_amd import shards as S
    from molkgnn_amd.sampling import task_index
    from molkgnn_amd.synthetic import NINE_ASSAYS, make_batch
    whole = make_batch(64, seed=12, assay="all9", with_receptive_fields=False)
    path = str(tmp_path / "all9.mkgs")
    S.write_shard(path, whole)
    shard = S.Shard(path)
    three = [int(NINE_ASSAYS[k]) for k in (1, 0, 5)]
    res = S.ResidentShard(shard, device="cpu", assays=three)
    want = task_index(torch.from_numpy(shard.assay_id.copy()), three)
    assert res.task.dtype == torch.int32 and torch.equal(res.task, want) and res.assays == tuple(three)
    assert torch.equal(want, task_index(whole.assay_id, three))
    assert len(set(want.tolist())) >= 3 and "task" not in res.tensors       # (nothing is uploaded on the CPU)
    assert S.ResidentShard(shard, device="cpu").task is None
