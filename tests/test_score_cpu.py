"""The evaluation-mode scoring path without a GPU: the additive C ABI surface of the forward-only tail (``mkgnn_tail_score``),
``GNNModel.predict``'s mode check and ``train.evaluate`` -- the reference's ``validation_step`` + ``validation_epoch_end`` +
``get_evaluations`` (model.py:221-296, 483-522) -- on a stub model."""
import ctypes
import os
import re

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL_METRICS = ("accuracy", "RMSE", "logAUC_0.001_0.1", "logAUC_0.001_1", "ppv", "f1_score", "AUC")


def _header() -> str:
    with open(os.path.join(REPO, "include", "molkgnn_hip.h")) as f:
        return f.read()


def test_score_entry_points_are_additive_to_abi_8():
    from molkgnn_amd import _lib
    h = _header()
    assert re.search(r"\bint mkgnn_tail_score\(const mkgnn_tail_args\* args, void\* workspace, size_t workspace_bytes, void\* stream\);", h)
    assert re.search(r"\bsize_t mkgnn_tail_score_workspace_bytes\(int32_t K, int32_t H, int32_t G, int64_t n_atoms, int64_t n_mols\);", h)
    m = re.search(r"#define\s+MKGNN_ABI_VERSION\s+(\d+)", h)
    assert m and int(m.group(1)) == 8 and _lib.ABI_VERSION == 8
    lib = ctypes.CDLL(_lib.LIB_PATH)
    lib.mkgnn_abi_version.restype = ctypes.c_int
    assert lib.mkgnn_abi_version() == 8
    for name in ("mkgnn_tail_score", "mkgnn_tail_score_workspace_bytes"):
        assert hasattr(lib, name), name
        assert name in _lib.EXPORTS, name
    # the argument block is the training tail's, unchanged: 312 bytes on the commit before this entry point existed
    assert ctypes.sizeof(_lib.TailArgs) == 312
    assert _lib.TailArgs._fields_[-1] == ("loss_kind", ctypes.c_int32)
    bound = _lib.load()
    assert bound.mkgnn_tail_score.argtypes == [ctypes.POINTER(_lib.TailArgs), ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    assert bound.mkgnn_tail_score_workspace_bytes.restype is ctypes.c_size_t
    # the z rows only: [n_atoms, 32] floats, rounded up to 256 bytes -- and never more than the training tail's workspace
    assert bound.mkgnn_tail_score_workspace_bytes(110, 32, 32, 1000, 40) == 1000 * 32 * 4
    assert bound.mkgnn_tail_score_workspace_bytes(110, 32, 32, 3, 1) == 512
    assert bound.mkgnn_tail_score_workspace_bytes(110, 32, 32, 1000, 40) < bound.mkgnn_tail_workspace_bytes(110, 32, 32, 1000, 40)
    assert bound.mkgnn_tail_score_workspace_bytes(110, 32, 32, 0, 40) == 0


def test_score_rejects_bad_arguments_on_the_host():
    """Checked before anything is launched: no device needed (no pointer is read)."""
    from molkgnn_amd import _lib
    lib = _lib.load()

    def last_error():
        return lib.mkgnn_last_error().decode()
    assert lib.mkgnn_tail_score(None, None, 0, None) != 0
    a = _lib.TailArgs()
    a.readout.F, a.readout.H, a.readout.G = 110, 64, 32         # H beyond the fused tail
    for i, L in enumerate((10, 20, 30, 50)):
        a.num_kernels[i] = L
    assert lib.mkgnn_tail_score(ctypes.byref(a), None, 0, None) != 0
    assert "outside the fused tail" in last_error()
    a.readout.H = 32
    a.n_atoms, a.n_mols, a.n_loss_mols = 10, 2, 3              # more predictions than molecules
    assert lib.mkgnn_tail_score(ctypes.byref(a), None, 0, None) != 0
    assert "bad sizes" in last_error()
    a.n_loss_mols = 2
    assert lib.mkgnn_tail_score(ctypes.byref(a), None, 0, None) != 0
    assert "null pointer" in last_error()


def test_predict_raises_in_training_mode():
    from molkgnn_amd.train import GNNModel
    model = GNNModel(num_layers=1)
    model.train()
    with pytest.raises(ValueError, match="evaluation mode"):
        model.predict(object())                               # (the mode is checked before the batch is looked at)
    assert model.training                                     # ... and it is not flipped behind the caller's back


class _Batch:
    def __init__(self, y):
        self.y = y


class _Stub(torch.nn.Module):
    """``predict`` hands out prepared predictions, batch by batch; records the mode it was called in."""

    def __init__(self, preds, loss_func, fail_at=None):
        super().__init__()
        self.preds, self.loss_func, self.fail_at = list(preds), loss_func, fail_at
        self.calls, self.modes = 0, []
        self.inner = torch.nn.Dropout(0.5)

    def predict(self, batch):
        self.modes.append((self.training, self.inner.training))
        i, self.calls = self.calls, self.calls + 1
        if self.fail_at == i:
            raise RuntimeError("batch %d is broken" % i)
        return self.preds[i].view(-1, 1), torch.zeros(self.preds[i].numel(), 4)


def _prepared(regression):
    g = torch.Generator().manual_seed(17)
    sizes = (5, 1, 9)
    preds = [2.0 * torch.randn(n, generator=g) for n in sizes]
    if regression:
        ys = [torch.randn(n, generator=g) - 8.0 for n in sizes]
    else:
        ys = [(torch.rand(n, generator=g) < 0.4).long() for n in sizes]
        ys[0][0], ys[0][1] = 0, 1                              # (both classes present)
    return preds, ys


@pytest.mark.parametrize("regression", [False, True])
@pytest.mark.parametrize("start_training", [False, True])
def test_evaluate_is_the_reference_epoch_end_on_the_concatenated_vectors(regression, start_training):
    from molkgnn_amd import evaluation as E
    from molkgnn_amd.train import evaluate
    preds, ys = _prepared(regression)
    loss_func = torch.nn.MSELoss(reduction="sum") if regression else torch.nn.BCEWithLogitsLoss()
    model = _Stub(preds, loss_func).train(start_training)
    got = evaluate(model, [_Batch(y.view(-1, 1)) for y in ys], metrics=ALL_METRICS)
    assert model.modes == [(False, False)] * 3                # evaluation mode inside, all the way down
    assert model.training is start_training and model.inner.training is start_training
    all_pred, all_true = torch.cat(preds), torch.cat(ys)
    assert torch.equal(got["pred_y"], all_pred) and torch.equal(got["true_y"], all_true)
    assert torch.equal(got["loss"], loss_func(all_pred, all_true.float()))
    want = {
        "accuracy": E.calculate_accuracy(all_true, all_pred),
        "RMSE": E.calculate_rmse(all_true, all_pred),
        "logAUC_0.001_0.1": E.calculate_logAUC(all_true, all_pred),
        "logAUC_0.001_1": E.calculate_logAUC(all_true, all_pred, FPR_range=(0.001, 1)),
        "ppv": E.calculate_ppv(all_true, all_pred),
        "f1_score": E.calculate_f1_score(all_true, all_pred),
        "AUC": E.calculate_auc(all_true, all_pred),
    }
    assert set(got) == set(want) | {"loss", "pred_y", "true_y"}
    for name, value in want.items():
        assert got[name] == value or (value != value and got[name] != got[name]), (name, got[name], value)
    # only what was asked for
    model = _Stub(preds, loss_func)
    assert set(evaluate(model, [_Batch(y) for y in ys])) == {"loss", "pred_y", "true_y"}


def test_evaluate_keeps_a_padded_batch_to_its_real_molecules():
    """``predict`` returns the real molecules' rows; the labels of a batch are cut to as many."""
    from molkgnn_amd.train import evaluate
    preds = [torch.tensor([0.5, -1.0]), torch.tensor([2.0])]
    ys = [torch.tensor([1, 0]), torch.tensor([1, 0, 0])]       # (the second batch carries two labels too many)
    got = evaluate(_Stub(preds, torch.nn.BCEWithLogitsLoss()), [_Batch(y) for y in ys], metrics=("accuracy",))
    assert torch.equal(got["true_y"], torch.tensor([1, 0, 1])) and got["accuracy"] == 1.0


@pytest.mark.parametrize("start_training", [False, True])
def test_evaluate_restores_the_mode_after_a_batch_that_raises(start_training):
    from molkgnn_amd.train import evaluate
    preds, ys = _prepared(False)
    model = _Stub(preds, torch.nn.BCEWithLogitsLoss(), fail_at=1).train(start_training)
    with pytest.raises(RuntimeError, match="batch 1 is broken"):
        evaluate(model, [_Batch(y) for y in ys], metrics=("AUC",))
    assert model.calls == 2 and model.modes == [(False, False)] * 2
    assert model.training is start_training and model.inner.training is start_training


def test_evaluate_rejects_an_unknown_metric_before_any_batch():
    from molkgnn_amd.train import evaluate
    preds, ys = _prepared(False)
    model = _Stub(preds, torch.nn.BCEWithLogitsLoss()).train()
    with pytest.raises(ValueError, match="unknown metric"):
        evaluate(model, [_Batch(y) for y in ys], metrics=("accuracy", "MCC"))
    assert model.calls == 0 and model.training
