"""The docking-score regression task without a GPU: RMSE, the ABI v8 surface (loss kinds, head entry points), the synthetic
docking score and the loss selection of ``GNNModel`` (reference data.py:49-53, model.py:156, 504-507)."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header() -> str:
    with open(os.path.join(REPO, "include", "molkgnn_hip.h")) as f:
        return f.read()


def _define(name: str) -> int:
    m = re.search(rf"#define\s+{name}\s+(\d+)", _header())
    assert m, name
    return int(m.group(1))


def _sklearn_rmse(y, s):
    try:
        from sklearn.metrics import mean_squared_error
    except ImportError:                      # (numpy in float64: what mean_squared_error computes)
        return math.sqrt(float(np.mean((np.asarray(y, np.float64) - np.asarray(s, np.float64)) ** 2)))
    return math.sqrt(mean_squared_error(np.asarray(y, np.float64), np.asarray(s, np.float64)))


@pytest.mark.parametrize("n", [1, 7, 1000])
def test_calculate_rmse_matches_sklearn_on_random_inputs(n):
    from molkgnn_amd.evaluation import calculate_rmse
    rng = np.random.default_rng(n)
    y = rng.normal(-8.0, 1.5, n).astype(np.float32)
    s = (y + rng.normal(0.0, 0.7, n)).astype(np.float32)
    want = _sklearn_rmse(y, s)
    assert want == pytest.approx(math.sqrt(float(np.mean((y.astype(np.float64) - s.astype(np.float64)) ** 2))), rel=1e-15)
    for got in (calculate_rmse(torch.from_numpy(y), torch.from_numpy(s)), calculate_rmse(y, s),
                calculate_rmse(torch.from_numpy(y).view(-1, 1), torch.from_numpy(s).view(-1, 1))):
        assert isinstance(got, float)
        assert got == pytest.approx(want, rel=1e-12, abs=1e-15)


def test_calculate_rmse_on_constant_inputs():
    from molkgnn_amd.evaluation import calculate_rmse
    y = torch.full((50,), -7.25)
    assert calculate_rmse(y, y.clone()) == 0.0
    assert calculate_rmse(y, torch.full((50,), -8.0)) == pytest.approx(0.75, rel=1e-15)
    assert calculate_rmse(y, torch.full((50,), -8.0)) == pytest.approx(_sklearn_rmse(y.numpy(), np.full(50, -8.0)), rel=1e-15)
    with pytest.raises(ValueError):
        calculate_rmse(torch.zeros(3), torch.zeros(4))


def test_library_is_abi_8_and_exports_the_loss_kind_head():
    from molkgnn_amd import _lib
    assert _lib.ABI_VERSION == 8 and _define("MKGNN_ABI_VERSION") == 8
    lib = ctypes.CDLL(_lib.LIB_PATH)
    lib.mkgnn_abi_version.restype = ctypes.c_int
    assert lib.mkgnn_abi_version() == 8
    for name in ("mkgnn_head_loss_forward", "mkgnn_head_loss_backward", "mkgnn_head_loss_dropout_forward",
                 "mkgnn_head_loss_dropout_backward", "mkgnn_head_loss_fused"):
        assert hasattr(lib, name), name
        assert name in _lib.EXPORTS, name
        assert re.search(rf"\bint {name}\(int32_t loss_kind,", _header()), name
    # the fused tail's argument block ends with the loss kind (appended in v8, after v7's defer_reduce)
    assert _lib.TailArgs._fields_[-1] == ("loss_kind", ctypes.c_int32)
    assert _lib.TailArgs._fields_[-2][0] == "defer_reduce"
    tail = _header().split("typedef struct mkgnn_tail_args {")[1].split("} mkgnn_tail_args;")[0]
    fields = re.findall(r"\b(\w+);", re.sub(r"/\*.*?\*/", "", tail, flags=re.S))
    assert fields[-2:] == ["defer_reduce", "loss_kind"]


def test_loss_kind_constants_equal_the_header():
    from molkgnn_amd import _lib
    from molkgnn_amd import readout as R
    assert _lib.LOSS_BCE_MEAN == _define("MKGNN_LOSS_BCE_MEAN") == 0
    assert _lib.LOSS_SQERR_MEAN == _define("MKGNN_LOSS_SQERR_MEAN")
    assert _lib.LOSS_SQERR_SUM == _define("MKGNN_LOSS_SQERR_SUM")
    assert _lib.MOLECULE_SQERR == _define("MKGNN_MOLECULE_SQERR")
    assert _lib.MOLECULE_SUM == _define("MKGNN_MOLECULE_SUM")
    assert _lib.MOLECULE_HEAD == _define("MKGNN_MOLECULE_HEAD")
    assert R.LOSS_KINDS == {"bce": _lib.LOSS_BCE_MEAN, "mse": _lib.LOSS_SQERR_MEAN, "mse_sum": _lib.LOSS_SQERR_SUM}
    with pytest.raises(ValueError):
        R.loss_kind("l1")


def test_head_entry_points_reject_an_unknown_loss_kind():
    """The kind is checked on the host before anything is launched: no device needed (the pointers are never read)."""
    from molkgnn_amd import _lib
    lib = _lib.load()
    buf = np.zeros(4096, dtype=np.float32)
    p = buf.ctypes.data
    ws_bytes = int(lib.mkgnn_bce_head_workspace_bytes(8, 4))
    assert ws_bytes <= buf.nbytes
    for kind in (3, -1):
        rc = lib.mkgnn_head_loss_forward(kind, p, 4, 8, 4, p, p, p, p, p, p, buf.nbytes, None)
        assert rc != 0
        assert b"unknown loss kind" in lib.mkgnn_last_error()
        rc = lib.mkgnn_head_loss_fused(kind, p, 4, 8, 4, p, p, p, 0.0, None, None, p, p, p, 4, p, p, p, buf.nbytes, None)
        assert rc != 0 and b"unknown loss kind" in lib.mkgnn_last_error()
        rc = lib.mkgnn_head_loss_backward(kind, p, 4, 8, 4, p, p, p, p, p, 4, p, p, p, buf.nbytes, None)
        assert rc != 0 and b"unknown loss kind" in lib.mkgnn_last_error()


def test_synthetic_docking_score_is_seeded_and_molecule_dependent():
    from molkgnn_amd.synthetic import make_batch
    a = make_batch(512, seed=11, target="docking_score", with_receptive_fields=False)
    b = make_batch(512, seed=11, target="docking_score", with_receptive_fields=False)
    c = make_batch(512, seed=12, target="docking_score", with_receptive_fields=False)
    act = make_batch(512, seed=11, with_receptive_fields=False)
    assert a.y.dtype == torch.float32 and a.y.shape == (512,)
    assert torch.equal(a.y, b.y) and not torch.equal(a.y, c.y)
    # the molecules themselves are those of the activity batch of the same seed
    assert torch.equal(a.x, act.x) and torch.equal(a.edge_index, act.edge_index) and torch.equal(a.batch, act.batch)
    assert -9.0 < float(a.y.mean()) < -7.0 and 0.7 < float(a.y.std()) < 2.0
    assert a.y.unique().numel() == 512                    # continuous
    sizes = torch.bincount(a.batch, minlength=512).double()
    corr = torch.corrcoef(torch.stack([sizes, a.y.double()]))[0, 1]
    assert float(corr) < -0.4                             # larger molecules dock lower: something a model can learn
    with pytest.raises(ValueError):
        make_batch(4, seed=1, target="logP")


def test_default_target_is_unchanged():
    """The activity labels of a fixed seed (recorded before the ``target`` keyword existed)."""
    from molkgnn_amd.synthetic import make_batch
    b = make_batch(200, seed=5, assay="9999", with_receptive_fields=False)
    assert b.y.dtype == torch.float32
    assert torch.nonzero(b.y).view(-1).tolist() == _ACTIVE_9999_SEED5
    assert torch.equal(b.y, make_batch(200, seed=5, assay="9999", with_receptive_fields=False, target="activity").y)


_ACTIVE_9999_SEED5 = [22, 24, 41, 43, 57, 67, 88, 96, 110, 112, 122, 157, 160, 167, 169, 180, 188, 197]


def test_gnn_model_loss_selection():
    from torch.nn import BCEWithLogitsLoss, L1Loss, MSELoss
    from molkgnn_amd.train import GNNModel
    m = GNNModel()
    assert type(m.loss_func) is BCEWithLogitsLoss and m._loss_kind() == "bce"
    assert GNNModel(loss_func=MSELoss())._loss_kind() == "mse"
    assert GNNModel(loss_func=MSELoss(reduction="sum"))._loss_kind() == "mse_sum"
    for other in (MSELoss(reduction="none"), L1Loss(), BCEWithLogitsLoss(pos_weight=torch.tensor([2.0])),
                  BCEWithLogitsLoss(reduction="sum")):
        assert GNNModel(loss_func=other)._loss_kind() is None
