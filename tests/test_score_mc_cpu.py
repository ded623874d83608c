"""Monte Carlo dropout scoring without a GPU: the additive C ABI surface (``mkgnn_tail_score_mc``, ``mkgnn_tail_mc_out``), the host
refusals of the entry point, ``readout.mc_statistics_reference`` -- the float32 definition of the kernel's statistics -- against
float64, and ``GNNModel.predict_mc``'s refusals, which come before the batch is looked at."""
import ctypes
import os
import re

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header() -> str:
    with open(os.path.join(REPO, "include", "molkgnn_hip.h")) as f:
        return f.read()


def test_mc_entry_points_are_additive_to_abi_8():
    from molkgnn_amd import _lib
    h = _header()
    assert re.search(r"\bsize_t mkgnn_tail_score_mc_workspace_bytes\(int32_t K, int32_t H, int32_t G, int64_t n_atoms, int64_t n_mols\);", h)
    assert re.search(r"\bint mkgnn_tail_score_mc\(const mkgnn_tail_args\* args, float readout_dropout_p, int32_t n_samples,\s*"
                     r"const int64_t\* rng_pair,\s*const mkgnn_tail_mc_out\* out,\s*void\* workspace, size_t workspace_bytes, void\* stream\);", h)
    assert re.search(r"typedef struct mkgnn_tail_mc_out \{\s*float\* samples; int64_t samples_stride;[^}]*float\* mean; float\* std; "
                     r"float\* acq;[^}]*float alpha, beta;[^}]*\} mkgnn_tail_mc_out;", h)
    m = re.search(r"#define\s+MKGNN_TAIL_MC_MAX_SAMPLES\s+(\d+)", h)
    assert m and int(m.group(1)) == 64 == _lib.TAIL_MC_MAX_SAMPLES
    m = re.search(r"#define\s+MKGNN_ABI_VERSION\s+(\d+)", h)
    assert m and int(m.group(1)) == 8 and _lib.ABI_VERSION == 8
    lib = ctypes.CDLL(_lib.LIB_PATH)
    lib.mkgnn_abi_version.restype = ctypes.c_int
    assert lib.mkgnn_abi_version() == 8
    for name in ("mkgnn_tail_score_mc", "mkgnn_tail_score_mc_workspace_bytes"):
        assert hasattr(lib, name), name
        assert name in _lib.EXPORTS, name
    # the argument block is the training tail's, unchanged; the output block: two pointers, a stride, three pointers... 48 bytes
    assert ctypes.sizeof(_lib.TailArgs) == 312
    assert ctypes.sizeof(_lib.TailMcOut) == 48
    assert [n for n, _ in _lib.TailMcOut._fields_] == ["samples", "samples_stride", "mean", "std", "acq", "alpha", "beta"]
    bound = _lib.load()
    assert bound.mkgnn_tail_score_mc.argtypes == [ctypes.POINTER(_lib.TailArgs), ctypes.c_float, ctypes.c_int32, ctypes.c_void_p,
                                                  ctypes.POINTER(_lib.TailMcOut), ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    assert bound.mkgnn_tail_score_mc_workspace_bytes.restype is ctypes.c_size_t
    # the z rows only, as the score tail
    for shape in ((110, 32, 32, 1000, 40), (110, 32, 32, 3, 1), (110, 30, 7, 77, 5), (110, 32, 32, 0, 40)):
        assert bound.mkgnn_tail_score_mc_workspace_bytes(*shape) == bound.mkgnn_tail_score_workspace_bytes(*shape)
    assert bound.mkgnn_tail_score_mc_workspace_bytes(110, 32, 32, 1000, 40) == 1000 * 32 * 4


def test_mc_rejects_bad_arguments_on_the_host():
    """Checked before anything is launched: no device needed (no pointer is read)."""
    from molkgnn_amd import _lib
    lib = _lib.load()

    def last_error():
        return lib.mkgnn_last_error().decode()

    out = _lib.TailMcOut()
    pair = (ctypes.c_int64 * 2)(1234, 7)                       # (a host address: never read -- every call below is refused first)
    assert lib.mkgnn_tail_score_mc(None, 0.0, 4, pair, ctypes.byref(out), None, 0, None) != 0
    a = _lib.TailArgs()
    a.readout.F, a.readout.H, a.readout.G = 110, 64, 32         # H beyond the fused tail
    for i, L in enumerate((10, 20, 30, 50)):
        a.num_kernels[i] = L
    assert lib.mkgnn_tail_score_mc(ctypes.byref(a), 0.0, 4, pair, ctypes.byref(out), None, 0, None) != 0
    assert "outside the fused tail" in last_error()
    a.readout.H = 32
    a.n_atoms, a.n_mols, a.n_loss_mols = 10, 2, 3
    assert lib.mkgnn_tail_score_mc(ctypes.byref(a), 0.0, 4, pair, ctypes.byref(out), None, 0, None) != 0
    assert "bad sizes" in last_error()
    a.n_loss_mols = 2
    assert lib.mkgnn_tail_score_mc(ctypes.byref(a), 0.0, 4, pair, ctypes.byref(out), None, 0, None) != 0
    assert "null pointer" in last_error()


def _f64_statistics(x, alpha, beta):
    x = x.astype(np.float64)
    mean = x.mean(axis=1)
    std = x.std(axis=1, ddof=1) if x.shape[1] > 1 else np.zeros(x.shape[0])
    return mean, std, alpha * mean + beta * std


@pytest.mark.parametrize("S", [1, 2, 64])
def test_mc_statistics_reference_against_float64(S):
    """Every step is one float32 operation on values of the samples' size: a sum of S terms is within S ulp of the largest partial
    sum; asked for here: 4 (S + 2) float32 ulp of the scale of the float64 result (the largest |sample| of the row, and for the
    standard deviation the row's spread)."""
    from molkgnn_amd.readout import mc_statistics_reference
    rng = np.random.default_rng(100 + S)
    x = (rng.standard_normal((257, S)) * 3.0 - 8.0).astype(np.float32)
    x[0] = 2.5                                                 # a row of equal values
    x[1, S // 2] = np.nan                                      # a row holding a NaN
    alpha, beta = -1.0, 1.5
    mean, std, acq = mc_statistics_reference(x, alpha, beta)
    assert mean.dtype == std.dtype == acq.dtype == np.float32 and mean.shape == std.shape == acq.shape == (257,)
    wm, ws, wa = _f64_statistics(x, alpha, beta)
    ok = np.ones(257, dtype=bool)
    ok[1] = False
    ulp = float(np.finfo(np.float32).eps)
    scale = np.abs(x[ok].astype(np.float64)).max(axis=1)
    tol = 4 * (S + 2) * ulp * scale
    for name, got, want in (("mean", mean, wm), ("std", std, ws), ("acq", acq, wa)):
        err = np.abs(got[ok].astype(np.float64) - want[ok])
        print(name, "max error", float(err.max()), "against", float(tol.min()))
        # (the spread is taken from differences of values of that scale: the same absolute bound, before the square root, whose
        # condition is 1/2 away from 0; at a spread of 0 -- the equal row -- the result is exact, checked below)
        assert (err <= tol * (1.0 + abs(beta) if name == "acq" else 1.0)).all(), name
    assert mean[0] == np.float32(2.5) and std[0] == 0.0 and acq[0] == np.float32(alpha * 2.5)
    assert np.isnan(mean[1]) and np.isnan(acq[1]) and (np.isnan(std[1]) if S > 1 else std[1] == 0.0)
    if S == 1:
        assert (std == 0.0).all() and np.array_equal(mean[ok], x[ok, 0])


def test_mc_statistics_reference_takes_tensors_and_refuses_other_shapes():
    import torch
    from molkgnn_amd.readout import mc_statistics_reference
    x = torch.tensor([[1.0, 2.0, 4.0]])
    mean, std, acq = mc_statistics_reference(x, 1.0, 1.0)
    assert mean[0] == np.float32(7.0) / np.float32(3.0) and abs(float(std[0]) - 1.5275252) < 1e-6
    assert acq[0] == mean[0] + std[0]
    with pytest.raises(ValueError):
        mc_statistics_reference(torch.zeros(3))
    with pytest.raises(ValueError):
        mc_statistics_reference(np.zeros((3, 0), dtype=np.float32))


def test_predict_mc_refuses_before_touching_the_batch():
    from molkgnn_amd.train import GNNModel
    model = GNNModel(num_layers=1, dropout_ratio=0.2, ffn_dropout_rate=0.25)
    model.train()
    with pytest.raises(ValueError, match="evaluation mode"):
        model.predict_mc(object(), 8)
    assert model.training                                     # ... and the mode is not flipped behind the caller's back
    model.eval()
    for bad in (0, 65, -3, 2.5):
        with pytest.raises(ValueError, match="n_samples"):
            model.predict_mc(object(), bad)
    plain = GNNModel(num_layers=1, dropout_ratio=0.0, ffn_dropout_rate=0.0).eval()
    with pytest.raises(ValueError, match="no dropout uncertainty"):
        plain.predict_mc(object(), 8)
    assert not model.training and not plain.training
