"""The fallback convolution families against float64 under their switches.  ``pytest -m gpu``.

Round 1's LDS-bank forward (``kc_forward_fused``), the MFMA rows kernel with the LDS bank kernel and the per-degree LDS pair
(``kc_backward_rows_lds`` / ``kc_backward_bank_lds``) serve what the streamed kernels refuse and are the other side of every A/B
switch.  For every setting of tests/_conv_families.SETTINGS one child process (tests/_conv_families_child.py: the library reads
its switches once) runs every case of the table through the automatic dispatch; here every (setting, case) is held to

* everything tests/test_conv_anyshape_f64.py::test_case_against_float64 asserts (``tests/_conv_f64.check_against_float64``): finite,
  both output storages equal, zeros outside the own block, the tie-aware criterion, the kept scores through ``tests/_f64.check``,
  chirality signs exactly, every gradient per element within ``32 * 2^-24 * sum |terms|`` of the float64 closed form, no gradient
  for a degenerate degree, the tweaks' marks;
* the dispatch: ``mkgnn_debug_conv_dispatch`` answers the table's literal, and the three streamed launch counters advanced exactly
  where it says a streamed kernel runs;
* for five cases, a second run with the same bits.

The float64 oracle of a case is computed once per distinct permutation choice and shared by the settings.

A child runs under a time limit of three times its measured wall time on the MI355X, at least 120 s (import and library load
dominate; the margin is for a busy shared machine).  Measured, seconds of wall time per child (of which 0.5 to 0.7 s between the
first import of the package and the written file): default 2.5, fwd_stream0 2.4, rows_stream0 2.4, bank_stream0 2.6,
no_mfma_bwd 2.5, bank_fused0 2.5, split0 2.7 -- so 120 s each.  A child that ends on a
signal, an abort or its time limit is a finding to be explained from the code: every later test of the module then fails at once
without starting another process on the GPU.
"""
import functools
import os
import subprocess
import sys
import time
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import _conv_f64 as C
from tests import _conv_families as Fam

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEASURED_S = {"default": 2.5, "fwd_stream0": 2.4, "rows_stream0": 2.4, "bank_stream0": 2.6, "no_mfma_bwd": 2.5, "bank_fused0": 2.5,
              "split0": 2.7}
TIMEOUT_S = {s: max(120.0, 3.0 * MEASURED_S[s]) for s in Fam.SETTING_NAMES}

_RESULTS = {}        # setting -> {npz key: array}
_FAILED = {}         # setting -> why its child gave no results (asked once)
_LATCH = []          # why no further child may start: a child died on a signal, aborted or ran into its time limit


def _results(setting, tmp_dir):
    """The arrays of the setting's child; it is started once, on first use."""
    if _LATCH:
        pytest.fail(f"no further child is started: {_LATCH[0]}")
    if setting in _FAILED:
        pytest.fail(_FAILED[setting])
    if setting not in _RESULTS:
        path = os.path.join(tmp_dir, setting + ".npz")
        cmd = [sys.executable, "-m", "tests._conv_families_child", setting, path]
        t0 = time.time()
        try:
            run = subprocess.run(cmd, cwd=REPO, env=Fam.environment(setting, os.environ), capture_output=True, text=True,
                                 timeout=TIMEOUT_S[setting])
        except subprocess.TimeoutExpired:
            _LATCH.append(f"the child of setting {setting!r} ran into its time limit of {TIMEOUT_S[setting]:.0f} s")
            pytest.fail(_LATCH[0])
        print(f"child {setting}: {time.time() - t0:.1f} s wall;", run.stdout.strip())
        if run.returncode < 0 or run.returncode in (134, 139):
            _LATCH.append(f"the child of setting {setting!r} ended with status {run.returncode}: {run.stderr[-2000:]}")
            pytest.fail(_LATCH[0])
        if run.returncode != 0:
            _FAILED[setting] = f"the child of setting {setting!r} failed ({run.returncode}): {run.stderr[-4000:]}"
            pytest.fail(_FAILED[setting])
        with np.load(path) as z:
            _RESULTS[setting] = {k: z[k] for k in z.files}
    return _RESULTS[setting]


@pytest.fixture(scope="module")
def tmp_dir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("conv_families"))


def _unpack(arrays, key):
    def get(part):
        a = arrays.get(f"{key}/{part}")
        return None if a is None else torch.from_numpy(a)
    grads = {k[len(key) + 6:]: torch.from_numpy(v) for k, v in arrays.items() if k.startswith(key + "/grad/")}
    return SimpleNamespace(out=get("out"), out_details=get("out_details"), gx=get("gx"), idx=[get(f"idx{d}") for d in range(4)],
                           scores=[get(f"scores{d}") for d in range(4)], chir=[get(f"chir{d}") for d in range(4)], grads=grads,
                           streamed=tuple(int(v) for v in arrays[f"{key}/streamed"]), dispatch=str(arrays[f"{key}/dispatch"]),
                           backward="auto")


@functools.lru_cache(maxsize=None)
def _oracle(name, idx_bytes):
    """The float64 closed form of the case at the permutation choices ``idx_bytes`` (per degree: the bytes of the int64 choices
    [L_d, N_d], or None): once per distinct choice, whatever setting made it."""
    built = C.build(name)
    idx = [None if b is None else torch.from_numpy(np.frombuffer(b, dtype=np.int64).reshape(built.info.counts[d], built.info.n[d]).copy())
           for d, b in enumerate(idx_bytes)]
    return C.oracle_gradients_f64(built, idx)


def _same_bits(a, b):
    assert torch.equal(a.out, b.out) and torch.equal(a.out_details, b.out_details) and torch.equal(a.gx, b.gx)
    for u, v in zip(a.idx + a.scores + a.chir, b.idx + b.scores + b.chir):
        assert (u is None) == (v is None) and (u is None or torch.equal(u, v))
    assert a.grads.keys() == b.grads.keys()
    for k in a.grads:
        assert torch.equal(a.grads[k], b.grads[k]), k
    assert a.dispatch == b.dispatch and a.streamed == b.streamed


@pytest.mark.parametrize("setting,name", Fam.PAIRS, ids=[f"{s}-{n}" for s, n in Fam.PAIRS])
def test_family_case_against_float64(setting, name, tmp_dir):
    arrays = _results(setting, tmp_dir)
    built = C.build(name)
    res = _unpack(arrays, name)
    tag = (name, setting)
    assert all(i is None or i.dtype == torch.int64 for i in res.idx)
    oracle = _oracle(name, tuple(None if i is None else i.numpy().tobytes() for i in res.idx))
    worst, _ = C.check_against_float64(built, res, tag, oracle=oracle)
    # ---- which kernels ran
    assert res.dispatch == Fam.EXPECTED[name][setting], (tag, res.dispatch)
    C.check_streamed_counters(res.dispatch, res.streamed, tag)
    # ---- fixed-order sums, no float atomics: a second run gives the same bits
    if name in Fam.TWICE:
        _same_bits(res, _unpack(arrays, name + "#2"))
    C.record({"case": name, "edge": built.case.edge, "setting": setting, "dispatch": res.dispatch, "streamed": list(res.streamed),
              "worst": worst, **C.worst_by_group(res.gx, res.grads, oracle)})
