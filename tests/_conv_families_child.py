"""Child process of tests/test_conv_families_gpu.py: ``python -m tests._conv_families_child <setting> <out.npz>``, started with that
setting's environment (tests/_conv_families.SETTINGS; the library reads its switches once per process).  Runs every case of the
setting through the automatic dispatch -- one forward with details, one forward + backward -- and writes what came out to the
``.npz``; the parent holds it to float64.  Five cases run a second time (``<name>#2/...``): their bits must not change."""
import os
import sys
import time

import numpy as np
import torch

from tests import _conv_f64 as C
from tests import _conv_families as Fam


def _poison_free_gpu_memory():
    """tests/conftest.py's fixture, which does not reach a child: the caching allocator's free blocks hold NaN bit patterns, so a
    kernel that reads a ``torch.empty`` buffer it never wrote does not pass by luck on zero-filled fresh memory."""
    junk = [torch.full((64 << 20,), float("nan"), device="cuda") for _ in range(4)]
    small = [torch.full((n,), float("nan"), device="cuda") for n in (128, 1024, 8192, 65536, 1 << 20) for _ in range(8)]
    torch.cuda.synchronize()
    del junk, small


def _store(out, key, res):
    out[f"{key}/out"], out[f"{key}/out_details"], out[f"{key}/gx"] = res.out.numpy(), res.out_details.numpy(), res.gx.numpy()
    for d in range(4):
        for part, t in (("idx", res.idx[d]), ("scores", res.scores[d]), ("chir", res.chir[d])):
            if t is not None:
                out[f"{key}/{part}{d}"] = t.contiguous().numpy()
    for name, g in res.grads.items():
        out[f"{key}/grad/{name}"] = g.numpy()
    out[f"{key}/streamed"] = np.asarray(res.streamed, dtype=np.int64)
    out[f"{key}/dispatch"] = np.asarray(res.dispatch)


def main(setting, path):
    t0 = time.time()
    switches = {k: v for k, v in os.environ.items() if k.startswith("MKGNN_")}
    assert switches == Fam.SETTINGS[setting], (setting, switches)                   # the switches arrived, and no other
    from molkgnn_amd import molecule, plan
    molecule._MODE = "0"                                                            # the per-operator path
    assert torch.cuda.is_available(), "the family tests need the MI355X"
    dev = torch.device("cuda:0")
    _poison_free_gpu_memory()
    out = {}
    e_unit = plan.Bucket.e_unit
    for name in Fam.cases_of(setting):
        built = C.build(name)
        if built.case.no_unit:
            plan.Bucket.e_unit = lambda self, E: None                               # a caller that passes no unit bond rows
        try:
            _store(out, name, C.run_build(built, dev, "auto", "auto"))
            if name in Fam.TWICE:
                _store(out, name + "#2", C.run_build(built, dev, "auto", "auto"))
        finally:
            plan.Bucket.e_unit = e_unit
    np.savez(path, **out)
    print(f"{setting}: {len(Fam.cases_of(setting))} cases in {time.time() - t0:.1f} s")


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
