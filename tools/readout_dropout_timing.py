"""Per-step time of the training step with the readout's dropout (``GNNModel(dropout_ratio=0.2)``, the authors' setting) on the
fused paths, against the same step without it and against the separate readout operators the dropout took before.

    python tools/readout_dropout_timing.py [--batches 16 256 4096] [--steps 50] [--warmup 10] [--timeout 300]

One JSON line per (batch, route, mode): ``ms_per_step`` over ``--steps`` steps timed with device events after ``--warmup``
untimed ones.  Modes: ``eager`` (``train.training_step`` launched from Python every step) and ``replayed``
(``train.CapturedSteps``: the step captured once, then replayed).  Routes: ``p0`` (``dropout_ratio=0``: the fused paths as
they were), ``p0.2_fused`` (``dropout_ratio=0.2``: molecule-resident step or fused tail with the mask drawn in the kernels) and
``p0.2_separate`` (``dropout_ratio=0.2`` with ``MKGNN_FUSED_TAIL=0 MKGNN_MOLECULE=0``: the separate readout operators with a
``torch.bernoulli`` mask, then the head kernels).  Those switches are read when the package is imported, so every route runs in
a child process of its own, under its own time limit.  Head dropout 0.25 (the default) and fused AdamW in every step.
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROUTES = {"p0": (0.0, {}), "p0.2_fused": (0.2, {}),
          "p0.2_separate": (0.2, {"MKGNN_FUSED_TAIL": "0", "MKGNN_MOLECULE": "0"})}


def _time(fn, steps, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(steps):
        loss = fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / steps, float(loss)


def run_route(route, batches, steps, warmup):
    import torch
    sys.path.insert(0, REPO)
    from molkgnn_amd.synthetic import make_batch
    from molkgnn_amd.train import CapturedSteps, GNNModel, configure_optimizer, training_step, tune_torch_backends
    dev = torch.device("cuda:0")
    tune_torch_backends()
    p = ROUTES[route][0]
    for B in batches:
        batch = make_batch(B, seed=B, assay="9999").to(dev)
        for mode in ("eager", "replayed"):
            torch.manual_seed(0)
            model = GNNModel(dropout_ratio=p).to(dev).train()
            opt = configure_optimizer(model, lr=1e-4)
            if mode == "eager":
                ms, loss = _time(lambda: training_step(model, batch, opt), steps, warmup)
            else:
                cs = CapturedSteps(model, opt, warmup=2)
                ms, loss = _time(lambda: cs(batch), steps, warmup)
                assert len(cs._graphs) == 1, "the step was not captured"
            print(json.dumps({"batch": B, "route": route, "mode": mode, "ms_per_step": round(ms, 4), "last_loss": loss,
                              "steps": steps}), flush=True)
            del model, opt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[16, 256, 4096])
    ap.add_argument("--routes", nargs="+", default=list(ROUTES))
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--timeout", type=float, default=300.0, help="seconds per route (child process)")
    ap.add_argument("--child", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        run_route(args.child, args.batches, args.steps, args.warmup)
        return
    for route in args.routes:
        env = dict(os.environ, **ROUTES[route][1])
        cmd = [sys.executable, os.path.abspath(__file__), "--child", route, "--steps", str(args.steps), "--warmup",
               str(args.warmup), "--batches", *map(str, args.batches)]
        try:
            rc = subprocess.run(cmd, env=env, timeout=args.timeout).returncode
        except subprocess.TimeoutExpired:
            print(json.dumps({"route": route, "error": f"timed out after {args.timeout} s"}), flush=True)
            sys.exit(124)
        if rc != 0:                               # (a failed route ends the run: nothing more is started on the GPU)
            print(json.dumps({"route": route, "error": f"exit status {rc}"}), flush=True)
            sys.exit(1)


if __name__ == "__main__":
    main()
