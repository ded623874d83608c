"""Per-step time of the docking-score regression training step (``GNNModel(loss_func=MSELoss(reduction='sum'))``) on the HIP
loss paths, against the PyTorch route the same loss took before they existed, with the BCE step alongside.

    python tools/regression_step_timing.py [--batches 16 256 4096] [--steps 50] [--warmup 10]

One JSON line per (batch, loss route, mode): ``ms_per_step`` over ``--steps`` steps timed with device events after ``--warmup``
untimed ones.  Modes: ``eager`` (``train.training_step`` launched from Python every step) and ``replayed``
(``train.CapturedSteps``: the step captured once, then replayed).  Routes: ``bce`` (``BCEWithLogitsLoss()``, the benchmark's
step), ``mse_sum`` (the HIP paths: molecule-resident step, fused tail or head kernels with the squared-error kind) and
``mse_sum_torch`` (the same loss through a subclass of ``MSELoss``, which ``GNNModel.loss`` does not recognise: the embedding,
then the PyTorch head and loss -- the route every ``MSELoss`` took before).  Fused AdamW in every step.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


class TorchRouteMSELoss(torch.nn.MSELoss):
    """``MSELoss`` under another type: ``GNNModel.loss`` takes its PyTorch route for it."""


def _loss_func(route):
    if route == "bce":
        return None
    if route == "mse_sum":
        return torch.nn.MSELoss(reduction="sum")
    return TorchRouteMSELoss(reduction="sum")


def _time(fn, steps, warmup):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[16, 256, 4096])
    ap.add_argument("--routes", nargs="+", default=["bce", "mse_sum", "mse_sum_torch"])
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    from molkgnn_amd.synthetic import make_batch
    from molkgnn_amd.train import CapturedSteps, GNNModel, configure_optimizer, training_step, tune_torch_backends
    dev = torch.device("cuda:0")
    tune_torch_backends()
    for B in args.batches:
        for route in args.routes:
            target = "activity" if route == "bce" else "docking_score"
            batch = make_batch(B, seed=B, target=target, assay="9999").to(dev)
            for mode in ("eager", "replayed"):
                torch.manual_seed(0)
                model = GNNModel(loss_func=_loss_func(route)).to(dev).train()
                opt = configure_optimizer(model, lr=1e-4)
                if mode == "eager":
                    ms, loss = _time(lambda: training_step(model, batch, opt), args.steps, args.warmup)
                else:
                    steps = CapturedSteps(model, opt, warmup=2)
                    ms, loss = _time(lambda: steps(batch), args.steps, args.warmup)
                    assert len(steps._graphs) == 1, "the step was not captured"
                print(json.dumps({"batch": B, "route": route, "mode": mode, "ms_per_step": round(ms, 4),
                                  "last_loss": loss, "steps": args.steps}), flush=True)
                del model, opt


if __name__ == "__main__":
    main()
