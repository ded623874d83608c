"""What gradient clipping by global norm costs a captured training step (``optim.FusedAdamW(max_grad_norm=...)``,
``mkgnn_adamw_step_clipped``), beside the unclipped step and beside PyTorch's own clipping in front of the unclipped step.

    python tools/clip_timing.py [--batches 16 256 4096] [--steps 200] [--warmup 20] [--rounds 5] [--max-norm 1.0]

Routes, each ``train.CapturedSteps`` over the same batch and the same initial model (``GNNModel()``, fused AdamW):

* ``unclipped``   -- the step as it is without the feature (``mkgnn_adamw_step``, one optimiser launch);
* ``fused_clip``  -- ``max_grad_norm`` set: the partial-sum launch and the clipped update (two optimiser launches);
* ``torch_clip``  -- ``torch.nn.utils.clip_grad_norm_(foreach=True)`` between backward and the unclipped fused step, captured as well.

and, under ``"what": "optimizer_only"``, the optimiser launches alone over the gradients of one step of the first batch size: one
graph that holds ``mkgnn_adamw_step`` and one that holds the two launches of ``mkgnn_adamw_step_clipped``, replayed back to back.

One JSON line per (batch, route, round): ``ms_per_step`` over ``--steps`` replays timed with device events after ``--warmup``
untimed ones; the routes alternate inside a round.  Then one ``"summary"`` line per batch: the median over the rounds and the
spread (min, max) of every route, ``fused_clip / unclipped`` and ``fused_clip / torch_clip`` of the medians.  Needs the GPU: there is
no CPU path.
"""
from __future__ import annotations

import argparse
import copy
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ROUTES = ("unclipped", "fused_clip", "torch_clip")


def _time(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(steps):
        out = fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / steps, out


def _summary(times: dict) -> dict:
    out = {r: {"median_ms": round(statistics.median(v), 5), "min_ms": round(min(v), 5), "max_ms": round(max(v), 5)} for r, v in times.items()}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[16, 256, 4096])
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--max-norm", type=float, default=1.0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("clip_timing.py measures on the GPU: none found")
    from molkgnn_amd.optim import FusedAdamW
    from molkgnn_amd.synthetic import make_batch
    from molkgnn_amd.train import CapturedSteps, GNNModel, configure_optimizer, training_step, tune_torch_backends

    class TorchClipThenFused(FusedAdamW):
        """``clip_grad_norm_(foreach=True)`` in front of the unclipped fused step (no read-back: capturable)."""

        def step(self, closure=None):
            params = [p for g in self.param_groups for p in g["params"] if p.grad is not None]
            torch.nn.utils.clip_grad_norm_(params, args.max_norm, foreach=True)
            return super().step(closure)

    def optimizer(model, route):
        if route == "torch_clip":
            base = configure_optimizer(model, lr=1e-4)
            opt = TorchClipThenFused(base.param_groups)
            opt.prepare_state()
            return opt
        return configure_optimizer(model, lr=1e-4, max_grad_norm=args.max_norm if route == "fused_clip" else None)

    dev = torch.device("cuda:0")
    tune_torch_backends()
    torch.manual_seed(0)
    model0 = GNNModel().to(dev).train()
    for B in args.batches:
        batch = make_batch(B, seed=B).to(dev)
        runs = {}
        for route in ROUTES:                                  # every route: its own model, optimiser and captured graph, built once
            model = copy.deepcopy(model0)
            steps = CapturedSteps(model, optimizer(model, route), warmup=2)
            _time(lambda: steps(batch), 3, 3)
            assert len(steps._graphs) == 1, "the step was not captured"
            runs[route] = (model, steps)
        times = {r: [] for r in ROUTES}
        for rnd in range(args.rounds):
            for route in ROUTES:
                ms, loss = _time(lambda: runs[route][1](batch), args.steps, args.warmup)
                times[route].append(ms)
                print(json.dumps({"what": "captured_step", "batch": B, "route": route, "round": rnd, "ms_per_step": round(ms, 5),
                                  "last_loss": float(loss.detach()), "steps": args.steps}), flush=True)
        s = _summary(times)
        print(json.dumps({"what": "summary", "batch": B, "routes": s,
                          "fused_clip_over_unclipped": round(s["fused_clip"]["median_ms"] / s["unclipped"]["median_ms"], 4),
                          "fused_clip_over_torch_clip": round(s["fused_clip"]["median_ms"] / s["torch_clip"]["median_ms"], 4)}), flush=True)
        del runs

    # the optimiser launches alone, over the gradients one step leaves behind
    batch = make_batch(args.batches[0], seed=args.batches[0]).to(dev)
    graphs = {}
    for route in ("unclipped", "fused_clip"):
        model = copy.deepcopy(model0)
        opt = optimizer(model, route)
        training_step(model, batch, opt)                     # gradients exist; the kernels' first launch is an eager one
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            opt.step()
        graphs[route] = (model, opt, g)
    times = {r: [] for r in graphs}
    for rnd in range(args.rounds):
        for route, (_, _, g) in graphs.items():
            ms, _ = _time(g.replay, args.steps, args.warmup)
            times[route].append(ms)
            print(json.dumps({"what": "optimizer_only", "route": route, "round": rnd, "us_per_replay": round(1e3 * ms, 3),
                              "steps": args.steps}), flush=True)
    s = _summary(times)
    print(json.dumps({"what": "optimizer_only_summary", "routes": s,
                      "two_launches_minus_one_us": round(1e3 * (s["fused_clip"]["median_ms"] - s["unclipped"]["median_ms"]), 3)}), flush=True)


if __name__ == "__main__":
    main()
