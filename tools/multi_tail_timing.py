"""Per-step time of the multi-output training step on the multi-output fused tail (``GNNModel.multi_output_tail = True``:
``readout.tail_labels_loss`` -> ``mkgnn_tail_fused_labels``), beside the default routes it is to be read against.

    python tools/multi_tail_timing.py [--batches 16 256 4096] [--tasks 9 32] [--present 1.0 0.15] [--windows 10] [--replays 32]

Routes, built on the same ``all9`` batch, each the captured training step (``train.CapturedSteps``, fused AdamW) replayed:

* ``label_tail``  -- ``task_dim=T``, ``batch.labels``, ``multi_output_tail = True``: the new route;
* ``label``       -- the same model on today's default route (separate readout operators + the label-matrix head): the yardstick;
* ``task_tail``   -- ``task_dim=T``, ``batch.task``, ``multi_output_tail = True``;
* ``task``        -- the task-indexed head on today's default route;
* ``single``      -- ``task_dim=1`` as it runs by default (molecule-resident step or fused tail).

The routes take turns inside a window and the windows repeat: one JSON line per (batch, T, present, route) with the median, the
minimum and the maximum over ``--windows`` windows of ``--replays`` replays timed with device events, so the spread of a route is
on the page next to the differences between routes.  Needs the GPU: there is no CPU path.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ROUTES = ("label_tail", "label", "task_tail", "task", "single")


def _window(fn, replays):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(replays):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / replays


def _labels(B, T, present, seed):
    g = torch.Generator().manual_seed(seed)
    y = (torch.rand(B, T, generator=g) < 0.3).float()
    if present >= 1.0:
        return y
    return torch.where(torch.rand(B, T, generator=g) < present, y, torch.full((), float("nan")))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[16, 256, 4096])
    ap.add_argument("--tasks", type=int, nargs="+", default=[9, 32])
    ap.add_argument("--present", type=float, nargs="+", default=[1.0, 0.15])
    ap.add_argument("--routes", nargs="+", default=list(ROUTES), choices=ROUTES)
    ap.add_argument("--windows", type=int, default=10)
    ap.add_argument("--replays", type=int, default=32)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("multi_tail_timing.py measures on the GPU: none found")
    from molkgnn_amd import _lib
    from molkgnn_amd.synthetic import make_batch
    from molkgnn_amd.train import CapturedSteps, GNNModel, configure_optimizer, tune_torch_backends
    dev = torch.device("cuda:0")
    tune_torch_backends()
    for B in args.batches:
        host = make_batch(B, seed=B, assay="all9")
        for T in args.tasks:
            for present in args.present:
                labels = _labels(B, T, present, B * 100 + T)
                # (the task-indexed routes: "present" is the share of molecules that name a task at all)
                task = (torch.arange(B) % T).to(torch.int32)
                if present < 1.0:
                    g = torch.Generator().manual_seed(B + T)
                    task = torch.where(torch.rand(B, generator=g) < present, task, torch.full_like(task, -1))
                fns = {}
                for route in args.routes:
                    batch = host.to(dev)                          # (a batch object of its own per route: CapturedSteps keys on it)
                    if route.startswith("label"):
                        batch.labels = labels.to(dev)
                    elif route.startswith("task"):
                        batch.task = task.to(dev)
                    torch.manual_seed(0)
                    model = GNNModel(task_dim=1 if route == "single" else T).to(dev).train()
                    model.multi_output_tail = route.endswith("_tail")
                    steps = CapturedSteps(model, configure_optimizer(model, lr=1e-4), warmup=2)
                    seen, real = [], _lib.check
                    _lib.check = lambda rc, what: (seen.append(what), real(rc, what))[1]
                    try:
                        for _ in range(4):                        # two eager steps, the capture, a replay
                            steps(batch)
                    finally:
                        _lib.check = real
                    assert len(steps._graphs) == 1, "the step was not captured"
                    assert ("mkgnn_tail_fused_labels" in seen) == route.endswith("_tail"), (route, sorted(set(seen)))
                    fns[route] = (lambda s=steps, b=batch: s(b))
                torch.cuda.synchronize()
                times = {route: [] for route in fns}
                for _ in range(args.windows):                      # the routes take turns inside a window
                    for route, fn in fns.items():
                        times[route].append(_window(fn, args.replays))
                for route, ms in times.items():
                    print(json.dumps({"batch": B, "tasks": T, "present": present, "route": route,
                                      "ms_per_step_median": round(statistics.median(ms), 4), "min": round(min(ms), 4),
                                      "max": round(max(ms), 4), "windows": args.windows, "replays": args.replays}), flush=True)
                del fns


if __name__ == "__main__":
    main()
