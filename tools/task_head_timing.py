"""Per-step time of the mixed-assay training step on the task-indexed head (``GNNModel(task_dim=9)`` on a batch that carries
``task``; ``readout.task_head_loss``), beside the two single-task steps it is to be read against.

    python tools/task_head_timing.py [--batches 16 256 4096] [--steps 50] [--warmup 10] [--rounds 3]

Routes, built on the same ``all9`` batch:

* ``task9``       -- ``task_dim=9``, ``batch.task`` from ``sampling.task_index``: embedding from the separate readout operators,
  then the task head (two launches, forward and gradients);
* ``single_ops``  -- ``task_dim=1`` with the fused tail and the molecule-resident step switched off (what ``MKGNN_FUSED_TAIL=0``
  with ``MKGNN_MOLECULE=0`` gives): the same separate-operator route with the single-task head -- the like-for-like comparison;
* ``single``      -- ``task_dim=1`` as it runs by default (molecule-resident step or fused tail): the known faster shape.

One JSON line per (batch, route, mode, round): ``ms_per_step`` over ``--steps`` steps timed with device events after ``--warmup``
untimed ones.  Modes: ``eager`` (``train.training_step`` every step) and ``replayed`` (``train.CapturedSteps``).  The routes
alternate inside a round and the rounds repeat, so the spread between rounds of one route is on the page next to the differences
between routes.  Fused AdamW in every step.  Needs the GPU: there is no CPU path.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ROUTES = ("task9", "single_ops", "single")


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
    return t0.elapsed_time(t1) / steps, float(loss.detach())


class _separate_operators:
    """Inside: ``GNNModel.loss`` takes neither the fused tail nor the molecule-resident step (the module switches the environment
    variables set at import)."""

    def __init__(self, on: bool):
        self.on = on

    def __enter__(self):
        from molkgnn_amd import molecule, readout
        self.prev = (readout._FUSED_TAIL, molecule._MODE)
        if self.on:
            readout._FUSED_TAIL, molecule._MODE = False, "0"

    def __exit__(self, *exc):
        from molkgnn_amd import molecule, readout
        readout._FUSED_TAIL, molecule._MODE = self.prev
        return False


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[16, 256, 4096])
    ap.add_argument("--routes", nargs="+", default=list(ROUTES), choices=ROUTES)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("task_head_timing.py measures on the GPU: none found")
    from molkgnn_amd.sampling import task_index
    from molkgnn_amd.synthetic import NINE_ASSAYS, make_batch
    from molkgnn_amd.train import CapturedSteps, GNNModel, configure_optimizer, training_step, tune_torch_backends
    dev = torch.device("cuda:0")
    tune_torch_backends()
    nine = [int(a) for a in NINE_ASSAYS]
    for B in args.batches:
        plain = make_batch(B, seed=B, assay="all9")
        tasked = make_batch(B, seed=B, assay="all9")
        tasked.task = task_index(tasked.assay_id, nine)
        plain, tasked = plain.to(dev), tasked.to(dev)
        for rnd in range(args.rounds):
            for route in args.routes:
                batch = tasked if route == "task9" else plain
                with _separate_operators(route == "single_ops"):
                    for mode in ("eager", "replayed"):
                        torch.manual_seed(0)
                        model = GNNModel(task_dim=9 if route == "task9" else 1).to(dev).train()
                        opt = configure_optimizer(model, lr=1e-4)
                        if mode == "eager":
                            ms, loss = _time(lambda: training_step(model, batch, opt), args.steps, args.warmup)
                        else:
                            steps = CapturedSteps(model, opt, warmup=2)
                            ms, loss = _time(lambda: steps(batch), args.steps, args.warmup)
                            assert len(steps._graphs) == 1, "the step was not captured"
                        print(json.dumps({"batch": B, "route": route, "mode": mode, "round": rnd, "ms_per_step": round(ms, 4),
                                          "last_loss": loss, "steps": args.steps}), flush=True)
                        del model, opt


if __name__ == "__main__":
    main()
