"""Per-step time of the training step with a weighted loss (``BCEWithLogitsLoss(pos_weight=...)``, per-molecule weights) on the
fused tail and the task-indexed head, beside the unweighted steps it is to be read against.

    python tools/weighted_loss_timing.py [--batches 16 256 4096] [--windows 10] [--replays 32]
    MKGNN_FUSED_TAIL=0 python tools/weighted_loss_timing.py --legs pos_weight        # the separate operators + weighted head
    python tools/weighted_loss_timing.py --parent-leg                                # on a checkout WITHOUT the weighted kernels

Legs, each the captured training step (``train.CapturedSteps``, fused AdamW) of its own model on the same batch:

* ``unweighted``        -- ``GNNModel()`` as it runs by default;
* ``pos_weight``        -- ``GNNModel(loss_func=BCEWithLogitsLoss(pos_weight=tensor([7.])))``: the weighted fused tail (under
  ``MKGNN_FUSED_TAIL=0``, set before the process starts, the separate operators + the weighted head);
* ``pos_weight+weight`` -- the same with ``batch.weight`` as well;
* ``task9``             -- ``GNNModel(task_dim=9)`` on a batch that carries ``task``, unweighted;
* ``task9_pos_weight``  -- the same with ``[9]`` positive weights.

``--parent-leg`` runs ``pos_weight`` alone and uses nothing a checkout before the weighted kernels lacks: there the loss takes
the PyTorch route, which is the yardstick for whether the kernels were worth it.

The graphs take turns inside one process: a window is ``--replays`` replays of one leg between two device events, the legs
alternate window by window, and a leg's figure is the median of its ``--windows`` windows (min and max beside it).  One JSON line
per (batch, leg).  Needs the GPU: there is no CPU path.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

LEGS = ("unweighted", "pos_weight", "pos_weight+weight", "task9", "task9_pos_weight")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[16, 256, 4096])
    ap.add_argument("--legs", nargs="+", default=list(LEGS), choices=LEGS)
    ap.add_argument("--parent-leg", action="store_true")
    ap.add_argument("--windows", type=int, default=10)
    ap.add_argument("--replays", type=int, default=32)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("weighted_loss_timing.py measures on the GPU: none found")
    from torch.nn import BCEWithLogitsLoss
    from molkgnn_amd.sampling import task_index
    from molkgnn_amd.synthetic import NINE_ASSAYS, make_batch
    from molkgnn_amd.train import CapturedSteps, GNNModel, configure_optimizer, tune_torch_backends
    dev = torch.device("cuda:0")
    tune_torch_backends()
    legs = ["pos_weight"] if args.parent_leg else list(args.legs)
    nine = [int(a) for a in NINE_ASSAYS]
    for B in args.batches:
        plain = make_batch(B, seed=B, assay="all9").to(dev)
        weighted = make_batch(B, seed=B, assay="all9").to(dev)
        weighted.weight = (torch.arange(B, device=dev) % 5).float() * 0.5
        tasked = make_batch(B, seed=B, assay="all9")
        tasked.task = task_index(tasked.assay_id, nine)
        tasked = tasked.to(dev)
        steps = {}
        for leg in legs:
            torch.manual_seed(0)
            nine_tasks = leg.startswith("task9")
            lf = None
            if "pos_weight" in leg:
                lf = BCEWithLogitsLoss(pos_weight=torch.linspace(0.5, 40.0, 9) if nine_tasks else torch.tensor([7.0]))
            model = GNNModel(task_dim=9 if nine_tasks else 1, loss_func=lf).to(dev).train()
            batch = tasked if nine_tasks else (weighted if leg.endswith("+weight") else plain)
            run = CapturedSteps(model, configure_optimizer(model, lr=1e-4), warmup=2)
            for _ in range(6):                                # eager, capture, replays
                run(batch)
            torch.cuda.synchronize()
            assert len(run._graphs) == 1, "the step was not captured"
            steps[leg] = (run, batch)
        times = {leg: [] for leg in legs}
        for _ in range(args.windows):
            for leg in legs:
                run, batch = steps[leg]
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                for _ in range(args.replays):
                    run(batch)
                t1.record()
                torch.cuda.synchronize()
                times[leg].append(t0.elapsed_time(t1) / args.replays)
        for leg in legs:
            t = times[leg]
            print(json.dumps({"batch": B, "leg": leg, "parent_leg": bool(args.parent_leg), "fused_tail": os.environ.get("MKGNN_FUSED_TAIL", "1"),
                              "ms_per_step_median": round(statistics.median(t), 4), "min": round(min(t), 4), "max": round(max(t), 4),
                              "windows": args.windows, "replays": args.replays}), flush=True)
        del steps


if __name__ == "__main__":
    main()
