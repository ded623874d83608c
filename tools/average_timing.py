"""What the average of the weights inside the AdamW launch costs a captured training step (``optim.FusedAdamW(average=...)``,
``mkgnn_adamw_step_averaged``), beside the unaveraged step and beside PyTorch's ``AveragedModel`` update behind the unaveraged step.

    python tools/average_timing.py [--batches 16 256 4096] [--windows 10] [--replays 32] [--decay 0.999]
                                   [--parent-tree DIR [--headline-runs 4] [--headline-only] [--headline-args --gpus 1 --full]]

Routes, each ``train.CapturedSteps`` over the same batch and the same initial model (``GNNModel()``, fused AdamW):

* ``averaged``    -- ``average='ema'``: the step with the average kept inside its one optimiser launch;
* ``unaveraged``  -- the step as it is without the feature (``mkgnn_adamw_step``);
* ``torch_ema``   -- the unaveraged step, and behind it, captured as well, the update of
  ``AveragedModel(model, multi_avg_fn=get_ema_multi_avg_fn(decay))``: its ``multi_avg_fn`` over its own parameter list
  (``torch._foreach_lerp_``).  ``update_parameters`` itself keeps ``n_averaged`` on the host and cannot be captured; its first,
  copying call is made eagerly before the capture.

One JSON line per (batch, route, window): ``ms_per_step`` over ``--replays`` replays timed with device events, the routes taking
turns window by window in one process; then a ``"summary"`` line per batch with the median and the spread of every route.

``"what": "optimizer_only"``: the optimiser launches alone over the gradients one step of the first batch size leaves behind,
``--replays`` calls back to back in ONE graph per route (the graph's own launch is shared by all of them), microseconds per call;
``"what": "swap_only"``: ``swap_averaged()`` the same way (an even number of calls: the weights are back where they were).

``--parent-tree DIR``: the unaveraged headline -- ``bench.py`` with ``--headline-args`` in this tree and in a built copy of the
parent commit under ``DIR``, taking turns, ``--headline-runs`` runs each, every run a process of its own; ``ms_per_step`` of each
and the medians (run this tool from a copy of this tree in a sibling directory of ``DIR``: where a tree is run from moves
``bench.py`` by a few microseconds).  Needs the GPU: there is no CPU path.
"""
from __future__ import annotations

import argparse
import copy
import json
import os
import statistics
import subprocess
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

ROUTES = ("averaged", "unaveraged", "torch_ema")


def _window(fn, replays):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(replays):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / replays


def _summary(times: dict, digits=5) -> dict:
    return {r: {"median": round(statistics.median(v), digits), "min": round(min(v), digits), "max": round(max(v), digits)}
            for r, v in times.items()}


def _turns(fns: dict, windows, replays, warm, emit):
    """``fns``: route -> callable; every route warmed, then the routes take turns window by window."""
    for fn in fns.values():
        _window(fn, warm)
    times = {r: [] for r in fns}
    for w in range(windows):
        for r, fn in fns.items():
            ms = _window(fn, replays)
            times[r].append(ms)
            emit(r, w, ms)
    return times


def _headline(tree, extra):
    out = subprocess.run([sys.executable, "bench.py"] + extra, cwd=tree, check=True, stdout=subprocess.PIPE, text=True).stdout
    return float(json.loads(out.strip().splitlines()[-1])["ms_per_step"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[16, 256, 4096])
    ap.add_argument("--windows", type=int, default=10)
    ap.add_argument("--replays", type=int, default=32)
    ap.add_argument("--decay", type=float, default=0.999)
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--headline-runs", type=int, default=4)
    ap.add_argument("--headline-only", action="store_true", help="skip everything but the --parent-tree comparison")
    ap.add_argument("--headline-args", nargs=argparse.REMAINDER, default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("average_timing.py measures on the GPU: none found")
    if not args.headline_only:
        _captured(args)
    if args.parent_tree:
        extra = args.headline_args if args.headline_args else ["--gpus", "1", "--full"]
        ms = {"this": [], "parent": []}
        for run in range(args.headline_runs):
            for name, tree in (("this", REPO), ("parent", os.path.abspath(args.parent_tree))):
                v = _headline(tree, extra)
                ms[name].append(v)
                print(json.dumps({"what": "headline", "tree": name, "run": run, "ms_per_step": v, "args": extra}), flush=True)
        print(json.dumps({"what": "headline_summary", "args": extra, "ms_per_step": ms,
                          "median": {k: round(statistics.median(v), 4) for k, v in ms.items()}}), flush=True)


def _captured(args):
    from torch.optim.swa_utils import AveragedModel, get_ema_multi_avg_fn
    from molkgnn_amd.optim import FusedAdamW
    from molkgnn_amd.synthetic import make_batch
    from molkgnn_amd.train import CapturedSteps, GNNModel, configure_optimizer, training_step, tune_torch_backends

    class FusedThenTorchEma(FusedAdamW):
        """The unaveraged fused step, then ``AveragedModel``'s EMA update of every parameter (no read-back: capturable)."""

        def attach(self, model):
            self.ema_fn = get_ema_multi_avg_fn(args.decay)
            self.swa = AveragedModel(model, multi_avg_fn=self.ema_fn)
            self.swa.update_parameters(model)                # the first call copies, eagerly
            self.avg_list = [p.detach() for p in self.swa.module.parameters()]
            self.cur_list = [p.detach() for p in model.parameters()]

        def step(self, closure=None):
            loss = super().step(closure)
            self.ema_fn(self.avg_list, self.cur_list, self.swa.n_averaged)
            return loss

    def optimizer(model, route):
        if route == "torch_ema":
            opt = FusedThenTorchEma(configure_optimizer(model, lr=1e-4).param_groups)
            opt.prepare_state()
            opt.attach(model)
            return opt
        return configure_optimizer(model, lr=1e-4, average="ema" if route == "averaged" else None, average_decay=args.decay)

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
            for _ in range(4):
                steps(batch)
            torch.cuda.synchronize()
            assert len(steps._graphs) == 1, "the step was not captured"
            runs[route] = (model, steps)
        times = _turns({r: (lambda s=runs[r][1]: s(batch)) for r in ROUTES}, args.windows, args.replays, args.replays,
                       lambda r, w, ms: print(json.dumps({"what": "captured_step", "batch": B, "route": r, "window": w,
                                                          "ms_per_step": round(ms, 5), "replays": args.replays}), flush=True))
        s = _summary(times)
        print(json.dumps({"what": "summary", "batch": B, "ms_per_step": s,
                          "averaged_minus_unaveraged_us": round(1e3 * (s["averaged"]["median"] - s["unaveraged"]["median"]), 2),
                          "torch_ema_minus_unaveraged_us": round(1e3 * (s["torch_ema"]["median"] - s["unaveraged"]["median"]), 2),
                          "averaged_over_unaveraged": round(s["averaged"]["median"] / s["unaveraged"]["median"], 4),
                          "averaged_over_torch_ema": round(s["averaged"]["median"] / s["torch_ema"]["median"], 4)}), flush=True)
        del runs

    # the optimiser launches alone, over the gradients one step leaves behind: --replays calls in one graph
    batch = make_batch(args.batches[0], seed=args.batches[0]).to(dev)
    graphs, keep = {}, []
    for route in ROUTES:
        model = copy.deepcopy(model0)
        opt = optimizer(model, route)
        training_step(model, batch, opt)                     # gradients exist; the kernels' first launch is an eager one
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(args.replays):
                opt.step()
        graphs[route] = g
        keep.append((model, opt))
    times = _turns({r: g.replay for r, g in graphs.items()}, args.windows, 1, 4,
                   lambda r, w, ms: print(json.dumps({"what": "optimizer_only", "route": r, "window": w,
                                                      "us_per_call": round(1e3 * ms / args.replays, 3), "calls_per_graph": args.replays}), flush=True))
    s = _summary({r: [1e3 * v / args.replays for v in vs] for r, vs in times.items()}, 3)
    print(json.dumps({"what": "optimizer_only_summary", "us_per_call": s}), flush=True)

    # swap_averaged alone
    model, opt = keep[ROUTES.index("averaged")]
    opt.swap_averaged()
    opt.swap_averaged()
    torch.cuda.synchronize()
    calls = args.replays + args.replays % 2
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(calls):
            opt.swap_averaged()
    times = _turns({"swap_averaged": g.replay}, args.windows, 1, 4,
                   lambda r, w, ms: print(json.dumps({"what": "swap_only", "window": w, "us_per_call": round(1e3 * ms / calls, 3),
                                                      "calls_per_graph": calls}), flush=True))
    print(json.dumps({"what": "swap_only_summary", "floats": sum(p.numel() for p in model.parameters()),
                      "us_per_call": _summary({"swap_averaged": [1e3 * v / calls for v in times["swap_averaged"]]}, 3)}), flush=True)
    del graphs, keep, g
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
