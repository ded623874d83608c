"""Time of ``GNNModel.predict`` (evaluation mode, ``torch.no_grad()``) on the forward-only fused tail against the separate
operators it replaces.

    python tools/score_timing.py [--batches 16 256 4096] [--steps 50] [--windows 5] [--warmup 10] [--rounds 2] [--timeout 300]

One JSON line per (batch, route, mode, round): ``ms_per_call`` = the median of ``--windows`` timed windows of ``--steps`` calls each
(device events, after ``--warmup`` untimed calls), with every window in ``windows_ms`` so that the spread is in the line.
Routes: ``score`` (``readout.tail_score``: two launches behind the last convolution) and ``separate`` (``MKGNN_SCORE_TAIL=0``:
``readout_blocks`` or ``readout``, dropout, the head's PyTorch operators -- the route before the score tail existed).  The switch
is read when the package is imported, so every route runs in a child process of its own, under its own ``timeout -k``; the
routes alternate over ``--rounds`` rounds, and nothing is started after a child that failed.  Modes: ``eager`` (launched from
Python every call) and ``replayed`` (a graph this tool captures around ``predict`` once, then replays).  The last line
(``"summary"``) holds, per batch and mode, the medians over all windows of both routes, ``separate``'s own spread
(max - min of its windows) and whether ``score`` is slower than ``separate`` by more than that spread.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROUTES = {"score": {}, "separate": {"MKGNN_SCORE_TAIL": "0"}}


def _windows(fn, steps, windows, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(windows):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(steps):
            fn()
        t1.record()
        torch.cuda.synchronize()
        out.append(t0.elapsed_time(t1) / steps)
    return out


def run_route(route, rnd, batches, steps, windows, warmup):
    import torch
    sys.path.insert(0, REPO)
    from molkgnn_amd import readout as R
    from molkgnn_amd.synthetic import make_batch
    from molkgnn_amd.train import GNNModel, tune_torch_backends
    assert R._SCORE_TAIL == (route == "score")
    dev = torch.device("cuda:0")
    tune_torch_backends()
    taken = []
    real = R.tail_score
    R.tail_score = lambda *a, **k: (taken.append(1), real(*a, **k))[1]
    for B in batches:
        batch = make_batch(B, seed=B, assay="9999").to(dev)
        torch.manual_seed(0)
        model = GNNModel().to(dev).eval()
        for mode in ("eager", "replayed"):
            del taken[:]
            if mode == "eager":
                fn = lambda: model.predict(batch)
                pred, _ = fn()
            else:
                side = torch.cuda.Stream(device=dev)
                side.wait_stream(torch.cuda.current_stream(dev))
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.stream(side), torch.cuda.graph(graph, stream=side):
                    pred, _ = model.predict(batch)
                torch.cuda.current_stream(dev).wait_stream(side)
                fn = graph.replay
                fn()
            assert bool(taken) == (route == "score"), "the route is not the one asked for"
            ms = _windows(fn, steps, windows, warmup)
            print(json.dumps({"batch": B, "route": route, "mode": mode, "round": rnd, "ms_per_call": round(statistics.median(ms), 5),
                              "windows_ms": [round(m, 5) for m in ms], "steps": steps, "pred_sum": float(pred.double().sum())}),
                  flush=True)
        del model


def _summary(lines):
    out = []
    for key in sorted({(r["batch"], r["mode"]) for r in lines}):
        w = {route: [m for r in lines if (r["batch"], r["mode"]) == key and r["route"] == route for m in r["windows_ms"]]
             for route in ROUTES}
        if not all(w.values()):
            continue
        score, sep = statistics.median(w["score"]), statistics.median(w["separate"])
        spread = max(w["separate"]) - min(w["separate"])
        out.append({"batch": key[0], "mode": key[1], "score_ms": round(score, 5), "separate_ms": round(sep, 5),
                    "separate_spread_ms": round(spread, 5), "score_slower_beyond_spread": bool(score > sep + spread)})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[16, 256, 4096])
    ap.add_argument("--routes", nargs="+", default=list(ROUTES))
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--windows", type=int, default=5, help="timed windows per line (at least 3)")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=2, help="the routes alternate this many times")
    ap.add_argument("--timeout", type=int, default=300, help="seconds per child process")
    ap.add_argument("--child", help=argparse.SUPPRESS)
    ap.add_argument("--round", type=int, default=0, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.windows < 3:
        ap.error("--windows: at least 3, so that the spread is in the line")
    if args.child:
        run_route(args.child, args.round, args.batches, args.steps, args.windows, args.warmup)
        return
    lines = []
    for rnd in range(args.rounds):
        for route in args.routes:
            env = dict(os.environ, **ROUTES[route])
            cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--child", route, "--round",
                   str(rnd), "--steps", str(args.steps), "--windows", str(args.windows), "--warmup", str(args.warmup), "--batches",
                   *map(str, args.batches)]
            done = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True)
            sys.stdout.write(done.stdout)
            sys.stdout.flush()
            if done.returncode != 0:              # (a failed child ends the run: nothing more is started on the GPU)
                print(json.dumps({"route": route, "round": rnd, "error": f"exit status {done.returncode}"}), flush=True)
                sys.exit(124 if done.returncode in (124, 137) else 1)
            lines += [json.loads(ln) for ln in done.stdout.splitlines() if ln.startswith("{")]
    print(json.dumps({"summary": _summary(lines)}), flush=True)


if __name__ == "__main__":
    main()
