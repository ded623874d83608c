"""What a bootstrap of AUC and logAUC costs: ``evaluation.bootstrap_metrics`` (one sort, then ``mkgnn_bootstrap_roc``) against the
only route there was -- a Python loop per replicate over ``evaluation.calculate_auc`` / ``calculate_logAUC`` on ``y[idx], s[idx]`` --
on the same tensors, in one process, the routes taking turns window by window.

    python tools/bootstrap_timing.py [--folds 16384 65536 1048576] [--n-boot 1000] [--loop-replicates 8] [--windows 10] [--steps 2]
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bootstrap_timing.py --passes-only [--folds ...] [--n-boot 1000]

Per fold of ``n`` synthetic molecules at 0.5 % actives (scores: a standard normal, the actives shifted up by 1.5, rounded to float32
as a model's are), unstratified and stratified:

``metrics``  ONE ``evaluation.bootstrap_metrics(y, s, n_boot)`` end to end, eager (it reads the class counts, the point estimates
             and the summary back: it cannot be captured): host clock around a synchronise, the median of ``--windows`` windows of
             ``--steps`` calls
``kernel``   ONE ``readout.bootstrap_roc`` on the prepared ``rank``, ``y_sorted``, ``group_last`` (the sort is outside), captured into a
             graph and replayed: device events, the median of ``--windows`` windows of ``--steps`` replays.  Which form ran (LDS, or
             the passes over the workspace and how many replicates one pass holds) is in the line
``loop``     ``--loop-replicates`` replicates of the loop: ``idx = randint(n)`` on the device, then the two existing functions on the
             gathered vectors (a device sort, several ``nonzero`` and a dozen host reads each).  Eager because it cannot be captured;
             host clock around a synchronise, the median of ``--windows`` windows.  ``loop_ms_per_replicate`` is what was measured,
             ``loop_ms_at_n_boot`` that figure times ``n_boot`` -- an extrapolation, named as one

``--passes-only`` launches the raw operator a few times per fold and nothing else: run under ``rocprofv3 --kernel-trace --stats`` (a
run of its own) the statistics give the clear, draw-and-count and walk launches each alone, by kernel name
(``bootstrap_clear_kernel``, ``bootstrap_draw_kernel``, ``bootstrap_walk_kernel``, ``bootstrap_lds_kernel``).

One JSON line per measurement with every window, then a summary line.  Nothing is measured without a GPU."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def fold(n, seed, dev):
    """``(y int64 [n], s float32 [n])`` on ``dev``: 0.5 % actives, the actives' scores shifted up by 1.5."""
    import torch
    g = torch.Generator().manual_seed(seed)
    y = torch.zeros(n, dtype=torch.int64)
    y[torch.randperm(n, generator=g)[:max(2, n // 200)]] = 1
    s = (torch.randn(n, generator=g) + 1.5 * y).float()
    return y.to(dev), s.to(dev)


def capture(fn, dev):
    """``fn`` run once on a side stream, then captured there: the graph, or None with the reason when the capture fails."""
    import torch
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    try:
        with torch.cuda.stream(side):
            fn()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=side):
                fn()
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize()
        return graph, None
    except Exception as exc:                                       # (reported in the line: the route is then timed eagerly)
        torch.cuda.synchronize()
        return None, f"{type(exc).__name__}: {exc}"[:200]


def window_ms(graph, fn, steps):
    import torch
    if graph is None:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / steps
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(steps):
        graph.replay()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / steps


def prepared(y, s, stratified):
    import torch
    from molkgnn_amd import evaluation as E
    return E.bootstrap_prepare(y == 1, s.to(torch.float64), stratified)


def form_of(n, n_boot):
    from molkgnn_amd import _lib
    from molkgnn_amd.readout import bootstrap_roc_replicates_per_pass
    if n <= _lib.BOOTSTRAP_LDS_MAX_N:
        return "LDS", None
    return "workspace", bootstrap_roc_replicates_per_pass(n, min(n_boot, _lib.BOOTSTRAP_MAX_REPLICATES))


def time_case(n, stratified, n_boot, loop_replicates, windows, steps, dev):
    import torch
    from molkgnn_amd import evaluation as E
    from molkgnn_amd.readout import bootstrap_roc
    y, s = fold(n, 3000 + n, dev)
    rank, y_sorted, group_last, split = prepared(y, s, stratified)
    state = {}

    def metrics():
        state["metrics"] = E.bootstrap_metrics(y, s, n_boot=n_boot, stratified=stratified)

    def kernel():
        state["kernel"] = bootstrap_roc(rank, y_sorted, group_last, split, n_boot, 0, 0, 0.001, 0.1)

    def loop():
        out = []
        for _ in range(loop_replicates):
            idx = torch.randint(0, n, (n,), device=dev)
            yb, sb = y[idx], s[idx]
            out.append((E.calculate_auc(yb, sb), E.calculate_logAUC(yb, sb)))
        state["loop"] = out

    metrics()
    loop()
    kernel_graph, kernel_why = capture(kernel, dev)
    ms = {"metrics": [], "kernel": [], "loop": []}
    for _ in range(windows):                                       # (the routes take turns: drift hits them alike)
        ms["metrics"].append(window_ms(None, metrics, steps))
        ms["kernel"].append(window_ms(kernel_graph, kernel, steps))
        ms["loop"].append(window_ms(None, loop, 1))
    med = {k: statistics.median(v) for k, v in ms.items()}
    form, per_pass = form_of(n, n_boot)
    m = state["metrics"]
    per_replicate = med["loop"] / loop_replicates
    return {"rows": n, "actives": int((y == 1).sum()), "stratified": stratified, "n_boot": n_boot, "form": form,
            "replicates_per_pass": per_pass, "metrics_ms": round(med["metrics"], 3),
            "metrics_windows_ms": [round(v, 3) for v in ms["metrics"]], "kernel_ms": round(med["kernel"], 3),
            "kernel_windows_ms": [round(v, 3) for v in ms["kernel"]], "kernel_captured": kernel_graph is not None,
            "kernel_capture_error": kernel_why, "loop_replicates": loop_replicates,
            "loop_ms_per_replicate": round(per_replicate, 3), "loop_windows_ms": [round(v, 3) for v in ms["loop"]],
            "loop_ms_at_n_boot": round(per_replicate * n_boot, 1), "loop_at_n_boot_over_metrics": round(per_replicate * n_boot / med["metrics"], 1),
            "windows": windows, "steps": steps, "point_logAUC": m["point"]["logAUC"], "ci_logAUC": m["logAUC"]["ci"],
            "n_undefined": m["n_undefined"]}


def passes_only(n, stratified, n_boot, repeats, dev):
    import torch
    from molkgnn_amd.readout import bootstrap_roc
    y, s = fold(n, 3000 + n, dev)
    rank, y_sorted, group_last, split = prepared(y, s, stratified)
    for _ in range(repeats):
        bootstrap_roc(rank, y_sorted, group_last, split, n_boot, 0, 0, 0.001, 0.1)
    torch.cuda.synchronize()
    form, per_pass = form_of(n, n_boot)
    return {"rows": n, "stratified": stratified, "n_boot": n_boot, "form": form, "replicates_per_pass": per_pass, "calls": repeats}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--folds", type=int, nargs="*", default=[16384, 65536, 1 << 20])
    ap.add_argument("--n-boot", type=int, default=1000)
    ap.add_argument("--loop-replicates", type=int, default=8)
    ap.add_argument("--windows", type=int, default=10)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--passes-only", action="store_true", help="only launch the raw operator (for a kernel trace)")
    ap.add_argument("--repeats", type=int, default=3, help="calls per fold with --passes-only")
    a = ap.parse_args()
    sys.path.insert(0, REPO)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bootstrap_timing.py measures on the GPU: none is available (nothing is measured on the CPU)")
    dev = torch.device("cuda:0")
    lines = []
    for n in a.folds:
        for stratified in (False, True):
            if a.passes_only:
                line = passes_only(n, stratified, a.n_boot, a.repeats, dev)
            else:
                line = time_case(n, stratified, a.n_boot, a.loop_replicates, a.windows, a.steps, dev)
            print(json.dumps(line), flush=True)
            lines.append(line)
    if not a.passes_only:
        keys = ("rows", "stratified", "form", "replicates_per_pass", "metrics_ms", "kernel_ms", "loop_replicates", "loop_ms_per_replicate",
                "loop_ms_at_n_boot", "loop_at_n_boot_over_metrics")
        print(json.dumps({"summary": [{key: r[key] for key in keys} for r in lines]}), flush=True)


if __name__ == "__main__":
    main()
