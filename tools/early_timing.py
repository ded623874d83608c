"""What the early-recognition metrics cost on top of the bootstrap of AUC and logAUC, on the same tensors, in one process, the
routes taking turns window by window.

    python tools/early_timing.py [--folds 16384 65536 1048576] [--n-boot 1000] [--loop-replicates 8] [--windows 10] [--steps 2]
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/early_timing.py --passes-only [--folds ...] [--n-boot 1000]

Per fold of ``n`` synthetic molecules at 0.5 % actives (``tools/bootstrap_timing.py``'s folds), unstratified, with ``J = 2`` cuts
(the enrichment factor at 0.1 % and 1 %) and ``A = 1`` alpha (BEDROC at 20), two comparisons:

``early`` against ``roc``       ONE ``readout.bootstrap_early`` against ONE ``readout.bootstrap_roc`` on the same prepared ``rank``,
                                ``y_sorted``, ``group_last`` (the sort is outside), each captured into a graph and replayed: device
                                events, the median of ``--windows`` windows of ``--steps`` replays.  The clear and draw launches are the
                                same kernels in both, so the difference is what the added work in the walk costs
``metrics`` against ``loop``    ONE ``evaluation.bootstrap_metrics(y, s, n_boot, early=('AP', 'EF_0.001', 'EF_0.01', 'BEDROC_20'))`` end to end
                                (eager: it reads the point estimates and the summary back) against the only route there was: per
                                replicate ``idx = randint(n)`` on the device, then ``calculate_average_precision``, two
                                ``calculate_enrichment_factor`` and ``calculate_bedroc`` on the gathered vectors (a device sort each).
                                ``--loop-replicates`` replicates are timed; ``loop_ms_at_n_boot`` is that figure times ``n_boot`` -- an
                                extrapolation, named as one.  ``metrics_roc_only`` is the same call without ``early``

``--passes-only`` launches the raw operator a few times per fold and nothing else: under ``rocprofv3 --kernel-trace --stats`` (a run of
its own) the statistics give ``bootstrap_walk_early_kernel`` / ``bootstrap_lds_early_kernel`` alone, beside the shared
``bootstrap_clear_kernel`` and ``bootstrap_draw_kernel``.

One JSON line per fold with every window, then a summary line.  Nothing is measured without a GPU."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bootstrap_timing import capture, fold, form_of, prepared, window_ms  # noqa: E402

NAMES = ("AP", "EF_0.001", "EF_0.01", "BEDROC_20")


def inputs(n, dev):
    import torch
    from molkgnn_amd import evaluation as E
    y, s = fold(n, 3000 + n, dev)
    rank, y_sorted, group_last, split = prepared(y, s, False)
    cuts = torch.tensor([E.early_cut(0.001, n), E.early_cut(0.01, n)], dtype=torch.int32, device=dev)
    alphas = torch.tensor([20.0], dtype=torch.float64, device=dev)
    return y, s, rank, y_sorted, group_last, split, cuts, alphas


def time_case(n, n_boot, loop_replicates, windows, steps, dev):
    import torch
    from molkgnn_amd import evaluation as E
    from molkgnn_amd.readout import bootstrap_early, bootstrap_roc
    y, s, rank, y_sorted, group_last, split, cuts, alphas = inputs(n, dev)
    state = {}

    def roc():
        state["roc"] = bootstrap_roc(rank, y_sorted, group_last, split, n_boot, 0, 0, 0.001, 0.1)

    def early():
        state["early"] = bootstrap_early(rank, y_sorted, group_last, split, n_boot, 0, 0, 0.001, 0.1, cuts, alphas)

    def metrics():
        state["metrics"] = E.bootstrap_metrics(y, s, n_boot=n_boot, early=NAMES)

    def metrics_roc_only():
        state["metrics_roc_only"] = E.bootstrap_metrics(y, s, n_boot=n_boot)

    def loop():
        out = []
        for _ in range(loop_replicates):
            idx = torch.randint(0, n, (n,), device=dev)
            yb, sb = y[idx], s[idx]
            out.append((E.calculate_average_precision(yb, sb), E.calculate_enrichment_factor(yb, sb, 0.001),
                        E.calculate_enrichment_factor(yb, sb, 0.01), E.calculate_bedroc(yb, sb, 20.0)))
        state["loop"] = out

    metrics()
    metrics_roc_only()
    loop()
    roc_graph, roc_why = capture(roc, dev)
    early_graph, early_why = capture(early, dev)
    ms = {"roc": [], "early": [], "metrics": [], "metrics_roc_only": [], "loop": []}
    for _ in range(windows):                                       # (the routes take turns: drift hits them alike)
        ms["roc"].append(window_ms(roc_graph, roc, steps))
        ms["early"].append(window_ms(early_graph, early, steps))
        ms["metrics"].append(window_ms(None, metrics, steps))
        ms["metrics_roc_only"].append(window_ms(None, metrics_roc_only, steps))
        ms["loop"].append(window_ms(None, loop, 1))
    med = {k: statistics.median(v) for k, v in ms.items()}
    form, per_pass = form_of(n, n_boot)
    m = state["metrics"]
    per_replicate = med["loop"] / loop_replicates
    line = {"rows": n, "actives": int((y == 1).sum()), "n_boot": n_boot, "form": form, "replicates_per_pass": per_pass,
            "cuts": [int(v) for v in cuts.cpu()], "alphas": [20.0], "roc_ms": round(med["roc"], 3), "early_ms": round(med["early"], 3),
            "early_over_roc": round(med["early"] / med["roc"], 3), "captured": roc_graph is not None and early_graph is not None,
            "capture_error": roc_why or early_why, "metrics_ms": round(med["metrics"], 3),
            "metrics_roc_only_ms": round(med["metrics_roc_only"], 3), "loop_replicates": loop_replicates,
            "loop_ms_per_replicate": round(per_replicate, 3), "loop_ms_at_n_boot": round(per_replicate * n_boot, 1),
            "loop_at_n_boot_over_metrics": round(per_replicate * n_boot / med["metrics"], 1), "windows": windows, "steps": steps,
            "point": {k: m["point"][k] for k in NAMES}, "ci": {k: m[k]["ci"] for k in NAMES}, "n_undefined": m["n_undefined"]}
    line.update({k + "_windows_ms": [round(v, 3) for v in v_] for k, v_ in ms.items()})
    return line


def passes_only(n, n_boot, repeats, dev):
    import torch
    from molkgnn_amd.readout import bootstrap_early
    _, _, rank, y_sorted, group_last, split, cuts, alphas = inputs(n, dev)
    for _ in range(repeats):
        bootstrap_early(rank, y_sorted, group_last, split, n_boot, 0, 0, 0.001, 0.1, cuts, alphas)
    torch.cuda.synchronize()
    form, per_pass = form_of(n, n_boot)
    return {"rows": n, "n_boot": n_boot, "form": form, "replicates_per_pass": per_pass, "calls": repeats}


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
        raise SystemExit("early_timing.py measures on the GPU: none is available (nothing is measured on the CPU)")
    dev = torch.device("cuda:0")
    lines = []
    for n in a.folds:
        line = passes_only(n, a.n_boot, a.repeats, dev) if a.passes_only else time_case(n, a.n_boot, a.loop_replicates, a.windows,
                                                                                       a.steps, dev)
        print(json.dumps(line), flush=True)
        lines.append(line)
    if not a.passes_only:
        keys = ("rows", "form", "replicates_per_pass", "roc_ms", "early_ms", "early_over_roc", "metrics_ms", "metrics_roc_only_ms",
                "loop_replicates", "loop_ms_per_replicate", "loop_ms_at_n_boot", "loop_at_n_boot_over_metrics")
        print(json.dumps({"summary": [{key: r[key] for key in keys} for r in lines]}), flush=True)


if __name__ == "__main__":
    main()
