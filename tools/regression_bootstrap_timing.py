"""What the bootstrap of the regression metrics costs, against the only route there was and against the classification bootstrap on
tensors of the same size, in one process, the routes taking turns window by window.

    python tools/regression_bootstrap_timing.py [--folds 16384 65536 1048576] [--n-boot 1000] [--loop-replicates 8] [--windows 10] [--steps 2]
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/regression_bootstrap_timing.py --passes-only [--folds ...] [--n-boot 1000]

Per fold of ``n`` synthetic molecules (a docking-score-like truth, a prediction that follows it, both float32 so that both orders
have ties at large ``n``), with ONE cut (the top 1 %):

``regression`` against ``roc``   ONE ``readout.bootstrap_regression`` on the prepared arrays (the two sorts are outside) against ONE
                                 ``readout.bootstrap_roc`` on ``tools/bootstrap_timing.py``'s fold of the same size -- the same clear and
                                 draw launches, another walk -- each captured into a graph and replayed: device events, the median of
                                 ``--windows`` windows of ``--steps`` replays
``metrics`` against ``loop``     ONE ``evaluation.bootstrap_regression(t, p, n_boot, top=(0.01,))`` end to end (eager: the sorts, the point
                                 estimates and the summary's read-back included) against the route there was: per replicate ``idx =
                                 randint(n)`` on the device, then ``calculate_rmse``, ``calculate_mae``, ``calculate_r2``,
                                 ``calculate_pearson``, ``calculate_spearman`` and ``calculate_top_recall`` on the gathered vectors.
                                 ``--loop-replicates`` replicates are timed; ``loop_ms_at_n_boot`` is that figure times ``n_boot`` -- an
                                 extrapolation, named as one.  ``loop_one_pass`` is the same loop with ONE ``regression_points`` per replicate
                                 (two sorts instead of ten): the fairest form of the loop

``--passes-only`` launches the raw operator a few times per fold and nothing else: under ``rocprofv3 --kernel-trace --stats`` (a run of
its own) the statistics give ``bootstrap_regression_walk_kernel`` beside the shared ``bootstrap_clear_kernel`` and
``bootstrap_draw_kernel``.  The walk's three sweeps are one kernel: a trace cannot split them.

One JSON line per fold with every window, then a summary line.  Nothing is measured without a GPU."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bootstrap_timing import capture, fold, prepared, window_ms  # noqa: E402

TOP = 0.01


def regression_fold(n, seed, dev):
    """``(t float32 [n], p float32 [n])`` on ``dev``: truths of a few units, predictions that follow them."""
    import torch
    g = torch.Generator().manual_seed(seed)
    t = (torch.randn(n, generator=g) * 2.0 - 8.0).float()
    p = (t + 0.7 * torch.randn(n, generator=g)).float()
    return t.to(dev), p.to(dev)


def inputs(n, dev):
    import torch
    from molkgnn_amd import evaluation as E
    t, p = regression_fold(n, 5000 + n, dev)
    arrays = E.regression_prepare(t, p, True)
    centre = torch.stack([p.double().mean(), t.double().mean()])
    cuts = torch.tensor([E.early_cut(TOP, n)], dtype=torch.int32, device=dev)
    return t, p, arrays, centre, cuts


def time_case(n, n_boot, loop_replicates, windows, steps, dev):
    import torch
    from molkgnn_amd import evaluation as E
    from molkgnn_amd.readout import bootstrap_regression, bootstrap_regression_replicates_per_pass, bootstrap_roc
    t, p, arrays, centre, cuts = inputs(n, dev)
    y, s = fold(n, 3000 + n, dev)
    rank, y_sorted, group_last, split = prepared(y, s, False)
    state = {}

    def roc():
        state["roc"] = bootstrap_roc(rank, y_sorted, group_last, split, n_boot, 0, 0, 0.001, 0.1)

    def regression():
        state["regression"] = bootstrap_regression(*arrays, centre, cuts, n_boot, 0, 0)

    def metrics():
        state["metrics"] = E.bootstrap_regression(t, p, n_boot=n_boot, top=(TOP,))

    def loop():
        out = []
        for _ in range(loop_replicates):
            idx = torch.randint(0, n, (n,), device=dev)
            tb, pb = t[idx], p[idx]
            out.append((E.calculate_rmse(tb, pb), E.calculate_mae(tb, pb), E.calculate_r2(tb, pb), E.calculate_pearson(tb, pb),
                        E.calculate_spearman(tb, pb), E.calculate_top_recall(tb, pb, TOP)))
        state["loop"] = out

    def loop_one_pass():
        out = []
        for _ in range(loop_replicates):
            idx = torch.randint(0, n, (n,), device=dev)
            out.append(E.regression_points(t[idx], p[idx], (TOP,)))
        state["loop_one_pass"] = out

    metrics()
    loop()
    loop_one_pass()
    roc_graph, roc_why = capture(roc, dev)
    reg_graph, reg_why = capture(regression, dev)
    ms = {"roc": [], "regression": [], "metrics": [], "loop": [], "loop_one_pass": []}
    for _ in range(windows):                                       # (the routes take turns: drift hits them alike)
        ms["roc"].append(window_ms(roc_graph, roc, steps))
        ms["regression"].append(window_ms(reg_graph, regression, steps))
        ms["metrics"].append(window_ms(None, metrics, steps))
        ms["loop"].append(window_ms(None, loop, 1))
        ms["loop_one_pass"].append(window_ms(None, loop_one_pass, 1))
    med = {k: statistics.median(v) for k, v in ms.items()}
    m = state["metrics"]
    per_replicate, per_replicate_one = med["loop"] / loop_replicates, med["loop_one_pass"] / loop_replicates
    names = ("RMSE", "MAE", "R2", "pearson", "spearman", E.top_name(TOP))
    line = {"rows": n, "n_boot": n_boot, "replicates_per_pass": bootstrap_regression_replicates_per_pass(n, n_boot),
            "cuts": [int(v) for v in cuts.cpu()], "roc_ms": round(med["roc"], 3), "regression_ms": round(med["regression"], 3),
            "regression_over_roc": round(med["regression"] / med["roc"], 3), "captured": roc_graph is not None and reg_graph is not None,
            "capture_error": roc_why or reg_why, "metrics_ms": round(med["metrics"], 3), "loop_replicates": loop_replicates,
            "loop_ms_per_replicate": round(per_replicate, 3), "loop_ms_at_n_boot": round(per_replicate * n_boot, 1),
            "loop_at_n_boot_over_metrics": round(per_replicate * n_boot / med["metrics"], 1),
            "loop_one_pass_ms_per_replicate": round(per_replicate_one, 3),
            "loop_one_pass_ms_at_n_boot": round(per_replicate_one * n_boot, 1),
            "loop_one_pass_at_n_boot_over_metrics": round(per_replicate_one * n_boot / med["metrics"], 1), "windows": windows,
            "steps": steps, "point": {k: m["point"][k] for k in names}, "ci": {k: m[k]["ci"] for k in names},
            "n_undefined": m["n_undefined"]}
    line.update({k + "_windows_ms": [round(v, 3) for v in v_] for k, v_ in ms.items()})
    return line


def passes_only(n, n_boot, repeats, dev):
    import torch
    from molkgnn_amd.readout import bootstrap_regression, bootstrap_regression_replicates_per_pass
    _, _, arrays, centre, cuts = inputs(n, dev)
    for _ in range(repeats):
        bootstrap_regression(*arrays, centre, cuts, n_boot, 0, 0)
    torch.cuda.synchronize()
    return {"rows": n, "n_boot": n_boot, "replicates_per_pass": bootstrap_regression_replicates_per_pass(n, n_boot), "calls": repeats}


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
        raise SystemExit("regression_bootstrap_timing.py measures on the GPU: none is available (nothing is measured on the CPU)")
    dev = torch.device("cuda:0")
    lines = []
    for n in a.folds:
        line = passes_only(n, a.n_boot, a.repeats, dev) if a.passes_only else time_case(n, a.n_boot, a.loop_replicates, a.windows,
                                                                                       a.steps, dev)
        print(json.dumps(line), flush=True)
        lines.append(line)
    if not a.passes_only:
        keys = ("rows", "replicates_per_pass", "roc_ms", "regression_ms", "regression_over_roc", "metrics_ms", "loop_replicates",
                "loop_ms_per_replicate", "loop_ms_at_n_boot", "loop_at_n_boot_over_metrics", "loop_one_pass_ms_per_replicate",
                "loop_one_pass_ms_at_n_boot", "loop_one_pass_at_n_boot_over_metrics")
        print(json.dumps({"summary": [{key: r[key] for key in keys} for r in lines]}), flush=True)


if __name__ == "__main__":
    main()
