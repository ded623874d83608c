"""What ranking a resident library in all nine assays costs per batch: the captured scoring step of
``screening.score_resident_tasks`` (a nine-task model, ``TopKTasks.update``: ONE ``mkgnn_topk_update_tasks``) against two things
measured in the same run, on a synthetic AID-1798-shaped shard, with K = 1024.

    python tools/screen_tasks_timing.py [--batches 256 4096] [--k 1024] [--tasks 9] [--shard-batches 4] [--steps 32] [--windows 5]
                                        [--rounds 2] [--timeout 300]

Per batch size the captured step (gather, expand, receptive fields, the model's scoring, scatter, ranking) is timed four ways:

``one``         the one-task step of ``score_resident`` (``model.predict``, ``TopK.update``) -- what a user pays per assay today
``tasks``       the nine-task step (``model.predict_tasks``: the network once, ``mkgnn_task_scores``; one ``TopKTasks.update``)
``columns``     the nine-task step with ``rank`` replaced by what the single-list kernel allows by hand: the ``[B, T]`` scores
                transposed into contiguous columns (one copy) and nine successive ``TopK.update`` calls, one per column
``tasks_none``  the nine-task step without any ranking (what the update itself adds is ``tasks`` - ``tasks_none``)

``ms_per_batch`` is the median of ``--windows`` windows of ``--steps`` replays each (device events; the replays cycle over the
shard's batches, so the lists are in their steady state: most of a batch ranks behind them), every window is in the line.  Each
variant runs in a fresh child process of its own under ``timeout -k``, the variants alternate ``--rounds`` times, and nothing is
started after a child that failed.  The last line holds the summary: medians over all windows of all rounds, the spread of the
one-task step, the nine-task step as a multiple of the one-task step, and the single update against the nine updates."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARIANTS = ("one", "tasks", "columns", "tasks_none")


def child(variant, shard_path, batches, k, n_tasks, steps, windows, warmup):
    import torch
    sys.path.insert(0, REPO)
    from molkgnn_amd import shards as S
    from molkgnn_amd.screening import TopK, TopKTasks, _ScoringStep
    from molkgnn_amd.train import GNNModel, tune_torch_backends
    dev = torch.device("cuda:0")
    tune_torch_backends()
    resident = S.ResidentShard(shard_path, dev)
    torch.manual_seed(0)
    T = 1 if variant == "one" else n_tasks
    model = GNNModel(task_dim=T).to(dev).eval()
    for B in batches:
        if variant == "one":
            lists = [TopK(k, dev)]
            rank = lambda pred, ids, n_live: lists[0].update(pred, ids, n_valid=n_live)               # noqa: E731
        elif variant == "tasks":
            lists = [TopKTasks(k, T, dev)]
            rank = lambda pred, ids, n_live: lists[0].update(pred, ids, n_valid=n_live)               # noqa: E731
        elif variant == "columns":
            lists = [TopK(k, dev) for _ in range(T)]

            def rank(pred, ids, n_live):
                cols = pred.t().contiguous()
                for t in range(T):
                    lists[t].update(cols[t], ids, n_valid=n_live)
        else:
            lists, rank = [], None
        for top in lists:
            top.reserve(B)
        if variant == "one":
            scoring = _ScoringStep(model, resident, B, lambda data: model.predict(data)[0].reshape(-1), (), rank)
        else:
            scoring = _ScoringStep(model, resident, B, lambda data: model.predict_tasks(data)[0], (T,), rank)
        nb = len(scoring)
        for i in range(warmup):
            scoring.run(i % nb)
        torch.cuda.synchronize()
        ms = []
        for _ in range(windows):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for i in range(steps):
                scoring.run(i % nb)
            t1.record()
            torch.cuda.synchronize()
            ms.append(t0.elapsed_time(t1) / steps)
        if scoring.csb.gather_status():
            raise RuntimeError("the gather reported a status")
        # a digest of the lists: `tasks` and `columns` rank the same scores, so their digests agree
        if variant == "tasks":
            mols = lists[0].top_mol.long()
        elif lists:
            mols = torch.stack([top.top_mol for top in lists]).long()
        else:
            mols = torch.full((1, 1), -1, dtype=torch.int64, device=dev)
        print(json.dumps({"batch": B, "variant": variant, "k": k, "tasks": T, "ms_per_batch": round(statistics.median(ms), 5),
                          "windows_ms": [round(v, 5) for v in ms], "steps": steps, "batches_in_shard": nb,
                          "occupied": int((mols >= 0).sum()), "top_mol_sum": int(mols.clamp(min=0).sum())}), flush=True)
        del scoring


def summary(lines):
    out = []
    for B in sorted({r["batch"] for r in lines}):
        w = {v: [m for r in lines if r["batch"] == B and r["variant"] == v for m in r["windows_ms"]] for v in VARIANTS}
        if not all(w.values()):
            continue
        med = {v: statistics.median(w[v]) for v in VARIANTS}
        digests = {v: {(r["occupied"], r["top_mol_sum"]) for r in lines if r["batch"] == B and r["variant"] == v} for v in ("tasks", "columns")}
        tasks = next(r["tasks"] for r in lines if r["batch"] == B and r["variant"] == "tasks")
        out.append({"batch": B, "tasks": tasks, **{f"{v}_ms": round(med[v], 5) for v in VARIANTS},
                    **{f"{v}_spread_ms": round(max(w[v]) - min(w[v]), 5) for v in VARIANTS},
                    "tasks_over_one": round(med["tasks"] / med["one"], 3),
                    "single_update_ms": round(med["tasks"] - med["tasks_none"], 5),
                    "column_updates_ms": round(med["columns"] - med["tasks_none"], 5),
                    "single_update_no_slower": bool(med["tasks"] <= med["columns"]),
                    "same_lists": digests["tasks"] == digests["columns"] and len(digests["tasks"]) == 1})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[256, 4096])
    ap.add_argument("--k", type=int, default=1024)
    ap.add_argument("--tasks", type=int, default=9)
    ap.add_argument("--shard-batches", type=int, default=4, help="the shard holds this many batches of the largest size")
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=2, help="the variants alternate this many times")
    ap.add_argument("--timeout", type=int, default=300, help="seconds per child process")
    ap.add_argument("--child", help=argparse.SUPPRESS)
    ap.add_argument("--shard", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child(a.child, a.shard, a.batches, a.k, a.tasks, a.steps, a.windows, a.warmup)
        return
    sys.path.insert(0, REPO)
    from molkgnn_amd import shards as S
    from molkgnn_amd.synthetic import make_batch
    lines = []
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "library.mkgs")
        S.write_shard(path, make_batch(a.shard_batches * max(a.batches), seed=1798000, assay="1798", with_receptive_fields=False))
        for rnd in range(a.rounds):
            for variant in VARIANTS:
                cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--child", variant, "--shard", path,
                       "--k", str(a.k), "--tasks", str(a.tasks), "--steps", str(a.steps), "--windows", str(a.windows), "--warmup",
                       str(a.warmup), "--batches", *map(str, a.batches)]
                done = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
                sys.stdout.write(done.stdout)
                sys.stdout.flush()
                if done.returncode != 0:              # (a failed child ends the run: nothing more is started on the GPU)
                    print(json.dumps({"variant": variant, "round": rnd, "error": f"exit status {done.returncode}"}), flush=True)
                    sys.exit(124 if done.returncode in (124, 137) else 1)
                lines += [json.loads(ln) for ln in done.stdout.splitlines() if ln.startswith("{")]
    print(json.dumps({"summary": summary(lines)}), flush=True)


if __name__ == "__main__":
    main()
