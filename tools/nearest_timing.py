"""What searching a resident library for the nearest embeddings costs per batch: the captured step of
``screening.nearest_resident`` (``model.embed``, ONE ``mkgnn_embed_cosine``, one ``TopKTasks.update`` over ``Q`` lists) against the
one-task scoring step, measured in the same run on a synthetic AID-1798-shaped shard, with K = 1024.

    python tools/nearest_timing.py [--batches 256 4096] [--k 1024] [--shard-batches 4] [--steps 32] [--windows 5] [--rounds 2]
                                   [--timeout 300]

Per batch size the captured step (gather, expand, receptive fields, the network, scatter, ranking) is timed six ways, all with the
same one-task model:

``one``       the one-task step of ``score_resident`` (``model.predict``, ``TopK.update``) -- what could be done before: the yardstick
``embed``     the embed-only step of ``embed_resident`` (``model.embed``, a ``[B, G]`` scatter, no ranking)
``search9``   the search step at ``Q = 9``: ``readout.embedding_cosine(model.embed(data), queries)`` and one ``TopKTasks.update``
``search32``  the same at ``Q = 32``, the most lists one update takes
``torch9``    the search step at ``Q = 9`` with the cosine written in torch operators
              (``torch.nn.functional.cosine_similarity`` on broadcast views) in place of the kernel
``torch32``   the same at ``Q = 32``

``ms_per_batch`` is the median of ``--windows`` windows of ``--steps`` replays each (device events; the replays cycle over the
shard's batches, so the lists are in their steady state: most of a batch ranks behind them), every window is in the line.  Each
variant runs in a fresh child process of its own under ``timeout -k``, the variants alternate ``--rounds`` times, and nothing is
started after a child that failed.  The last line holds the summary: medians over all windows of all rounds and their spread
(max - min), the search steps as multiples of the one-task step, and the kernel against the torch operators."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARIANTS = ("one", "embed", "search9", "search32", "torch9", "torch32")


def child(variant, shard_path, batches, k, steps, windows, warmup):
    import torch
    sys.path.insert(0, REPO)
    from molkgnn_amd import shards as S
    from molkgnn_amd.readout import embedding_cosine
    from molkgnn_amd.screening import TopK, TopKTasks, _ScoringStep
    from molkgnn_amd.train import GNNModel, tune_torch_backends
    dev = torch.device("cuda:0")
    tune_torch_backends()
    resident = S.ResidentShard(shard_path, dev)
    torch.manual_seed(0)
    model = GNNModel(task_dim=1).to(dev).eval()
    G = model.ffn.in_features
    Q = int(variant[6:]) if variant.startswith("search") else int(variant[5:]) if variant.startswith("torch") else 0
    queries = torch.randn(max(Q, 1), G, generator=torch.Generator().manual_seed(1)).to(dev)
    for B in batches:
        lists = None
        if variant == "one":
            lists = TopK(k, dev)
            lists.reserve(B)
            scoring = _ScoringStep(model, resident, B, lambda data: model.predict(data)[0].reshape(-1), (),
                                   lambda pred, ids, n_live: lists.update(pred, ids, n_valid=n_live))
        elif variant == "embed":
            scoring = _ScoringStep(model, resident, B, model.embed, (G,))
        else:
            lists = TopKTasks(k, Q, dev)
            lists.reserve(B)
            if variant.startswith("search"):
                predict = lambda data: embedding_cosine(model.embed(data), queries)                              # noqa: E731
            else:
                predict = lambda data: torch.nn.functional.cosine_similarity(                                   # noqa: E731
                    model.embed(data)[:, None, :], queries[None, :, :], dim=-1).contiguous()
            scoring = _ScoringStep(model, resident, B, predict, (Q,),
                                   lambda sim, ids, n_live: lists.update(sim, ids, n_valid=n_live))
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
        # a digest of the lists: the kernel and the torch operators rank nearly the same similarities
        mols = lists.top_mol.long() if lists is not None else torch.full((1,), -1, dtype=torch.int64, device=dev)
        seen = min(scoring.n, min(nb, max(steps, warmup)) * B)           # (the replays reach the first `steps` batches only)
        print(json.dumps({"batch": B, "variant": variant, "k": k, "queries": Q, "ms_per_batch": round(statistics.median(ms), 5),
                          "windows_ms": [round(v, 5) for v in ms], "steps": steps, "batches_in_shard": nb,
                          "occupied": int((mols >= 0).sum()), "nan": bool(torch.isnan(scoring.ext[:seen]).any())}), flush=True)
        del scoring


def summary(lines):
    out = []
    for B in sorted({r["batch"] for r in lines}):
        w = {v: [m for r in lines if r["batch"] == B and r["variant"] == v for m in r["windows_ms"]] for v in VARIANTS}
        if not all(w.values()):
            continue
        med = {v: statistics.median(w[v]) for v in VARIANTS}
        out.append({"batch": B, **{f"{v}_ms": round(med[v], 5) for v in VARIANTS},
                    **{f"{v}_spread_ms": round(max(w[v]) - min(w[v]), 5) for v in VARIANTS},
                    "search9_over_one": round(med["search9"] / med["one"], 3),
                    "search32_over_one": round(med["search32"] / med["one"], 3),
                    "cosine_and_update9_ms": round(med["search9"] - med["embed"], 5),
                    "cosine_and_update32_ms": round(med["search32"] - med["embed"], 5),
                    "torch9_minus_kernel_ms": round(med["torch9"] - med["search9"], 5),
                    "torch32_minus_kernel_ms": round(med["torch32"] - med["search32"], 5),
                    "any_nan": any(r["nan"] for r in lines if r["batch"] == B)})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[256, 4096])
    ap.add_argument("--k", type=int, default=1024)
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
        child(a.child, a.shard, a.batches, a.k, a.steps, a.windows, a.warmup)
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
                       "--k", str(a.k), "--steps", str(a.steps), "--windows", str(a.windows), "--warmup", str(a.warmup),
                       "--batches", *map(str, a.batches)]
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
