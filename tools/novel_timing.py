"""What the novelty filter costs per batch: the captured step of ``screening.screen_novel`` (``model.predict``, ONE
``mkgnn_embed_max_cosine`` against ``R`` references, ``mkgnn_select_rows``, ``TopK.update`` of the kept rows, the kept count) against
the plain scoring step of ``score_resident``, measured in the same run on a synthetic AID-1798-shaped shard, with K = 1024.

    python tools/novel_timing.py [--batches 256 4096] [--refs 1024 16384] [--k 1024] [--shard-batches 4] [--steps 32]
                                 [--windows 10] [--chain 16]

Per batch size ``B`` and reference count ``R`` four graphs are captured in ONE process and take turns, window by window:

``score``   the step of ``score_resident`` (``model.predict``, ``TopK.update``): what a screen costs without the filter
``novel``   the step of ``screen_novel``: the same network run, then ``readout.embedding_max_cosine``, ``readout.select_rows`` with
            ``max_sim`` at the median similarity of the first batch (about half of every batch is kept), ``TopK.update`` of the kept
            rows, the running total
``torch``   the ``novel`` step with the nearest reference written in torch operators -- normalise both matrices, ``matmul``, ``max``
            (an ``[B, R]`` matrix per batch) -- in place of the kernel
``kernel``  ``--chain`` launches of ``mkgnn_embed_max_cosine`` alone, back to back in one graph, on the embeddings of one batch;
            reported per call

``ms`` is the median of ``--windows`` windows of ``--steps`` replays each (device events; the replays cycle over the shard's
batches, so the list is in its steady state).  One JSON line per (B, R, graph) with every window, then a summary line: the
medians, their spread (max - min), the filter's cost over the plain step and the kernel against the torch operators."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRAPHS = ("score", "novel", "torch", "kernel")


def torch_max_cosine(emb, refs):
    """The nearest reference in torch operators: normalise (each norm clamped at 1e-8), one GEMM, one max."""
    import torch
    sim = torch.nn.functional.normalize(emb, dim=1, eps=1e-8) @ torch.nn.functional.normalize(refs, dim=1, eps=1e-8).t()
    value, index = sim.max(dim=1)
    return value, index.int()


def measure(model, resident, B, R, k, steps, windows, warmup, chain):
    import torch
    from molkgnn_amd.readout import embedding_max_cosine, select_rows
    from molkgnn_amd.screening import TopK, _ScoringStep
    dev = resident.device
    G = model.ffn.in_features
    refs = torch.randn(R, G, generator=torch.Generator().manual_seed(R)).to(dev)
    plain = TopK(k, dev)
    plain.reserve(B)
    score = _ScoringStep(model, resident, B, lambda data: model.predict(data)[0].reshape(-1), (),
                         lambda pred, ids, n_live: plain.update(pred, ids, n_valid=n_live))
    # the references: the embeddings of the first batch's molecules among random rows, so the similarities spread out
    score.run(0)
    emb0 = model.embed(score.csb.data).clone()
    refs[:min(R, B) // 2] = emb0[:min(R, B) // 2]
    sim0, _ = embedding_max_cosine(emb0, refs)
    bounds = torch.tensor([float("-inf"), float(sim0.median())], dtype=torch.float32, device=dev)
    extras = ((torch.float32, float("nan")), (torch.int32, -1))

    def filtered(max_cosine):
        lists = TopK(k, dev)
        lists.reserve(B)
        kept = (torch.empty(B, dtype=torch.float32, device=dev), torch.empty(B, dtype=torch.int32, device=dev),
                torch.empty(1, dtype=torch.int32, device=dev))
        total = torch.zeros(1, dtype=torch.int64, device=dev)

        def predict(data):
            pred, emb = model.predict(data)
            return (pred.reshape(-1), *max_cosine(emb, refs))

        def rank(pred, ids, n_live, sim, arg):
            select_rows(pred, ids, sim, n_live, bounds, out=kept)
            lists.update(kept[0], kept[1], n_valid=kept[2])
            total.add_(kept[2])

        return _ScoringStep(model, resident, B, predict, (), rank, extras), total

    novel, novel_total = filtered(embedding_max_cosine)
    by_torch, torch_total = filtered(torch_max_cosine)
    out = (torch.empty(B, dtype=torch.float32, device=dev), torch.empty(B, dtype=torch.int32, device=dev))
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        embedding_max_cosine(emb0, refs, out=out)
        alone = torch.cuda.CUDAGraph()
        with torch.cuda.graph(alone, stream=side):
            for _ in range(chain):
                embedding_max_cosine(emb0, refs, out=out)
    torch.cuda.current_stream(dev).wait_stream(side)

    nb = len(score)
    runs = {"score": (lambda i: score.run(i % nb), 1), "novel": (lambda i: novel.run(i % nb), 1),
            "torch": (lambda i: by_torch.run(i % nb), 1), "kernel": (lambda i: alone.replay(), chain)}
    for name in GRAPHS:
        for i in range(warmup):
            runs[name][0](i)
    torch.cuda.synchronize()
    ms = {name: [] for name in GRAPHS}
    for _ in range(windows):
        for name in GRAPHS:                              # (the graphs take turns: drift hits them alike)
            run, per = runs[name]
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for i in range(steps):
                run(i)
            t1.record()
            torch.cuda.synchronize()
            ms[name].append(t0.elapsed_time(t1) / steps / per)
    if any(s.csb.gather_status() for s in (score, novel, by_torch)):
        raise RuntimeError("the gather reported a status")
    replays = windows * steps + warmup
    lines = [{"batch": B, "refs": R, "graph": name, "ms": round(statistics.median(ms[name]), 5),
              "windows_ms": [round(v, 5) for v in ms[name]], "steps": steps, "batches_in_shard": nb} for name in GRAPHS]
    lines[1]["kept_share"] = round(int(novel_total) / (replays * B), 4)
    lines[2]["kept_share"] = round(int(torch_total) / (replays * B), 4)
    return lines


def summary(lines):
    out = []
    for B, R in sorted({(r["batch"], r["refs"]) for r in lines}):
        w = {r["graph"]: r["windows_ms"] for r in lines if (r["batch"], r["refs"]) == (B, R)}
        med = {g: statistics.median(w[g]) for g in GRAPHS}
        out.append({"batch": B, "refs": R, **{f"{g}_ms": round(med[g], 5) for g in GRAPHS},
                    **{f"{g}_spread_ms": round(max(w[g]) - min(w[g]), 5) for g in GRAPHS},
                    "novel_minus_score_ms": round(med["novel"] - med["score"], 5),
                    "novel_over_score": round(med["novel"] / med["score"], 3),
                    "torch_minus_novel_ms": round(med["torch"] - med["novel"], 5)})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[256, 4096])
    ap.add_argument("--refs", type=int, nargs="+", default=[1024, 16384])
    ap.add_argument("--k", type=int, default=1024)
    ap.add_argument("--shard-batches", type=int, default=4, help="the shard holds this many batches of the largest size")
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--windows", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--chain", type=int, default=16, help="launches of the kernel alone in one graph")
    a = ap.parse_args()
    sys.path.insert(0, REPO)
    import torch
    from molkgnn_amd import shards as S
    from molkgnn_amd.synthetic import make_batch
    from molkgnn_amd.train import GNNModel, tune_torch_backends
    dev = torch.device("cuda:0")
    tune_torch_backends()
    torch.manual_seed(0)
    model = GNNModel(task_dim=1).to(dev).eval()
    lines = []
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "library.mkgs")
        S.write_shard(path, make_batch(a.shard_batches * max(a.batches), seed=1798000, assay="1798", with_receptive_fields=False))
        resident = S.ResidentShard(path, dev)
        for B in a.batches:
            for R in a.refs:
                for line in measure(model, resident, B, R, a.k, a.steps, a.windows, a.warmup, a.chain):
                    print(json.dumps(line), flush=True)
                    lines.append(line)
    print(json.dumps({"summary": summary(lines)}), flush=True)


if __name__ == "__main__":
    main()
