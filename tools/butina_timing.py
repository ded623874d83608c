"""What the neighbour counts and the Butina clustering cost: ``mkgnn_embed_count_within`` beside ``mkgnn_embed_max_cosine`` (the
same walk) and beside the same count through torch operators, the self-join, and ``screening.cluster_butina_embeddings`` end to end.

    python tools/butina_timing.py [--pairs 4096x16384 256x1024] [--rows 1024 65536] [--once 1048576] [--width 32] [--min-sim 0.9]
                                  [--windows 10] [--steps 8] [--end-windows 3]

Clustered embeddings as in ``tools/diverse_timing.py`` (``n // 6`` random centres, rows = centre + 0.08 noise at a random scale).

``pairs``  per ``n x R``: three graphs captured in ONE process take turns, window by window -- ``count`` (``chain`` calls of
           ``mkgnn_embed_count_within`` back to back), ``max`` (as many of ``mkgnn_embed_max_cosine`` on the same tensors) and ``torch``
           (the count through torch operators: normalise both sets, one ``matmul`` per chunk of references, compare, sum -- the only
           route there was, captured like the others); per call, the median of ``--windows`` windows of ``--steps`` replays (device
           events); and whether the torch counts agree with the kernel's
``rows``   per ``n``: the self-join (``refs`` is ``emb``) the same way, ``count`` against ``torch``; then
           ``cluster_butina_embeddings`` end to end (count, sort, walk, mapping; it reads the number of clusters on the host, so: a
           host clock around a synchronise, the median of ``--end-windows`` runs after one warm-up) beside the same function with the
           torch count in place of the kernel, and whether the two clusterings agree
``once``   per ``n``: the self-join and the clustering ONCE each (one run after a warm-up at 1 024 rows; no windows)

The torch chunk is ``min(4096, 2^30 // n)`` references, so its ``[n, chunk]`` matrix stays at 4 GiB.  One JSON line per measurement
with every window, then a summary line."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def clustered(n, H, seed, dev):
    import torch
    g = torch.Generator().manual_seed(seed)
    centres = torch.randn(max(2, n // 6), H, generator=g)
    rows = centres[torch.randint(0, len(centres), (n,), generator=g)] + 0.08 * torch.randn(n, H, generator=g)
    rows *= torch.exp(torch.empty(n).uniform_(-3.0, 3.0, generator=g))[:, None]
    return rows.to(dev)


def torch_chunk(n):
    return max(1, min(4096, (1 << 30) // max(n, 1)))


def torch_count(emb, refs, min_sim, out):
    """The count in torch operators: normalise, one ``matmul`` per chunk of references, compare, sum -> ``out`` int64 ``[n]``."""
    import torch
    e = torch.nn.functional.normalize(emb, dim=1, eps=1e-8)
    q = e if refs is emb else torch.nn.functional.normalize(refs, dim=1, eps=1e-8)
    out.zero_()
    chunk = torch_chunk(emb.shape[0])
    for a in range(0, q.shape[0], chunk):
        out += (e @ q[a:a + chunk].t() > min_sim).sum(dim=1)
    return out


def capture(fn, chain, dev):
    import torch
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        fn()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            for _ in range(chain):
                fn()
    torch.cuda.current_stream(dev).wait_stream(side)
    graph.replay()
    torch.cuda.synchronize()
    return graph


def take_turns(graphs, chain, windows, steps):
    """``{name: [ms per call, one per window]}``: the graphs take turns window by window, so drift hits them alike."""
    import torch
    ms = {name: [] for name in graphs}
    for _ in range(windows):
        for name, graph in graphs.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(steps):
                graph.replay()
            t1.record()
            torch.cuda.synchronize()
            ms[name].append(t0.elapsed_time(t1) / steps / chain)
    return ms


def chain_for(n, R):
    return 4 if n * R <= 1 << 28 else 1


def report(ms):
    line = {}
    for name, v in ms.items():
        line[f"{name}_ms"] = round(statistics.median(v), 5)
        line[f"{name}_windows_ms"] = [round(x, 5) for x in v]
    return line


def time_pair(n, R, H, min_sim, windows, steps, dev):
    import torch
    from molkgnn_amd.readout import embedding_count_within, embedding_max_cosine
    pool = clustered(n + R, H, 2000 + n + R, dev)
    emb, refs = pool[:n].contiguous(), pool[n:].contiguous()
    counts = torch.empty(n, dtype=torch.int32, device=dev)
    best = (torch.empty(n, dtype=torch.float32, device=dev), torch.empty(n, dtype=torch.int32, device=dev))
    by_torch = torch.empty(n, dtype=torch.int64, device=dev)
    chain = chain_for(n, R)
    graphs = {"count": capture(lambda: embedding_count_within(emb, refs, min_sim, out=counts), chain, dev),
              "max": capture(lambda: embedding_max_cosine(emb, refs, out=best), chain, dev),
              "torch": capture(lambda: torch_count(emb, refs, min_sim, by_torch), chain, dev)}
    line = {"measure": "pair", "rows": n, "refs": R, "width": H, "min_sim": min_sim, "chain": chain, "steps": steps,
            "torch_chunk": torch_chunk(n)}
    line.update(report(take_turns(graphs, chain, windows, steps)))
    line["count_over_max"] = round(line["count_ms"] / line["max_ms"], 3)
    line["torch_over_count"] = round(line["torch_ms"] / line["count_ms"], 3)
    line["mean_count"] = round(float(counts.float().mean()), 3)
    line["torch_counts_agree"] = bool((by_torch == counts.long()).all())
    return line


def butina_by_torch_count(emb, min_sim):
    """``cluster_butina_embeddings`` with the torch count in place of the kernel: ``(centroids, leader)``."""
    import torch
    from molkgnn_amd import screening
    counts = torch_count(emb, emb, min_sim, torch.empty(emb.shape[0], dtype=torch.int64, device=emb.device))
    order = torch.sort(counts, descending=True, stable=True).indices
    picks, name, _, leader, _, _ = screening._walk_in_order(emb, order, min_sim, emb.shape[0], None)
    return name[picks], leader


def host_ms(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    result = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, result


def time_self(n, H, min_sim, windows, steps, end_windows, dev, once):
    import torch
    from molkgnn_amd.readout import embedding_count_within
    from molkgnn_amd.screening import cluster_butina_embeddings
    emb = clustered(n, H, 1000 + n, dev)
    counts = torch.empty(n, dtype=torch.int32, device=dev)
    by_torch = torch.empty(n, dtype=torch.int64, device=dev)
    line = {"measure": "self_join", "rows": n, "width": H, "min_sim": min_sim, "pairs": n * n, "torch_chunk": torch_chunk(n),
            "once": once}
    if once:
        line["count_ms"] = round(host_ms(lambda: embedding_count_within(emb, emb, min_sim, out=counts))[0], 3)
        line["torch_ms"] = round(host_ms(lambda: torch_count(emb, emb, min_sim, by_torch))[0], 3)
    else:
        chain = chain_for(n, n)
        graphs = {"count": capture(lambda: embedding_count_within(emb, emb, min_sim, out=counts), chain, dev),
                  "torch": capture(lambda: torch_count(emb, emb, min_sim, by_torch), chain, dev)}
        line.update({"chain": chain, "steps": steps})
        line.update(report(take_turns(graphs, chain, windows, steps)))
    line["torch_over_count"] = round(line["torch_ms"] / line["count_ms"], 3)
    line["mean_count"] = round(float(counts.float().mean()), 3)
    line["torch_counts_agree"] = bool((by_torch == counts.long()).all())
    print(json.dumps(line), flush=True)
    end = {"measure": "butina", "rows": n, "width": H, "min_sim": min_sim, "once": once}
    runs = {"butina": lambda: cluster_butina_embeddings(emb, min_sim), "butina_torch_count": lambda: butina_by_torch_count(emb, min_sim)}
    results = {}
    for name, fn in runs.items():
        if not once:
            fn()                                                   # (the warm-up of this shape)
        ms = []
        for _ in range(1 if once else end_windows):
            t, results[name] = host_ms(fn)
            ms.append(t)
        end[f"{name}_ms"] = round(statistics.median(ms), 3)
        end[f"{name}_windows_ms"] = [round(v, 3) for v in ms]
    res = results["butina"]
    end["n_clusters"] = int(res["centroids"].numel())
    end["largest_cluster"] = int(res["cluster_size"].max())
    end["same_clusters"] = bool(torch.equal(res["centroids"], results["butina_torch_count"][0])
                                and torch.equal(res["leader"], results["butina_torch_count"][1]))
    print(json.dumps(end), flush=True)
    return line, end


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", nargs="*", default=["4096x16384", "256x1024"], help="rows x references")
    ap.add_argument("--rows", type=int, nargs="*", default=[1024, 65536], help="self-joins measured in windows")
    ap.add_argument("--once", type=int, nargs="*", default=[1 << 20], help="self-joins measured once")
    ap.add_argument("--width", type=int, default=32)
    ap.add_argument("--min-sim", type=float, default=0.9)
    ap.add_argument("--windows", type=int, default=10)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--end-windows", type=int, default=3)
    a = ap.parse_args()
    sys.path.insert(0, REPO)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("butina_timing.py measures on the GPU: none is available (nothing is measured on the CPU)")
    from molkgnn_amd.train import tune_torch_backends
    dev = torch.device("cuda:0")
    tune_torch_backends()
    pairs, joins, ends = [], [], []
    for text in a.pairs:
        n, R = (int(v) for v in text.lower().split("x"))
        line = time_pair(n, R, a.width, a.min_sim, a.windows, a.steps, dev)
        print(json.dumps(line), flush=True)
        pairs.append(line)
    for n, once in [(n, False) for n in a.rows] + [(n, True) for n in a.once]:
        if once and not a.rows:
            time_self(1024, a.width, a.min_sim, 1, 1, 1, dev, False)           # (the warm-up of the code objects)
        line, end = time_self(n, a.width, a.min_sim, a.windows, a.steps, a.end_windows, dev, once)
        joins.append(line)
        ends.append(end)
    print(json.dumps({"summary": {
        "pair": [{k: r[k] for k in ("rows", "refs", "count_ms", "max_ms", "torch_ms", "count_over_max", "torch_over_count",
                                    "torch_counts_agree")} for r in pairs],
        "self_join": [{k: r[k] for k in ("rows", "once", "count_ms", "torch_ms", "torch_over_count", "torch_counts_agree")} for r in joins],
        "butina": [{k: r[k] for k in ("rows", "once", "butina_ms", "butina_torch_count_ms", "n_clusters", "same_clusters")}
                   for r in ends]}}), flush=True)


if __name__ == "__main__":
    main()
