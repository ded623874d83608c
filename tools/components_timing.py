"""What the neighbour lists and the linked components cost: ``mkgnn_embed_neighbours_within`` (the fill) beside
``mkgnn_embed_count_within`` on the same tensors and beside the same lists through torch operators, ``mkgnn_graph_components`` on the
self-joins' lists, and ``screening.cluster_components_embeddings`` end to end.

    python tools/components_timing.py [--pairs 4096x16384 256x1024] [--rows 1024 65536] [--width 32] [--min-sim 0.9]
                                      [--windows 10] [--steps 8] [--end-windows 3]

Clustered embeddings as in ``tools/butina_timing.py`` (``n // 6`` random centres, rows = centre + 0.08 noise at a random scale).

``pairs``  per ``n x R``: the count once (for the row pointers and ``nnz``), then three pieces of work take turns in ONE process, window
           by window -- ``count`` (``chain`` calls of ``mkgnn_embed_count_within`` back to back, captured), ``fill`` (as many raw calls of
           ``mkgnn_embed_neighbours_within`` into lists of ``nnz`` slots, captured: a split call walks the references twice, count
           policy then fill policy, an unsplit one once) and ``torch`` (normalise both sets, one ``matmul`` per chunk of references,
           compare, ``nonzero``, concatenate -- the only route there was; ``nonzero`` reads its size on the host, so this one cannot be
           captured and runs eagerly, with its host work inside the window); per call, the median of ``--windows`` windows of
           ``--steps`` rounds (device events); and whether the torch lists name the same pairs as the kernel's
``rows``   per ``n``: the self-join (``refs`` is ``emb``) the same way; then ``mkgnn_graph_components`` on its lists (one captured raw call:
           all the rounds it enqueues, those behind the last changing one returning at once) with the rounds that changed a label;
           then ``cluster_components_embeddings`` end to end (count, cumsum, fill, components, sizes; it reads ``nnz``, the
           components' state and their number on the host, so: a host clock around a synchronise, the median of ``--end-windows`` runs
           after one warm-up)

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


def torch_lists(emb, refs, min_sim):
    """The lists in torch operators: normalise, one ``matmul`` per chunk of references, compare, ``nonzero`` -> ``(rows, refs)`` int64,
    chunk by chunk (within a chunk by row, then by reference)."""
    import torch
    e = torch.nn.functional.normalize(emb, dim=1, eps=1e-8)
    q = e if refs is emb else torch.nn.functional.normalize(refs, dim=1, eps=1e-8)
    chunk = torch_chunk(emb.shape[0])
    rows, cols = [], []
    for a in range(0, q.shape[0], chunk):
        hit = (e @ q[a:a + chunk].t() > min_sim).nonzero()
        rows.append(hit[:, 0])
        cols.append(hit[:, 1] + a)
    return torch.cat(rows), torch.cat(cols)


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


def take_turns(work, chain, windows, steps):
    """``{name: [ms per call, one per window]}``: the pieces of work take turns window by window, so drift hits them alike.  A
    captured graph holds ``chain`` calls and is replayed; a plain function (what cannot be captured) is called ``chain`` times."""
    import torch
    ms = {name: [] for name in work}
    for _ in range(windows):
        for name, item in work.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(steps):
                if isinstance(item, torch.cuda.CUDAGraph):
                    item.replay()
                else:
                    for _ in range(chain):
                        item()
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


def host_ms(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    result = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, result


def time_lists(emb, refs, H, min_sim, windows, steps, dev, measure):
    """The fill against the count and the torch route on one pair of tensors: the JSON line, and the kernel's lists."""
    import torch
    from molkgnn_amd import _lib
    from molkgnn_amd.readout import embedding_count_within, embedding_neighbours_within
    n, R = emb.shape[0], refs.shape[0]
    counts = embedding_count_within(emb, refs, min_sim)
    row_ptr = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    row_ptr[1:] = torch.cumsum(counts, dim=0, dtype=torch.int64)
    nnz = int(row_ptr[n])
    out = (torch.empty(nnz, dtype=torch.int32, device=dev), torch.empty(nnz, dtype=torch.float32, device=dev))
    found = torch.empty(n, dtype=torch.int32, device=dev)
    spare = torch.empty(n, dtype=torch.int32, device=dev)
    chain = chain_for(n, R)
    work = {"count": capture(lambda: embedding_count_within(emb, refs, min_sim, out=spare), chain, dev),
            "fill": capture(lambda: embedding_neighbours_within(emb, refs, min_sim, row_ptr=row_ptr, out=out, found=found), chain, dev),
            "torch": lambda: torch_lists(emb, refs, min_sim)}
    work["torch"]()                                                # (its warm-up)
    line = {"measure": measure, "rows": n, "refs": R, "width": H, "min_sim": min_sim, "chain": chain, "steps": steps, "nnz": nnz,
            "mean_list": round(nnz / n, 3), "parts": _lib.count_within_split(n, R)[1], "torch_chunk": torch_chunk(n),
            "torch_captured": False}
    line.update(report(take_turns(work, chain, windows, steps)))
    line["fill_over_count"] = round(line["fill_ms"] / line["count_ms"], 3)
    line["torch_over_fill"] = round(line["torch_ms"] / line["fill_ms"], 3)
    line["torch_over_count_plus_fill"] = round(line["torch_ms"] / (line["count_ms"] + line["fill_ms"]), 3)
    line["found_is_count"] = bool(torch.equal(found, counts))
    rows, cols = torch_lists(emb, refs, min_sim)
    order = torch.sort(rows, stable=True).indices
    line["torch_lists_agree"] = bool(rows.numel() == nnz and torch.equal(cols[order].int(), out[0]))
    return line, row_ptr, out[0]


def time_components(row_ptr, col, n, windows, steps, dev):
    import torch
    from molkgnn_amd import _lib
    from molkgnn_amd.readout import graph_components
    labels = torch.empty(n, dtype=torch.int32, device=dev)
    state = torch.empty(4, dtype=torch.int32, device=dev)
    work = {"components": capture(lambda: graph_components(row_ptr, col, n, out=labels, state=state), 1, dev)}
    line = report(take_turns(work, 1, windows, steps))
    rounds, converged, skipped, _ = state.tolist()
    line.update({"changing_rounds": rounds, "enqueued_rounds": _lib.components_rounds(n), "converged": bool(converged),
                 "skipped_input": bool(skipped), "n_components": int(torch.unique(labels).numel())})
    return line


def time_self(n, H, min_sim, windows, steps, end_windows, dev):
    from molkgnn_amd.screening import cluster_components_embeddings
    emb = clustered(n, H, 1000 + n, dev)
    line, row_ptr, col = time_lists(emb, emb, H, min_sim, windows, steps, dev, "self_join")
    line["pairs"] = n * n
    print(json.dumps(line), flush=True)
    comp = {"measure": "components", "rows": n, "width": H, "min_sim": min_sim, "nnz": line["nnz"]}
    comp.update(time_components(row_ptr, col, n, windows, steps, dev))
    print(json.dumps(comp), flush=True)
    end = {"measure": "cluster_components", "rows": n, "width": H, "min_sim": min_sim}
    cluster_components_embeddings(emb, min_sim)                    # (the warm-up of this shape)
    ms = []
    for _ in range(end_windows):
        t, result = host_ms(lambda: cluster_components_embeddings(emb, min_sim))
        ms.append(t)
    end["end_to_end_ms"] = round(statistics.median(ms), 3)
    end["end_to_end_windows_ms"] = [round(v, 3) for v in ms]
    end["n_components"] = result["n_components"]
    end["largest_component"] = int(result["component_size"].max())
    print(json.dumps(end), flush=True)
    return line, comp, end


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", nargs="*", default=["4096x16384", "256x1024"], help="rows x references")
    ap.add_argument("--rows", type=int, nargs="*", default=[1024, 65536], help="self-joins")
    ap.add_argument("--width", type=int, default=32)
    ap.add_argument("--min-sim", type=float, default=0.9)
    ap.add_argument("--windows", type=int, default=10)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--end-windows", type=int, default=3)
    a = ap.parse_args()
    sys.path.insert(0, REPO)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("components_timing.py measures on the GPU: none is available (nothing is measured on the CPU)")
    from molkgnn_amd.train import tune_torch_backends
    dev = torch.device("cuda:0")
    tune_torch_backends()
    pairs, joins, comps, ends = [], [], [], []
    for text in a.pairs:
        n, R = (int(v) for v in text.lower().split("x"))
        pool = clustered(n + R, a.width, 2000 + n + R, dev)
        line, _, _ = time_lists(pool[:n].contiguous(), pool[n:].contiguous(), a.width, a.min_sim, a.windows, a.steps, dev, "pair")
        print(json.dumps(line), flush=True)
        pairs.append(line)
    for n in a.rows:
        line, comp, end = time_self(n, a.width, a.min_sim, a.windows, a.steps, a.end_windows, dev)
        joins.append(line)
        comps.append(comp)
        ends.append(end)
    keys = ("rows", "refs", "parts", "nnz", "count_ms", "fill_ms", "torch_ms", "fill_over_count", "torch_over_fill",
            "torch_over_count_plus_fill", "found_is_count", "torch_lists_agree")
    print(json.dumps({"summary": {
        "width": a.width,
        "pair": [{k: r[k] for k in keys} for r in pairs],
        "self_join": [{k: r[k] for k in keys} for r in joins],
        "components": [{k: r[k] for k in ("rows", "nnz", "components_ms", "changing_rounds", "enqueued_rounds", "converged",
                                          "n_components")} for r in comps],
        "cluster_components": [{k: r[k] for k in ("rows", "end_to_end_ms", "n_components", "largest_component")} for r in ends]}}),
        flush=True)


if __name__ == "__main__":
    main()
