"""What the analogue search for any number of queries costs: the fused cosine and top-k (``mkgnn_embed_knn_update``) against the
route that was there before, measured in ONE process with the captured graphs taking turns.

    python tools/knn_timing.py [--rows 65536 1048576] [--queries 32 256 2048] [--k 16 64] [--width 32] [--batches 256 4096]
                               [--steps 32] [--windows 10] [--yardstick-launches 5000] [--skip-stored] [--skip-step]

``stored``  the stored-embedding route at ``H = --width`` (32): ``screening.nearest_embeddings`` -- one ``NearestLists.update`` over
            all rows -- against the yardstick ``screening.rank_embeddings`` called per group of 32 queries with its default chunk, a
            ``TopKTasks`` per group, on the same random embeddings.  Both are captured and replayed; the lists are in their steady
            state (a replay feeds the candidates the lists already hold: nothing enters).  A yardstick of more than
            ``--yardstick-launches`` launches per replay is not timed (``null``): it is the measured one times the number of groups.
``step``    the captured screening step (gather, expand, receptive fields, the network, scatter, ranking) per batch: ``embed`` (no
            ranking), ``nearest32`` (``nearest``'s step: ``mkgnn_embed_cosine`` and a ``TopKTasks.update`` at 32 queries) and
            ``many256`` (``nearest_many``'s step: one ``NearestLists.update`` at 256 queries), ``k = 16``.

Every figure is the median of ``--windows`` windows of ``--steps`` replays (device events); within a window round the graphs of a
group are timed one after the other, so drift hits them alike.  One JSON line per measurement, a summary line at the end."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _capture(fn, dev):
    import torch
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        fn()                                             # (eager once: workspaces and lazily made buffers exist)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            fn()
    torch.cuda.current_stream(dev).wait_stream(side)
    return graph


def _take_turns(runs: dict, steps: int, windows: int, warmup: int = 3):
    """``{name: [ms per replay, one per window]}``: per window every entry of ``runs`` (name -> a callable that enqueues one replay
    number ``i``) is timed over ``steps`` replays, one after the other."""
    import torch
    for run in runs.values():
        for i in range(warmup):
            run(i)
    torch.cuda.synchronize()
    ms = {name: [] for name in runs}
    for _ in range(windows):
        for name, run in runs.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for i in range(steps):
                run(i)
            t1.record()
            torch.cuda.synchronize()
            ms[name].append(t0.elapsed_time(t1) / steps)
    return ms


def _line(kind, ms, **what):
    out = {"kind": kind, **what}
    for name, w in ms.items():
        out[f"{name}_ms"] = round(statistics.median(w), 5)
        out[f"{name}_spread_ms"] = round(max(w) - min(w), 5)
    print(json.dumps(out), flush=True)
    return out


def stored(a, dev):
    import torch
    from molkgnn_amd.screening import NearestLists, TopKTasks, nearest_embeddings, rank_embeddings
    H, lines = a.width, []
    gen = torch.Generator(device=dev).manual_seed(0)
    for n in a.rows:
        emb = torch.randn(n, H, generator=gen, device=dev)
        for k in a.k:
            for Q in a.queries:
                queries = torch.randn(Q, H, generator=gen, device=dev)
                new = NearestLists(k, Q, dev)
                new.reserve(min(n, 1 << 20))
                runs = {"knn": _capture(lambda: nearest_embeddings(emb, queries, new), dev).replay}
                groups = -(-Q // 32)
                launches = groups * -(-n // 4096) * 2
                if launches <= a.yardstick_launches:
                    old = [TopKTasks(k, min(32, Q - 32 * g), dev) for g in range(groups)]
                    for t in old:
                        t.reserve(min(4096, n))

                    def yardstick():
                        for g, t in enumerate(old):
                            rank_embeddings(emb, queries[32 * g:32 * g + 32], t)
                    runs["rank_embeddings"] = _capture(yardstick, dev).replay
                ms = _take_turns({name: (lambda i, r=r: r()) for name, r in runs.items()}, a.steps, a.windows)
                same = None
                if "rank_embeddings" in runs:            # the two routes agree, list for list
                    same = all(bool((new.top_mol[32 * g:32 * g + 32] == t.top_mol).all()) and
                               bool((new.top_score[32 * g:32 * g + 32].view(torch.int32) == t.top_score.view(torch.int32)).all())
                               for g, t in enumerate(old))
                line = _line("stored", ms, rows=n, H=H, k=k, queries=Q, yardstick_launches=launches, same_lists=same)
                if "rank_embeddings_ms" in line:
                    line["speedup"] = round(line["rank_embeddings_ms"] / line["knn_ms"], 2)
                lines.append(line)
                del runs, new
    return lines


def step(a, dev):
    import torch
    from molkgnn_amd import shards as S
    from molkgnn_amd.readout import embedding_cosine
    from molkgnn_amd.screening import NearestLists, TopKTasks, _ScoringStep
    from molkgnn_amd.synthetic import make_batch
    from molkgnn_amd.train import GNNModel, tune_torch_backends
    tune_torch_backends()
    lines, k = [], 16
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "library.mkgs")
        S.write_shard(path, make_batch(a.shard_batches * max(a.batches), seed=1798000, assay="1798", with_receptive_fields=False))
        resident = S.ResidentShard(path, dev)
        torch.manual_seed(0)
        model = GNNModel(task_dim=1).to(dev).eval()
        G = model.ffn.in_features
        q256 = torch.randn(256, G, generator=torch.Generator().manual_seed(1)).to(dev)
        q32 = q256[:32].contiguous()
        for B in a.batches:
            many, few = NearestLists(k, 256, dev), TopKTasks(k, 32, dev)
            many.reserve(B)
            few.reserve(B)
            steps = {"embed": _ScoringStep(model, resident, B, model.embed, (G,)),
                     "nearest32": _ScoringStep(model, resident, B, lambda data: embedding_cosine(model.embed(data), q32), (32,),
                                               lambda sim, ids, n_live: few.update(sim, ids, n_valid=n_live)),
                     "many256": _ScoringStep(model, resident, B, model.embed, (G,),
                                             lambda emb, ids, n_live: many.update(emb, q256, ids, n_valid=n_live))}
            nb = len(steps["embed"])
            ms = _take_turns({name: (lambda i, s=s: s.run(i % nb)) for name, s in steps.items()}, a.steps, a.windows, warmup=nb)
            if any(s.csb.gather_status() for s in steps.values()):
                raise RuntimeError("the gather reported a status")
            line = _line("step", ms, batch=B, k=k, batches_in_shard=nb, occupied=int((many.top_mol >= 0).sum()))
            line["knn_update_ms"] = round(line["many256_ms"] - line["embed_ms"], 5)
            line["cosine_and_update32_ms"] = round(line["nearest32_ms"] - line["embed_ms"], 5)
            lines.append(line)
            del steps
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[65536, 1048576])
    ap.add_argument("--queries", type=int, nargs="+", default=[32, 256, 2048])
    ap.add_argument("--k", type=int, nargs="+", default=[16, 64])
    ap.add_argument("--width", type=int, default=32, help="H of the stored route's random embeddings")
    ap.add_argument("--batches", type=int, nargs="+", default=[256, 4096])
    ap.add_argument("--shard-batches", type=int, default=2, help="the shard holds this many batches of the largest size")
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--windows", type=int, default=10)
    ap.add_argument("--yardstick-launches", type=int, default=5000, help="the most launches per replay of a yardstick that is timed")
    ap.add_argument("--skip-stored", action="store_true")
    ap.add_argument("--skip-step", action="store_true")
    a = ap.parse_args()
    import torch
    sys.path.insert(0, REPO)
    dev = torch.device("cuda:0")
    out = {}
    with torch.no_grad():
        if not a.skip_stored:
            out["stored"] = stored(a, dev)
        if not a.skip_step:
            out["step"] = step(a, dev)
    print(json.dumps({"summary": out}), flush=True)


if __name__ == "__main__":
    main()
