"""What the diverse picks cost: ``mkgnn_diverse_pick`` alone against the same selection written in torch operators, and the captured
step of ``screening.screen_diverse`` against the plain scoring step of ``score_resident`` on the same shard.

    python tools/diverse_timing.py [--rows 1024 65536] [--width 32] [--max-sim 0.9] [--chain 4] [--windows 10] [--steps 8]
                                   [--torch-windows 3] [--batches 256 4096] [--shard-batches 4] [--step-steps 32]

Per row count ``n`` (clustered embeddings: ``n // 6`` random centres, rows = centre + 0.08 noise at a random scale, so about ``n / 6``
picks spread over every tile):

``kernel``  ``--chain`` calls of ``mkgnn_diverse_pick`` (its init launch and two launches per tile) back to back in one graph,
            reported per call: the median of ``--windows`` windows of ``--steps`` replays (device events)
``torch``   the same walk in torch operators, launched eagerly: normalise once, per tile of 1 024 rows ONE ``matmul`` of every row
            from the tile on against the tile's rows, then per row of the tile the dependent masked updates (is it still alive? then it
            is a pick and covers the alive rows above the threshold).  ``n`` dependent steps of a handful of launches each -- the
            formulation the kernel replaces; the median of ``--torch-windows`` single runs (host clock around a synchronise)

and whether the two agree on the picks (the torch similarities are not the kernel's bits; on clustered rows no similarity lies
near the threshold).  Per batch size ``B`` two graphs are captured in ONE process and take turns, window by window:

``score``    the step of ``score_resident`` (``model.predict``, one scatter, ``TopK.update``)
``diverse``  the step of ``screen_diverse``: the same network run, the embedding scattered as the main result (``4 G`` bytes per
             molecule), the score scattered as the extra vector, ``TopK.update``

One JSON line per measurement with every window, then a summary line."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TORCH_TILE = 1024


def clustered(n, H, seed, dev):
    import torch
    g = torch.Generator().manual_seed(seed)
    centres = torch.randn(max(2, n // 6), H, generator=g)
    rows = centres[torch.randint(0, len(centres), (n,), generator=g)] + 0.08 * torch.randn(n, H, generator=g)
    rows *= torch.exp(torch.empty(n).uniform_(-3.0, 3.0, generator=g))[:, None]
    return rows.to(dev)


def torch_diverse(emb, max_sim):
    """The walk in torch operators (no cap): ``(leader int64 [n], n_picks)``, everything on the device."""
    import torch
    n, dev = emb.shape[0], emb.device
    unit = torch.nn.functional.normalize(emb, dim=1, eps=1e-8)
    alive = torch.ones(n, dtype=torch.bool, device=dev)
    leader = torch.full((n,), -1, dtype=torch.int64, device=dev)
    row = torch.arange(n, device=dev)
    for base in range(0, n, TORCH_TILE):
        sim = unit[base:] @ unit[base:base + TORCH_TILE].t()       # every row from the tile on, against the tile's rows
        rest, left = row[base:], alive[base:]
        lead = leader[base:]
        for j in range(sim.shape[1]):
            took = left[j] & left & ((sim[:, j] > max_sim) | (rest == base + j))
            lead = torch.where(took, base + j, lead)
            left = left & ~took
        leader[base:], alive[base:] = lead, left
    return leader, (leader == row).sum()


def time_selection(n, H, max_sim, chain, windows, steps, torch_windows, dev):
    import torch
    from molkgnn_amd.readout import diverse_pick
    emb = clustered(n, H, 1000 + n, dev)
    out = (torch.empty(n, dtype=torch.int32, device=dev), torch.empty(1, dtype=torch.int32, device=dev),
           torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.float32, device=dev))
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        diverse_pick(emb, max_sim, out=out)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            for _ in range(chain):
                diverse_pick(emb, max_sim, out=out)
    torch.cuda.current_stream(dev).wait_stream(side)
    graph.replay()
    torch.cuda.synchronize()
    kernel_ms = []
    for _ in range(windows):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(steps):
            graph.replay()
        t1.record()
        torch.cuda.synchronize()
        kernel_ms.append(t0.elapsed_time(t1) / steps / chain)
    leader, count = torch_diverse(emb, max_sim)                    # (the warm-up of every shape, and the comparison)
    torch.cuda.synchronize()
    torch_ms = []
    for _ in range(torch_windows):
        t0 = time.perf_counter()
        torch_diverse(emb, max_sim)
        torch.cuda.synchronize()
        torch_ms.append((time.perf_counter() - t0) * 1e3)
    return {"rows": n, "width": H, "max_sim": max_sim, "n_picks": int(out[1]), "kernel_ms": round(statistics.median(kernel_ms), 5),
            "kernel_windows_ms": [round(v, 5) for v in kernel_ms], "torch_ms": round(statistics.median(torch_ms), 3),
            "torch_windows_ms": [round(v, 3) for v in torch_ms], "chain": chain, "steps": steps,
            "torch_n_picks": int(count), "same_leaders": bool((leader == out[2].long()).all())}


def time_step(model, resident, B, pool, steps, windows, warmup):
    import torch
    from molkgnn_amd.screening import TopK, _ScoringStep
    dev = resident.device
    G = model.ffn.in_features
    plain, lists = TopK(pool, dev), TopK(pool, dev)
    plain.reserve(B)
    lists.reserve(B)
    score = _ScoringStep(model, resident, B, lambda data: model.predict(data)[0].reshape(-1), (),
                         lambda pred, ids, n_live: plain.update(pred, ids, n_valid=n_live))

    def predict(data):
        pred, emb = model.predict(data)
        return emb.float(), pred.reshape(-1)

    diverse = _ScoringStep(model, resident, B, predict, (G,), lambda emb, ids, n_live, pred: lists.update(pred, ids, n_valid=n_live),
                           ((torch.float32, float("nan")),))
    nb = len(score)
    runs = {"score": score, "diverse": diverse}
    for step in runs.values():
        for i in range(warmup):
            step.run(i % nb)
    torch.cuda.synchronize()
    ms = {name: [] for name in runs}
    for _ in range(windows):
        for name, step in runs.items():                            # (the graphs take turns: drift hits them alike)
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for i in range(steps):
                step.run(i % nb)
            t1.record()
            torch.cuda.synchronize()
            ms[name].append(t0.elapsed_time(t1) / steps)
    if score.csb.gather_status() or diverse.csb.gather_status():
        raise RuntimeError("the gather reported a status")
    med = {name: statistics.median(v) for name, v in ms.items()}
    return {"batch": B, "pool": pool, "embedding_width": G, "score_ms": round(med["score"], 5), "diverse_ms": round(med["diverse"], 5),
            "score_windows_ms": [round(v, 5) for v in ms["score"]], "diverse_windows_ms": [round(v, 5) for v in ms["diverse"]],
            "diverse_minus_score_ms": round(med["diverse"] - med["score"], 5), "diverse_over_score": round(med["diverse"] / med["score"], 4),
            "steps": steps, "batches_in_shard": nb}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="*", default=[1024, 65536])
    ap.add_argument("--width", type=int, default=32)
    ap.add_argument("--max-sim", type=float, default=0.9)
    ap.add_argument("--chain", type=int, default=4, help="calls of the kernel alone in one graph")
    ap.add_argument("--windows", type=int, default=10)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--torch-windows", type=int, default=3)
    ap.add_argument("--batches", type=int, nargs="*", default=[256, 4096])
    ap.add_argument("--pool", type=int, default=1024)
    ap.add_argument("--shard-batches", type=int, default=4, help="the shard holds this many batches of the largest size")
    ap.add_argument("--step-steps", type=int, default=32)
    ap.add_argument("--warmup", type=int, default=8)
    a = ap.parse_args()
    sys.path.insert(0, REPO)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("diverse_timing.py measures on the GPU: none is available (nothing is measured on the CPU)")
    from molkgnn_amd import shards as S
    from molkgnn_amd.synthetic import make_batch
    from molkgnn_amd.train import GNNModel, tune_torch_backends
    dev = torch.device("cuda:0")
    tune_torch_backends()
    selection, steps = [], []
    for n in a.rows:
        line = time_selection(n, a.width, a.max_sim, a.chain, a.windows, a.steps, a.torch_windows, dev)
        print(json.dumps(line), flush=True)
        selection.append(line)
    if a.batches:
        torch.manual_seed(0)
        model = GNNModel(task_dim=1).to(dev).eval()
        with tempfile.TemporaryDirectory() as d:
            path = os.path.join(d, "library.mkgs")
            S.write_shard(path, make_batch(a.shard_batches * max(a.batches), seed=1798000, assay="1798", with_receptive_fields=False))
            resident = S.ResidentShard(path, dev)
            for B in a.batches:
                line = time_step(model, resident, B, a.pool, a.step_steps, a.windows, a.warmup)
                print(json.dumps(line), flush=True)
                steps.append(line)
    print(json.dumps({"summary": {
        "selection": [{k: r[k] for k in ("rows", "width", "n_picks", "kernel_ms", "torch_ms", "same_leaders")} |
                      {"torch_over_kernel": round(r["torch_ms"] / r["kernel_ms"], 1)} for r in selection],
        "step": [{k: r[k] for k in ("batch", "score_ms", "diverse_ms", "diverse_minus_score_ms", "diverse_over_score")} for r in steps]}}),
        flush=True)


if __name__ == "__main__":
    main()
