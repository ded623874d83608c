"""What the kernel exemplars cost: the captured step of ``screening.kernel_exemplars`` for the first and for the last convolution
layer against the plain scoring step of ``score_resident`` on the same shard, and ``mkgnn_kernel_exemplars_update`` alone.

    python tools/exemplars_timing.py [--batches 256 4096] [--k 8] [--chain 4] [--windows 10] [--steps 32] [--shard-batches 4]

Per batch size ``B`` three graphs are captured in ONE process and take turns, window by window (the median of ``--windows`` windows
of ``--steps`` replays, device events; each replay is one small copy and the graph, as the passes run it):

``score``     the step of ``score_resident`` (``model.predict``, one scatter, ``TopK.update``): code the exemplars do not touch
``layer0``    the step of ``kernel_exemplars`` for layer 0: gather, expand, receptive fields, ``kernel_scores``, one update
``last``      the same for the last layer

(the exemplar steps are warmed up for ``k + 1`` passes over the shard: repeats are kept, so by then every list holds ``k`` copies of
its best atom and the windows time the steady state of a long screen, in which next to nothing enters) and the update alone on the last layer's scores of one batch, ``--chain`` calls back to back in one graph, reported per call:

``filling``   every call starts from empty lists (four small fills in front of it, inside the graph; ``reset`` is those fills alone)
``steady``    the lists already hold the whole shard's answer: no candidate displaces anything, every (tile, column) is passed over

One JSON line per batch size with every window, then a summary line."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def chained(dev, chain, body):
    """``chain`` calls of ``body`` in one captured graph (after one eager call on the side stream)."""
    import torch
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        body()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            for _ in range(chain):
                body()
    torch.cuda.current_stream(dev).wait_stream(side)
    return graph


def windows_of(runs, windows, steps):
    """``{name: [ms per call]}``: the callables of ``runs`` take turns, window by window (drift hits them alike)."""
    import torch
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


def time_batch(model, resident, B, k, chain, steps, windows, warmup):
    import torch
    from molkgnn_amd.screening import KernelExemplars, TopK, _ExemplarStep, _ScoringStep
    dev = resident.device
    layers = model.gnn_model.gnn.layers
    last = len(layers) - 1
    plain = TopK(1024, dev)
    plain.reserve(B)
    score = _ScoringStep(model, resident, B, lambda data: model.predict(data)[0].reshape(-1), (),
                         lambda pred, ids, n_live: plain.update(pred, ids, n_valid=n_live))
    lists, step = {}, {}
    for name, layer in (("layer0", 0), ("last", last)):
        Ls = [int(x) for x in layers[layer].L]
        lists[name] = KernelExemplars(sum(Ls), k, dev)
        step[name] = _ExemplarStep(model, resident, B, layer, lists[name], Ls)
    nb = len(score)
    runs = {"score": lambda i: score.run(i % nb), "layer0": lambda i: step["layer0"].run(i % nb), "last": lambda i: step["last"].run(i % nb)}
    # the passes replay the shard's batches over and over, and repeats are kept: after k passes every list holds k copies of its best
    # atom and nothing enters any more -- the steady state of a long screen, which is what the windows then time
    for name, run in runs.items():
        for i in range(warmup if name == "score" else max(warmup, (k + 1) * nb)):
            run(i)
    torch.cuda.synchronize()
    settled = [t.clone() for t in (lists["last"].top_score, lists["last"].top_mol, lists["last"].top_atom)]
    ms = windows_of(runs, windows, steps)
    settled = all(torch.equal(a.view(torch.int32), b.view(torch.int32))
                  for a, b in zip(settled, (lists["last"].top_score, lists["last"].top_mol, lists["last"].top_atom)))
    if score.csb.gather_status() or any(s.csb.gather_status() for s in step.values()):
        raise RuntimeError("the gather reported a status")
    # the update alone: the last layer's scores of the batch the static buffers hold now
    data = step["last"].csb.data
    Ls = [int(x) for x in layers[last].L]
    begin = [sum(Ls[:d]) for d in range(4)]
    sim = model.kernel_scores(data, last)[0].clone()
    sels = [getattr(data, f"selected_index_deg{d}").clone() for d in range(1, 5)]
    atom_mol, mol_ptr, nva = data.atom_mol.clone(), data.mol_ptr.clone(), data.n_valid_atoms.clone()
    ids = step["last"].feed[:B].clone()
    live = step["last"].feed[B:B + 1].clone()
    steady, filling = lists["last"], KernelExemplars(sum(Ls), k, dev)
    filling.reserve([int(s.numel()) for s in sels], Ls)

    def update(target):
        target.update(sim, sels, begin, atom_mol, mol_ptr, ids, live, nva, num_kernels=Ls)

    def fill():
        filling.reset()
        update(filling)

    held = [t.clone() for t in (steady.top_score, steady.top_shard, steady.top_mol, steady.top_atom)]
    graphs = {"reset": chained(dev, chain, filling.reset), "filling": chained(dev, chain, fill),
              "steady": chained(dev, chain, lambda: update(steady))}
    alone = windows_of({name: (lambda i, g=g: g.replay()) for name, g in graphs.items()}, windows, steps)
    unchanged = all(torch.equal(a.view(torch.int32), b.view(torch.int32))
                    for a, b in zip(held, (steady.top_score, steady.top_shard, steady.top_mol, steady.top_atom)))
    med = {name: statistics.median(v) for name, v in ms.items()}
    med_alone = {name: statistics.median(v) / chain for name, v in alone.items()}
    line = {"batch": B, "k": k, "atoms": int(sim.shape[0]), "columns": sum(Ls), "batches_in_shard": nb, "steps": steps, "chain": chain,
            "steady_lists_unchanged": bool(unchanged), "step_lists_unchanged": bool(settled)}
    for name in runs:
        line[f"{name}_ms"] = round(med[name], 5)
        line[f"{name}_windows_ms"] = [round(v, 5) for v in ms[name]]
    for name in graphs:
        line[f"update_{name}_ms"] = round(med_alone[name], 5)
        line[f"update_{name}_windows_ms"] = [round(v / chain, 5) for v in alone[name]]
    line["layer0_over_score"] = round(med["layer0"] / med["score"], 4)
    line["last_over_score"] = round(med["last"] / med["score"], 4)
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="*", default=[256, 4096])
    ap.add_argument("--k", type=int, default=8)
    ap.add_argument("--chain", type=int, default=4, help="calls of the update alone in one graph")
    ap.add_argument("--windows", type=int, default=10)
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--shard-batches", type=int, default=4, help="the shard holds this many batches of the largest size")
    ap.add_argument("--warmup", type=int, default=8)
    a = ap.parse_args()
    sys.path.insert(0, REPO)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("exemplars_timing.py measures on the GPU: none is available (nothing is measured on the CPU)")
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
            line = time_batch(model, resident, B, a.k, a.chain, a.steps, a.windows, a.warmup)
            print(json.dumps(line), flush=True)
            lines.append(line)
    keys = ("batch", "atoms", "score_ms", "layer0_ms", "last_ms", "layer0_over_score", "last_over_score", "update_reset_ms",
            "update_filling_ms", "update_steady_ms", "steady_lists_unchanged")
    print(json.dumps({"summary": [{key: r[key] for key in keys} for r in lines]}), flush=True)


if __name__ == "__main__":
    main()
