"""What explaining a batch costs: ``GNNModel.atom_contributions`` (every atom's exact share of every output,
``mkgnn_atom_contributions``) against scoring the same batch (``predict`` for a one-task model, ``predict_tasks`` for nine tasks),
measured in the same run on a synthetic AID-1798-shaped resident shard, and the two launches of the C call on their own.

    python tools/explain_timing.py [--batches 256 4096] [--tasks 1 9] [--shard-batches 2] [--steps 32] [--windows 10] [--timeout 300]

Per task count one child process, and per batch size three captured graphs in it, each over the SAME static batch buffers:

``score``   gather, expand, receptive fields, ``model.predict`` (``T = 1``) / ``model.predict_tasks`` (``T = 9``)
``atoms``   gather, expand, receptive fields, ``model.atom_contributions``
``call``    ``readout.atom_contributions`` alone on the block rows the last convolution left for one batch: the projection and
            the per-atom kernel, ``--steps`` times back to back in one graph (``us_per_call``: a window over ``--steps``)

``ms_per_batch`` is the median of ``--windows`` windows of ``--steps`` replays each (device events; the replays cycle over the
shard's batches); the three graphs take turns window by window, every window is in the line.  Each child runs under
``timeout -k`` and nothing is started after a child that failed.  The per-atom kernel WITHOUT the projection is not separable
from here: take it from ``rocprofv3 --kernel-trace --stats -- python tools/explain_timing.py --child 9 --shard <file> ...`` in a
run of its own (``atom_contrib_kernel``)."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Step:
    """One captured graph over ``gather`` -> ``expand`` -> ``attach_receptive_fields`` -> ``fn(data)`` on shared static buffers."""

    def __init__(self, csb, resident, fn, dev):
        import torch
        from molkgnn_amd.receptive_field import attach_receptive_fields

        def step():
            csb.gather(resident)                         # (what csb.ids holds: refilled between replays)
            csb.expand()
            attach_receptive_fields(csb.data, sizes=csb.data.bucket_sizes, overlap=True)
            return fn(csb.data)

        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            step()                                       # (eager once: lazily made buffers exist before the capture)
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph, stream=side):
                self.out = step()
        torch.cuda.current_stream(dev).wait_stream(side)


def child(T, shard_path, batches, steps, windows, warmup):
    import numpy as np
    import torch
    sys.path.insert(0, REPO)
    from molkgnn_amd import readout as R
    from molkgnn_amd import shards as S
    from molkgnn_amd.screening import static_batch_for
    from molkgnn_amd.train import GNNModel, tune_torch_backends
    dev = torch.device("cuda:0")
    tune_torch_backends()
    resident = S.ResidentShard(shard_path, dev)
    torch.manual_seed(0)
    model = GNNModel(task_dim=T).to(dev).eval()
    score = (lambda data: model.predict(data)[0]) if T == 1 else (lambda data: model.predict_tasks(data)[0])
    for B in batches:
        loader = S.ResidentLoader(resident, B, np.arange(resident.n_molecules, dtype=np.int64), dev, drop_last=True)
        ids = list(loader)
        csb = static_batch_for(loader, resident)
        csb.gather(resident, ids[0])                     # (makes csb.ids)
        # the block rows of one batch, caught on their way into the HIP call
        caught = []
        real = R.atom_contributions

        def catching(sim, plan, blocks, *mods, **kw):
            if not caught:                               # (the eager step's: not a tensor of a graph's private pool)
                n, K = sim.shape
                keep = torch.zeros((n, K + (-K) % 4), dtype=sim.dtype, device=sim.device)     # (16-byte rows, as the layer leaves them)
                keep[:, :K] = sim
                caught.append((keep[:, :K], plan, blocks, mods))
            return real(sim, plan, blocks, *mods, **kw)

        R.atom_contributions = catching
        try:
            graphs = {"score": _Step(csb, resident, score, dev), "atoms": _Step(csb, resident, model.atom_contributions, dev)}
        finally:
            R.atom_contributions = real
        if not caught:
            raise RuntimeError("GNNModel.atom_contributions did not take the HIP route")
        sim, plan, blocks, mods = caught[0]
        n_atoms = int(sim.shape[0])
        out = torch.empty((n_atoms, T), dtype=torch.float32, device=dev)
        with torch.no_grad():
            real(sim, plan, blocks, *mods, out=out)
            call = torch.cuda.CUDAGraph()
            side = torch.cuda.Stream(device=dev)
            side.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(side), torch.cuda.graph(call, stream=side):
                for _ in range(steps):
                    real(sim, plan, blocks, *mods, out=out)
            torch.cuda.current_stream(dev).wait_stream(side)

        def window(name):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            if name == "call":
                call.replay()
            else:
                for i in range(steps):
                    csb.ids.copy_(ids[i % len(ids)], non_blocking=True)
                    graphs[name].graph.replay()
            t1.record()
            torch.cuda.synchronize()
            return t0.elapsed_time(t1) / steps

        for _ in range(max(1, warmup // steps + 1)):
            for name in ("score", "atoms", "call"):
                window(name)
        ms = {"score": [], "atoms": [], "call": []}
        for _ in range(windows):
            for name in ms:
                ms[name].append(window(name))
        if csb.gather_status():
            raise RuntimeError("the gather reported a status")
        med = {k: statistics.median(v) for k, v in ms.items()}
        print(json.dumps({"batch": B, "tasks": T, "atoms_in_batch": n_atoms, "steps": steps, "batches_in_shard": len(ids),
                          "score_ms_per_batch": round(med["score"], 5), "atoms_ms_per_batch": round(med["atoms"], 5),
                          "atoms_over_score": round(med["atoms"] / med["score"], 4), "us_per_call": round(1e3 * med["call"], 3),
                          "score_windows_ms": [round(v, 5) for v in ms["score"]], "atoms_windows_ms": [round(v, 5) for v in ms["atoms"]],
                          "call_windows_us": [round(1e3 * v, 3) for v in ms["call"]],
                          "nan": bool(torch.isnan(graphs["atoms"].out).any() or torch.isnan(out).any())}), flush=True)
        del graphs, call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[256, 4096])
    ap.add_argument("--tasks", type=int, nargs="+", default=[1, 9])
    ap.add_argument("--shard-batches", type=int, default=2, help="the shard holds this many batches of the largest size")
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--windows", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--timeout", type=int, default=300, help="seconds per child process")
    ap.add_argument("--child", type=int, help=argparse.SUPPRESS)
    ap.add_argument("--shard", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child(a.child, a.shard, a.batches, a.steps, a.windows, a.warmup)
        return
    sys.path.insert(0, REPO)
    from molkgnn_amd import shards as S
    from molkgnn_amd.synthetic import make_batch
    lines = []
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "library.mkgs")
        S.write_shard(path, make_batch(a.shard_batches * max(a.batches), seed=1798000, assay="1798", with_receptive_fields=False))
        for T in a.tasks:
            cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--child", str(T), "--shard", path,
                   "--steps", str(a.steps), "--windows", str(a.windows), "--warmup", str(a.warmup), "--batches", *map(str, a.batches)]
            done = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
            sys.stdout.write(done.stdout)
            sys.stdout.flush()
            if done.returncode != 0:                  # (a failed child ends the run: nothing more is started on the GPU)
                print(json.dumps({"tasks": T, "error": f"exit status {done.returncode}"}), flush=True)
                sys.exit(124 if done.returncode in (124, 137) else 1)
            lines += [json.loads(ln) for ln in done.stdout.splitlines() if ln.startswith("{")]
    print(json.dumps({"summary": [{k: r[k] for k in ("batch", "tasks", "atoms_in_batch", "score_ms_per_batch", "atoms_ms_per_batch",
                                                      "atoms_over_score", "us_per_call", "nan")} for r in lines]}), flush=True)


if __name__ == "__main__":
    main()
