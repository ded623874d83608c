"""What the running top-k costs inside the captured scoring step of ``screening.score_resident``, on synthetic AID-1798-shaped
shards, with K = 1024.

    python tools/screen_timing.py [--batches 256 4096] [--k 1024] [--shard-batches 4] [--steps 32] [--windows 5] [--timeout 300]
                                  [--packed]

Per batch size the same captured step (gather, expand, receptive fields, the model's scoring, scatter) is timed three ways:
``none`` (no ranking), ``hip`` (``TopK.update``: ``mkgnn_topk_update``) and ``torch`` (the PyTorch formulation in its place:
``torch.cat`` of the running and the batch triples, two stable sorts by the same key, the first K copied back).  ``ms_per_batch`` is
the median of ``--windows`` windows of ``--steps`` replays each (device events; the replays cycle over the shard's batches, so the
list is in its steady state: most of a batch ranks behind it), every window is in the line.  Each variant runs in a child
process of its own under ``timeout -k``; nothing is started after a child that failed.  The last line holds the summary.
``--packed`` writes the library with the reference's feature column pattern (``synthetic.with_reference_features``) and holds it as
``ResidentShard(..., packed=True)``: the same three variants, fed by ``mkgnn_gather_compact_packed``; every line says which form it is
and how many bytes the shard takes on the device."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARIANTS = ("none", "hip", "torch")


def torch_ranker(topk, tag: int):
    """``rank(pred, ids, n_live)``: the update of ``topk``'s tensors in PyTorch operators, by the order of the header."""
    import torch
    K, dev = topk.k, topk.device
    neg_inf = torch.tensor(float("-inf"), device=dev)
    minus1 = torch.tensor(-1, dtype=torch.int32, device=dev)
    tag_t = torch.tensor(tag, dtype=torch.int32, device=dev)

    def rank(pred, ids, n_live):
        live = torch.arange(pred.numel(), device=dev, dtype=torch.int32) < n_live
        s = torch.cat([topk.top_score, torch.where(live, pred, neg_inf)])
        h = torch.cat([topk.top_shard, torch.where(live, tag_t, minus1)])
        m = torch.cat([topk.top_mol, torch.where(live, ids, minus1)])
        bits = (s + 0.0).view(torch.int32).to(torch.int64) & 0xFFFFFFFF                       # (-0.0 + 0.0 = +0.0)
        falling = torch.where(bits >= 0x80000000, bits, (~(bits | 0x80000000)) & 0xFFFFFFFF)  # smaller = larger score
        key = torch.where(torch.isnan(s), torch.full_like(falling, 0xFFFFFFFE), falling)
        empty = (s == neg_inf) & (h == -1) & (m == -1)
        key = torch.where(empty, torch.full_like(falling, 0xFFFFFFFF), key)
        first = torch.sort(m, stable=True).indices                                            # minor key, then the major ones
        major = ((key - 0x80000000) << 32) | (h.to(torch.int64) + 0x80000000)                # (signed int64 keeps the order)
        order = first[torch.sort(major[first], stable=True).indices][:K]
        topk.top_score.copy_(s[order])
        topk.top_shard.copy_(h[order])
        topk.top_mol.copy_(m[order])
    return rank


def child(variant, shard_path, batches, k, steps, windows, warmup, packed=False):
    import torch
    sys.path.insert(0, REPO)
    from molkgnn_amd import shards as S
    from molkgnn_amd.screening import TopK, _ScoringStep
    from molkgnn_amd.train import GNNModel, tune_torch_backends
    dev = torch.device("cuda:0")
    tune_torch_backends()
    resident = S.ResidentShard(shard_path, dev, packed=packed)
    torch.manual_seed(0)
    model = GNNModel().to(dev).eval()
    for B in batches:
        topk = TopK(k, dev)
        topk.reserve(B)
        rank = {"none": None, "hip": lambda pred, ids, n_live: topk.update(pred, ids, n_valid=n_live),
                "torch": torch_ranker(topk, 0)}[variant]
        scoring = _ScoringStep(model, resident, B, lambda data: model.predict(data)[0].reshape(-1), (), rank)
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
        top = topk.result()
        print(json.dumps({"batch": B, "variant": variant, "k": k, "ms_per_batch": round(statistics.median(ms), 5),
                          "windows_ms": [round(v, 5) for v in ms], "steps": steps, "batches_in_shard": nb, "occupied": top[3],
                          "packed": bool(packed), "shard_bytes": resident.nbytes(),
                          "top_score_sum": float(top[0][:top[3]].double().sum()), "top_mol_sum": int(top[2][:top[3]].sum())}), flush=True)
        del scoring


def summary(lines):
    out = []
    for B in sorted({r["batch"] for r in lines}):
        w = {v: [m for r in lines if r["batch"] == B and r["variant"] == v for m in r["windows_ms"]] for v in VARIANTS}
        if not all(w.values()):
            continue
        med = {v: statistics.median(w[v]) for v in VARIANTS}
        out.append({"batch": B, **{f"{v}_ms": round(med[v], 5) for v in VARIANTS},
                    "hip_update_ms": round(med["hip"] - med["none"], 5), "torch_update_ms": round(med["torch"] - med["none"], 5),
                    "none_spread_ms": round(max(w["none"]) - min(w["none"]), 5), "hip_faster_than_torch": bool(med["hip"] < med["torch"])})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[256, 4096])
    ap.add_argument("--k", type=int, default=1024)
    ap.add_argument("--shard-batches", type=int, default=4, help="the shard holds this many batches of the largest size")
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=1, help="the variants alternate this many times")
    ap.add_argument("--timeout", type=int, default=300, help="seconds per child process")
    ap.add_argument("--packed", action="store_true", help="hold the library with its byte-valued feature columns packed as int8")
    ap.add_argument("--child", help=argparse.SUPPRESS)
    ap.add_argument("--shard", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child(a.child, a.shard, a.batches, a.k, a.steps, a.windows, a.warmup, a.packed)
        return
    sys.path.insert(0, REPO)
    from molkgnn_amd import shards as S
    from molkgnn_amd.synthetic import make_batch, with_reference_features
    lines = []
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "library.mkgs")
        library = make_batch(a.shard_batches * max(a.batches), seed=1798000, assay="1798", with_receptive_fields=False)
        S.write_shard(path, with_reference_features(library) if a.packed else library)
        for rnd in range(a.rounds):
            for variant in VARIANTS:
                cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--child", variant, "--shard", path,
                       "--k", str(a.k), "--steps", str(a.steps), "--windows", str(a.windows), "--warmup", str(a.warmup), "--batches",
                       *map(str, a.batches)] + (["--packed"] if a.packed else [])
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
