"""What an oversampled epoch from a device-resident shard costs, next to the shard-fed path, on the AID-1798-shaped synthetic
data bench.py uses.  Per batch size (4096 and 256 molecules):
  (a) ms per step of a captured oversampled epoch through ResidentLoader (ids -> mkgnn_gather_compact -> expand -> receptive
      fields -> plan -> forward + backward + AdamW, one graph),
  (b) the same captured step fed by ShardLoader(fixed_shape=True, compact=True) from contiguous shards (host staging + one
      host-to-device copy per batch), timed in the same run, windows alternating with (a),
  (c) the gather alone (HIP events around runs of launches) next to a device-to-device copy of a buffer of the wire form's size,
  (d) the packed form of the resident shard (ResidentShard(..., packed=True): byte-valued feature columns as int8, decoded by
      mkgnn_gather_compact_packed) in the same run: its captured step in windows alternating with (a) and (b), its gather alone in
      windows alternating with (c)'s, and the wall time of ResidentShard(...) -- host packing plus upload, what a streamed screen
      pays per shard -- in both forms, alternating.
The atom features carry the reference's column pattern (synthetic.with_reference_features: 20 byte-valued columns of 28), so
that the packed form has something to pack; their values do not enter any of the times.
Five windows each; median, min and max are reported.  One JSON line at the end.
tools/resident_epoch_timing.py [--batch-sizes 4096,256] [--batches 16] [--out FILE]"""
import argparse
import json
import os
import sys
import tempfile
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from molkgnn_amd import padding as P                                                # noqa: E402
from molkgnn_amd import shards as S                                                 # noqa: E402
from molkgnn_amd.receptive_field import GraphBatch, attach_receptive_fields         # noqa: E402
from molkgnn_amd.sampling import oversampling_sampler                               # noqa: E402
from molkgnn_amd.synthetic import make_batch, with_reference_features               # noqa: E402
from molkgnn_amd.train import GNNModel, configure_optimizer, training_step          # noqa: E402


def concat(parts):
    off, ei = 0, []
    for q in parts:
        ei.append(q.edge_index + off)
        off += q.x.shape[0]
    nm = [int(q.y.shape[0]) for q in parts]
    base = [sum(nm[:k]) for k in range(len(parts))]
    return GraphBatch(x=torch.cat([q.x for q in parts]), p=torch.cat([q.p for q in parts]), edge_index=torch.cat(ei, dim=1),
                      edge_attr=torch.cat([q.edge_attr for q in parts]), batch=torch.cat([q.batch + b for q, b in zip(parts, base)]),
                      y=torch.cat([q.y for q in parts]).float(), assay_id=torch.cat([q.assay_id for q in parts]))


def capture(step):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            step()
    torch.cuda.current_stream().wait_stream(side)
    return g


def stats(ws):
    ws = sorted(ws)
    return {"median": round(ws[len(ws) // 2], 4), "min": round(ws[0], 4), "max": round(ws[-1], 4)}


def run(B, nb, dev, log):
    raws = [with_reference_features(make_batch(B, seed=1798 * 1000 + 500 + i, assay="1798", with_receptive_fields=False), seed=i)
            for i in range(nb)]
    for i, r in enumerate(raws):
        r.y = ((torch.arange(B) + i) % 50 == 0).float()                     # (2 % active: the sampler has something to balance)
    out = {"batch_size": B, "batches_per_epoch": nb}
    with tempfile.TemporaryDirectory() as d:
        paths = S.write_shards(d, raws)
        whole = os.path.join(d, "whole.mkgs")
        S.write_shard(whole, concat(raws))
        # (d) construction, both forms alternating: the first pair warms up (the shard file's pages, the allocator)
        build = {"unpacked": [], "packed": []}
        for w in range(4):
            for name, packed in (("unpacked", False), ("packed", True)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                r = S.ResidentShard(whole, dev, packed=packed)
                torch.cuda.synchronize()
                if w:
                    build[name].append(1e3 * (time.perf_counter() - t0))
                del r
        out["d_construct_ms"] = {k: stats(v) for k, v in build.items()}
        resident = S.ResidentShard(whole, dev)
        resident_p = S.ResidentShard(whole, dev, packed=True)
        sampler = oversampling_sampler(resident.y, 0)
        # five draws, made up front so that the shape (and with it the one graph) covers all of them; each timed window
        # re-plans and uploads them one after the other
        draws = [list(sampler) for _ in range(5)]
        rl = S.ResidentLoader(resident, B, sum(draws, []), dev)
        sl = S.ShardLoader(paths * 5, B, device=dev, prefetch=3, workers=3, fixed_shape=True, compact=True)
        dims = (resident.x_dim, resident.p_dim, resident.e_dim)
        out["resident_shard_bytes"] = resident.nbytes()
        out["packed_shard_bytes"] = resident_p.nbytes()
        out["packed_rec_bytes"], out["packed_byte_columns"] = resident_p.rec_bytes, len(resident_p.byte_columns)
        out["ids_bytes_per_batch"] = 4 * B
        torch.manual_seed(0)
        model = GNNModel().to(dev)
        opt = configure_optimizer(model, lr=1e-3, capturable=True)
        csb_r = P.CompactStaticBatch(rl.shape, B, *dims, dev, max_mol_atoms=rl.max_mol_atoms, max_mol_edges=rl.max_mol_edges)
        csb_p = P.CompactStaticBatch(rl.shape, B, *dims, dev, max_mol_atoms=rl.max_mol_atoms, max_mol_edges=rl.max_mol_edges)
        csb_s = P.CompactStaticBatch(sl.shape, B, *dims, dev)
        out["wire_bytes_per_batch"] = {"resident": int(csb_r.wire.numel()), "shard_fed": int(csb_s.wire.numel())}

        def tail(csb):
            csb.expand()
            attach_receptive_fields(csb.data, sizes=csb.data.bucket_sizes, overlap=True)
            return training_step(model, csb.data, opt)

        csb_r.gather(resident, next(iter(rl)))
        g_r = capture(lambda: (csb_r.gather(resident), tail(csb_r)))
        csb_p.gather(resident_p, next(iter(rl)))
        g_p = capture(lambda: (csb_p.gather(resident_p), tail(csb_p)))
        csb_s.load(next(iter(sl)))
        g_s = capture(lambda: tail(csb_s))

        def epoch_resident(csb=csb_r, g=g_r):
            n = 0
            for draw in draws:
                rl.set_epoch(draw)                                          # (planning and the id upload are inside the window)
                for ids in rl:
                    csb.ids.copy_(ids, non_blocking=True)
                    g.replay()
                    n += 1
            return n

        def epoch_shards():
            n = 0
            for cb in sl:
                csb_s.load(cb)
                g_s.replay()
                n += 1
            return n

        wins = {"resident": [], "resident_packed": [], "shard_fed": []}
        for w in range(6):                                                  # window 0 warms the paths up
            for name, fn in (("resident", epoch_resident), ("resident_packed", lambda: epoch_resident(csb_p, g_p)),
                             ("shard_fed", epoch_shards)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                n = fn()
                torch.cuda.synchronize()
                if w:
                    wins[name].append(1e3 * (time.perf_counter() - t0) / n)
        if csb_r.gather_status() or csb_p.gather_status():
            raise RuntimeError(f"gather status {csb_r.gather_status()} / packed {csb_p.gather_status()}")
        if not torch.equal(csb_r.wire, csb_p.wire):                         # (both ended on the same batch of the same draw)
            raise RuntimeError("the packed gather's wire buffer differs from the unpacked gather's")
        out["a_resident_ms_per_step"] = stats(wins["resident"])
        out["d_resident_packed_ms_per_step"] = stats(wins["resident_packed"])
        out["b_shard_fed_ms_per_step"] = stats(wins["shard_fed"])
        out["steps_per_window"] = {"resident": len(draws) * len(rl), "shard_fed": len(sl)}
        # (c) the gather alone against a copy of the same bytes
        src = torch.empty_like(csb_r.wire)
        reps = 200

        def timed(fns):
            """Windows of `reps` launches of each of `fns`, alternating; window 0 warms up."""
            ws = {k: [] for k in fns}
            for w in range(6):
                for k, fn in fns.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(reps):
                        fn()
                    e1.record()
                    e1.synchronize()
                    if w:
                        ws[k].append(1e3 * e0.elapsed_time(e1) / reps)
            return {k: stats(v) for k, v in ws.items()}

        t = timed({"gather": lambda: csb_r.gather(resident), "gather_packed": lambda: csb_p.gather(resident_p),
                   "copy": lambda: src.copy_(csb_r.wire)})
        out["c_gather_us"], out["d_gather_packed_us"], out["c_copy_us"] = t["gather"], t["gather_packed"], t["copy"]
        sl.close()
    log(json.dumps(out))
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch-sizes", default="4096,256")
    ap.add_argument("--batches", type=int, default=16)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("resident_epoch_timing.py measures on the GPU: no device found")
    res = [run(int(b), a.batches, torch.device("cuda:0"), lambda s: print(s, flush=True)) for b in a.batch_sizes.split(",")]
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
