"""What an oversampled epoch from a device-resident shard costs, next to the shard-fed path, on the AID-1798-shaped synthetic
data bench.py uses.  Per batch size (4096 and 256 molecules):
  (a) ms per step of a captured oversampled epoch through ResidentLoader (ids -> mkgnn_gather_compact -> expand -> receptive
      fields -> plan -> forward + backward + AdamW, one graph),
  (b) the same captured step fed by ShardLoader(fixed_shape=True, compact=True) from contiguous shards (host staging + one
      host-to-device copy per batch), timed in the same run, windows alternating with (a),
  (c) the gather alone (HIP events around runs of launches) next to a device-to-device copy of a buffer of the wire form's size.
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
from molkgnn_amd.synthetic import make_batch                                        # noqa: E402
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
    raws = [make_batch(B, seed=1798 * 1000 + 500 + i, assay="1798", with_receptive_fields=False) for i in range(nb)]
    for i, r in enumerate(raws):
        r.y = ((torch.arange(B) + i) % 50 == 0).float()                     # (2 % active: the sampler has something to balance)
    out = {"batch_size": B, "batches_per_epoch": nb}
    with tempfile.TemporaryDirectory() as d:
        paths = S.write_shards(d, raws)
        whole = os.path.join(d, "whole.mkgs")
        S.write_shard(whole, concat(raws))
        resident = S.ResidentShard(whole, dev)
        sampler = oversampling_sampler(resident.y, 0)
        # five draws, made up front so that the shape (and with it the one graph) covers all of them; each timed window
        # re-plans and uploads them one after the other
        draws = [list(sampler) for _ in range(5)]
        rl = S.ResidentLoader(resident, B, sum(draws, []), dev)
        sl = S.ShardLoader(paths * 5, B, device=dev, prefetch=3, workers=3, fixed_shape=True, compact=True)
        dims = (resident.x_dim, resident.p_dim, resident.e_dim)
        out["resident_shard_bytes"] = resident.nbytes()
        out["ids_bytes_per_batch"] = 4 * B
        torch.manual_seed(0)
        model = GNNModel().to(dev)
        opt = configure_optimizer(model, lr=1e-3, capturable=True)
        csb_r = P.CompactStaticBatch(rl.shape, B, *dims, dev, max_mol_atoms=rl.max_mol_atoms, max_mol_edges=rl.max_mol_edges)
        csb_s = P.CompactStaticBatch(sl.shape, B, *dims, dev)
        out["wire_bytes_per_batch"] = {"resident": int(csb_r.wire.numel()), "shard_fed": int(csb_s.wire.numel())}

        def tail(csb):
            csb.expand()
            attach_receptive_fields(csb.data, sizes=csb.data.bucket_sizes, overlap=True)
            return training_step(model, csb.data, opt)

        csb_r.gather(resident, next(iter(rl)))
        g_r = capture(lambda: (csb_r.gather(resident), tail(csb_r)))
        csb_s.load(next(iter(sl)))
        g_s = capture(lambda: tail(csb_s))

        def epoch_resident():
            n = 0
            for draw in draws:
                rl.set_epoch(draw)                                          # (planning and the id upload are inside the window)
                for ids in rl:
                    csb_r.ids.copy_(ids, non_blocking=True)
                    g_r.replay()
                    n += 1
            return n

        def epoch_shards():
            n = 0
            for cb in sl:
                csb_s.load(cb)
                g_s.replay()
                n += 1
            return n

        wins = {"resident": [], "shard_fed": []}
        for w in range(6):                                                  # window 0 warms both paths up
            for name, fn in (("resident", epoch_resident), ("shard_fed", epoch_shards)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                n = fn()
                torch.cuda.synchronize()
                if w:
                    wins[name].append(1e3 * (time.perf_counter() - t0) / n)
        if csb_r.gather_status():
            raise RuntimeError(f"gather status {csb_r.gather_status()}")
        out["a_resident_ms_per_step"] = stats(wins["resident"])
        out["b_shard_fed_ms_per_step"] = stats(wins["shard_fed"])
        out["steps_per_window"] = {"resident": len(draws) * len(rl), "shard_fed": len(sl)}
        # (c) the gather alone against a copy of the same bytes
        src = torch.empty_like(csb_r.wire)
        reps = 200

        def timed(fn):
            ws = []
            for w in range(6):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(reps):
                    fn()
                e1.record()
                e1.synchronize()
                if w:
                    ws.append(1e3 * e0.elapsed_time(e1) / reps)
            return stats(ws)

        out["c_gather_us"] = timed(lambda: csb_r.gather(resident))
        out["c_copy_us"] = timed(lambda: src.copy_(csb_r.wire))
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
