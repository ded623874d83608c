"""Oversampled training from a device-resident shard, end to end on one GPU: synthetic molecules with a RARE label the graph
determines (at least three degree-4 atoms) -> one packed shard -> shards.ResidentShard (the data set lives in device memory) ->
sampling.oversampling_sampler (the reference's WeightedRandomSampler: a draw with replacement, re-drawn every epoch) ->
shards.ResidentLoader (plans the epoch on the host, uploads the ids once) -> ONE captured graph per run: CompactStaticBatch.gather
(mkgnn_gather_compact: the batch is formed on the device from its id list), expand, receptive fields, index plan, train.training_step
(forward, backward with deferred bank gradients, FusedAdamW), replayed for every batch of every epoch.  The only per-batch
traffic from the host is the id list.  The held-out set is a resident shard as well, scored by train.evaluate_resident before and
after.  The loss must fall and the held-out AUC must rise if every piece is right.
tools/train_oversampled.py [--molecules 16384] [--batch-size 1024] [--epochs 6] [--headroom 0.05]"""
import argparse
import os
import sys
import tempfile
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from molkgnn_amd import padding as P                                                # noqa: E402
from molkgnn_amd import shards as S                                                 # noqa: E402
from molkgnn_amd.receptive_field import attach_receptive_fields                     # noqa: E402
from molkgnn_amd.sampling import oversampling_sampler                               # noqa: E402
from molkgnn_amd.synthetic import make_batch                                        # noqa: E402
from molkgnn_amd.train import GNNModel, configure_optimizer, evaluate_resident, training_step   # noqa: E402


def labelled(n, seed, min_deg4=3):
    b = make_batch(n, seed=seed, assay="all9", with_receptive_fields=False)
    deg = torch.bincount(b.edge_index[0], minlength=b.x.shape[0])
    n4 = torch.zeros(n).index_add_(0, b.batch, (deg == 4).float())
    b.y = (n4 >= min_deg4).float()
    return b


def run(molecules=16384, batch_size=1024, epochs=6, lr=3e-3, headroom=0.05, seed=0, log=print):
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "train.mkgs")
        S.write_shard(path, labelled(molecules, 100))
        resident = S.ResidentShard(path, dev)
        log(f"{resident.n_molecules} molecules resident in {resident.nbytes() / 1e6:.1f} MB, {float(resident.y.mean()):.3f} active")
        # (one sampler for the run, as the reference's DataLoader keeps one: every epoch is the generator's next draw)
        sampler = oversampling_sampler(resident.y, seed)
        # the first epoch's shape with some headroom is kept for the run, so that ONE graph serves every later draw
        loader = S.ResidentLoader(resident, batch_size, sampler, dev, headroom=headroom)
        held_path = os.path.join(d, "held_out.mkgs")
        S.write_shard(held_path, labelled(2048, 999))
        held_out = S.ResidentShard(held_path, dev)       # (the held-out set is resident too: scored by train.evaluate_resident)
        model = GNNModel(num_layers=3).to(dev)
        opt = configure_optimizer(model, lr=lr, capturable=True)
        csb = P.CompactStaticBatch(loader.shape, batch_size, resident.x_dim, resident.p_dim, resident.e_dim, dev)
        loss_box = []

        def step():
            csb.gather(resident)                         # (the ids are in csb.ids: refilled before every replay)
            csb.expand()
            attach_receptive_fields(csb.data, sizes=csb.data.bucket_sizes, overlap=True)
            return training_step(model, csb.data, opt)

        def evaluate():
            r = evaluate_resident(model, held_out, batch_size, metrics=("logAUC_0.001_0.1", "AUC"))
            return float(r["logAUC_0.001_0.1"]), float(r["AUC"])

        before = evaluate()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            csb.gather(resident, next(iter(loader)))
            for _ in range(2):
                step()                                   # (two real steps on the first batch: warm-up before the capture)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=side):
                loss_box.append(step())
        torch.cuda.current_stream().wait_stream(side)
        losses = []
        t0 = time.perf_counter()
        n = 0
        for ep in range(epochs):
            if ep:
                loader.set_epoch(sampler)                # a new draw under the kept shape (raises if a batch does not fit it)
            for ids in loader:
                csb.ids.copy_(ids, non_blocking=True)
                g.replay()
                n += 1
            losses.append(float(loss_box[0].detach()))   # (the last batch's loss: one host read per epoch ...)
            status = csb.gather_status()                 # (... and the gather's status word with it)
            if status:
                raise RuntimeError(f"mkgnn_gather_compact reported status {status} in epoch {ep}")
            log(f"epoch {ep}: loss of its last batch {losses[-1]:.4f}")
        torch.cuda.synchronize()
        el = time.perf_counter() - t0
        after = evaluate()
        log(f"{n} steps of {batch_size} molecules in {el:.2f} s ({n * batch_size / el / 1e6:.2f} M molecules/s, oversampled, "
            f"from the resident shard); held-out logAUC {before[0]:.3f} -> {after[0]:.3f}, AUC {before[1]:.3f} -> {after[1]:.3f}")
        return losses, before, after


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--molecules", type=int, default=16384)
    ap.add_argument("--batch-size", type=int, default=1024)
    ap.add_argument("--epochs", type=int, default=6)
    ap.add_argument("--headroom", type=float, default=0.05)
    a = ap.parse_args()
    run(a.molecules, a.batch_size, a.epochs, headroom=a.headroom)
