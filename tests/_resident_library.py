"""The set-up the end-to-end screening tests on the GPU share (test_screen_gpu.py, test_screen_tasks_gpu.py, test_nearest_gpu.py):
a few small resident shards, a model whose running statistics are not the initial ones, and the eager walk over a shard's gathered
batches that every captured pass is compared with.  Seeds, molecule counts, labels and model arguments are the caller's."""
import numpy as np
import torch


def bits(t):
    """A float32 tensor as int32 bit patterns on the host: what "equal" means in these tests."""
    return t.detach().contiguous().view(torch.int32).cpu().numpy()


def eval_model(device, seed, **model_kw):
    """``GNNModel(**model_kw)`` on ``device`` from ``torch.manual_seed(seed)``, with running statistics that are not the initial
    0 / 1, in evaluation mode."""
    from molkgnn_amd.train import GNNModel
    torch.manual_seed(seed)
    model = GNNModel(**model_kw).to(device)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, torch.nn.modules.batchnorm._BatchNorm):
                m.running_mean.uniform_(-0.2, 0.2)
                m.running_var.uniform_(0.5, 1.5)
    return model.eval()


def build_library(tmp_dir, device, *, counts, shard_seed, labels, model_seed, batch_size=32, **model_kw):
    """``(model, residents, gathered)``: shard ``j`` holds ``counts[j]`` synthetic molecules (``make_batch(seed=shard_seed + j)``,
    labelled ``labels(n)``), written to ``tmp_dir/lib-j.mkgs`` and resident on ``device``; ``model`` is ``eval_model(device,
    model_seed, **model_kw)``; ``gathered(resident)`` yields ``(data, live)`` per batch of ``batch_size`` -- the static batch after
    ``gather`` -> ``expand`` -> ``attach_receptive_fields`` (refilled for the next batch: clone what is kept) and its live slots."""
    from molkgnn_amd import shards as S
    from molkgnn_amd.receptive_field import attach_receptive_fields
    from molkgnn_amd.screening import static_batch_for
    from molkgnn_amd.synthetic import make_batch
    residents = []
    for j, n in enumerate(counts):
        b = make_batch(n, seed=shard_seed + j, assay="all9", with_receptive_fields=False)
        b.y = labels(n)
        path = str(tmp_dir / f"lib-{j}.mkgs")
        S.write_shard(path, b)
        residents.append(S.ResidentShard(path, device))
    model = eval_model(device, model_seed, **model_kw)

    def gathered(resident):
        loader = S.ResidentLoader(resident, batch_size, np.arange(resident.n_molecules), device, drop_last=False)
        csb = static_batch_for(loader, resident)
        for ids, live in zip(loader, loader.n_live.tolist()):
            csb.gather(resident, ids)
            csb.expand()
            attach_receptive_fields(csb.data, sizes=csb.data.bucket_sizes, overlap=True)
            yield csb.data, live

    return model, residents, gathered
