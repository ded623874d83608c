"""The label-matrix training fixtures of ``tests/test_label_training_gpu.py``, and -- run as ``python -m
tests._label_training_child OUT`` -- one ``GNNModel.loss`` + backward on them in a process of its own (the test starts it with
``MKGNN_LABEL_HEAD=0``, which is read once at import), saved to ``OUT``: the loss, the head's gradients and the embedding."""
from __future__ import annotations

import sys

import torch

T = 9
NAN = float("nan")


def label_matrix(n: int, seed: int, present: float = 0.3) -> torch.Tensor:
    """float32 ``[n, T]``: binary labels, about ``present`` of the entries measured, NaN elsewhere."""
    g = torch.Generator().manual_seed(seed)
    y = (torch.rand(n, T, generator=g) < 0.35).float()
    return torch.where(torch.rand(n, T, generator=g) < present, y, torch.full((), NAN))


def model_and_batch(dev, mols: int = 40, seed: int = 7, **kw):
    from molkgnn_amd.synthetic import make_batch
    from molkgnn_amd.train import GNNModel
    batch = make_batch(mols, seed=seed, assay="all9")
    batch.labels = label_matrix(mols, seed + 1)
    torch.manual_seed(0)
    model = GNNModel(num_layers=2, task_dim=T, dropout_ratio=0.0, ffn_dropout_rate=0.0, **kw).to(dev).train()
    return model, batch


def loss_and_head_gradients(model, bd) -> dict:
    from molkgnn_amd.train import backward
    model.zero_grad(set_to_none=True)
    box = []                                                 # (the embedding this very loss was computed on)
    hook = model.gnn_model.register_forward_hook(lambda mod, args, out: box.append(out.detach().clone()))
    try:
        loss = model.loss(bd)
    finally:
        hook.remove()
    backward(loss)
    torch.cuda.synchronize()
    return {"loss": loss.detach().clone(), "ffn.weight": model.ffn.weight.grad.clone(), "ffn.bias": model.ffn.bias.grad.clone(),
            "emb": box[0]}


if __name__ == "__main__":
    device = torch.device("cuda:0")
    m, b = model_and_batch(device)
    from molkgnn_amd import readout
    out = loss_and_head_gradients(m, b.to(device))
    out["label_head"] = readout._LABEL_HEAD
    torch.save({k: (v.cpu() if torch.is_tensor(v) else v) for k, v in out.items()}, sys.argv[1])
