"""Oversampling with replacement for the imbalanced QSAR assays (reference ``data.py:136-166``).

The reference weights every training molecule by the inverse size of its class and draws ``len(dataset)`` indices
per epoch with ``torch.utils.data.WeightedRandomSampler`` seeded from the run's seed.  Same weights, same sampler
class, same generator seeding here -- so the same labels and seed give the same index stream -- computed from a label
tensor in one pass instead of a Python loop over ``Data`` objects.
"""
from __future__ import annotations

import torch
from torch.utils.data import WeightedRandomSampler


def oversampling_weights(labels: torch.Tensor) -> torch.Tensor:
    """``1 / #inactive`` for label 0, ``1 / #active`` otherwise (``data.py:146-151``), float32 like the reference's."""
    y = torch.as_tensor(labels).reshape(-1)
    active = y != 0
    n_active = int(active.sum())
    n_inactive = y.numel() - n_active
    w_active = torch.tensor(1. / n_active if n_active else float("inf"))
    w_inactive = torch.tensor(1. / n_inactive if n_inactive else float("inf"))
    return torch.where(active.cpu(), w_active, w_inactive)


def oversampling_sampler(labels: torch.Tensor, seed: int) -> WeightedRandomSampler:
    """The sampler ``train_dataloader`` builds when ``enable_oversampling_with_replacement`` is set (``data.py:153-159``)."""
    weights = oversampling_weights(labels)
    generator = torch.Generator()
    generator.manual_seed(seed)
    return WeightedRandomSampler(weights=weights, num_samples=len(weights), generator=generator)


def task_index(assay_id, assays) -> torch.Tensor:
    """The task of every molecule of a mixed-assay set: the position of its ``assay_id`` in ``assays`` (``0 .. T - 1``, in the
    order given), ``-1`` for an id that is not listed -- int32, on the device of ``assay_id``.  What ``GNNModel.loss`` takes as
    ``batch.task`` and ``shards.ResidentShard(..., assays=...)`` keeps per molecule."""
    ids = [int(a) for a in assays]
    if not ids:
        raise ValueError("task_index needs at least one assay")
    if len(set(ids)) != len(ids):
        raise ValueError(f"assays holds an id twice: {ids}")
    a = torch.as_tensor(assay_id).reshape(-1).long()
    out = torch.full(a.shape, -1, dtype=torch.int32, device=a.device)
    for t, aid in enumerate(ids):
        out[a == aid] = t
    return out


def task_oversampling_weights(labels: torch.Tensor, tasks: torch.Tensor) -> torch.Tensor:
    """``oversampling_weights`` per task: a labelled molecule (``tasks >= 0``) gets ``1 / #(molecules of its task and its
    class)``, so every (task, class) cell draws the same total weight; an unlabelled one gets 0 and is never drawn.  For one
    task with every molecule labelled this is ``oversampling_weights(labels)`` bit for bit."""
    y = torch.as_tensor(labels).reshape(-1).cpu()
    t = torch.as_tensor(tasks).reshape(-1).cpu().long()
    if y.numel() != t.numel():
        raise ValueError("labels and tasks differ in length")
    w = torch.zeros(y.numel(), dtype=torch.float32)
    active = y != 0
    for task in torch.unique(t[t >= 0]).tolist():
        for cell in ((t == task) & active, (t == task) & ~active):
            n = int(cell.sum())
            if n:
                w[cell] = torch.tensor(1. / n)
    return w
