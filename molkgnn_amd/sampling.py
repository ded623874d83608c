"""Oversampling with replacement for the imbalanced QSAR assays (reference ``data.py:136-166``).

The reference weights every training molecule by the inverse size of its class and draws ``len(dataset)`` indices
per epoch with ``torch.utils.data.WeightedRandomSampler`` seeded from the run's seed.  Same weights, same sampler
class, same generator seeding here -- so the same labels and seed give the same index stream -- computed from a label
tensor in one pass instead of a Python loop over ``Data`` objects.

``cluster_split`` is not the reference's: its split is random (``data.py``), which puts near-copies of a training molecule into
the test set; given the clusters of ``screening.cluster_butina_embeddings`` it keeps every cluster in one fold.
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


def cluster_split(leader, fractions=(0.8, 0.1, 0.1), seed: int = 0) -> torch.Tensor:
    """A cluster-based split: the fold (``0 .. len(fractions) - 1``; train / validation / test for the default) of every row, int64
    ``[n]`` on the device of ``leader``, with WHOLE clusters per fold -- so the members of a cluster are not spread over training and
    test set, which the reference's random split does not prevent.  What that is worth depends on the clusters.  "No pair above the
    threshold across folds" holds for the labels of ``screening.cluster_components_embeddings`` (``["component"]``: the connected
    components of the threshold graph, the only partition that carries it) and does NOT hold for Butina's or the leader walk's: a
    row joins the FIRST centroid above the threshold, so rows of different clusters can be closer than it.
    ``screening.split_leakage`` counts the pairs a split lets through.  ``leader`` is an integer ``[n]`` tensor naming every row's
    cluster, as ``screening.cluster_components_embeddings``, ``cluster_butina_embeddings`` or ``pick_diverse_embeddings`` return it:
    rows with the same value ``>= 0`` form one cluster, and a row with ``-1`` is a cluster of its own.  The clusters are taken in an order drawn from a ``torch.Generator``
    seeded with ``seed`` (over the clusters by ascending name, the ``-1`` rows behind them in row order), and each goes to the fold
    furthest below its target count ``fractions[f] / sum(fractions) * n`` at that moment, ties to the lower fold.  A fold below its
    target exists while rows remain, so no fold is filled beyond its target by more than one cluster, and none ends further below
    it than the largest cluster's size.  Host logic (the walk is sequential), deterministic in its arguments."""
    lead = torch.as_tensor(leader)
    if lead.dim() != 1 or lead.dtype not in (torch.int8, torch.int16, torch.int32, torch.int64, torch.uint8):
        raise ValueError("cluster_split: leader is an integer [n] tensor")
    share = [float(f) for f in fractions]
    if not share or any(f != f or f < 0 or f == float("inf") for f in share) or sum(share) <= 0:
        raise ValueError(f"cluster_split: fractions = {tuple(fractions)}: finite, not negative, and not all zero")
    host = lead.detach().cpu().long()
    n = host.numel()
    if n and int(host.min()) < -1:
        raise ValueError("cluster_split: leader holds a value below -1")
    named = host >= 0
    _, which = torch.unique(host[named], return_inverse=True)     # rows with a leader -> their cluster, by ascending name
    n_named = int(which.max()) + 1 if which.numel() else 0
    cluster = torch.empty(n, dtype=torch.int64)
    cluster[named] = which
    cluster[~named] = n_named + torch.arange(n - int(named.sum()))
    sizes = torch.bincount(cluster, minlength=1)[:int(cluster.max()) + 1 if n else 0].tolist()
    generator = torch.Generator()
    generator.manual_seed(int(seed))
    target = [f / sum(share) * n for f in share]
    filled = [0] * len(share)
    fold_of = [0] * len(sizes)
    for c in torch.randperm(len(sizes), generator=generator).tolist():
        f = max(range(len(share)), key=lambda j: (target[j] - filled[j], -j))
        fold_of[c] = f
        filled[f] += sizes[c]
    folds = torch.tensor(fold_of, dtype=torch.int64)[cluster] if n else torch.zeros(0, dtype=torch.int64)
    return folds.to(lead.device)


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


def pos_weights(labels, tasks=None, num_tasks: int = 1) -> torch.Tensor:
    """``BCEWithLogitsLoss``'s ``pos_weight`` per task: float32 ``[num_tasks]`` with ``n_negative / n_positive`` over the task's
    labelled molecules (``tasks``: one task index per molecule, anything outside ``[0, num_tasks)``: no label; None: every
    molecule has task 0).  A task without a positive or without a molecule gets 1."""
    y = torch.as_tensor(labels).reshape(-1).cpu()
    t = torch.zeros(y.numel(), dtype=torch.int64) if tasks is None else torch.as_tensor(tasks).reshape(-1).cpu().long()
    if y.numel() != t.numel():
        raise ValueError("labels and tasks differ in length")
    if num_tasks < 1:
        raise ValueError("pos_weights needs at least one task")
    out = torch.ones(int(num_tasks), dtype=torch.float32)
    active = y != 0
    for task in range(int(num_tasks)):
        pos, neg = int(((t == task) & active).sum()), int(((t == task) & ~active).sum())
        if pos > 0:
            out[task] = neg / pos
    return out


def label_pos_weights(labels) -> torch.Tensor:
    """``pos_weights`` for a label matrix with holes (``labels [n, T]``, NaN: not measured; ``readout.label_head_loss``): float32
    ``[T]`` with ``n_negative / n_positive`` per column over its non-NaN entries, 1 for a column without a positive.  With a label
    matrix a molecule carries many labels at once, so oversampling cannot balance (task, class) cells: this is what does."""
    y = torch.as_tensor(labels).detach().cpu()
    if y.dim() != 2 or not y.is_floating_point():
        raise ValueError("label_pos_weights needs a float [n, T] label matrix (NaN: not measured)")
    known = ~torch.isnan(y)
    pos = (known & (y != 0)).sum(dim=0)
    neg = (known & (y == 0)).sum(dim=0)
    out = torch.ones(y.shape[1], dtype=torch.float32)
    has = pos > 0
    out[has] = (neg[has].double() / pos[has].double()).float()
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
