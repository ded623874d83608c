"""The training step the throughput metric is quoted on: the reference's ``GNNModel``
(``model.py:127-198``) around the HIP kernel convolution, without Lightning.

Only what a forward + backward (+ optimiser) step needs is restated here: the module tree with the
reference's parameter names (``gnn_model.*``, ``lin1``, ``lin2``, ``ffn``; 132 300 parameters), the
loss the data module selects -- ``BCEWithLogitsLoss()`` for the QSAR assays (``data.py:37``), ``MSELoss(reduction='sum')``
for the docking-score set (``data.py:49-53``) -- and the AdamW groups chosen by parameter name (``model.py:373-382``).
Scoring: ``GNNModel.predict``, ``evaluate`` (the reference's validation / test loop, ``model.py:221-358, 483-522``) and
``evaluate_resident`` (the same from a device-resident shard; ranking a library: ``molkgnn_amd.screening``).
Multi-task models: ``GNNModel.predict_tasks`` (all outputs of every molecule), ``evaluate_tasks``, ``evaluate_resident_tasks``;
on a label matrix with holes (``batch.labels``, NaN: not measured): ``evaluate_labels``, ``evaluate_resident_labels``.
The graph embedding alone: ``GNNModel.embed`` (analogue search: ``screening.nearest``).
Every atom's exact share of every output: ``GNNModel.atom_contributions`` (a hit list explained: ``screening.explain_resident``).
All of them, and ``screening``'s shard passes, run the model inside ``evaluation_mode``.
Logging, checkpoints, file output and the LR schedule are out of scope.
"""
from __future__ import annotations

import weakref
from contextlib import contextmanager
from typing import Optional

import torch
from torch.nn import BCEWithLogitsLoss, Dropout, Linear, MSELoss, ReLU

from .MolKGNNNet import MolKGNNNet

KERNEL_COUNTS = (10, 20, 30, 50)    # paper / README kernels per degree


class GNNModel(torch.nn.Module):
    def __init__(self, num_layers=3, kernels_1hop=KERNEL_COUNTS, kernels_Nhop=KERNEL_COUNTS, node_feature_dim=28,
                 edge_feature_dim=7, hidden_dim=32, dropout_ratio=0.0, ffn_dropout_rate=0.25, ffn_hidden_dim=64,
                 task_dim=1, loss_func=None):
        super().__init__()
        kw = {f"num_kernel{d}_1hop": k for d, k in zip(range(1, 5), kernels_1hop)}
        kw.update({f"num_kernel{d}_Nhop": k for d, k in zip(range(1, 5), kernels_Nhop)})
        self.gnn_model = MolKGNNNet(num_layers=num_layers, x_dim=node_feature_dim, edge_attr_dim=edge_feature_dim,
                                    graph_embedding_dim=hidden_dim, drop_ratio=dropout_ratio, **kw)
        self.lin1 = Linear(hidden_dim, ffn_hidden_dim)     # unused by forward, as in the reference (model.py:147-148)
        self.lin2 = Linear(ffn_hidden_dim, task_dim)
        self.ffn = Linear(hidden_dim, task_dim)
        self.dropout = Dropout(p=ffn_dropout_rate)
        self.activate_func = ReLU()
        self.loss_func = BCEWithLogitsLoss() if loss_func is None else loss_func     # model.py:156: the data module's loss

    # The multi-output fused tail (readout.tail_labels_loss) for label-matrix and task-indexed batches: None follows
    # MKGNN_MULTI_TAIL (read once at import; the default is off), True / False force it.  Where it does not apply -- a CPU batch,
    # head dropout p >= 1, more than 32 outputs, a molecule beyond a chunk, an unknown batch inside a capture -- the loss takes
    # exactly the route it takes with the attribute off.
    multi_output_tail: Optional[bool] = None

    def forward(self, data):
        return self._head(self.dropout(self.gnn_model(data)))

    def _multi_tail_embedding(self, data, kind: str, pw, source: dict, srows, sw, table, rows, nreal):
        """``self.gnn_model(data)`` for a multi-output loss -- with ``multi_output_tail`` on, asked for the fused tail first:
        ``("loss", value)`` where it applies, the embedding as usual where it does not.  ``source``: ``tail_labels_loss``'s label
        source (read through ``srows``); ``sw, table, rows``: the batch's weight fields."""
        from . import readout as R
        on = R._MULTI_TAIL if self.multi_output_tail is None else bool(self.multi_output_tail)
        # (a weight table read through other ids than the labels' is looked up per molecule: that needs the molecule count)
        known = not (table is not None and srows is not None and rows is not srows and nreal is None)
        if not (on and data.x.is_cuda and known and not (self.training and self.dropout.p >= 1.0)):
            return self.gnn_model(data)
        w, wtable, ids = _weights_for(None, nreal, sw, table, rows, srows)
        kw = dict(source, row_ids=ids, sample_weight=w, pos_weight=pw, weight_table=wtable)
        return self.gnn_model(data, _tail=dict(ffn=self.ffn, p_head=self.dropout.p if self.training else 0.0, n_rows=nreal,
                                               loss=kind, kw=kw))

    def _head(self, graph_embedding):
        if self.ffn.out_features == 1 and self.ffn.bias is not None and graph_embedding.dim() == 2:
            # ffn(graph_embedding) for a single task as multiply + row sum: the [1 x B] @ [B x H] weight gradient of
            # the GEMM form runs a 25 us rocBLAS kernel at B = 4096 (the gemv form 29 us), this takes a few
            pred = (graph_embedding * self.ffn.weight[0]).sum(dim=1, keepdim=True) + self.ffn.bias
        else:
            pred = self.ffn(graph_embedding)
        return pred, graph_embedding

    def _needs_eval(self, who: str, hint: str = "") -> None:
        if self.training:
            raise ValueError(f"GNNModel.{who} needs evaluation mode: call model.eval() first{hint}")

    def predict(self, data):
        """``(pred [n, 1], graph_embedding [n, G])`` of a model in evaluation mode, under ``torch.no_grad()``: what the reference's
        ``validation_step`` / ``test_step`` take from ``self(batch)`` (``model.py:221-232, 299-305``).  ``n``: the batch's real
        molecules, as ``loss`` counts them (``n_valid_molecules`` of a batch padded to a fixed shape).  Where the model and the batch
        qualify (one task, CUDA, the fused tail's shapes and molecule sizes) everything behind the last convolution is the
        forward-only tail -- two launches, ``readout.tail_score``; ``MKGNN_SCORE_TAIL=0`` or ``MKGNN_FUSED_TAIL=0``: never --
        and the separate operators of ``self(data)`` otherwise.  The mode is the caller's: in training mode this raises."""
        self._needs_eval("predict", " (train.evaluate does)")
        with torch.no_grad():
            nreal = getattr(data, 'n_valid_molecules', None)
            score = (self.ffn, nreal) if (self.ffn.out_features == 1 and data.x.is_cuda) else None
            out = self.gnn_model(data, _score=score)
            if isinstance(out, tuple):
                _, pred, graph_embedding = out
                pred = pred.view(-1, 1)
            else:                                        # (the embedding: the head of forward(); its dropout is the identity here)
                pred, graph_embedding = self._head(self.dropout(out))
            n = pred.shape[0] if nreal is None else int(nreal)
            return pred[:n], graph_embedding[:n]

    def predict_mc(self, data, n_samples: int, alpha: float = 1.0, beta: float = 0.0, return_samples: bool = False) -> dict:
        """Score with uncertainty -- Monte Carlo dropout: ``n_samples`` (1 to 64) stochastic predictions of every molecule from a
        model in evaluation mode (the batch norms use their running statistics) with BOTH dropouts left on -- the head's
        (``ffn_dropout_rate``) and the readout's (``dropout_ratio``) -- under ``torch.no_grad()``.  Returns a dict: ``pred``, the
        evaluation-mode prediction (``predict``'s bits; the masks are inverted dropout in front of linear layers, so it is the
        samples' expectation); ``mean`` and ``std`` (unbiased) of the samples; ``acq = alpha * mean + beta * std``, the
        acquisition value of an active-learning round (``alpha = -1`` where lower is better, as for docking scores); each ``[n]``
        for a one-task model (``n`` as in ``predict``); with ``return_samples`` also ``samples [n, n_samples]``.

        Both dropouts sit behind the last convolution, so the network runs ONCE.  Where model and batch qualify as for ``predict``
        (one task, CUDA, the fused tail's shapes and molecule sizes; ``dropout_ratio < 1``) everything behind the last
        convolution is ``readout.tail_score_mc`` -- two launches for all samples, the statistics included, no ``[n, S]`` matrix
        unless asked for; sample ``s`` is bit for bit the prediction of a training step with generator state ``{seed, offset +
        s}`` of ``readout.head_rng_state``, whose offset the call advances by ``n_samples`` on the device (inside a captured
        graph too: every replay draws fresh masks; ``MKGNN_MOLECULE=1`` does not reroute this call).  Otherwise -- more than one
        task (then every result is ``[n, T]``, ``samples [n, n_samples, T]``, ``pred`` is ``predict_tasks``'s), a shape or a
        molecule outside the fused tail, the CPU, ``MKGNN_SCORE_MC=0`` or ``MKGNN_FUSED_TAIL=0`` -- the PyTorch route: ``pred`` from
        ``predict`` / ``predict_tasks``, then the last layer's ``h`` once and per sample ``F.dropout``, ``lin2``, add-pool,
        ``F.dropout``, ``ffn``, then ``torch.var_mean``.  That is the same definition and the same distribution, but the masks come
        from PyTorch's generator, so the samples differ from the kernel route's.

        In training mode this raises, as ``predict`` does; a model whose two dropouts are both 0 has no dropout uncertainty:
        ``ValueError``; so is ``n_samples`` outside ``[1, 64]`` -- all before the batch is looked at."""
        from . import readout as R
        self._needs_eval("predict_mc")
        net = self.gnn_model
        p_head, p_readout = float(self.dropout.p), float(net.dropout.p)
        if p_head == 0.0 and p_readout == 0.0:
            raise ValueError("GNNModel.predict_mc: both dropouts of this model are 0 -- it has no dropout uncertainty (predict scores it)")
        S = R._check_mc_samples(n_samples)
        one_task = self.ffn.out_features == 1
        with torch.no_grad():
            nreal = getattr(data, 'n_valid_molecules', None)
            mc = (self.ffn, nreal, S, p_head, float(alpha), float(beta), bool(return_samples))
            out = net(data, _mc=mc if (one_task and data.x.is_cuda and p_head < 1.0) else ())
            if out[0] == "mc":
                result = out[1]
                result.pop("emb")
                return result
            # the PyTorch route: h once, the part behind the masks per sample
            pred = self.predict(data)[0].reshape(-1) if one_task else self.predict_tasks(data)[0]
            n, F = pred.shape[0], torch.nn.functional
            act = R.swish(net.graph_embedding_lin1(out[1]))
            slots = getattr(data, 'num_graphs', None)
            draws = []
            for _ in range(S):
                emb = net.pool(net.graph_embedding_lin2(F.dropout(act, p_readout, True)), data.batch, slots)
                draws.append(self.ffn(F.dropout(emb, p_head, True))[:n])
            samples = torch.stack(draws, dim=1)             # [n, S, T]
            if one_task:
                samples = samples.reshape(n, S)
            if S > 1:
                var, mean = torch.var_mean(samples, dim=1, unbiased=True)
                std = var.sqrt()
            else:
                mean = samples.select(1, 0).clone()
                std = torch.zeros_like(mean)
            result = {"pred": pred, "mean": mean, "std": std, "acq": float(alpha) * mean + float(beta) * std}
            if return_samples:
                result["samples"] = samples
            return result

    def _embedding(self, data):
        """``(graph_embedding [all slots, G], n)`` of a model in evaluation mode, inside the caller's ``no_grad``: the route
        ``predict_tasks`` and ``embed`` share.  On the GPU the forward-only tail is handed a one-row view of the head (which it needs;
        its own ``pred`` is dropped) and supplies the embedding where model and batch qualify; the separate operators otherwise."""
        nreal = getattr(data, 'n_valid_molecules', None)
        score = None
        if data.x.is_cuda:
            from types import SimpleNamespace
            bias = self.ffn.bias
            row = SimpleNamespace(weight=self.ffn.weight[:1], bias=None if bias is None else bias[:1], out_features=1)
            score = (row, nreal)
        out = self.gnn_model(data, _score=score)
        graph_embedding = out[2] if isinstance(out, tuple) else self.dropout(out)     # (the dropout is the identity here)
        return graph_embedding, (graph_embedding.shape[0] if nreal is None else int(nreal))

    def embed(self, data):
        """``graph_embedding [n, G]`` of a model in evaluation mode, under ``torch.no_grad()``: what the reference's embedding
        analysis compares molecules by, and what analogue search ranks (``screening.nearest``); ``n`` as in ``predict``.  It is
        ``predict_tasks(data)[1]`` bit for bit without the scores -- the same route (``_embedding``), for any ``task_dim``.  In
        training mode this raises."""
        self._needs_eval("embed")
        with torch.no_grad():
            graph_embedding, n = self._embedding(data)
            return graph_embedding[:n]

    def predict_tasks(self, data):
        """``(pred [n, T], graph_embedding [n, G])``: ALL ``T`` outputs of every molecule, for a model in evaluation mode, under
        ``torch.no_grad()`` -- what ranking a library per assay needs (``screening.score_resident_tasks``); ``n`` as in ``predict``.
        The network runs once: the embedding comes from the forward-only tail under ``predict``'s conditions (the tail is handed a
        one-row view of the head, which it needs, and its own ``pred`` is dropped) and from the separate operators otherwise; on the
        GPU ``pred`` is ``readout.task_scores`` of it -- one launch, bit for bit the task-indexed head's ``pred`` of every (molecule,
        task) pair.  ``predict`` keeps its own route (and bits) for a multi-task model.  In training mode this raises."""
        self._needs_eval("predict_tasks")
        with torch.no_grad():
            graph_embedding, n = self._embedding(data)
            if graph_embedding.is_cuda:
                from .readout import task_scores
                emb = graph_embedding if graph_embedding.dtype == torch.float32 else graph_embedding.float()
                pred = task_scores(emb, self.ffn, n_rows=n)
            else:
                pred = self.ffn(graph_embedding[:n])
            return pred, graph_embedding[:n]

    def atom_contributions(self, data):
        """``contrib [N, T]``: the exact share of every atom in every output, for a model in evaluation mode, under
        ``torch.no_grad()`` -- why a molecule scores what it scores.  ``lin2``, the add-pool and ``ffn`` are linear, so
        ``predict_tasks(data)[0][g, t] = ffn.bias[t] + sum of contrib[n, t] over the atoms n of molecule g``, exactly (up to float32
        rounding), for any ``task_dim``; for the docking-score model it explains the predicted score.  On the GPU, where
        ``readout.atom_contributions_supported`` holds, the last convolution leaves its block rows and ``mkgnn_atom_contributions``
        takes them (two launches; molecules of any size; the molecule-resident step is not taken); otherwise, and with
        ``MKGNN_ATOM_CONTRIB=0``, the same quantity comes from ``h`` through PyTorch operators (``readout.atom_contributions_torch``).
        ``N`` counts ALL atom rows of the batch: for a batch padded to a fixed shape the rows from ``n_valid_atoms`` on belong to
        padding atoms -- cut them, and find a molecule's rows, with ``data.mol_ptr``.  Nothing is read back to the host.  In
        training mode this raises, before the batch is looked at."""
        self._needs_eval("atom_contributions")
        with torch.no_grad():
            return self.gnn_model(data, _atoms=self.ffn)

    def kernel_scores(self, data, layer: int):
        """``(sim [N, K_layer], column_degree [K_layer], column_kernel [K_layer])``: what every kernel of convolution layer ``layer``
        (0: the 1-hop layer) scores on every atom, for a model in evaluation mode, under ``torch.no_grad()`` --
        ``MolKGNNNet.kernel_scores``, which is the definition: the node batch norm, then the public ``KernelSetConv`` layers
        ``0 .. layer`` with ``MolGCN.propagate`` between them; the layers behind, the readout and the head are not run, so any
        ``task_dim`` will do.  Row ``n`` holds the scores of atom ``n``'s own degree in that degree's columns (``column_degree``,
        ``column_kernel``: int32); nothing else of the row may be read.  The best-matching atoms of a library per kernel:
        ``screening.kernel_exemplars``.  The training and scoring forwards may choose differently among mathematically tied
        neighbour permutations in a few entries ("Ties"), so their scores can differ from these there.  In training
        mode, and for a ``layer`` outside ``[0, num_layers)``, this raises ``ValueError``."""
        self._needs_eval("kernel_scores")
        with torch.no_grad():
            return self.gnn_model.kernel_scores(data, layer)

    def _loss_kind(self) -> Optional[str]:
        """The loss as a kind of the HIP head (``readout.LOSS_KINDS``), or None: any other loss takes the PyTorch route."""
        lf = self.loss_func
        if type(lf) is BCEWithLogitsLoss and lf.reduction == "mean" and lf.pos_weight is None and lf.weight is None:
            return "bce"
        if type(lf) is MSELoss and lf.reduction in ("mean", "sum"):
            return "mse" if lf.reduction == "mean" else "mse_sum"
        return None

    def _task_loss(self, data, kind: str):
        """The masked multi-task loss (``readout.task_head_loss``): every molecule contributes the loss of the ONE output its task
        names -- ``data.task`` (one int32 task index per molecule, -1: no label; ``sampling.task_index``) or ``data.task_table`` +
        ``data.task_rows`` (a resident shard's table and the batch's molecule ids, ``padding.CompactStaticBatch.gather``).  The
        embedding comes from the separate readout operators (the molecule-resident step is single-task); with
        ``multi_output_tail`` on, the multi-output fused tail is asked first (``_multi_tail_embedding``)."""
        from .readout import task_head_loss
        p = self.dropout.p if (self.training and self.dropout.p < 1.0) else 0.0
        task, table, rows = _batch_tasks(data)
        graph_embedding = self._multi_tail_embedding(data, kind, None, dict(task=task, task_table=table, target=data.y), rows,
                                                     None, None, None, getattr(data, 'n_valid_molecules', None))
        if isinstance(graph_embedding, tuple):               # (multi_output_tail: the fused tail took it)
            return graph_embedding[1]
        if self.training and self.dropout.p >= 1.0:
            graph_embedding = self.dropout(graph_embedding)
        return task_head_loss(graph_embedding, self.ffn, data.y, task, kind, dropout_p=p,
                              n_rows=getattr(data, 'n_valid_molecules', None), task_table=table, row_ids=rows)

    def _kind_and_pos_weight(self, dev):
        """``(kind, pos_weight)``: ``_loss_kind()`` with no positive weight, or ``("bce", p [task_dim])`` for
        ``BCEWithLogitsLoss(reduction='mean', weight=None, pos_weight=p)`` (see ``_weighted_loss``); ``(None, None)`` otherwise."""
        lf, T = self.loss_func, self.ffn.out_features
        kind, pw = self._loss_kind(), None
        if kind is None and type(lf) is BCEWithLogitsLoss and lf.reduction == "mean" and lf.weight is None and lf.pos_weight is not None:
            p = lf.pos_weight
            if p.dtype != torch.float32 or p.device != dev or p.numel() not in (1, T):
                return None, None
            kind, pw = "bce", p.detach().reshape(-1)
            if pw.numel() != T:
                held = getattr(self, "_pos_weight_held", None)
                if held is None or held[0] is not p or held[1] != p._version:
                    held = self._pos_weight_held = (p, p._version, pw.expand(T).contiguous())
                pw = held[2]
        return kind, pw

    def _label_eval_kind(self, who: str) -> str:
        """The loss kind an evaluation of a label matrix reports (unweighted): ``_loss_kind()``, or ``"bce"`` for the ``pos_weight``
        BCE a multi-label model trains with."""
        lf = self.loss_func
        if type(lf) is BCEWithLogitsLoss and lf.reduction == "mean" and lf.weight is None:
            return "bce"
        return _required_loss_kind(self, who)

    def _weighted_loss(self, data):
        """``(kind, pos_weight, sample_weight, weight_table, weight_rows)`` when the loss is one of the HIP head's WEIGHTED losses
        (``readout.task_head_reference``), else None -- ``_loss_kind`` knows nothing of weights and stays as it is.
        ``pos_weight``: ``BCEWithLogitsLoss(reduction='mean', weight=None, pos_weight=p)`` with ``p`` a float32 tensor on the batch's
        device (a buffer of ``loss_func``: ``model.to(device)`` moves it) of ``task_dim`` elements, or of one, broadcast once and
        kept by tensor identity and version.  Sample weights: with any loss kind of ``_loss_kind`` (or that ``pos_weight`` loss), a
        batch that carries ``weight`` (float32, one per molecule) or ``weight_table`` with ``weight_rows`` (a resident shard's
        weights and the batch's molecule ids, ``padding.CompactStaticBatch.gather``).  A model with several outputs needs the
        batch's tasks (``task`` / ``task_table``) as well."""
        T, dev = self.ffn.out_features, data.x.device
        kind, pw = self._kind_and_pos_weight(dev)
        if kind is None:
            return None
        sw, table, rows = _batch_weight_fields(data)
        if sw is not None and not (torch.is_tensor(sw) and sw.dtype == torch.float32 and sw.device == dev):
            raise ValueError("batch.weight must be a float32 tensor on the batch's device (one loss weight per molecule)")
        if pw is None and sw is None and table is None:
            return None
        if T != 1 and not _has_tasks(data):
            return None
        return kind, pw, sw, table, rows

    def _weighted(self, data, kind: str, pw, sw, table, rows):
        """The weighted loss on its HIP route: mixed-assay batches on the task-indexed head (as ``_task_loss``), single-task ones on
        the fused tail where model and batch qualify and on the separate readout operators + the weighted head otherwise
        (``MKGNN_WEIGHTED_LOSS=0``: the definition in torch operators behind the separate readout).  The molecule-resident step is
        not taken."""
        from . import readout as R
        p = self.dropout.p if self.training else 0.0
        nreal = getattr(data, 'n_valid_molecules', None)
        task, ttable, trows = _batch_tasks(data)
        if task is not None or ttable is not None:
            graph_embedding = self._multi_tail_embedding(data, kind, pw, dict(task=task, task_table=ttable, target=data.y), trows,
                                                         sw, table, rows, nreal)
            if isinstance(graph_embedding, tuple):           # (multi_output_tail: the fused tail took it)
                return graph_embedding[1]
            sw, table, ids = _weights_for(graph_embedding, nreal, sw, table, rows, trows)
            return R.task_head_loss(graph_embedding, self.ffn, data.y, task, kind, dropout_p=p, n_rows=nreal, task_table=ttable,
                                    row_ids=ids, sample_weight=sw, pos_weight=pw, weight_table=table)
        kw = dict(sample_weight=sw, pos_weight=pw, weight_table=table, row_ids=rows)
        tail = (self.ffn, data.y, p, nreal, kind, kw) if R._WEIGHTED_LOSS else None
        graph_embedding = self.gnn_model(data, _tail=tail)
        if isinstance(graph_embedding, tuple):
            return graph_embedding[1]
        return R.head_loss(graph_embedding, self.ffn, data.y, kind, dropout_p=p, n_rows=nreal, **kw)

    def _weighted_definition(self, data, kind: str, pw, sw, table, rows):
        """The weighted loss as its definition in torch operators (``readout.task_head_reference``) behind the separate readout
        and ``self.dropout``: what a batch with weights gets where the HIP route does not apply (head dropout ``p >= 1``)."""
        from .readout import task_head_reference
        graph_embedding = self.dropout(self.gnn_model(data))
        task, ttable, trows = _batch_tasks(data)
        nreal = getattr(data, 'n_valid_molecules', None)
        sw, table, ids = _weights_for(graph_embedding, nreal, sw, table, rows, trows)
        return task_head_reference(graph_embedding, self.ffn.weight, self.ffn.bias, data.y, task, kind, None, nreal, ttable, ids,
                                   sw, pw, table)[0]

    def _label_loss(self, data):
        """The multi-label loss on a label matrix with holes (``readout.label_head_loss``): every molecule carries a row of labels
        -- ``data.labels`` (float32 ``[n, T]``, NaN: not measured) or ``data.label_table`` + ``data.label_rows`` (a resident shard's
        matrix and the batch's molecule ids, ``padding.CompactStaticBatch.gather``) -- so the network runs once per molecule.  The
        loss is one of ``_loss_kind()`` or the ``pos_weight`` BCE of ``_weighted_loss``; ``batch.weight`` / ``weight_table`` are passed
        on; ``n_valid_molecules`` is honoured.  The embedding comes from the separate readout operators, as for the task head (with
        ``multi_output_tail`` on, the multi-output fused tail is asked first).  A
        CPU batch, or head dropout ``p >= 1``, takes the definition (``readout.label_head_reference``) behind ``self.dropout``."""
        from . import readout as R
        if _has_tasks(data):
            raise ValueError("the batch carries both tasks (task / task_table) and a label matrix (labels / label_table): one "
                             "molecule names one task, or carries a row of labels, not both")
        kind, pw = self._kind_and_pos_weight(data.x.device)
        if kind is None:
            raise ValueError("the batch carries a label matrix (labels / label_table), which GNNModel.loss takes with "
                             "BCEWithLogitsLoss (optionally pos_weight) or MSELoss; it is never trained on batch.y instead")
        labels, ltable, lrows = _batch_fields(data, 'labels', 'label_table', 'label_rows')
        sw, table, rows = _batch_weight_fields(data)
        nreal = getattr(data, 'n_valid_molecules', None)
        graph_embedding = self._multi_tail_embedding(data, kind, pw, dict(labels=labels, label_table=ltable), lrows, sw, table,
                                                     rows, nreal)
        if isinstance(graph_embedding, tuple):               # (multi_output_tail: the fused tail took it)
            return graph_embedding[1]
        sw, table, ids = _weights_for(graph_embedding, nreal, sw, table, rows, lrows)
        if data.x.is_cuda and not (self.training and self.dropout.p >= 1.0):
            return R.label_head_loss(graph_embedding, self.ffn, labels, kind, dropout_p=self.dropout.p if self.training else 0.0,
                                     n_rows=nreal, label_table=ltable, row_ids=ids, sample_weight=sw, pos_weight=pw,
                                     weight_table=table)
        return R.label_head_reference(self.dropout(graph_embedding), self.ffn.weight, self.ffn.bias, labels, kind, None, nreal,
                                      ltable, ids, sw, pw, table)[0]

    def loss(self, data):
        if _has_labels(data):                                # (new field names: no batch without them changes its route)
            return self._label_loss(data)
        # a batch that carries loss weights gets them, or an error: never the unweighted loss in silence
        carries = any(f is not None for f in _batch_weight_fields(data))
        weighted = self._weighted_loss(data) if data.x.is_cuda else None
        full_dropout = self.training and self.dropout.p >= 1.0           # (head dropout p >= 1 keeps the PyTorch operator)
        if weighted is not None:
            if not full_dropout:
                return self._weighted(data, *weighted)
            if carries:                                      # (head dropout p >= 1 keeps its route; with weights: their definition)
                return self._weighted_definition(data, *weighted)
        elif carries:
            raise ValueError("the batch carries loss weights (weight / weight_table), which GNNModel.loss takes on a CUDA batch with "
                             "BCEWithLogitsLoss (optionally pos_weight) or MSELoss, and for several outputs with the batch's tasks")
        if data.x.is_cuda and _has_tasks(data):
            kind = self._loss_kind()
            if kind is not None:
                return self._task_loss(data, kind)
        kind = self._loss_kind() if self.ffn.out_features == 1 else None
        if kind is not None and data.x.is_cuda:
            from .readout import bce_head_loss, head_loss
            # dropout -> ffn -> loss in one kernel each way (same formula, 2 kernels instead of ~25; the dropout mask
            # comes from the kernels' own counter-based generator, see readout.head_rng_state)
            p = self.dropout.p if (self.training and not full_dropout) else 0.0
            if not full_dropout:
                # small batches: forward, loss and (when a gradient will be asked for) the whole backward in one launch
                from . import molecule as _mol
                fused = _mol.loss_forward(self, data, p, kind)
                if fused is not None:
                    return fused
            nreal = getattr(data, 'n_valid_molecules', None)
            # large batches: everything behind the last convolution -- readout, head, loss and their gradients -- in one launch
            # (readout.tail_loss) where the model and the batch qualify; the embedding otherwise
            tail = None if full_dropout else (self.ffn, data.y, p, nreal, kind)
            graph_embedding = self.gnn_model(data, _tail=tail)
            if isinstance(graph_embedding, tuple):
                return graph_embedding[1]
            if full_dropout:
                graph_embedding = self.dropout(graph_embedding)
            # (a padded batch: the padding molecules' rows take no part in the loss -- the head reads the first nreal rows)
            if kind != "bce":
                return head_loss(graph_embedding, self.ffn, data.y, kind, dropout_p=p, n_rows=nreal)
            return bce_head_loss(graph_embedding, self.ffn, data.y, dropout_p=p, n_rows=nreal)
        pred, _ = self(data)
        return self.loss_func(pred.view(-1), data.y.view(-1).float())


def _batch_fields(data, direct: str = 'task', table: str = 'task_table', rows: str = 'task_rows'):
    """``(task, task_table, task_rows)`` of a batch (or the weight fields, by name): one given directly is taken before a table; a
    table needs its rows."""
    d, t, r = (getattr(data, name, None) for name in (direct, table, rows))
    return (d, None, None) if (d is not None or t is None or r is None) else (None, t, r)


def _batch_tasks(data):
    return _batch_fields(data)


def _has_tasks(data) -> bool:
    return any(f is not None for f in _batch_fields(data))


def _has_labels(data) -> bool:
    return any(f is not None for f in _batch_fields(data, 'labels', 'label_table', 'label_rows'))


def _batch_weight_fields(data):
    return _batch_fields(data, 'weight', 'weight_table', 'weight_rows')


def _weights_for(graph_embedding, nreal, sw, table, rows, trows):
    """``(sample_weight, weight_table, row_ids)`` for a weighted call whose tasks are read through ``trows`` (or None): the kernels
    read ONE id vector, so a weight table read through a different one than the task table is looked up here."""
    if table is not None and trows is not None and rows is not trows:
        from .readout import _row_weights
        return _row_weights(None, table, rows, graph_embedding.shape[0] if nreal is None else int(nreal)), None, trows
    return sw, table, trows if trows is not None else rows


_ONES: dict = {}


def backward(loss: torch.Tensor) -> None:
    """``loss.backward()`` with the kernel-bank gradients of every KernelSetConv left running beside the layers below
    (functional.deferred_bank_gradients); all of them are complete, in stream order, when this returns -- which is
    all the optimiser (or a gradient all-reduce) that follows needs.  Use it where parameters' ``.grad`` start out as
    None (``zero_grad(set_to_none=True)``); calls that would accumulate are simply not deferred."""
    from .functional import deferred_bank_gradients
    # d loss / d loss = 1 from a tensor that already exists (autograd otherwise fills a fresh one: a launch per step)
    key = (loss.device, loss.dtype)
    one = _ONES.get(key)
    if one is None:
        if loss.is_cuda and torch.cuda.is_current_stream_capturing():
            one = None                        # (first use inside a capture: let autograd make its own this once)
        else:
            one = _ONES[key] = torch.ones((), dtype=loss.dtype, device=loss.device)
            from .readout import register_unit_gradient
            register_unit_gradient(one)       # the head's fused forward has d loss = 1 gradients ready: nothing to launch
    with deferred_bank_gradients():
        if one is not None and loss.dim() == 0:
            loss.backward(one)
        else:
            loss.backward()


def training_step(model, batch, optimizer=None) -> torch.Tensor:
    """``loss = model.loss(batch); backward(loss); optimizer.step()`` as ONE unit (gradients start out as None): what a training loop
    does per batch, with the licence that gives -- nothing reads the loss or a parameter gradient between the forward and the
    optimiser, so the fused tail's last reduction leaves the critical chain (``readout.deferred_tail_reduce``).  Returns the loss
    (complete, in stream order, when this returns).  Same kernels, same arithmetic, same bits as the three calls.

    The deferral is skipped (the reduction runs in the forward, as outside a region) when a tail parameter -- the readout's
    ``graph_embedding_lin1`` / ``graph_embedding_lin2`` and ``ffn`` -- has a tensor hook or a post-accumulate-grad hook, or is
    not contiguous.  A hook registered on a parameter's AccumulateGrad node (``p.view_as(p).grad_fn.next_functions[0][0]``, the
    older DDP mechanism) cannot be seen from the parameter: such code opts out with ``MKGNN_TAIL_DEFER=0`` or calls
    ``model.loss`` + ``backward`` itself, outside ``training_step``."""
    from .readout import deferred_tail_reduce
    model.zero_grad(set_to_none=True)
    with deferred_tail_reduce(batch.x.device if batch.x.is_cuda else None):
        loss = model.loss(batch)
        backward(loss)
    if optimizer is not None:
        optimizer.step()
    return loss


def _metric_functions() -> dict:
    """The metric names of the reference's ``get_evaluations`` (``model.py:499-522``) -> ``f(true_y, pred_y)`` of
    ``molkgnn_amd.evaluation``."""
    from . import evaluation as E
    return {
        'accuracy': E.calculate_accuracy,
        'RMSE': E.calculate_rmse,
        'logAUC_0.001_0.1': E.calculate_logAUC,
        'logAUC_0.001_1': lambda true_y, pred_y: E.calculate_logAUC(true_y, pred_y, FPR_range=(0.001, 1)),
        'ppv': E.calculate_ppv,
        'f1_score': E.calculate_f1_score,
        'AUC': E.calculate_auc,
    }


def _early_metric(name):
    """``f(true_y, pred_y)`` for an early-recognition name (``'AP'``, ``'EF_<fraction>'``, ``'BEDROC_<alpha>'``), ``None`` for any other
    name; a malformed one raises ``ValueError``."""
    from . import evaluation as E
    if not E.is_early_name(name):
        return None
    kind, value = E.parse_early_name(name)
    if kind == 'AP':
        return E.calculate_average_precision
    if kind == 'EF':
        return lambda true_y, pred_y: E.calculate_enrichment_factor(true_y, pred_y, value)
    return lambda true_y, pred_y: E.calculate_bedroc(true_y, pred_y, value)


def _regression_metric(name, lower_is_better: bool = True):
    """``f(true_y, pred_y)`` for a regression name beyond ``'RMSE'`` (``'MAE'``, ``'R2'``, ``'pearson'``, ``'spearman'``,
    ``'top_<fraction>'``), ``None`` for any other name; a malformed ``'top_'`` name raises ``ValueError``."""
    from . import evaluation as E
    plain = {'MAE': E.calculate_mae, 'R2': E.calculate_r2, 'pearson': E.calculate_pearson, 'spearman': E.calculate_spearman}
    if isinstance(name, str) and name in plain:
        return plain[name]
    if not E.is_top_name(name):
        return None
    fraction = E.parse_top_name(name)
    return lambda true_y, pred_y: E.calculate_top_recall(true_y, pred_y, fraction, lower_is_better)


def _check_metrics(metrics, lower_is_better: bool = True) -> dict:
    """``_metric_functions()`` and the early-recognition and regression names among ``metrics``, once every name in ``metrics`` is
    known to be one of them."""
    table = _metric_functions()
    for m in metrics:
        if m not in table:
            fn = _early_metric(m) or _regression_metric(m, lower_is_better)
            if fn is not None:
                table[m] = fn
    unknown = [m for m in metrics if m not in table]
    if unknown:
        raise ValueError(f"unknown metric(s) {unknown}: one of {sorted(_metric_functions())}, 'AP', 'EF_<fraction>' or "
                         f"'BEDROC_<alpha>', or the regression metrics 'MAE', 'R2', 'pearson', 'spearman' or 'top_<fraction>'")
    _early_names(metrics)
    _top_fractions(metrics)
    return table


def _top_fractions(metrics) -> tuple:
    """The distinct fractions of the ``'top_<fraction>'`` names among ``metrics``, which the evaluate functions hand to the regression
    bootstrap (too many: refused before anything is launched)."""
    from .evaluation import BOOTSTRAP_MAX_CUTS, is_top_name, parse_top_name
    fractions = []
    for m in metrics:
        if is_top_name(m) and parse_top_name(m) not in fractions:
            fractions.append(parse_top_name(m))
    if len(fractions) > BOOTSTRAP_MAX_CUTS:
        raise ValueError(f"{len(fractions)} distinct top fractions, at most {BOOTSTRAP_MAX_CUTS} per call")
    return tuple(fractions)


def _early_names(metrics) -> tuple:
    """The early-recognition names among ``metrics``, which the evaluate functions hand to the bootstrap."""
    from .evaluation import EarlySpec, is_early_name
    names = tuple(m for m in metrics if is_early_name(m))
    EarlySpec(names)                             # (too many distinct fractions or alphas: refused before anything is launched)
    return names


def _required_loss_kind(model, who: str) -> str:
    kind = model._loss_kind()
    if kind is None:
        raise ValueError(f"{who} needs one of the head's loss kinds (BCEWithLogitsLoss(), MSELoss(), MSELoss('sum'))")
    return kind


@contextmanager
def evaluation_mode(model):
    """``with evaluation_mode(model):`` -- the model in evaluation mode inside, and back in the mode it came in afterwards, also
    when the body raises."""
    was_training = model.training
    model.eval()
    try:
        yield model
    finally:
        model.train(was_training)


def _check_bootstrap(bootstrap) -> Optional[int]:
    """The ``bootstrap`` keyword of the evaluate functions: ``None`` (no bootstrap: results and launches as without the keyword) or
    the number of replicates, an integer of at least 1; anything else raises before a batch is run."""
    if bootstrap is None:
        return None
    if isinstance(bootstrap, bool) or not isinstance(bootstrap, int) or bootstrap < 1:
        raise ValueError(f"bootstrap = {bootstrap!r}: None, or the number of replicates (an integer >= 1)")
    return bootstrap


def _results(model, pred_y: torch.Tensor, true_y: torch.Tensor, metrics, table: dict, bootstrap: Optional[int] = None,
             lower_is_better: bool = True) -> dict:
    """The second half of ``evaluate`` and of ``evaluate_resident``: ``validation_epoch_end`` + ``get_evaluations`` on the whole
    vectors -- the model's loss, every metric, and the two vectors themselves; with ``bootstrap`` replicates also
    ``evaluation.bootstrap_metrics`` of them (``results['bootstrap']``), or, for a model that trains a squared error (``_loss_kind()``
    ``'mse'`` or ``'mse_sum'``), ``evaluation.bootstrap_regression``."""
    with torch.no_grad():
        results = {'loss': model.loss_func(pred_y, true_y.float())}
    for m in metrics:
        results[m] = table[m](true_y, pred_y)
    if bootstrap is not None:
        kind = getattr(model, '_loss_kind', None)
        if kind is not None and kind() in ('mse', 'mse_sum'):
            from .evaluation import bootstrap_regression
            results['bootstrap'] = bootstrap_regression(true_y, pred_y.detach(), n_boot=bootstrap, top=_top_fractions(metrics),
                                                        lower_is_better=lower_is_better)
        else:
            from .evaluation import bootstrap_metrics
            results['bootstrap'] = bootstrap_metrics(true_y, pred_y.detach(), n_boot=bootstrap, early=_early_names(metrics))
    results['pred_y'], results['true_y'] = pred_y, true_y
    return results


def evaluate(model, batches, metrics=(), bootstrap: Optional[int] = None, lower_is_better: bool = True) -> dict:
    """The reference's validation / test loop without Lightning: ``validation_step`` per batch (``model.py:221-244``:
    ``pred_y = self(batch)[0].view(-1)``, ``true_y = batch.y.view(-1)``), then ``validation_epoch_end`` + ``get_evaluations``
    (``model.py:246-296, 483-522``) on the concatenated vectors: ``loss = model.loss_func(all_pred, all_true.float())`` and
    every metric named in ``metrics`` (``accuracy``, ``RMSE``, ``logAUC_0.001_0.1``, ``logAUC_0.001_1``, ``ppv``, ``f1_score``,
    ``AUC``; any other name raises ``ValueError`` before a batch is run) through ``molkgnn_amd.evaluation``.  The result also
    holds ``pred_y`` and ``true_y``, the two vectors ``record_valid_pred`` writes out.

    The model is put in evaluation mode and handed back in the mode it came in, also when a batch raises.  Predictions come
    from ``model.predict``; they and the labels (the first ``len(pred)`` of a batch's ``y``: a padded batch's real molecules)
    stay on their device, and nothing synchronises with the host before the last batch is launched.  Writing files and
    logging are the caller's.

    ``bootstrap``: ``None``, or a number of replicates -- then ``results['bootstrap']`` is ``evaluation.bootstrap_metrics(true_y,
    pred_y, n_boot=bootstrap)``: the percentile intervals of AUC and ``logAUC_0.001_0.1`` under resampling of the molecules.

    ``metrics`` also takes the early-recognition names ``'AP'``, ``'EF_<fraction>'`` and ``'BEDROC_<alpha>'`` (``evaluation.
    calculate_average_precision``, ``calculate_enrichment_factor``, ``calculate_bedroc``); with ``bootstrap`` those named are handed on as
    ``bootstrap_metrics(..., early=...)`` and get their intervals from the same resamples.  A call that names none behaves as before.

    The regression names ``'MAE'``, ``'R2'``, ``'pearson'``, ``'spearman'`` and ``'top_<fraction>'`` (``evaluation.calculate_mae``,
    ``calculate_r2``, ``calculate_pearson``, ``calculate_spearman``, ``calculate_top_recall``) are taken too; ``lower_is_better`` (lower
    docking scores are the better ones) is read by the ``'top_'`` names alone.  For a model whose loss is ``MSELoss`` (mean or sum)
    ``bootstrap`` gives ``results['bootstrap'] = evaluation.bootstrap_regression(true_y, pred_y, n_boot=bootstrap, top=<the fractions
    named>, lower_is_better=...)`` -- intervals for RMSE, MAE, R2, Pearson, Spearman and every named recall; a model with any other loss,
    and a call that names none of these, behaves as before."""
    table = _check_metrics(metrics, lower_is_better)
    bootstrap = _check_bootstrap(bootstrap)
    with evaluation_mode(model):
        all_pred, all_true = [], []
        for batch in batches:
            pred, _ = model.predict(batch)
            pred = pred.view(-1)
            all_pred.append(pred)
            all_true.append(batch.y.view(-1)[:pred.shape[0]])
        if not all_pred:
            raise ValueError("evaluate needs at least one batch")
        return _results(model, torch.cat(all_pred), torch.cat(all_true), metrics, table, bootstrap, lower_is_better)


def _task_results(pred: torch.Tensor, true_y: torch.Tensor, task: torch.Tensor, T: int, kind: str, metrics, table: dict,
                  bootstrap: Optional[int] = None) -> dict:
    """The second half of ``evaluate_tasks`` and of ``evaluate_resident_tasks``: from ``pred [n, >= 1]``, the labels and every
    molecule's task (int64) to the result dictionary -- the column selection, ``evaluation.per_task`` per metric and the masked
    multi-task loss (``readout.task_head_reference`` on the selected column)."""
    import math
    from .evaluation import per_task
    from .readout import task_head_reference
    lab = (task >= 0) & (task < min(T, pred.shape[1]))
    col = torch.where(lab, task, torch.zeros_like(task))
    pred_y = torch.where(lab, pred.gather(1, col[:, None]).view(-1), torch.full((), float("nan"), dtype=pred.dtype, device=pred.device))
    with torch.no_grad():
        # (the head's expression on the selected column: an identity "embedding" of width 1 per task is the column itself)
        sel = torch.where(lab, pred_y, torch.zeros_like(pred_y))
        results = {'loss': task_head_reference(sel[:, None], torch.ones(T, 1, dtype=pred.dtype, device=pred.device), None,
                                               true_y, torch.where(lab, task, torch.full_like(task, -1)), kind)[0]}
    for m in metrics:
        results[m] = per_task(true_y, pred_y, torch.where(lab, task, torch.full_like(task, -1)), table[m], T)
        defined = [float(v) for v in results[m] if not math.isnan(float(v))]
        results[m + '_mean'] = sum(defined) / len(defined) if defined else float("nan")
    if bootstrap is not None:                    # (per task: evaluation.bootstrap_per_task, None for a task it cannot resample)
        from .evaluation import bootstrap_per_task
        results['bootstrap'] = bootstrap_per_task(true_y, pred_y.detach(), torch.where(lab, task, torch.full_like(task, -1)), T,
                                                  n_boot=bootstrap, early=_early_names(metrics))
    results['pred_y'], results['true_y'], results['task'] = pred_y, true_y, task
    return results


def evaluate_tasks(model, batches, metrics=(), num_tasks: Optional[int] = None, bootstrap: Optional[int] = None) -> dict:
    """``evaluate`` for a multi-task model on mixed-assay batches that carry ``task`` (one task index per molecule, -1: no label;
    ``sampling.task_index``): ``model.predict`` per batch, keeping ``pred [n, T]``.  ``results[m]`` is the list of metric ``m``
    per task over that task's labelled molecules (``evaluation.per_task``; ``nan`` for a task without any), ``results[m + '_mean']``
    its mean over the tasks with a defined (non-NaN) value, ``results['loss']`` the masked multi-task loss of the concatenated
    vectors (``readout.task_head_reference`` on the model's loss kind), ``pred_y`` every molecule's prediction for ITS task (NaN
    where it has none), ``true_y`` and ``task``.  ``num_tasks`` defaults to the model's outputs.  The model is put in evaluation
    mode and handed back in the mode it came in, also when a batch raises.  ``bootstrap``: ``None``, or a number of replicates --
    then ``results['bootstrap']`` is ``evaluation.bootstrap_per_task`` of the vectors, one entry per task."""
    table = _check_metrics(metrics)
    bootstrap = _check_bootstrap(bootstrap)
    kind = _required_loss_kind(model, "evaluate_tasks")
    T = model.ffn.out_features if num_tasks is None else int(num_tasks)
    with evaluation_mode(model):
        all_pred, all_true, all_task = [], [], []
        for batch in batches:
            task = getattr(batch, 'task', None)
            if task is None:
                raise ValueError("evaluate_tasks needs batch.task (sampling.task_index of the batch's assay ids)")
            pred, _ = model.predict(batch)
            n = pred.shape[0]
            all_pred.append(pred.reshape(n, -1))
            all_true.append(batch.y.view(-1)[:n])
            all_task.append(task.view(-1)[:n].to(pred.device))
        if not all_pred:
            raise ValueError("evaluate_tasks needs at least one batch")
        return _task_results(torch.cat(all_pred), torch.cat(all_true), torch.cat(all_task).long(), T, kind, metrics, table,
                             bootstrap)


def evaluate_resident(model, resident, batch_size: int, metrics=(), bootstrap: Optional[int] = None,
                      lower_is_better: bool = True) -> dict:
    """``evaluate`` for a data set that lives in device memory (``shards.ResidentShard``): the same result dictionary, with
    ``pred_y`` from ``screening.score_resident`` -- every molecule of the shard in id order, the short tail included, from one
    captured graph -- and ``true_y`` from ``resident.y``.  Unknown metric names raise before anything is launched; the model
    comes back in the mode it came in.  ``bootstrap`` and ``lower_is_better``: as in ``evaluate``."""
    from .screening import score_resident
    table = _check_metrics(metrics, lower_is_better)
    bootstrap = _check_bootstrap(bootstrap)
    pred_y = score_resident(model, resident, batch_size)
    return _results(model, pred_y, resident.y.to(pred_y.device).view(-1), metrics, table, bootstrap, lower_is_better)


def evaluate_resident_tasks(model, resident, batch_size: int, metrics=(), bootstrap: Optional[int] = None) -> dict:
    """``evaluate_tasks`` for a mixed-assay data set that lives in device memory (``shards.ResidentShard(..., assays=...)``): the
    same result dictionary, from ``screening.score_resident_tasks`` -- all ``T`` outputs of every molecule of the shard in id
    order, the short tail included, from one captured graph -- with ``resident.y`` as the labels and ``resident.task`` as every
    molecule's task; then exactly what ``evaluate_tasks`` does with its concatenated vectors (``_task_results``).  The predictions
    are ``readout.task_scores``' (``evaluate_tasks`` takes ``model.predict``'s, a GEMM: equal in value, not in every bit).  Unknown
    metric names, a shard without ``assays`` and a loss that is none of the head's kinds raise before anything is launched; the
    model comes back in the mode it came in.  ``bootstrap``: as in ``evaluate_tasks``."""
    from .screening import score_resident_tasks
    table = _check_metrics(metrics)
    bootstrap = _check_bootstrap(bootstrap)
    if getattr(resident, "task", None) is None:
        raise ValueError("evaluate_resident_tasks needs a shard that knows every molecule's task: ResidentShard(..., assays=...)")
    kind = _required_loss_kind(model, "evaluate_resident_tasks")
    pred = score_resident_tasks(model, resident, batch_size)
    true_y = resident.y.to(pred.device).view(-1)
    task = resident.task.to(pred.device).view(-1).long()
    return _task_results(pred, true_y, task, model.ffn.out_features, kind, metrics, table, bootstrap)


def _label_results(model, who: str, pred: torch.Tensor, labels: torch.Tensor, metrics, table: dict, bootstrap) -> dict:
    """The second half of ``evaluate_labels`` and ``evaluate_resident_labels``: the labelled (non-NaN) entries of ``labels [n, T]``,
    in row-major order, as ``(true, pred row, task)`` triples for ``_task_results``; plus ``n_labelled`` per task."""
    T = model.ffn.out_features
    if labels.dim() != 2 or tuple(labels.shape) != (pred.shape[0], T):
        raise ValueError(f"{who}: the labels must be [{pred.shape[0]}, {T}], not {tuple(labels.shape)}")
    lab = ~torch.isnan(labels)
    row, task = lab.nonzero(as_tuple=True)
    results = _task_results(pred[row], labels[row, task].to(pred.dtype), task, T, model._label_eval_kind(who), metrics, table,
                            bootstrap)
    results['n_labelled'] = lab.sum(dim=0).tolist()
    return results


def evaluate_labels(model, batches, metrics=(), bootstrap: Optional[int] = None) -> dict:
    """``evaluate_tasks`` for a multi-label model on batches that carry a label matrix ``labels`` (float ``[n, T]``, NaN: not
    measured): ``model.predict_tasks`` per batch (the network runs once per molecule), the labelled entries flattened to ``(true,
    pred, task)`` triples in row-major order and handed to the per-task machinery of ``evaluate_tasks`` (``_task_results``,
    ``evaluation.bootstrap_per_task``).  The result has ``evaluate_tasks``' keys -- ``pred_y``, ``true_y`` and ``task`` have one
    element per labelled ENTRY, ``loss`` is the unweighted multi-label loss -- plus ``n_labelled``, the labelled entries per task."""
    table = _check_metrics(metrics)
    bootstrap = _check_bootstrap(bootstrap)
    model._label_eval_kind("evaluate_labels")
    with evaluation_mode(model):
        all_pred, all_labels = [], []
        for batch in batches:
            labels = getattr(batch, 'labels', None)
            if labels is None:
                raise ValueError("evaluate_labels needs batch.labels (float [n, T], NaN: not measured)")
            pred, _ = model.predict_tasks(batch)
            all_pred.append(pred)
            all_labels.append(labels[:pred.shape[0]].to(pred.device))
        if not all_pred:
            raise ValueError("evaluate_labels needs at least one batch")
        return _label_results(model, "evaluate_labels", torch.cat(all_pred), torch.cat(all_labels), metrics, table, bootstrap)


def evaluate_resident_labels(model, resident, batch_size: int, metrics=(), bootstrap: Optional[int] = None) -> dict:
    """``evaluate_labels`` for a multi-label data set that lives in device memory (``shards.ResidentShard(..., labels=...)``): the
    same result dictionary, from ``screening.score_resident_tasks`` -- all ``T`` outputs of every molecule of the shard in id
    order from one captured graph -- with ``resident.labels`` as the label matrix.  Unknown metric names, a shard without
    ``labels`` and a loss that is none of the head's kinds raise before anything is launched."""
    from .screening import score_resident_tasks
    table = _check_metrics(metrics)
    bootstrap = _check_bootstrap(bootstrap)
    if getattr(resident, "labels", None) is None:
        raise ValueError("evaluate_resident_labels needs a shard that holds a label matrix: ResidentShard(..., labels=...)")
    model._label_eval_kind("evaluate_resident_labels")
    pred = score_resident_tasks(model, resident, batch_size)
    return _label_results(model, "evaluate_resident_labels", pred, resident.labels.to(pred.device), metrics, table, bootstrap)


def tune_torch_backends() -> None:
    """PyTorch-side knobs for the plain-PyTorch parts of the step (readout GEMMs).  The weight-gradient GEMM
    [32 x N] @ [N x 110] (N ~ 1e5) takes ~225 us through hipBLASLt and ~53 us through rocBLAS on MI355X."""
    try:
        torch.backends.cuda.preferred_blas_library("cublas")     # = rocBLAS on ROCm
    except Exception:
        pass


def configure_optimizer(model: torch.nn.Module, weight_decay: float = 0.0, lr: float = 1e-3, fused: Optional[bool] = None,
                        capturable: bool = False, max_grad_norm: Optional[float] = None, skip_nonfinite: bool = False,
                        average: Optional[str] = None, average_decay: float = 0.999, average_warmup: bool = True,
                        average_start: int = 0):
    """AdamW with the kernel parameters exempt from weight decay, selected by name (model.py:373-382).

    ``max_grad_norm`` / ``skip_nonfinite``: clip the gradients by their global norm (Lightning's ``gradient_clip_val`` with
    ``gradient_clip_algorithm='norm'``) and skip a step whose norm is not finite, inside the fused step and on the device
    (``optim.FusedAdamW``).  The ``torch.optim.AdamW`` route has neither: asking for one there is an error, not ignored.

    ``average='ema' | 'mean'`` (with ``average_decay`` / ``average_warmup`` / ``average_start``): an average of the weights kept
    inside the fused step (``optim.FusedAdamW``); evaluate with it through ``averaged_weights(model, optimizer)``.  The
    ``torch.optim.AdamW`` route has none: asking for it there is an error (``torch.optim.swa_utils.AveragedModel`` is torch's)."""
    decay, nodecay = [], []
    for name, p in model.named_parameters():
        if ('x_center' in name) or ('p_support' in name) or (
                ('edge_attr_support' in name) and ('edge_attr_support_sc' not in name)) or ('x_support' in name):
            nodecay.append(p)
        else:
            decay.append(p)
    groups = [{'params': nodecay, 'weight_decay': 0}, {'params': decay, 'weight_decay': weight_decay}]
    if fused is None:
        fused = all(p.is_cuda and p.dtype == torch.float32 for p in model.parameters())
    if fused:
        from .optim import FusedAdamW     # one HIP launch for the whole model; step counters on the device (capturable)
        opt = FusedAdamW(groups, lr=lr, max_grad_norm=max_grad_norm, skip_nonfinite=skip_nonfinite, average=average,
                         average_decay=average_decay, average_warmup=average_warmup, average_start=average_start)
        opt.prepare_state()               # state exists before anything can be captured (a fill inside a graph would replay)
        return opt
    if max_grad_norm is not None or skip_nonfinite:
        raise ValueError("max_grad_norm / skip_nonfinite are part of the fused AdamW step (fused=True); with torch.optim.AdamW call "
                         "torch.nn.utils.clip_grad_norm_ between backward and step")
    if average is not None:
        raise ValueError("average is part of the fused AdamW step (fused=True); with torch.optim.AdamW wrap the model in "
                         "torch.optim.swa_utils.AveragedModel")
    kw = {}
    if capturable:
        kw["capturable"] = True          # step counters live on the device: the step can be replayed from a hipGraph
    return torch.optim.AdamW(groups, lr=lr, **kw)


def _averaging(optimizer, who: str):
    from .optim import FusedAdamW
    if not isinstance(optimizer, FusedAdamW) or optimizer.average is None:
        raise ValueError(f"{who}: the optimiser keeps no average (configure_optimizer(..., average='ema' | 'mean'))")
    return optimizer


@contextmanager
def averaged_weights(model, optimizer):
    """``with averaged_weights(model, optimizer): evaluate(model, ...)`` -- inside the block ``model``'s parameters hold the
    averages the optimiser keeps (exchanged in place in one launch, ``FusedAdamW.swap_averaged``), after it the live weights
    again, also when the block raises; ``optimizer.step()`` inside it raises.  The banks are prepared from the parameters on every
    forward call, so nothing cached needs invalidating.  Buffers -- the batch-norm running statistics -- are the live model's."""
    opt = _averaging(optimizer, "averaged_weights")
    held = opt.averaged_parameters()
    missing = [n for n, p in model.named_parameters() if p.numel() and p not in held]
    if missing:
        raise ValueError(f"averaged_weights: the optimiser holds no average of {missing[:3]} ({len(missing)} parameters)")
    with opt.averaged_weights():
        yield model


def averaged_state_dict(model, optimizer) -> dict:
    """``model.state_dict()`` with a copy of the averaged value in place of every parameter the optimiser averages; buffers, and
    parameters the optimiser does not hold, as they stand."""
    held = _averaging(optimizer, "averaged_state_dict").averaged_parameters()
    sd = model.state_dict()
    prefix_of = {id(p): n for n, p in model.named_parameters()}
    for p, avg in held.items():
        name = prefix_of.get(id(p))
        if name is not None and name in sd:
            sd[name] = avg.detach().clone()
    return sd


class CapturedSteps:
    """``loss = steps(batch)``: one training step (``model.loss`` -> ``backward`` -> ``optimizer.step``) per call, launched eagerly
    the first ``warmup`` times a batch is seen and from a hipGraph captured on its next visit afterwards.

    The reference's harness launches every operator of every step from Python (Lightning's loop around ``model.py``); with the
    HIP operators that costs 2-3 ms of host time per step at batch 16-256, against 0.25-0.28 ms of GPU work (bench.py,
    ``small_batch.*.paths.eager_ms_per_step``).  A loop that revisits its batches -- several epochs over resident data -- gets the
    replayed step with two lines::

        steps = CapturedSteps(model, optimizer)
        for epoch in range(E):
            for batch in resident_batches:
                loss = steps(batch)            # a 0-d tensor, valid until the next call with the SAME batch

    A batch is recognised by the identity of its object and of its ``x`` tensor (held weakly until it is captured: a batch that
    is freed leaves no count behind, and a new batch at a recycled address starts from zero); it must stay alive and unchanged to
    be captured (a batch whose tensors are refilled in place belongs in ``padding.StaticBatch``, which is built for that).  Each
    captured batch keeps its own graph (and the memory of one step's activations): ``max_graphs`` bounds their number, batches
    beyond it stay eager.  At most ``4 * max_graphs`` uncaptured batches are counted; beyond that the least recently seen is
    forgotten.  A streaming loader whose batches are seen once is therefore never captured and runs ``training_step``.
    ``optimizer`` must be capturable to be captured at all (``configure_optimizer(..., capturable=True)`` or the fused AdamW);
    with any other optimiser every step stays eager."""

    def __init__(self, model: torch.nn.Module, optimizer=None, warmup: int = 2, max_graphs: int = 64):
        self.model, self.optimizer = model, optimizer
        self.warmup, self.max_graphs = int(warmup), int(max_graphs)
        self.max_seen = 4 * self.max_graphs
        self._seen: dict = {}          # key -> [visits, weakref to the batch, weakref to its x], least recently seen first
        self._graphs: dict = {}        # key -> (graph, loss, batch, x)
        self._stream = None
        self._capturable = _optimizer_capturable(optimizer)

    def _key(self, batch):
        return (id(batch), batch.x.data_ptr(), batch.x._version)

    def _eager(self, batch):
        return training_step(self.model, batch, self.optimizer).detach()

    def _count(self, key, batch) -> int:
        """Visits of ``batch`` before this one (and this one recorded)."""
        hit = self._seen.pop(key, None)
        n = hit[0] if hit is not None and hit[1]() is batch and hit[2]() is batch.x else 0
        if n == 0:
            me = weakref.ref(self)

            def forget(ref, key=key):              # (the batch or its x is gone: so is its count -- unless the slot was reused)
                d = None if me() is None else me()._seen
                entry = None if d is None else d.get(key)
                if entry is not None and (entry[1] is ref or entry[2] is ref):
                    del d[key]
            hit = [0, weakref.ref(batch, forget), weakref.ref(batch.x, forget)]
        hit[0] = n + 1
        self._seen[key] = hit
        while len(self._seen) > self.max_seen:
            del self._seen[next(iter(self._seen))]
        return n

    def __call__(self, batch):
        key = self._key(batch)
        hit = self._graphs.get(key)
        if hit is not None and hit[2] is batch and hit[3] is batch.x:
            graph, static_loss = hit[0], hit[1]
            graph.replay()
            return static_loss
        n = self._count(key, batch)
        if n < self.warmup or len(self._graphs) >= self.max_graphs or not batch.x.is_cuda or not self._capturable:
            return self._eager(batch)
        self._seen.pop(key, None)
        if self._stream is None:
            self._stream = torch.cuda.Stream(device=batch.x.device)
        side = self._stream
        side.wait_stream(torch.cuda.current_stream(batch.x.device))
        with torch.cuda.stream(side):
            self.model.zero_grad(set_to_none=True)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=side):
                static_loss = training_step(self.model, batch, self.optimizer).detach()
        torch.cuda.current_stream(batch.x.device).wait_stream(side)
        self._graphs[key] = (graph, static_loss, batch, batch.x)     # (the batch is kept: its id and x's address stay its own)
        graph.replay()                                        # (a capture launches nothing: this visit's step)
        return static_loss


def _optimizer_capturable(optimizer) -> bool:
    """Can ``optimizer.step()`` be captured and replayed: the fused AdamW (step counters on the device), or a torch optimiser
    with ``capturable=True`` in every parameter group.  (None: no optimiser step to capture.)"""
    if optimizer is None:
        return True
    from .optim import FusedAdamW
    if isinstance(optimizer, FusedAdamW):
        return True
    return all(g.get("capturable", False) for g in optimizer.param_groups)
