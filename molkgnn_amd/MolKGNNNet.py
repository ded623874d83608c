"""Consumer of the hot path, kept so that the reference's ``model.py`` can build
it unchanged: BatchNorm(x) -> MolGCN -> lin2(dropout(swish(lin1(h)))) -> add-pool
(reference ``models/MolKGNN/MolKGNNNet.py:10-149``).  ``MolGCN`` is the hot
path; the batch norm in front of it and the readout behind it run as HIP
operators too (``readout.py``).
"""
from __future__ import annotations

import torch
from torch.nn import BatchNorm1d, Dropout, Linear

from .KernelLayer import MolGCN
from . import readout as R


def swish(x):
    return x * torch.sigmoid(x)


def global_add_pool(x, batch, size=None):
    size = int(batch.max().item()) + 1 if size is None else size
    return torch.zeros(size, x.shape[1], dtype=x.dtype, device=x.device).index_add_(0, batch, x)


import os as _os

# MKGNN_PROJECT_FIRST: '1' always / '0' never take the block-row readout; default: from _PROJECT_FIRST_ATOMS atoms on (the
# three small passes cost one more dependent launch each way than the two big ones: a loss below a few thousand atoms)
_PROJECT_FIRST = _os.environ.get('MKGNN_PROJECT_FIRST', '')
_PROJECT_FIRST_ATOMS = 16384


class MolKGNNNet(torch.nn.Module):
    def __init__(self, num_layers=1, num_kernel1_1hop=0, num_kernel2_1hop=0, num_kernel3_1hop=0,
                 num_kernel4_1hop=0, num_kernel1_Nhop=0, num_kernel2_Nhop=0, num_kernel3_Nhop=0,
                 num_kernel4_Nhop=0, predefined_kernelsets=True, x_dim=5, p_dim=3, edge_attr_dim=1,
                 drop_ratio=0.25, graph_embedding_dim=5):
        super(MolKGNNNet, self).__init__()
        self.num_layers = num_layers
        self.D = p_dim
        n_hop = num_kernel1_Nhop + num_kernel2_Nhop + num_kernel3_Nhop + num_kernel4_Nhop
        # module creation order = the reference's (MolKGNNNet.py:20-57), so a seeded init draws the same numbers
        self.graph_embedding_linear = Linear(n_hop, graph_embedding_dim)
        self.node_batch_norm = BatchNorm1d(x_dim)
        self.edge_batch_norm = BatchNorm1d(edge_attr_dim)
        self.graph_embedding_lin1 = Linear(n_hop, graph_embedding_dim)
        self.graph_embedding_lin2 = Linear(graph_embedding_dim, graph_embedding_dim)
        self.dropout = Dropout(drop_ratio)
        self.act = swish
        if self.num_layers < 1:
            raise ValueError("GNN_graphpred: Number of GNN layers must be greater than 0.")
        self.gnn = MolGCN(num_layers=num_layers, num_kernel1_1hop=num_kernel1_1hop,
                          num_kernel2_1hop=num_kernel2_1hop, num_kernel3_1hop=num_kernel3_1hop,
                          num_kernel4_1hop=num_kernel4_1hop, num_kernel1_Nhop=num_kernel1_Nhop,
                          num_kernel2_Nhop=num_kernel2_Nhop, num_kernel3_Nhop=num_kernel3_Nhop,
                          num_kernel4_Nhop=num_kernel4_Nhop, x_dim=x_dim, p_dim=p_dim,
                          edge_attr_dim=edge_attr_dim)
        self.pool = global_add_pool

    def save_kernellayer(self, path, time_stamp):
        layers = self.gnn.layers
        print(f'{self.D}D, there are {len(layers)} layers')
        for i, layer in enumerate(layers):
            print(f'saving {i}th layer')
            torch.save(layer.state_dict(), f'{path}/{time_stamp}_{i}th_layer.pth')

    def _edge_stats(self, data):
        """(edge_attr, edge_batch_norm, key, key_limit) for ``readout.update_running_stats`` or None (eval mode, no bonds).  A
        batch padded to a fixed shape counts the bonds of its real atoms only: padding bonds start at padding atoms."""
        bn = self.edge_batch_norm
        ea = getattr(data, 'edge_attr', None)
        if not (bn.training and bn.track_running_stats and bn.running_mean is not None) or ea is None or ea.shape[0] == 0:
            return None
        nv = getattr(data, 'n_valid_atoms', None)
        if nv is None:
            return (ea, bn, None, None)
        src = data.edge_index[0]
        return (ea, bn, src if src.is_contiguous() else src.contiguous(), nv)

    def forward(self, *argv, save_score=False, _tail=None, _score=None, _atoms=None, _mc=None):
        if len(argv) != 1:
            # the reference's 33-positional-argument form reads ``data`` afterwards and cannot work
            # (MolKGNNNet.py:70-89 then :115); only the single-``data`` form is meaningful
            raise ValueError("unmatched number of arguments.")
        data = argv[0]
        # small batches (the reference's own regime, README.md:81): batch norm, every layer and the readout in ONE launch, a
        # workgroup per chunk of whole molecules (molkgnn_amd.molecule); None where the model or the batch does not qualify
        # (_atoms: the per-atom contributions are asked for -- the molecule-resident step sums them away inside LDS)
        # (private: a dict as _tail asks for the MULTI-OUTPUT fused tail, readout.tail_labels_loss -- train.GNNModel with
        # multi_output_tail on.  Where model and mode qualify the molecule-resident step, which hands back an embedding, is not
        # taken: the tail is asked first.  What only the batch decides -- _tail_limits_ok -- is seen below; the embedding then comes
        # from the separate readout operators as usual.)
        multi_tail = isinstance(_tail, dict) and self._multi_tail_applies(_tail, data)
        if data.x.is_cuda and not save_score and _atoms is None and _mc is None and not multi_tail:
            from . import molecule as _mol
            emb = _mol.net_forward(self, data)
            if emb is not None:                          # (edge_batch_norm's statistics moved inside: molecule.net_forward)
                return emb
        # (a batch padded to a fixed shape -- molkgnn_amd.padding -- carries its real atom count and its molecule segments)
        # edge_batch_norm(data.edge_attr) (reference MolKGNNNet.py:116): its output never reaches the kernel convolution
        # (SURVEY 8 a-1), but in training mode the call moves the module's running statistics and num_batches_tracked, which
        # are state-dict contents -- that side effect rides along in the node batch norm's launches (readout.batch_norm)
        kw = {f'{nm}_deg{d}': getattr(data, f'{nm}_deg{d}')
              for nm in ('p_focal', 'nei_p', 'nei_edge_attr', 'selected_index', 'nei_index') for d in range(1, 5)}
        for d in range(1, 5):                          # unit bond rows built with the receptive fields (mkgnn_rf_fill), if any
            u = getattr(data, f'nei_edge_unit_deg{d}', None)
            if u is not None:
                kw[f'nei_edge_unit_deg{d}'] = u
        # the normalised features go nowhere but into the first kernel convolution: where that layer takes pre-split rows
        # (functional.ROWS_SPLIT) the batch norm writes them so -- asked from shapes alone, nothing is launched or awaited
        split_x, plan0 = False, None
        if data.x.is_cuda and not save_score:
            from . import KernelLayer as _KL
            from .plan import plan_from_lists_cached
            names = ('p_focal', 'nei_p', 'nei_edge_attr', 'selected_index', 'nei_index')
            units = [kw.get(f'nei_edge_unit_deg{d}') for d in range(1, 5)]
            plan0 = plan_from_lists_cached(data.x.shape[0], *[[kw[f'{nm}_deg{d}'] for d in range(1, 5)] for nm in names],
                                           data.edge_index, units if any(u is not None for u in units) else None)
            # (the banks depend on the parameters only: their one launch can run beside the batch norm, on the side stream)
            self.gnn.prepare_banks_early(data.x, sum(int(kw[f'nei_index_deg{d}'].numel()) for d in range(1, 5)))
            if _KL._ROWS_SPLIT:
                split_x = self.gnn.layers[0]._accepts_split_rows(plan0, data.x)
        try:                                             # (a bank preparation may be pending from here to self.gnn: see except)
            # (round 6: spare blocks of the batch norm's statistics launch read the batch's index arrays once -- cold after the
            # previous step's backward, and otherwise paid for by the first convolution: functional.touch_hint)
            from . import functional as _Fn
            with _Fn.touch_hint(_Fn.plan_touch_list(plan0) if plan0 is not None else None) as hint:
                x = R.batch_norm(data.x, self.node_batch_norm, getattr(data, 'n_valid_atoms', None), companion=self._edge_stats(data),
                                 split_out=split_x)
            if plan0 is not None:
                plan0._touch_done = hint.taken
            if getattr(data, '_rf_ready', None) is not None:     # degree buckets still being built on the index stream
                from .receptive_field import await_receptive_fields
                await_receptive_fields(data)
            seg = None
            if getattr(data, 'mol_ptr', None) is not None and getattr(data, 'atom_mol', None) is not None:
                seg = R.MoleculeSegments.from_tensors(data.mol_ptr, data.atom_mol, getattr(data, 'max_mol_atoms', None),
                                                      getattr(data, 'max_mol_edges', None))
            # The last layer's output goes nowhere but through propagate into lin1: where it applies (large batches: it trades
            # two big passes for three small ones), the readout takes the last convolution's BLOCK ROWS and projects them
            # before the propagate step (readout.readout_blocks); MKGNN_PROJECT_FIRST=0 / 1 forces the choice (diagnostics)
            blocks_out = []
            lin1, lin2 = self.graph_embedding_lin1, self.graph_embedding_lin2
            Ls = self.gnn.layers[-1].L
            dims = (sum(Ls), lin1.weight.shape[0], lin2.weight.shape[0])
            # (from _PROJECT_FIRST_ATOMS atoms on -- or at any size where the dense readout kernels do not take the shape, e.g. 160
            # kernels per layer: the block-row form takes up to 255 columns and keeps such a model off the PyTorch-operator path)
            # (... or at any size when the caller wants the loss itself: the fused tail -- readout.tail_loss -- starts from block rows)
            # (the readout's dropout, p < 1, runs inside the fused tail; p >= 1 keeps the separate operators)
            p_readout = self.dropout.p if (self.dropout is not None and self.dropout.training) else 0.0
            want_tail = (_tail is not None and R._FUSED_TAIL and torch.is_grad_enabled() and p_readout < 1.0 and x.is_cuda
                         and R.tail_supported(*dims, Ls) and (multi_tail or not isinstance(_tail, dict)))
            # (private: train.GNNModel.predict asks for the predictions themselves -- the forward-only tail, readout.tail_score --
            # with grad mode off and no readout dropout to draw, i.e. in evaluation mode)
            want_score = (_score is not None and R._FUSED_TAIL and R._SCORE_TAIL and not torch.is_grad_enabled() and p_readout == 0.0
                          and x.is_cuda and R.tail_supported(*dims, Ls))
            # (private: train.GNNModel.predict_mc asks for Monte Carlo dropout samples -- readout.tail_score_mc, next to _score and
            # under its conditions, with one difference: the readout's drop_ratio, which evaluation mode switches off, is handed
            # on (it must be < 1).  _mc = None asks for nothing; a tuple (ffn, n_rows, n_samples, p_head, alpha, beta,
            # return_samples) for the kernel route where it applies; and where it does not, or for _mc = (), the caller gets
            # ("h", the last layer's propagated output) for its PyTorch route.)
            want_mc = (bool(_mc) and R._FUSED_TAIL and R._SCORE_MC and not torch.is_grad_enabled() and p_readout == 0.0
                       and self.dropout.p < 1.0 and x.is_cuda and not save_score and R.tail_supported(*dims, Ls))
            want = x.is_cuda and not save_score and (_PROJECT_FIRST == '1' or (_PROJECT_FIRST != '0' and (
                x.shape[0] >= _PROJECT_FIRST_ATOMS or not R.readout_supported(*dims) or want_tail or want_score)))
            if _mc is not None:                          # (block rows where the kernel takes them, h otherwise: nothing else)
                want = want_mc
                if want and seg is None:
                    seg = R.molecule_segments(data.batch, getattr(data, 'num_graphs', None))
                want = want and seg.sorted and seg.size > 0 and R._tail_limits_ok(seg, plan0)
            # (private: train.GNNModel.atom_contributions asks for every atom's share of every output of the head `_atoms` --
            # readout.atom_contributions, from the block rows, where that applies, else from h through PyTorch operators; it
            # needs no molecule segments, so none are derived, and it alone decides which of the two the last layer leaves)
            want_atoms = (_atoms is not None and R._ATOM_CONTRIB and _PROJECT_FIRST != '0' and not torch.is_grad_enabled() and x.is_cuda
                          and not save_score and R.atom_contributions_supported(*dims, Ls, _atoms.out_features))
            if _atoms is not None:
                want = False
            if want:
                want = R.readout_blocks_supported(*dims, Ls)
            if want and seg is None:
                seg = R.molecule_segments(data.batch, getattr(data, 'num_graphs', None))
            want = want_atoms or (want and seg.sorted and seg.size > 0)
            node_representation = self.gnn(x=x, edge_index=data.edge_index, edge_attr=data.edge_attr, p=data.p,
                                           save_score=save_score, **kw, **({'_defer_last_propagate': blocks_out} if want else {}))
        except BaseException:
            # the deferred bank preparation (MolGCN.prepare_banks_early) must not outlive this call: its workspaces would
            self.gnn.drop_pending_prepare(data.x.device)
            raise
        if _atoms is not None:
            if node_representation is None:
                sim_sc, plan, Ls = blocks_out[0]
                return R.atom_contributions(sim_sc, plan, Ls, lin1, lin2, _atoms)
            return R.atom_contributions_torch(node_representation, lin1, lin2, _atoms)
        if _mc is not None:
            if node_representation is not None:
                return ("h", node_representation)
            sim_sc, plan, Ls = blocks_out[0]
            ffn, n_rows, n_samples, p_head, alpha, beta, return_samples = _mc
            return ("mc", R.tail_score_mc(sim_sc, plan, Ls, lin1, lin2, ffn, seg, n_samples, p_head, self.dropout.p, n_rows,
                                          alpha, beta, return_samples=return_samples, return_pred=True))
        if node_representation is None:                     # the last propagate was left to the readout
            sim_sc, plan, Ls = blocks_out[0]
            # (private: train.GNNModel.loss asks for the loss itself -- readout, head, loss and all their gradients in one
            # launch, readout.tail_loss -- where that applies; it gets ("loss", value) back, or the embedding as usual)
            if want_tail and sim_sc.requires_grad and R._tail_limits_ok(seg, plan):
                if multi_tail:                               # {ffn, p_head, n_rows, loss, kw: tail_labels_loss's label source and weights}
                    return ("loss", R.tail_labels_loss(sim_sc, plan, Ls, lin1, lin2, _tail["ffn"], seg, loss=_tail["loss"],
                                                       dropout_p=_tail["p_head"], n_rows=_tail["n_rows"],
                                                       readout_dropout_p=p_readout, **_tail["kw"]))
                # (ffn, y, dropout p, real molecules[, loss kind: "bce"[, the weighted loss's keywords of tail_loss]])
                ffn, target, p_head, n_rows, *kind = _tail
                loss = kind[0] if kind else "bce"
                return ("loss", R.tail_loss(sim_sc, plan, Ls, lin1, lin2, ffn, target, seg, p_head, n_rows, loss,
                                            readout_dropout_p=p_readout, **(kind[1] if len(kind) > 1 else {})))
            if want_score and R._tail_limits_ok(seg, plan):      # ("score", pred, embedding), or the embedding as usual
                ffn, n_rows = _score
                return ("score", *R.tail_score(sim_sc, plan, Ls, lin1, lin2, ffn, seg, n_rows))
            return R.readout_blocks(sim_sc, plan, Ls, lin1, lin2, self.dropout, seg)
        # pool(lin2(dropout(act(lin1(h)))), batch) -- MolKGNNNet.py:144-146 -- as one operator
        return R.readout(node_representation, lin1, lin2, self.dropout, data.batch, getattr(data, 'num_graphs', None), segments=seg)

    def _multi_tail_applies(self, tail: dict, data) -> bool:
        """What model and mode decide about the multi-output fused tail, before anything runs: ``want_tail``'s conditions in
        ``forward`` and a head of at most 32 outputs."""
        if not (data.x.is_cuda and R._FUSED_TAIL and torch.is_grad_enabled()):
            return False
        p_readout = self.dropout.p if (self.dropout is not None and self.dropout.training) else 0.0
        Ls = self.gnn.layers[-1].L
        dims = (sum(Ls), self.graph_embedding_lin1.weight.shape[0], self.graph_embedding_lin2.weight.shape[0])
        return p_readout < 1.0 and R.tail_labels_supported(tail["ffn"].out_features) and R.tail_supported(*dims, Ls)

    def kernel_column_layout(self, layer: int, device=None):
        """``(column_degree, column_kernel)`` of convolution layer ``layer`` (int32 ``[K_layer]`` each): column ``c`` of that layer's
        output is kernel ``column_kernel[c]`` of the bank of degree ``column_degree[c]`` (1 to 4).  Made once per (layer, device)
        and kept, so a captured step copies nothing from the host."""
        Ls = tuple(int(k) for k in self.gnn.layers[layer].L)
        key = (int(layer), Ls, None if device is None else str(device))
        kept = self.__dict__.setdefault("_column_layouts", {})
        if key not in kept:
            degree = torch.tensor([d + 1 for d, L in enumerate(Ls) for _ in range(L)], dtype=torch.int32)
            kernel = torch.tensor([k for L in Ls for k in range(L)], dtype=torch.int32)
            kept[key] = (degree.to(device), kernel.to(device)) if device is not None else (degree, kernel)
        return kept[key]

    def kernel_scores(self, data, layer: int):
        """``(sim [N, K_layer], column_degree [K_layer], column_kernel [K_layer])``: the output of convolution layer ``layer`` (0 is
        the 1-hop layer) of a model in evaluation mode, under ``torch.no_grad()`` -- ``sim[n, c]`` is how well kernel ``c`` matches
        the neighbourhood of atom ``n``.  Row ``n`` holds the scores of its own degree ``d`` in the columns of that degree's bank
        (``column_degree == d``; ``column_kernel`` is the index inside the bank); what lies elsewhere in the row is unspecified and
        must not be read.  ``N`` counts all atom rows of the batch, padding atoms included.

        It is this composition of the public modules, which is what runs: the node batch norm (``readout.batch_norm`` with the
        batch's ``n_valid_atoms``), then for ``i = 0 .. layer`` ``gnn.layers[i](i == num_layers - 1, data=..., save_score=False)``
        on ``x, p, edge_index, edge_attr`` and the twenty per-degree fields, with ``gnn.propagate(edge_index=..., sim_sc=...)``
        between two layers.  The layers behind ``layer``, the readout and the head are not run.  The training and scoring forwards
        (``forward``, ``predict``, the molecule-resident step) take other kernels for the same layers and may choose differently
        among mathematically tied neighbour permutations in a few entries ("Ties"): their scores can differ from
        these there.  In training mode, and for a ``layer`` outside ``[0, num_layers)``, this raises ``ValueError``."""
        if self.training:
            raise ValueError("MolKGNNNet.kernel_scores needs evaluation mode: call model.eval() first")
        layer = int(layer)
        if not 0 <= layer < self.num_layers:
            raise ValueError(f"layer = {layer} outside [0, {self.num_layers})")
        from .KernelLayer import Data
        with torch.no_grad():
            x = R.batch_norm(data.x, self.node_batch_norm, getattr(data, 'n_valid_atoms', None))
            names = ('p_focal', 'nei_p', 'nei_edge_attr', 'selected_index', 'nei_index')
            fields = {f'{nm}_deg{d}': getattr(data, f'{nm}_deg{d}') for nm in names for d in range(1, 5)}
            if getattr(data, '_rf_ready', None) is not None:     # degree buckets still being built on the index stream
                from .plan import plan_from_lists_cached
                from .receptive_field import await_receptive_fields
                await_receptive_fields(data)
                # ... and behind them the batch's index plan (attach_receptive_fields(overlap=True) leaves it in the plan cache):
                # forward's first propagate joins that stream; nothing here reads the plan, so it is joined now -- a captured step
                # must not end with work of another stream still open
                plan_from_lists_cached(data.x.shape[0], *[[fields[f'{nm}_deg{d}'] for d in range(1, 5)] for nm in names],
                                       data.edge_index)._await()
            step = Data(x=x, p=data.p, edge_index=data.edge_index, edge_attr=data.edge_attr, **fields)
            for i in range(layer + 1):
                sim = self.gnn.layers[i](i == self.num_layers - 1, data=step, save_score=False)
                if i < layer:
                    step.x = self.gnn.propagate(edge_index=data.edge_index, sim_sc=sim)
            return (sim, *self.kernel_column_layout(layer, sim.device))

    @staticmethod
    def add_model_specific_args(parent_parser):
        parser = parent_parser.add_argument_group("MolKGNNNet")
        parser.add_argument('--num_layers', type=int, default=4)
        for hop in ('1hop', 'Nhop'):
            for d, dflt in zip(range(1, 5), (10, 20, 30, 50)):
                parser.add_argument(f'--num_kernel{d}_{hop}', type=int, default=dflt)
        parser.add_argument('--node_feature_dim', type=int, default=28)
        parser.add_argument('--edge_feature_dim', type=int, default=7)
        parser.add_argument('--hidden_dim', type=int, default=32)
        parser.add_argument('--dropout_ratio', type=float, default=0)
        return parent_parser
