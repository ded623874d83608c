"""Drop-in for the reference's ``models/MolKGNN/kernels.py``: ``KernelConv``,
``BaseKernelSetConv`` and ``KernelSetConv`` with the reference's constructor
signatures, parameter names, shapes, initialisation order and keyword-style
``forward`` -- computed by hand-written gfx950 HIP kernels instead of ~40
ATen calls per degree.

Behavioural notes (each is also in DESIGN.md):

* the modules run on an MI355X only; a CPU tensor raises (no fallback path);
* permutation ties are broken by the fixed rule of SURVEY.md 8 a-5;
* an atom whose degree is 0 or > 4 is in no bucket: the reference then returns
  fewer rows than atoms and misaligns the rest (kernels.py:743-747); here its
  output row is zero and every other row stays in place.
"""
from __future__ import annotations

import torch
from torch.nn import Module, ModuleList
from torch.nn.parameter import Parameter

from . import functional as Fn
from .plan import BatchPlan, plan_from_data, plan_from_lists
from .receptive_field import GraphBatch

try:  # the reference stores the initial kernels in a PyG ``Data``; any attribute bag will do
    from torch_geometric.data import Data  # type: ignore
except Exception:  # PyG absent
    Data = GraphBatch


class KernelConv(Module):
    """One degree's kernel bank (reference kernels.py:9-448)."""

    def __init__(self, L=None, D=None, num_supports=None, node_attr_dim=None, edge_attr_dim=None,
                 init_kernel=None, requires_grad=True, init_length_sc_weight=0.2, init_angle_sc_weight=0.2,
                 init_center_attr_sc_weight=0.2, init_support_attr_sc_weight=0.2,
                 init_edge_attr_support_sc_weight=0.2, weight_requires_grad=True):
        super(KernelConv, self).__init__()
        if init_kernel is None:
            if (L is None) or (D is None) or (num_supports is None) or (node_attr_dim is None) or (
                    edge_attr_dim is None):
                raise Exception('either number of kernels L, convolution dimention D, number of support '
                                'num_supports or feature dimension node_attr_dim is not specified')
            # same draw order as the reference (kernels.py:50-53): centre, supports, edge supports, coordinates
            init_kernel = Data(x_center=torch.randn(L, node_attr_dim),
                               x_support=torch.randn(L, num_supports, node_attr_dim),
                               edge_attr_support=torch.randn(L, num_supports, edge_attr_dim),
                               p_support=torch.randn(L, num_supports, D))
        self.num_kernels = init_kernel.x_center.shape[0]
        self.x_center = Parameter(init_kernel.x_center, requires_grad=requires_grad)
        self.x_support = Parameter(init_kernel.x_support, requires_grad=requires_grad)
        self.edge_attr_support = Parameter(init_kernel.edge_attr_support, requires_grad=requires_grad)
        self.p_support = Parameter(init_kernel.p_support, requires_grad=requires_grad)
        self.length_sc_weight = Parameter(torch.tensor(init_length_sc_weight), requires_grad=weight_requires_grad)
        self.angle_sc_weight = Parameter(torch.tensor(init_angle_sc_weight), requires_grad=weight_requires_grad)
        self.center_attr_sc_weight = Parameter(torch.tensor(init_center_attr_sc_weight),
                                               requires_grad=weight_requires_grad)
        self.support_attr_sc_weight = Parameter(torch.tensor(init_support_attr_sc_weight),
                                                requires_grad=weight_requires_grad)
        self.edge_attr_support_sc_weight = Parameter(torch.tensor(init_edge_attr_support_sc_weight),
                                                     requires_grad=weight_requires_grad)
        self.variant = "auto"
        self.backward_variant = None      # None: follows ``variant`` (functional.BACKWARD_VARIANTS)

    def get_num_kernels(self):
        return self.num_kernels

    @property
    def degree(self):
        return self.x_support.shape[1]

    OP_PARAM_NAMES = ("x_center", "x_support", "edge_attr_support", "p_support",
                      "support_attr_sc_weight", "center_attr_sc_weight", "edge_attr_support_sc_weight")

    def op_params(self):
        """The seven tensors the HIP operator takes for this degree (``OP_PARAM_NAMES``, in this order)."""
        return [self.x_center, self.x_support, self.edge_attr_support, self.p_support,
                self.support_attr_sc_weight, self.center_attr_sc_weight, self.edge_attr_support_sc_weight]

    def single_degree_problem(self, x_focal, p_focal, x_neighbor, p_neighbor, edge_attr_neighbor):
        """Lay already-gathered neighbourhoods out as one atom table with a one-bucket plan:
        returns ``(x_all, plan, flat operator parameters)``."""
        deg = self.degree
        n = x_focal.shape[0]
        dev = x_focal.device
        x_all = torch.cat([x_focal, x_neighbor.reshape(n * deg, -1)], dim=0)
        empty_i = torch.zeros(0, dtype=torch.long, device=dev)
        empty_f = torch.zeros(0, dtype=torch.float32, device=dev)
        sel, nei = [empty_i] * 4, [empty_i] * 4
        e_nei, pf, pn = [empty_f] * 4, [empty_f] * 4, [empty_f] * 4
        sel[deg - 1] = torch.arange(n, device=dev)
        nei[deg - 1] = n + torch.arange(n * deg, device=dev)
        e_nei[deg - 1], pf[deg - 1], pn[deg - 1] = edge_attr_neighbor, p_focal, p_neighbor
        plan = plan_from_lists(x_all.shape[0], pf, pn, e_nei, sel, nei)
        params = []
        for d in range(1, 5):
            if d == deg:
                params += self.op_params()
            else:
                params += [x_all.new_zeros((0, x_all.shape[1])), x_all.new_zeros((0, d, x_all.shape[1])),
                           x_all.new_zeros((0, d, self.edge_attr_support.shape[-1])), x_all.new_zeros((0, d, 3)),
                           self.support_attr_sc_weight, self.center_attr_sc_weight, self.edge_attr_support_sc_weight]
        return x_all, plan, params

    def forward(self, is_last_layer, **kwargv):
        """``[L, N_d]`` scores of ``N_d`` neighbourhoods of this degree (kernels.py:428-448)."""
        if len(kwargv) == 1:
            d = kwargv['data']
            x_focal, p_focal, x_neighbor, p_neighbor, edge_attr_neighbor = \
                d.x_focal, d.p_focal, d.x_neighbor, d.p_neighbor, d.edge_attr_neighbor
        else:
            x_focal, p_focal, x_neighbor = kwargv['x_focal'], kwargv['p_focal'], kwargv['x_neighbor']
            p_neighbor, edge_attr_neighbor = kwargv['p_neighbor'], kwargv['edge_attr_neighbor']
        if p_focal.shape[-1] != self.p_support.shape[-1]:
            raise Exception(f'data coordinates is of {p_focal.shape[-1]}D, but the kernel is '
                            f'{self.p_support.shape[-1]}D')
        x_all, plan, params = self.single_degree_problem(x_focal, p_focal, x_neighbor, p_neighbor, edge_attr_neighbor)
        n = x_focal.shape[0]
        out = Fn.kernelsetconv(x_all, plan, is_last_layer, params, self.edge_attr_support.shape[-1], self.variant,
                               backward_variant=self.backward_variant)
        return out[:n].T


class BaseKernelSetConv(Module):
    """Degree bucketing + the four banks (reference kernels.py:451-751)."""

    def __init__(self, fixed_kernelconv1=None, fixed_kernelconv2=None, fixed_kernelconv3=None,
                 fixed_kernelconv4=None, trainable_kernelconv1=None, trainable_kernelconv2=None,
                 trainable_kernelconv3=None, trainable_kernelconv4=None):
        super(BaseKernelSetConv, self).__init__()
        fixed = [fixed_kernelconv1, fixed_kernelconv2, fixed_kernelconv3, fixed_kernelconv4]
        train = [trainable_kernelconv1, trainable_kernelconv2, trainable_kernelconv3, trainable_kernelconv4]
        self.fixed_kernelconv_set = ModuleList(fixed)
        self.num_fixed_kernel_list = [k.get_num_kernels() if k is not None else None for k in fixed]
        self.trainable_kernelconv_set = ModuleList(train)
        self.num_trainable_kernel_list = [k.get_num_kernels() if k is not None else None for k in train]
        self.num_kernel_list = [(f or 0) + (t or 0) for f, t in
                                zip(self.num_fixed_kernel_list, self.num_trainable_kernel_list)]
        self.variant = "auto"     # "auto" | "generic" | "mfma" | "bf16": which HIP kernels serve the forward
        self.backward_variant = None   # None (follows variant) | "auto" | "generic" | "fast": ... the backward
        self.out_pad = None       # None: output storage rows padded to 16 bytes (the result is a view); 0: contiguous

    # -- helpers kept for API parity with the reference ----------------------
    def get_focal_nodes_of_degree(self, x, p, selected_index):
        return torch.index_select(input=x, dim=0, index=selected_index)

    def get_neighbor_nodes_and_edges_of_degree(self, deg, x, p, nei_index):
        nei_x = torch.index_select(x, 0, nei_index)
        return nei_x.reshape(-1, deg, nei_x.shape[-1])

    def get_reorder_index(self, index):
        return torch.sort(index, dim=0)[1]

    def format_output(self, output):
        return torch.cat([output[i, :, :] for i in range(output.shape[0])], dim=1)

    def save_score(self, sc):
        import pandas as pd
        print('saving score...')
        headers = []
        for d, num in enumerate(self.num_kernel_list):
            headers += [f'deg{d + 1}_kernel{i}' for i in range(num)]
        pd.DataFrame(sc.cpu().detach().numpy(), columns=headers).transpose().to_csv('scores.csv')

    def _bank_params(self, which, template):
        """Flat operator parameters of the fixed or the trainable set; a missing degree gets an empty bank."""
        # (called several times per layer and step: the list is remembered while the modules still hold the very Parameter
        # objects it was made of -- nn.Module attribute lookups were a fifth of an eager step's host time at batch 256)
        key = (which, template.device, template.dtype)
        cache = self.__dict__.setdefault("_bank_params_cache", {})
        hit = cache.get(key)
        convs = self.fixed_kernelconv_set if which == "fixed" else self.trainable_kernelconv_set
        if hit is not None:
            params, E, owners = hit
            # (every one of a degree's seven entries: a re-assigned x_support or sc weight is a new object the kernels must read)
            if all(c is o and (c is None or all(c._parameters.get(name) is params[7 * i + k]
                                                for k, name in enumerate(KernelConv.OP_PARAM_NAMES)))
                   for i, (c, o) in enumerate(zip(convs, owners))):
                return list(params), E
        some = next(c for c in convs if c is not None)
        out = []
        for d in range(1, 5):
            c = convs[d - 1]
            if c is not None:
                out += c.op_params()
            else:
                F, E = some.x_center.shape[1], some.edge_attr_support.shape[-1]
                out += [template.new_zeros((0, F)), template.new_zeros((0, d, F)), template.new_zeros((0, d, E)),
                        template.new_zeros((0, d, 3)), some.support_attr_sc_weight, some.center_attr_sc_weight,
                        some.edge_attr_support_sc_weight]
        cache[key] = (list(out), some.edge_attr_support.shape[-1], list(convs))
        return out, some.edge_attr_support.shape[-1]

    def forward(self, is_last_layer, *argv, **kwargv):
        if len(argv) != 0:
            raise Exception('Kernel does not take positional argument, use keyword argument instead. '
                            'e.g. model(data=data)')
        if len(kwargv) == 2:
            data = kwargv['data']
            x = data.x
            save_score = kwargv['save_score']
            plan = plan_from_data(data)
        else:
            x = kwargv['x']
            # edge_index / edge_attr / p are accepted and, as in the reference, not read here
            _ = kwargv['edge_index'], kwargv['edge_attr'], kwargv['p']
            save_score = kwargv['save_score']
            plan = plan_from_lists(
                x.shape[0],
                [kwargv[f'p_focal_deg{d}'] for d in range(1, 5)], [kwargv[f'nei_p_deg{d}'] for d in range(1, 5)],
                [kwargv[f'nei_edge_attr_deg{d}'] for d in range(1, 5)],
                [kwargv[f'selected_index_deg{d}'] for d in range(1, 5)],
                [kwargv[f'nei_index_deg{d}'] for d in range(1, 5)], kwargv['edge_index'])
        return self._run(x, plan, is_last_layer, save_score)

    def _can_prepare(self) -> bool:
        """One trainable KernelConv per degree and no fixed ones (the reference's KernelSetConv): one bank per call."""
        return all(k is not None for k in self.trainable_kernelconv_set) and all(k is None for k in self.fixed_kernelconv_set)

    def _run(self, x, plan: BatchPlan, is_last_layer, save_score=False, block_rows=False, fuse_propagate=False, prepared=None,
             split_next=False, grad_blocks=False):
        """``sim_sc`` of this layer; with ``fuse_propagate`` (and block rows applicable) ``(h, True)`` where
        ``h = propagate(sim_sc)`` came out of the same operator (functional.kernelsetconv(propagate=True)), else
        ``(sim_sc, False)``.  ``split_next``: the only reader of that ``h`` is a layer that takes pre-split rows
        (``_accepts_split_rows``): it is written in that form (functional.ROWS_SPLIT).  ``grad_blocks``: that ``h`` goes to the
        next layer and nowhere else -- it is tagged (functional.mark_grad_blocks)."""
        out = self._run_impl(x, plan, is_last_layer, save_score, block_rows, fuse_propagate, prepared, split_next, grad_blocks)
        return out if fuse_propagate else out[0]

    def _accepts_split_rows(self, plan: BatchPlan, template: torch.Tensor) -> bool:
        """Would this layer's forward and backward take its input as pre-split rows (functional.ROWS_SPLIT)?  One
        trainable bank per degree, the default kernels, and the library's own answer for these shapes."""
        if not template.is_cuda or self.variant not in ("auto", "mfma") or self.backward_variant not in (None, "auto", "fast"):
            return False
        if not self._can_prepare():
            return False
        params, E = self._bank_params("train", template)
        F = int(params[0].shape[1])
        # (the answer depends on shapes only: remembered on the plan, which lives as long as its batch)
        cache = plan.__dict__.setdefault("_rows_split_ok", {})
        key = (F, E, tuple(int(p.shape[0]) for p in params[0::7]), Fn._PRODUCTS_EPOCH)
        if key not in cache:
            cache[key] = Fn.rows_split_supported(plan, params, F, E, plan.n_atoms)
        return cache[key]

    def _run_block_rows(self, x, plan: BatchPlan, is_last_layer, prepared=None):
        """The block rows of this layer's output for a consumer that is not ``propagate_add`` (the block-row readout), or
        None where block rows do not apply (a fixed / trainable split, more than 255 kernels, ``out_pad`` set)."""
        has_fixed = any(k is not None for k in self.fixed_kernelconv_set)
        has_train = any(k is not None for k in self.trainable_kernelconv_set)
        if not has_train or has_fixed or self.out_pad is not None:
            return None
        params, E = self._bank_params("train", x)
        if not plan.block_rows_ok(sum(int(p.shape[0]) for p in params[0::7])):
            return None
        for d in range(1, 5):
            if plan.buckets[d - 1].count and self.trainable_kernelconv_set[d - 1] is None:
                return None
        return Fn.kernelsetconv(x, plan, is_last_layer, params, E, self.variant, self.out_pad, block_rows=True,
                                backward_variant=self.backward_variant, prepared=prepared)

    def _run_impl(self, x, plan: BatchPlan, is_last_layer, save_score, block_rows, fuse_propagate, prepared=None, split_next=False,
                  grad_blocks=False):
        for d in range(1, 5):
            if plan.buckets[d - 1].count and self.fixed_kernelconv_set[d - 1] is None \
                    and self.trainable_kernelconv_set[d - 1] is None:
                raise Exception(f'kernels.py::BaseKernelSet:both fixed and trainable kernelconv_set are '
                                f'None for degree {d}')
        has_fixed = any(k is not None for k in self.fixed_kernelconv_set)
        has_train = any(k is not None for k in self.trainable_kernelconv_set)
        if has_train and not has_fixed:
            params, E = self._bank_params("train", x)
            block_rows = (bool(block_rows) and not save_score and self.out_pad is None
                          and plan.block_rows_ok(sum(int(p.shape[0]) for p in params[0::7])))
            if block_rows and fuse_propagate:
                return Fn.kernelsetconv(x, plan, is_last_layer, params, E, self.variant, self.out_pad, block_rows=True,
                                        backward_variant=self.backward_variant, propagate="split" if split_next else True,
                                        prepared=prepared, grad_blocks=grad_blocks), True
            sc = Fn.kernelsetconv(x, plan, is_last_layer, params, E, self.variant, self.out_pad, block_rows=block_rows,
                                  backward_variant=self.backward_variant, prepared=prepared)
        else:
            # fixed kernels come first inside every degree block (kernels.py:702-710)
            parts = {}
            for which, present in (("fixed", has_fixed), ("train", has_train)):
                if present:
                    params, E = self._bank_params(which, x)
                    parts[which] = Fn.kernelsetconv(x, plan, is_last_layer, params, E, self.variant,
                                                    backward_variant=self.backward_variant)
            cols = []
            of = ot = 0
            for d in range(4):
                nf, nt = self.num_fixed_kernel_list[d] or 0, self.num_trainable_kernel_list[d] or 0
                if nf:
                    cols.append(parts["fixed"][:, of:of + nf])
                if nt:
                    cols.append(parts["train"][:, ot:ot + nt])
                of += nf
                ot += nt
            sc = torch.cat(cols, dim=1)
        if save_score == True:  # noqa: E712  (the reference compares with ==)
            self.save_score(sc)
        return sc, False


class KernelSetConv(BaseKernelSetConv):
    """Convolution on kernels of degree 1 to 4 (reference kernels.py:754-781)."""

    def __init__(self, L1, L2, L3, L4, D, node_attr_dim, edge_attr_dim):
        self.L = [L1, L2, L3, L4]
        # constructed in degree order so that the random draws match the reference (kernels.py:762-774)
        kernelconv1 = KernelConv(L=L1, D=D, num_supports=1, node_attr_dim=node_attr_dim, edge_attr_dim=edge_attr_dim)
        kernelconv2 = KernelConv(L=L2, D=D, num_supports=2, node_attr_dim=node_attr_dim, edge_attr_dim=edge_attr_dim)
        kernelconv3 = KernelConv(L=L3, D=D, num_supports=3, node_attr_dim=node_attr_dim, edge_attr_dim=edge_attr_dim)
        kernelconv4 = KernelConv(L=L4, D=D, num_supports=4, node_attr_dim=node_attr_dim, edge_attr_dim=edge_attr_dim)
        super(KernelSetConv, self).__init__(trainable_kernelconv1=kernelconv1, trainable_kernelconv2=kernelconv2,
                                            trainable_kernelconv3=kernelconv3, trainable_kernelconv4=kernelconv4)

    def get_num_kernel(self):
        return sum(self.L)


if __name__ == "__main__":
    print('testing')
