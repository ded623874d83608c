"""The two consumers either side of the kernel-convolution stack as HIP operators:

* ``batch_norm(x, bn)``  -- ``self.node_batch_norm(data.x)`` (reference ``MolKGNNNet.py:115``) for a
  ``torch.nn.BatchNorm1d`` module ``bn`` (its parameters, running statistics and flags are used as is);
* ``readout(h, lin1, lin2, dropout, batch, size)`` -- ``pool(lin2(dropout(swish(lin1(h)))), batch)``
  (reference ``MolKGNNNet.py:144-146``).

Both call ``libmolkgnn_hip.so`` through the C ABI (``mkgnn_batchnorm_*``, ``mkgnn_readout_*``); shapes
outside the kernels' limits (hidden width > 64, node width > 128, an unsorted ``batch`` vector,
``momentum=None``) take the same formula through PyTorch operators on the GPU instead.
"""
from __future__ import annotations

import ctypes

import weakref
from typing import Optional, Tuple

import os

import torch

from . import _lib
from .functional import _aligned_rows, _row_major, _stride0

_SEG_CACHE: dict = {}
_SEG_CACHE_MAX = 32


class MoleculeSegments:
    """``batch`` (atom -> molecule id) as contiguous segments: ``mol_ptr [B+1]``, ``atom_mol [N]`` (int32)."""

    @classmethod
    def from_tensors(cls, mol_ptr: torch.Tensor, atom_mol: torch.Tensor, max_atoms: Optional[int] = None,
                     max_edges: Optional[int] = None) -> "MoleculeSegments":
        """Segments handed over by the loader (int32, on the GPU, atoms of a molecule contiguous): no derivation, no
        host synchronisation; the tensors may be refilled in place between replays of a captured step.  ``max_atoms`` /
        ``max_edges``: the loader's bound on a molecule's atoms / directed edges for EVERY batch these tensors will hold
        (``padding.pad_batch`` knows them) -- without it the fused tail (``tail_loss``), which needs the bound, is not taken:
        the contents cannot be inspected without a host synchronisation, and must not decide differently in an eager step
        and in a captured one."""
        if mol_ptr.dtype != torch.int32 or atom_mol.dtype != torch.int32:
            raise TypeError("mol_ptr and atom_mol must be int32")
        seg = cls.__new__(cls)
        seg.size = int(mol_ptr.numel()) - 1
        seg.sorted = True
        seg.mol_ptr, seg.atom_mol = mol_ptr, atom_mol
        seg.from_loader = True
        seg.max_atoms = None if max_atoms is None else int(max_atoms)
        seg.max_edges = None if max_edges is None else int(max_edges)
        return seg

    def __init__(self, batch: torch.Tensor, size: int):
        self.size = int(size)
        b = batch.long()
        self.sorted = bool((b[1:] >= b[:-1]).all().item()) if b.numel() > 1 else True
        counts = torch.bincount(b, minlength=self.size)
        if counts.numel() > self.size:
            raise ValueError(f"batch holds molecule ids >= size ({counts.numel()} > {self.size})")
        ptr = torch.zeros(self.size + 1, dtype=torch.int32, device=batch.device)
        ptr[1:] = torch.cumsum(counts, 0).to(torch.int32)
        self.mol_ptr = ptr
        self.atom_mol = b.to(torch.int32).contiguous()


def molecule_segments(batch: torch.Tensor, size: Optional[int]) -> MoleculeSegments:
    """Cached on the identity of ``batch`` (resident batches keep their tensors alive): built once per
    batch, so a step contains no host synchronisation for it (hipGraph capture)."""
    if size is None:
        size = int(batch.max().item()) + 1 if batch.numel() else 0
    key = (batch.data_ptr(), batch.numel(), str(batch.device), int(size), batch._version)   # (refilled in place: rebuilt)
    hit = _SEG_CACHE.get(key)
    if hit is not None:
        seg, ref = hit
        if ref() is batch:                       # addresses are recycled: only the very tensor it was built from counts
            return seg
        del _SEG_CACHE[key]
    seg = MoleculeSegments(batch, size)
    if len(_SEG_CACHE) >= _SEG_CACHE_MAX:
        _SEG_CACHE.pop(next(iter(_SEG_CACHE)))
    _SEG_CACHE[key] = (seg, weakref.ref(batch))
    return seg


def swish(x):
    return x * torch.sigmoid(x)


def readout_supported(F: int, H: int, G: int) -> bool:
    return 1 <= F <= 128 and 1 <= H <= 64 and 1 <= G <= 64


def _params(w1, b1, w2, b2):
    p = _lib.ReadoutParams()
    p.lin1_weight, p.lin1_bias = w1.data_ptr(), _lib.ptr(b1)
    p.lin2_weight, p.lin2_bias = w2.data_ptr(), _lib.ptr(b2)
    p.H, p.F = w1.shape
    p.G = w2.shape[0]
    return p


class _ReadoutFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, h, w1, b1, w2, b2, keep, seg: MoleculeSegments):
        lib = _lib.load()
        _lib.require_gpu_tensor(h, "node_representation")
        h = _aligned_rows(h if h.dtype == torch.float32 else h.float())
        w1c, w2c = w1.contiguous(), w2.contiguous()
        n, F = h.shape
        H, G = w1c.shape[0], w2c.shape[0]
        dev = h.device
        hs = lib.mkgnn_readout_hidden_stride(H)
        pre = torch.empty((n, hs), dtype=torch.float32, device=dev)
        pooled = torch.empty((seg.size, hs), dtype=torch.float32, device=dev)
        out = torch.empty((seg.size, G), dtype=torch.float32, device=dev)
        keepc = None if keep is None else keep.contiguous()
        p = _params(w1c, b1, w2c, b2)
        with torch.cuda.device(dev):
            _lib.check(lib.mkgnn_readout_forward(p, h.data_ptr(), _stride0(h), n, seg.mol_ptr.data_ptr(), seg.size,
                                                 _lib.ptr(keepc), _lib.ptr(pre), _lib.ptr(pooled), _lib.ptr(out), G,
                                                 _lib.stream_ptr(dev)), "mkgnn_readout_forward")
        ctx.seg = seg
        ctx.has_bias = (b1 is not None, b2 is not None)
        ctx.save_for_backward(h, w1c, b1, w2c, b2, keepc, pre, pooled)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        lib = _lib.load()
        h, w1, b1, w2, b2, keep, pre, pooled = ctx.saved_tensors
        seg = ctx.seg
        n, F = h.shape
        H, G = w1.shape[0], w2.shape[0]
        dev = h.device
        g = _row_major(grad_out if grad_out.dtype == torch.float32 else grad_out.float())
        F4 = F + (-F) % 4                       # 16-byte rows for the consumer of the gradient (propagate's backward)
        gh = torch.empty((n, F4), dtype=torch.float32, device=dev)[:, :F] if ctx.needs_input_grad[0] else None
        gw1, gw2 = torch.empty_like(w1), torch.empty_like(w2)
        gb1 = torch.empty_like(b1) if b1 is not None else None
        gb2 = torch.empty_like(b2) if b2 is not None else None
        if n == 0 or seg.size == 0:
            for t in (gh, gw1, gw2, gb1, gb2):
                if t is not None:
                    t.zero_()
            return gh, gw1, gb1, gw2, gb2, None, None
        p = _params(w1, b1, w2, b2)
        with torch.cuda.device(dev):
            ws_bytes = int(lib.mkgnn_readout_workspace_bytes(F, H, G, n, seg.size))
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
            _lib.check(lib.mkgnn_readout_backward(
                p, h.data_ptr(), _stride0(h), n, seg.mol_ptr.data_ptr(), seg.atom_mol.data_ptr(), seg.size,
                _lib.ptr(keep), pre.data_ptr(), pooled.data_ptr(), g.data_ptr(), _stride0(g),
                _lib.ptr(gh), F4, gw1.data_ptr(), _lib.ptr(gb1), gw2.data_ptr(), _lib.ptr(gb2),
                ws.data_ptr(), ws_bytes, _lib.stream_ptr(dev)), "mkgnn_readout_backward")
        return gh, gw1, gb1, gw2, gb2, None, None


def _sel_buckets(plan):
    bk = _lib.Buckets4()
    for i, b in enumerate(plan.buckets):
        bk[i].count = b.count
        if b.count:
            bk[i].selected_index = b.sel.data_ptr()
    return bk


class _ReadoutBlocksFn(torch.autograd.Function):
    """``pool(lin2(dropout(swish(lin1(propagate(sim))))))`` from the block rows ``sim`` of the last kernel convolution:
    ``mkgnn_readout_blocks_forward`` / ``_backward`` (projection first, then the propagate step on H-wide rows)."""

    @staticmethod
    def forward(ctx, sim, w1, b1, w2, b2, keep, seg: MoleculeSegments, plan, blocks):
        lib = _lib.load()
        _lib.require_gpu_tensor(sim, "sim_sc")
        n, K = sim.shape
        w1c, w2c = w1.contiguous(), w2.contiguous()
        H, G = w1c.shape[0], w2c.shape[0]
        dev = sim.device
        hs = lib.mkgnn_readout_hidden_stride(H)
        z = torch.empty((n, hs), dtype=torch.float32, device=dev)
        pre = torch.empty((n, hs), dtype=torch.float32, device=dev)
        pooled = torch.empty((seg.size, hs), dtype=torch.float32, device=dev)
        out = torch.empty((seg.size, G), dtype=torch.float32, device=dev)
        # a backward will follow: the forward leaves the gate keep * swish'(pre + b1) in place of pre, and its sums per molecule
        gsum = torch.empty((seg.size, hs), dtype=torch.float32, device=dev) if any(ctx.needs_input_grad) else None
        keepc = None if keep is None else keep.contiguous()
        p = _params(w1c, b1, w2c, b2)
        rowptr, col = plan.csr_in
        with torch.cuda.device(dev):
            _lib.check(lib.mkgnn_readout_blocks_forward(
                p, sim.data_ptr(), _stride0(sim), _lib.Int32x4(*blocks), _sel_buckets(plan), n, rowptr.data_ptr(), col.data_ptr(),
                seg.mol_ptr.data_ptr(), seg.size, _lib.ptr(keepc), z.data_ptr(), pre.data_ptr(), pooled.data_ptr(), _lib.ptr(gsum),
                out.data_ptr(), G, _lib.stream_ptr(dev)), "mkgnn_readout_blocks_forward")
        ctx.seg, ctx.plan, ctx.blocks = seg, plan, tuple(blocks)
        ctx.save_for_backward(sim, w1c, b1, w2c, b2, pre, gsum, pooled)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        lib = _lib.load()
        sim, w1, b1, w2, b2, gate, gsum, pooled = ctx.saved_tensors
        seg, plan, blocks = ctx.seg, ctx.plan, ctx.blocks
        n, K = sim.shape
        H, G = w1.shape[0], w2.shape[0]
        dev = sim.device
        g = _row_major(grad_out if grad_out.dtype == torch.float32 else grad_out.float())
        hs = gate.shape[1]
        dz = torch.empty((n, hs), dtype=torch.float32, device=dev)
        K4 = K + (-K) % 4
        # block rows: only every atom's own block of the gradient is defined -- all the convolution's backward reads
        gsim = torch.empty((n, K4), dtype=torch.float32, device=dev)[:, :K] if ctx.needs_input_grad[0] else None
        gw1, gw2 = torch.empty_like(w1), torch.empty_like(w2)
        gb1 = torch.empty_like(b1) if b1 is not None else None
        gb2 = torch.empty_like(b2) if b2 is not None else None
        p = _params(w1, b1, w2, b2)
        bk = _sel_buckets(plan)
        rowptr, col = plan.csr_out
        with torch.cuda.device(dev):
            ws_bytes = int(lib.mkgnn_readout_blocks_workspace_bytes(K, H, G, seg.size))
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
            _lib.check(lib.mkgnn_readout_blocks_backward(
                p, sim.data_ptr(), _stride0(sim), _lib.Int32x4(*blocks), bk, n, rowptr.data_ptr(), col.data_ptr(),
                seg.mol_ptr.data_ptr(), seg.atom_mol.data_ptr(), seg.size, gate.data_ptr(), gsum.data_ptr(), pooled.data_ptr(),
                g.data_ptr(), _stride0(g), dz.data_ptr(), _lib.ptr(gsim), K4, gw1.data_ptr(), _lib.ptr(gb1),
                gw2.data_ptr(), _lib.ptr(gb2), ws.data_ptr(), ws_bytes, _lib.stream_ptr(dev)), "mkgnn_readout_blocks_backward")
        return gsim, gw1, gb1, gw2, gb2, None, None, None, None


def readout_blocks_supported(K: int, H: int, G: int, blocks) -> bool:
    return bool(_lib.load().mkgnn_readout_blocks_supported(int(K), int(H), int(G), _lib.Int32x4(*[int(b) for b in blocks])))


def readout_blocks(sim: torch.Tensor, plan, blocks, lin1: torch.nn.Linear, lin2: torch.nn.Linear,
                   dropout: Optional[torch.nn.Dropout], seg: "MoleculeSegments") -> torch.Tensor:
    """``readout(propagate_add(sim), ...)`` for the block rows ``sim`` of the LAST kernel convolution (``kernelsetconv(...,
    block_rows=True)``; ``blocks`` = its four kernel counts): the projection ``lin1`` runs on every atom's own block first
    and the propagate step carries H-wide rows (``_ReadoutBlocksFn``).  The caller checks ``readout_blocks_supported`` and
    that the molecule segments are sorted."""
    H = lin1.weight.shape[0]
    p_drop = dropout.p if (dropout is not None and dropout.training) else 0.0
    keep = None
    if p_drop > 0.0:
        keep = torch.empty((sim.shape[0], H), dtype=torch.float32, device=sim.device)
        if p_drop >= 1.0:
            keep.zero_()
        else:
            keep.bernoulli_(1.0 - p_drop).mul_(1.0 / (1.0 - p_drop))
    return _ReadoutBlocksFn.apply(sim, lin1.weight, lin1.bias, lin2.weight, lin2.bias, keep, seg, plan, tuple(blocks))


_TORCH_READOUT_OK = os.environ.get("MKGNN_TORCH_READOUT", "") == "1"


def readout(h: torch.Tensor, lin1: torch.nn.Linear, lin2: torch.nn.Linear, dropout: Optional[torch.nn.Dropout],
            batch: torch.Tensor, size: Optional[int] = None, segments: Optional["MoleculeSegments"] = None) -> torch.Tensor:
    """``global_add_pool(lin2(dropout(swish(lin1(h)))), batch, size)`` -> ``[size, G]``.  ``segments``: the molecule
    segments of ``batch`` when the caller already has them (a loader knows the molecule sizes; deriving them from
    ``batch`` costs a host synchronisation, which a captured step cannot have)."""
    _lib.require_gpu_tensor(h, "node_representation")
    seg = segments if segments is not None else molecule_segments(batch, size)
    H, F = lin1.weight.shape
    G = lin2.weight.shape[0]
    p_drop = dropout.p if (dropout is not None and dropout.training) else 0.0
    if not readout_supported(F, H, G) and not _TORCH_READOUT_OK:
        # no silent PyTorch-operator path for a shape the HIP kernels do not take: the caller decides
        raise _lib.MolKGNNLibraryError(
            f"readout: lin1 {F} -> {H}, lin2 -> {G} is outside the HIP readout kernels (F <= 128, H <= 64, G <= 64; inside "
            "MolKGNNNet the block-row readout takes up to 255 kernel columns); set MKGNN_TORCH_READOUT=1 to run this shape "
            "through PyTorch operators on the GPU instead")
    if not (seg.sorted and readout_supported(F, H, G) and h.shape[0] > 0 and seg.size > 0):
        # (an unsorted `batch` vector or an empty batch: the same formula through PyTorch operators)
        z = swish(lin1(h))
        if dropout is not None:
            z = dropout(z)
        z = lin2(z)
        return torch.zeros(seg.size, G, dtype=z.dtype, device=z.device).index_add_(0, batch, z)
    keep = None
    if p_drop > 0.0:
        # the multipliers torch's dropout would apply: 0 with probability p, else 1 / (1 - p)
        keep = torch.empty((h.shape[0], H), dtype=torch.float32, device=h.device)
        if p_drop >= 1.0:
            keep.zero_()
        else:
            keep.bernoulli_(1.0 - p_drop).mul_(1.0 / (1.0 - p_drop))
    return _ReadoutFn.apply(h, lin1.weight, lin1.bias, lin2.weight, lin2.bias, keep, seg)


# ------------------------------------------------------------------------------------------ batch norm --
class _BatchNormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, bn: torch.nn.BatchNorm1d, use_batch_stats: bool, n_valid=None, companion=None, split_out=False):
        lib = _lib.load()
        ctx.n_valid = n_valid
        x = _row_major(x if x.dtype == torch.float32 else x.float())
        n, C = x.shape
        dev = x.device
        out = torch.empty((n, C), dtype=torch.float32, device=dev)
        save_mean = torch.empty(C, dtype=torch.float32, device=dev)
        save_invstd = torch.empty(C, dtype=torch.float32, device=dev)
        update = bn.training and bn.track_running_stats and bn.running_mean is not None
        rm = bn.running_mean if (update or not use_batch_stats) else None
        rv = bn.running_var if (update or not use_batch_stats) else None
        nbt = bn.num_batches_tracked if (update and bn.num_batches_tracked is not None) else None
        if nbt is not None and (nbt.dtype != torch.int64 or nbt.device != dev):
            raise _lib.MolKGNNLibraryError("num_batches_tracked must be an int64 tensor on the input's device")
        # the row norms of the output ride along for the kernel convolution that reads it next (<= 32 channels, 16-byte rows)
        inv = torch.empty(n, dtype=torch.float32, device=dev) \
            if (C <= 32 and C % 4 == 0 and _stride0(x) % 4 == 0 and x.data_ptr() % 16 == 0) else None
        with torch.cuda.device(dev):
            ws_bytes = int(lib.mkgnn_batchnorm_workspace_bytes(C))
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
            st, keep, cws, cws_bytes = None, None, None, 0
            if companion is not None and use_batch_stats and bn.training:
                st, keep = _bn_stats_struct(*companion)      # (statistics move in training mode only)
                cws_bytes = int(lib.mkgnn_batchnorm_stats_workspace_bytes(st.C))
                cws = torch.empty(cws_bytes, dtype=torch.uint8, device=dev)
            _lib.check(lib.mkgnn_batchnorm_forward_with_stats(
                x.data_ptr(), _stride0(x), n, C, _lib.ptr(weight), _lib.ptr(bias), _lib.ptr(rm), _lib.ptr(rv),
                float(bn.momentum if bn.momentum is not None else 0.0), float(bn.eps),
                int(use_batch_stats) | (2 if (split_out and inv is not None) else 0),       # (MKGNN_BN_SPLIT_ROWS)
                out.data_ptr(), C, save_mean.data_ptr(), save_invstd.data_ptr(), _lib.ptr(inv), _lib.ptr(nbt),
                _lib.ptr(n_valid), ws.data_ptr(), ws_bytes, None if st is None else ctypes.byref(st), _lib.ptr(cws), cws_bytes,
                _lib.stream_ptr(dev)), "mkgnn_batchnorm_forward_with_stats")
            del keep
        ctx.use_batch_stats = use_batch_stats
        ctx.save_for_backward(x, weight, save_mean, save_invstd)
        ctx.wrote_split = bool(split_out and inv is not None)
        if inv is None:
            inv = torch.empty(0, dtype=torch.float32, device=dev)
        ctx.mark_non_differentiable(inv)
        ctx.set_materialize_grads(False)
        return out, inv

    @staticmethod
    def backward(ctx, grad_out, _g_inv=None):
        lib = _lib.load()
        if grad_out is None:
            return None, None, None, None, None, None, None, None
        x, weight, save_mean, save_invstd = ctx.saved_tensors
        n, C = x.shape
        dev = x.device
        g = _row_major(grad_out if grad_out.dtype == torch.float32 else grad_out.float())
        gx = torch.empty((n, C), dtype=torch.float32, device=dev) if ctx.needs_input_grad[0] else None
        gw = torch.empty(C, dtype=torch.float32, device=dev) if (weight is not None and ctx.needs_input_grad[1]) else None
        gb = torch.empty(C, dtype=torch.float32, device=dev) if ctx.needs_input_grad[2] else None
        with torch.cuda.device(dev):
            ws_bytes = int(lib.mkgnn_batchnorm_workspace_bytes(C))
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
            _lib.check(lib.mkgnn_batchnorm_backward(
                g.data_ptr(), _stride0(g), x.data_ptr(), _stride0(x), n, C, _lib.ptr(weight), save_mean.data_ptr(),
                save_invstd.data_ptr(), int(ctx.use_batch_stats), _lib.ptr(gx), C, _lib.ptr(gw), _lib.ptr(gb),
                _lib.ptr(ctx.n_valid), ws.data_ptr(), ws_bytes, _lib.stream_ptr(dev)), "mkgnn_batchnorm_backward")
        return gx, gw, gb, None, None, None, None, None


def _stats_supported(x: torch.Tensor, bn: torch.nn.BatchNorm1d) -> bool:
    return (x.is_cuda and x.dim() == 2 and 1 <= x.shape[1] <= 256 and x.shape[0] >= 1 and x.shape[1] == bn.num_features
            and bn.momentum is not None and bn.running_mean is not None and bn.running_mean.is_cuda)


def _bn_stats_struct(x: torch.Tensor, bn: torch.nn.BatchNorm1d, key: Optional[torch.Tensor], key_limit: Optional[torch.Tensor]):
    """The C struct of a statistics companion and the tensors it points at (to be kept alive across the call)."""
    x = _row_major(x if x.dtype == torch.float32 else x.float())
    if (key is None) != (key_limit is None):
        raise ValueError("key and key_limit come together")
    if key is not None:
        if not (key.is_cuda and key.dtype == torch.int64 and key.is_contiguous() and key.numel() == x.shape[0]):
            raise ValueError("key must be a contiguous int64 GPU tensor with one entry per row")
        if not (key_limit.is_cuda and key_limit.dtype == torch.int64 and key_limit.numel() == 1):
            raise ValueError("key_limit must be a one-element int64 tensor on the GPU")
    nbt = bn.num_batches_tracked
    if nbt is not None and (nbt.dtype != torch.int64 or nbt.device != x.device):
        raise _lib.MolKGNNLibraryError("num_batches_tracked must be an int64 tensor on the input's device")
    st = _lib.BnStats(x.data_ptr(), _stride0(x), x.shape[0], x.shape[1], _lib.ptr(bn.running_mean), _lib.ptr(bn.running_var),
                      float(bn.momentum), _lib.ptr(nbt), _lib.ptr(key), _lib.ptr(key_limit))
    return st, (x, key, key_limit)


def update_running_stats(x: torch.Tensor, bn: torch.nn.BatchNorm1d, key: Optional[torch.Tensor] = None,
                         key_limit: Optional[torch.Tensor] = None) -> None:
    """What ``bn(x)`` does to the module's buffers in training mode, without computing ``bn(x)``: the reference calls
    ``edge_batch_norm(data.edge_attr)`` in every forward (``MolKGNNNet.py:116``) and the kernel convolution never reads the
    result -- ``running_mean``, ``running_var`` and ``num_batches_tracked`` still move, and they are
    state-dict contents.  ``key`` / ``key_limit``: only rows with ``key[r] < key_limit`` count (padded batches: the bonds of
    real atoms).  No-op in eval mode or without tracked statistics."""
    if not (bn.training and bn.track_running_stats and bn.running_mean is not None):
        return
    _lib.require_gpu_tensor(x, "x")
    if not _stats_supported(x, bn):
        if key is not None:
            if torch.cuda.is_current_stream_capturing():
                # (a boolean-mask index synchronises with the host: illegal inside a capture -- say so instead of failing obscurely)
                raise _lib.MolKGNNLibraryError("update_running_stats: a keyed batch outside the HIP kernels' limits (> 256 channels, "
                                               "momentum None, statistics off the GPU) cannot run inside a hipGraph capture")
            x = x[key < key_limit]
        bn(x)                                             # (PyTorch's operator on the GPU: cumulative-average momentum, > 256 channels)
        return
    lib = _lib.load()
    dev = x.device
    st, keep = _bn_stats_struct(x, bn, key, key_limit)
    with torch.cuda.device(dev):
        ws_bytes = int(lib.mkgnn_batchnorm_stats_workspace_bytes(st.C))
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        _lib.check(lib.mkgnn_batchnorm_update_stats(ctypes.byref(st), ws.data_ptr(), ws_bytes, _lib.stream_ptr(dev)),
                   "mkgnn_batchnorm_update_stats")
    del keep


def batch_norm(x: torch.Tensor, bn: torch.nn.BatchNorm1d, n_valid: Optional[torch.Tensor] = None,
               companion=None, split_out: bool = False) -> torch.Tensor:
    """``bn(x)`` for a 2-D input on the GPU, with ``torch.nn.BatchNorm1d``'s semantics (batch statistics in
    training mode or when no running statistics are tracked; running statistics updated in place).

    ``companion`` = ``(x2, bn2, key, key_limit)``: ``update_running_stats(x2, bn2, key, key_limit)`` done by extra blocks of
    this batch norm's own launches (training mode).

    ``split_out`` (round 6): write the result as pre-split rows (``functional.ROWS_SPLIT``) where the kernels can (<= 32 channels,
    a multiple of 4, 16-byte rows) -- for a caller whose only reader of it is a kernel convolution that takes them.

    ``n_valid`` (a one-element int64 CUDA tensor): only the leading ``n_valid`` rows enter the batch statistics; the
    remaining rows are padding (``molkgnn_amd.padding``) -- normalised with the same statistics, excluded from every sum.
    The value is read on the device, so a captured step serves batches with different numbers of real atoms."""
    _lib.require_gpu_tensor(x, "x")
    if n_valid is not None and not (n_valid.is_cuda and n_valid.dtype == torch.int64 and n_valid.numel() == 1):
        raise ValueError("n_valid must be a one-element int64 tensor on the GPU")
    if x.dim() != 2 or x.shape[1] != bn.num_features:
        raise ValueError(f"expected a [N, {bn.num_features}] input, got {tuple(x.shape)}")
    use_batch_stats = bn.training or bn.running_mean is None
    if companion is not None:
        x2, bn2 = companion[0], companion[1]
        if not (bn2.training and bn2.track_running_stats and bn2.running_mean is not None):
            companion = None                              # nothing of bn2 moves
        elif not (_stats_supported(x2, bn2) and bn.training and use_batch_stats):
            update_running_stats(*companion)              # (on its own)
            companion = None
    if x.shape[1] > 256 or x.shape[0] == 0 or (bn.training and bn.track_running_stats and bn.momentum is None):
        if n_valid is not None:
            raise ValueError("n_valid needs the HIP batch norm (<= 256 channels, momentum set)")
        if companion is not None:
            update_running_stats(*companion)
        return bn(x)
    if use_batch_stats and bn.training and x.shape[0] == 1:
        raise ValueError(f"Expected more than 1 value per channel when training, got input size {tuple(x.shape)}")
    out, inv = _BatchNormFn.apply(x, bn.weight, bn.bias, bn, use_batch_stats, n_valid, companion, split_out)
    if inv.numel():
        from .functional import _INV_ATTR, mark_rows_split
        setattr(out, _INV_ATTR, (inv, out._version))
        if split_out:
            # (``split_out``: the caller's promise that nothing but the first kernel convolution reads the result -- its rows are
            # the fp16 hi | lo halves that convolution's matrix instructions take, functional.ROWS_SPLIT)
            mark_rows_split(out)
    return out


# ------------------------------------------------------------------------------- single-task head + loss --
_HEAD_WS: dict = {}


def _head_workspace(dev, nbytes: int) -> torch.Tensor:
    """Per-device scratch for the head kernels' per-block partials.  Calls on one device are ordered on the autograd /
    capture stream, so one buffer per device is enough.  A buffer that has been handed out is never released: a
    captured graph has its address baked in, so when a larger one is needed the old ones stay referenced here."""
    held = _HEAD_WS.setdefault(str(dev), [])
    if not held or held[-1].numel() < nbytes:
        held.append(torch.empty(max(nbytes, 1 << 16), dtype=torch.uint8, device=dev))
    return held[-1]


_HEAD_RNG: dict = {}
# MKGNN_SPLIT_HEAD=1 (diagnostics): the head's forward and backward as separate launches (two each) even in a training step
_SPLIT_HEAD = os.environ.get("MKGNN_SPLIT_HEAD") == "1"


def head_rng_state(dev) -> torch.Tensor:
    """Per-device ``{seed, offset}`` (int64) of the head kernels' dropout generator.  The seed is drawn from PyTorch's
    default CPU generator the first time a device needs it, so ``torch.manual_seed`` fixes the sequence; every forward
    with dropout advances ``offset`` on the device (also inside a replayed graph)."""
    st = _HEAD_RNG.get(str(dev))
    if st is None:
        seed = int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item())
        st = torch.tensor([seed, 0], dtype=torch.int64, device=dev)
        _HEAD_RNG[str(dev)] = st
    return st


def reset_head_rng(dev=None, seed=None) -> None:
    """Forget the generator state (of one device, or all): the next use draws a new seed, or uses ``seed``."""
    for k in ([str(dev)] if dev is not None else list(_HEAD_RNG)):
        _HEAD_RNG.pop(k, None)
        if seed is not None:
            _HEAD_RNG[k] = torch.tensor([int(seed), 0], dtype=torch.int64, device=torch.device(k))


_UNIT_SEEDS: list = []        # (tensor, its version counter when registered): held, so the address cannot be reused


def register_unit_gradient(one: torch.Tensor) -> None:
    """Tell the head that ``one`` is a resident tensor holding 1.0 which seeds ``backward`` (``train.backward`` does):
    when the loss's incoming gradient IS that tensor, the gradients the fused forward already wrote are the answer and the
    backward launches nothing.  Any other incoming gradient scales them.  The tensor is kept alive here (its storage
    address stays its own) and a later in-place write to it (a changed version counter) retires the registration."""
    if not any(t is one for t, _ in _UNIT_SEEDS):
        _UNIT_SEEDS.append((one, one._version))


def _is_unit_seed(grad: torch.Tensor) -> bool:
    for t, version in _UNIT_SEEDS:
        if t._version == version and t.device == grad.device and (grad is t or (
                grad.data_ptr() == t.data_ptr() and grad.numel() == 1 and grad.dtype == t.dtype)):
            return True
    return False


# the head's loss kinds (MKGNN_LOSS_*): BCEWithLogitsLoss() (the QSAR assays, reference data.py:37), MSELoss() and
# MSELoss(reduction='sum') (the docking-score task, data.py:49-53)
LOSS_KINDS = {"bce": _lib.LOSS_BCE_MEAN, "mse": _lib.LOSS_SQERR_MEAN, "mse_sum": _lib.LOSS_SQERR_SUM}


def loss_kind(loss: str) -> int:
    if loss not in LOSS_KINDS:
        raise ValueError(f"unknown loss {loss!r}: one of {sorted(LOSS_KINDS)}")
    return LOSS_KINDS[loss]


def _i32(t: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    if t is None:
        return None
    t = t.reshape(-1)
    return t if (t.dtype == torch.int32 and t.is_contiguous()) else t.to(torch.int32).contiguous()


def _f32(t: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    if t is None:
        return None
    t = t.detach().reshape(-1)
    return t if (t.dtype == torch.float32 and t.is_contiguous()) else t.float().contiguous()


class _HeadFnBase(torch.autograd.Function):
    """The one forward (``_run``) and the one backward of the three head Functions: the fused entry (forward and the gradients for
    d loss = 1 in the same two launches) when a gradient is needed, the split forward / backward entries otherwise, under
    ``MKGNN_SPLIT_HEAD=1``, and for a second backward over a retained graph.  A subclass describes its entry-point family:
    ``SYMS``, the C symbols of the fused / forward / backward entry; ``_weight(weight)``, the weight as the kernels read it, whose
    shape is ``gw``'s -- ``[H]`` (``gb [1]``) for the single-task head, ``[T, H]`` (``gb [T]``) otherwise; ``_workspace_bytes``; and
    ``_extra(w, vectors)``, the family's extra positional arguments ``(dims, index, tail)`` -- behind ``H``, behind the target,
    ahead of the workspace -- from ``vectors``, the index / weight vectors its forward handed ``_run`` (``_i32`` / ``_f32``)."""
    SYMS: tuple = ()

    @classmethod
    def _entries(cls, kind):
        return cls.SYMS, (int(kind),)                    # (the symbols, the arguments ahead of ``emb``)

    @classmethod
    def _call(cls, which: int, kind, emb, B: int, w, vectors, mid_a: tuple, mid_b: tuple) -> None:
        """``SYMS[which](lead, emb, stride, B, H, dims, w, *mid_a, index, *mid_b, tail, workspace, stream)``."""
        lib, dev, H = _lib.load(), emb.device, emb.shape[1]
        names, lead = cls._entries(kind)
        dims, index, tail = cls._extra(w, vectors)
        with torch.cuda.device(dev):
            ws = _head_workspace(dev, int(cls._workspace_bytes(lib, B, H, w)))
            _lib.check(getattr(lib, names[which])(*lead, emb.data_ptr(), _stride0(emb), B, H, *dims, w.data_ptr(), *mid_a, *index,
                                                  *mid_b, *tail, ws.data_ptr(), ws.numel(), _lib.stream_ptr(dev)), names[which])

    @staticmethod
    def _grads(ctx, emb, w):
        """``(gemb, gw, gb)`` to be written and their arguments; rows beyond ``n_rows`` (padding molecules) get a zero gradient:
        one small fill, only when there are any."""
        H, dev = emb.shape[1], emb.device
        gemb = None
        if ctx.needs_input_grad[0]:
            gemb = torch.empty((emb.shape[0], H), dtype=torch.float32, device=dev)
            if emb.shape[0] > ctx.n_rows:
                gemb[ctx.n_rows:].zero_()
        gw = torch.empty(w.shape, dtype=torch.float32, device=dev)
        gb = torch.empty(w.numel() // H, dtype=torch.float32, device=dev) if ctx.has_bias else None
        return (gemb, gw, gb), (_lib.ptr(gemb), H, gw.data_ptr(), _lib.ptr(gb))

    @classmethod
    def _run(cls, ctx, emb, weight, bias, target, p_drop, n_rows, kind, vectors: tuple = ()):
        emb = _row_major(emb if emb.dtype == torch.float32 else emb.float())
        w, y = cls._weight(weight), _f32(target)
        B, dev = int(n_rows), emb.device                 # the leading n_rows rows enter the loss (the rest: padding molecules)
        ctx.family, ctx.kind, ctx.n_rows = cls, kind, B
        ctx.wshape, ctx.has_bias, ctx.p_drop = weight.shape, bias is not None, float(p_drop)
        pred = torch.empty(B, dtype=torch.float32, device=dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        rng = head_rng_state(dev) if p_drop > 0.0 else None
        used = torch.empty(2, dtype=torch.int64, device=dev) if p_drop > 0.0 else None
        mid_a = (_lib.ptr(bias), y.data_ptr())
        mid_b = (ctx.p_drop, _lib.ptr(rng), _lib.ptr(used), pred.data_ptr(), loss.data_ptr())
        ctx.unit = None
        if any(ctx.needs_input_grad[:3]) and not _SPLIT_HEAD:
            # a training step: forward and the gradients for d loss = 1 in the same two launches
            ctx.unit, gargs = cls._grads(ctx, emb, w)
            cls._call(0, kind, emb, B, w, vectors, mid_a, mid_b + gargs)
        else:
            cls._call(1, kind, emb, B, w, vectors, mid_a, mid_b)
        # (with ctx.unit, references only: a second backward over a retained graph takes the separate backward kernel)
        ctx.save_for_backward(emb, w, y, pred, used, *vectors)
        return loss

    @staticmethod
    def backward(ctx, grad_loss):
        if ctx.unit is not None:
            grads, ctx.unit = ctx.unit, None
            if not _is_unit_seed(grad_loss):                 # d loss is not the registered 1: scale
                gl = grad_loss.reshape(()).float()
                grads = tuple(None if g is None else g * gl for g in grads)
        else:
            emb, w, y, pred, used, *vectors = ctx.saved_tensors
            gl = grad_loss.reshape(1).float().contiguous()
            grads, gargs = ctx.family._grads(ctx, emb, w)
            ctx.family._call(2, ctx.kind, emb, ctx.n_rows, w, vectors, (y.data_ptr(),),
                             (pred.data_ptr(), gl.data_ptr(), ctx.p_drop, _lib.ptr(used)) + gargs)
        gemb, gw, gb = grads
        return (gemb, gw if gw.shape == ctx.wshape else gw.reshape(ctx.wshape), gb) + (None,) * (len(ctx.needs_input_grad) - 3)


class _BceHeadFn(_HeadFnBase):
    """The single-task head: ``mkgnn_bce_head_*`` (``kind`` None: the BCE entry points as they were) and ``mkgnn_head_loss_*``."""
    SYMS = ("mkgnn_bce_head_fused", "mkgnn_bce_head_dropout_forward", "mkgnn_bce_head_dropout_backward")
    SYMS_KIND = ("mkgnn_head_loss_fused", "mkgnn_head_loss_dropout_forward", "mkgnn_head_loss_dropout_backward")

    @classmethod
    def _entries(cls, kind):
        return (cls.SYMS, ()) if kind is None else (cls.SYMS_KIND, (int(kind),))

    @staticmethod
    def _weight(weight):
        return weight.reshape(-1).contiguous()

    @staticmethod
    def _workspace_bytes(lib, B, H, w):
        return lib.mkgnn_bce_head_workspace_bytes(B, H)

    @staticmethod
    def _extra(w, vectors):
        return (), (), ()

    @staticmethod
    def forward(ctx, emb, weight, bias, target, p_drop, n_rows, kind=None):
        return _BceHeadFn._run(ctx, emb, weight, bias, target, p_drop, n_rows, kind)


def _head_loss(who: str, emb: torch.Tensor, ffn: torch.nn.Linear, target: torch.Tensor, kind: Optional[int], dropout_p: float,
               n_rows: Optional[int]) -> torch.Tensor:
    """The body of ``bce_head_loss`` (``kind`` None: the ``mkgnn_bce_head_*`` entry points) and ``head_loss``."""
    _lib.require_gpu_tensor(emb, "graph_embedding")
    n_rows = emb.shape[0] if n_rows is None else int(n_rows)
    if ffn.out_features != 1 or emb.dim() != 2 or n_rows <= 0 or n_rows > emb.shape[0] or target.numel() != n_rows:
        raise ValueError(f"{who} needs a one-output linear layer and one target per (leading) row")
    if not 0.0 <= dropout_p < 1.0:
        raise ValueError(f"dropout probability {dropout_p} outside [0, 1)")
    return _BceHeadFn.apply(emb, ffn.weight, ffn.bias, target, float(dropout_p), n_rows, kind)


def bce_head_loss(emb: torch.Tensor, ffn: torch.nn.Linear, target: torch.Tensor, dropout_p: float = 0.0,
                  n_rows: Optional[int] = None) -> torch.Tensor:
    """``BCEWithLogitsLoss()(ffn(dropout(emb)).view(-1), target.view(-1).float())`` for a one-output ``ffn`` (reference
    ``model.py:147-150, 169, 190-198``) as one forward and one backward kernel; ``dropout_p`` is the probability of
    zeroing an element of ``emb`` (``nn.Dropout(ffn_dropout_rate)`` in training mode; 0 otherwise), its mask drawn
    inside the kernels from ``head_rng_state``.  ``n_rows``: only the leading rows of ``emb`` enter the loss (a padded batch's
    real molecules); the others get a zero gradient."""
    return _head_loss("bce_head_loss", emb, ffn, target, None, dropout_p, n_rows)             # (None: mkgnn_bce_head_*)


def head_loss(emb: torch.Tensor, ffn: torch.nn.Linear, target: torch.Tensor, loss: str = "bce", dropout_p: float = 0.0,
              n_rows: Optional[int] = None, sample_weight: Optional[torch.Tensor] = None,
              pos_weight: Optional[torch.Tensor] = None, weight_table: Optional[torch.Tensor] = None,
              row_ids: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``bce_head_loss`` for any loss kind of ``LOSS_KINDS``: ``"bce"`` (``BCEWithLogitsLoss()``, the same bits as
    ``bce_head_loss``), ``"mse"`` (``MSELoss()``) or ``"mse_sum"`` (``MSELoss(reduction='sum')``, the reference's docking-score
    task) of ``ffn(dropout(emb)).view(-1)`` against ``target.view(-1).float()``.  Same kernels (the kind a template parameter),
    same dropout mask for the same generator state, same padding rule.

    ``sample_weight [>= n_rows]`` (or ``weight_table [M]`` read through ``row_ids [>= n_rows]``) and ``pos_weight [1]``: the weighted
    loss of ``task_head_reference`` with every row in task 0, on the task-indexed head's weighted kernels
    (``mkgnn_task_head_weighted_*`` with a null task); with none of them given nothing changes."""
    if sample_weight is None and pos_weight is None and weight_table is None:
        return _head_loss("head_loss", emb, ffn, target, loss_kind(loss), dropout_p, n_rows)
    if ffn.out_features != 1:
        raise ValueError("head_loss needs a one-output linear layer")
    return _task_head_loss("head_loss", emb, ffn, target, None, loss, dropout_p, n_rows, None, row_ids, sample_weight, pos_weight,
                           weight_table)


# ---------------------------------------------------------------- task-indexed head with masked labels --
def task_head_supported(T: int, H: int) -> bool:
    """The shapes ``mkgnn_task_head_*`` take; anything else goes through ``task_head_reference`` on the GPU."""
    return 1 <= T <= _lib.TASK_HEAD_MAX_TASKS and 1 <= H <= _lib.TASK_HEAD_MAX_H


def _row_tasks(task, task_table, row_ids, n_rows: int) -> torch.Tensor:
    """The task of each of the leading ``n_rows`` rows (int64): ``task`` itself, or ``task_table[row_ids]`` with an id outside
    the table read as -1."""
    if task is not None:
        return task.reshape(-1)[:n_rows].long()
    ids = row_ids.reshape(-1)[:n_rows].long()
    m = task_table.numel()
    inside = (ids >= 0) & (ids < m)
    return torch.where(inside, task_table.reshape(-1).long()[ids.clamp(0, max(m - 1, 0))], torch.full_like(ids, -1))


# MKGNN_WEIGHTED_LOSS=0 (A/B, diagnostics): a weighted loss runs its definition (task_head_reference) in torch operators on the GPU
# instead of the weighted kernels; an unweighted loss is not touched by it
_WEIGHTED_LOSS = os.environ.get("MKGNN_WEIGHTED_LOSS", "1") != "0"


def _check_loss_weights(loss: str, T: int, sample_weight, pos_weight, weight_table, row_ids) -> None:
    """What every weighted entry refuses: a weight that requires a gradient, ``pos_weight`` with a squared-error kind or of a
    length other than ``T``, both weight forms at once, a table without ids."""
    for name, w in (("sample_weight", sample_weight), ("pos_weight", pos_weight), ("weight_table", weight_table)):
        if w is not None and w.requires_grad:
            raise ValueError(f"{name} is a constant of the loss: it must not require a gradient")
    if pos_weight is not None:
        if loss != "bce":
            raise ValueError(f"pos_weight belongs to the 'bce' loss, not to {loss!r}")
        if pos_weight.numel() != T:
            raise ValueError(f"pos_weight holds {pos_weight.numel()} elements for {T} task(s)")
    if sample_weight is not None and weight_table is not None:
        raise ValueError("either sample_weight or weight_table (with row_ids), not both")
    if weight_table is not None and (row_ids is None or weight_table.numel() < 1):
        raise ValueError("weight_table needs row_ids and at least one entry")


def _row_weights(sample_weight, weight_table, row_ids, n_rows: int) -> Optional[torch.Tensor]:
    """The sample weight of each of the leading ``n_rows`` rows, or None: ``sample_weight`` itself, or ``weight_table[row_ids]``
    with an id outside the table read as +0.0."""
    if sample_weight is not None:
        if sample_weight.numel() < n_rows:
            raise ValueError(f"sample_weight holds {sample_weight.numel()} elements for {n_rows} rows")
        return sample_weight.detach().reshape(-1)[:n_rows]
    if weight_table is None:
        return None
    table = weight_table.detach().reshape(-1)
    ids = row_ids.reshape(-1)[:n_rows].long().to(table.device)
    m = table.numel()
    inside = (ids >= 0) & (ids < m)
    return torch.where(inside, table[ids.clamp(0, m - 1)], torch.zeros((), dtype=table.dtype, device=table.device))


def task_head_reference(emb: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor], target: torch.Tensor,
                        task: Optional[torch.Tensor], loss: str = "bce", keep: Optional[torch.Tensor] = None,
                        n_rows: Optional[int] = None, task_table: Optional[torch.Tensor] = None,
                        row_ids: Optional[torch.Tensor] = None, sample_weight: Optional[torch.Tensor] = None,
                        pos_weight: Optional[torch.Tensor] = None,
                        weight_table: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """``(loss, pred [n_rows])`` of the task-indexed head in torch operators, in the dtype of ``emb``, differentiable: the
    DEFINITION of ``task_head_loss`` (and what it runs for more than 32 tasks or an embedding wider than 64).

    Row ``i < n_rows`` has the task ``t_i = task[i]`` (or ``task_table[row_ids[i]]``) and is labelled when ``0 <= t_i < T``
    (-1 by convention otherwise); ``pred_i = (keep_i * emb_i) . weight[t_i] + bias[t_i]`` for a labelled row and +0.0 for any
    other; ``loss`` is the sum of the labelled rows' terms -- ``"bce"``: BCE with logits, ``"mse"`` / ``"mse_sum"``: squared
    error -- over ``max(n_labelled, 1)`` (``"mse_sum"``: not divided).  ``keep [n_rows, H]``: explicit dropout multipliers, or
    None.  ``target`` of an unlabelled row is not used (a NaN there is harmless); rows from ``n_rows`` on take no part.

    The weighted loss -- ``torch.nn.functional.binary_cross_entropy_with_logits(x, y, weight=s, pos_weight=p)`` with
    ``reduction='mean'``, and its squared-error counterpart: a labelled row's term is multiplied by its sample weight ``s_i``
    (``sample_weight[i]``, or ``weight_table[row_ids[i]]`` with an id outside the table read as +0.0; absent: 1), and with
    ``pos_weight [T]`` (``"bce"`` only) the term is ``s_i ((1 - y) x + L (log1p(e^-|x|) + max(-x, 0)))`` with ``L = 1 + (p_t - 1) y``.
    The mean still divides by the number of labelled rows, not by the sum of the weights.  Weights are constants (one that
    requires a gradient raises ``ValueError``) and plain multipliers: zero gives zero, a NaN on a labelled row propagates, the
    weight of an unlabelled row or of a row from ``n_rows`` on is never used.  Neither ``task`` nor ``task_table``: every row has
    task 0 (``T`` must be 1)."""
    loss_kind(loss)
    n = emb.shape[0] if n_rows is None else int(n_rows)
    T = weight.shape[0]
    _check_loss_weights(loss, T, sample_weight, pos_weight, weight_table, row_ids)
    if task is None and task_table is None:
        if T != 1:
            raise ValueError("task_head_reference without task or task_table needs a one-output head")
        t = torch.zeros(n, dtype=torch.int64, device=emb.device)
    else:
        t = _row_tasks(task, task_table, row_ids, n).to(emb.device)
    lab = (t >= 0) & (t < T)
    t = torch.where(lab, t, torch.zeros_like(t))
    e = emb[:n]
    if keep is not None:
        e = e * keep[:n].to(e.dtype)
    pred = (e * weight[t]).sum(dim=1)
    if bias is not None:
        pred = pred + bias[t]
    zero = torch.zeros((), dtype=pred.dtype, device=pred.device)
    pred = torch.where(lab, pred, zero)
    y = torch.where(lab, target.reshape(-1)[:n].to(pred.dtype), zero)
    if loss == "bce" and pos_weight is not None:
        # (1 - y) x + L log(1 + e^-x): torch's form in value, with (1 - y) - L sigmoid(-x) as its derivative
        L = 1 + (pos_weight.detach().reshape(-1).to(device=pred.device, dtype=pred.dtype)[t] - 1) * y
        term = (1 - y) * pred + L * torch.logaddexp(-pred, torch.zeros_like(pred))
    elif loss == "bce":
        # log(1 + e^x) - x y: torch's max(x, 0) - x y + log1p(e^-|x|) in value, with sigmoid(x) - y as its derivative at x = 0 too
        term = torch.logaddexp(pred, torch.zeros_like(pred)) - pred * y
    else:
        term = (pred - y) ** 2
    s = _row_weights(sample_weight, weight_table, row_ids, n)
    if s is not None:
        # (an unlabelled row's weight is not used: zeroed BEFORE the product, so a NaN there reaches neither value nor gradient)
        term = torch.where(lab, s.to(device=pred.device, dtype=pred.dtype), zero) * term
    total = torch.where(lab, term, zero).sum()
    if loss != "mse_sum":
        total = total / lab.sum().clamp(min=1).to(pred.dtype)
    return total, pred


class _TaskHeadFn(_HeadFnBase):
    """``mkgnn_task_head_*``: ``_BceHeadFn`` with a task per row (``task [>= n_rows]``, or a task table read through ``row_ids``)."""
    SYMS = ("mkgnn_task_head_fused", "mkgnn_task_head_forward", "mkgnn_task_head_backward")

    @staticmethod
    def _weight(weight):
        return weight.contiguous()

    @staticmethod
    def _workspace_bytes(lib, B, H, w):
        return lib.mkgnn_task_head_workspace_bytes(B, H, w.shape[0])

    @staticmethod
    def _extra(w, vectors):
        task, row_ids = vectors[:2]
        return (w.shape[0],), (_lib.ptr(task), _lib.ptr(row_ids), 0 if task is None else task.numel()), ()

    @staticmethod
    def forward(ctx, emb, weight, bias, target, task, row_ids, p_drop, n_rows, kind):
        return _TaskHeadFn._run(ctx, emb, weight, bias, target, p_drop, n_rows, kind, (_i32(task), _i32(row_ids)))


def _loss_weights(sw: Optional[torch.Tensor], wids: Optional[torch.Tensor], pw: Optional[torch.Tensor]) -> "_lib.LossWeights":
    """``mkgnn_loss_weights`` over float32 / int32 contiguous device tensors (the caller keeps them alive across the call)."""
    lw = _lib.LossWeights()
    lw.sample_weight, lw.weight_ids, lw.pos_weight = _lib.ptr(sw), _lib.ptr(wids), _lib.ptr(pw)
    lw.n_sample_weight = 0 if sw is None else sw.numel()
    return lw


class _WeightedTaskHeadFn(_TaskHeadFn):
    """``mkgnn_task_head_weighted_*``: ``_TaskHeadFn`` with a sample weight per row (``sw``, read directly or through ``wids``), a
    positive weight per task (``pw``), and ``task`` None for "every row has task 0" (a one-output head).  ``task_ids``: the ids the
    TASK is read through (a task table); ``wids``: the ids the WEIGHT is read through -- one id vector may serve as both."""
    SYMS = ("mkgnn_task_head_weighted_fused", "mkgnn_task_head_weighted_forward", "mkgnn_task_head_weighted_backward")

    @staticmethod
    def _extra(w, vectors):
        dims, index, _ = _TaskHeadFn._extra(w, vectors)
        return dims, index, (ctypes.byref(_loss_weights(*vectors[2:])),)

    @staticmethod
    def forward(ctx, emb, weight, bias, target, task, task_ids, sw, wids, pw, p_drop, n_rows, kind):
        return _WeightedTaskHeadFn._run(ctx, emb, weight, bias, target, p_drop, n_rows, kind,
                                        (_i32(task), _i32(task_ids), _f32(sw), _i32(wids), _f32(pw)))


def _task_head_loss(who: str, emb, ffn, target, task, loss: str, dropout_p: float, n_rows, task_table, row_ids,
                    sample_weight, pos_weight, weight_table) -> torch.Tensor:
    """The body of ``task_head_loss`` and of a weighted ``head_loss``: the checks, then ``_TaskHeadFn``, or with any of the three
    weights ``_WeightedTaskHeadFn`` (where ``task`` and ``task_table`` may both be None: every row has task 0), or the definition
    in torch operators for a shape the kernels do not take."""
    weighted = sample_weight is not None or pos_weight is not None or weight_table is not None
    _lib.require_gpu_tensor(emb, "graph_embedding")
    kind = loss_kind(loss)
    n_rows = emb.shape[0] if n_rows is None else int(n_rows)
    T, H = ffn.weight.shape
    if (task is not None and task_table is not None) or (not weighted and (
            (task is None) == (task_table is None) or (task_table is None) != (row_ids is None))):
        raise ValueError(f"{who} needs either task, or task_table together with row_ids")
    if task is None and task_table is None and T != 1:
        raise ValueError(f"{who} without task or task_table needs a one-output linear layer")
    if task_table is not None and (row_ids is None or task_table.numel() < 1):
        raise ValueError(f"{who}: task_table needs row_ids and at least one entry")
    _check_loss_weights(loss, T, sample_weight, pos_weight, weight_table, row_ids)
    per_row = [t for t in (task, sample_weight, row_ids if (task_table is not None or weight_table is not None) else None)
               if t is not None]
    if emb.dim() != 2 or ffn.in_features != emb.shape[1] or n_rows <= 0 or n_rows > emb.shape[0] or target.numel() < n_rows \
            or any(t.numel() < n_rows for t in per_row):
        raise ValueError(f"{who} needs an [n, H] embedding, an H-input linear layer and a target, a task, a weight (or a row id) "
                         "per (leading) row")
    if not 0.0 <= dropout_p < 1.0:
        raise ValueError(f"dropout probability {dropout_p} outside [0, 1)")
    for name, t in (("task", task), ("task_table", task_table), ("row_ids", row_ids), ("target", target),
                    ("sample_weight", sample_weight), ("pos_weight", pos_weight), ("weight_table", weight_table)):
        if t is not None:
            _lib.require_gpu_tensor(t, name)
    if not task_head_supported(T, H) or (weighted and not _WEIGHTED_LOSS):
        keep = None
        if dropout_p > 0.0:
            keep = torch.empty((n_rows, H), dtype=emb.dtype, device=emb.device).bernoulli_(1.0 - dropout_p).mul_(1.0 / (1.0 - dropout_p))
        return task_head_reference(emb, ffn.weight, ffn.bias, target, task, loss, keep, n_rows, task_table, row_ids,
                                   sample_weight, pos_weight, weight_table)[0]
    tasks, task_ids = (task, None) if task_table is None else (task_table, row_ids)
    if not weighted:
        return _TaskHeadFn.apply(emb, ffn.weight, ffn.bias, target, tasks, task_ids, float(dropout_p), n_rows, kind)
    return _WeightedTaskHeadFn.apply(emb, ffn.weight, ffn.bias, target, tasks, task_ids,
                                     sample_weight if sample_weight is not None else weight_table,
                                     row_ids if weight_table is not None else None, pos_weight, float(dropout_p), n_rows, kind)


def task_head_loss(emb: torch.Tensor, ffn: torch.nn.Linear, target: torch.Tensor, task: Optional[torch.Tensor] = None,
                   loss: str = "bce", dropout_p: float = 0.0, n_rows: Optional[int] = None,
                   task_table: Optional[torch.Tensor] = None, row_ids: Optional[torch.Tensor] = None,
                   sample_weight: Optional[torch.Tensor] = None, pos_weight: Optional[torch.Tensor] = None,
                   weight_table: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The masked multi-task loss of a ``T``-output ``ffn``: ``task_head_reference(dropout(emb), ffn.weight, ffn.bias, target,
    ...)[0]`` as two launches each way (``_TaskHeadFn``).  Every row names ONE task -- ``task [>= n_rows]`` (int32; -1, or anything
    outside ``[0, T)``: no label), or ``task_table [M]`` with ``row_ids [>= n_rows]`` (int32, on the device: row i has
    ``task_table[row_ids[i]]``; both may be static buffers a captured step refills) -- and contributes the loss of that output
    alone; the mean kinds divide by the number of labelled rows.  ``dropout_p``, its generator (``head_rng_state``) and mask,
    ``n_rows`` and the loss kinds are ``head_loss``'s.  More than 32 tasks or an embedding wider than 64: the same expression
    through torch operators on the GPU.

    ``sample_weight [>= n_rows]`` (or ``weight_table [M]`` read through the same ``row_ids``) and ``pos_weight [T]``: the weighted
    loss of ``task_head_reference`` on ``mkgnn_task_head_weighted_*`` (``_WeightedTaskHeadFn``), and then ``task`` and ``task_table``
    may both be absent for a one-output ``ffn`` (every row has task 0).  ``MKGNN_WEIGHTED_LOSS=0`` runs the definition in torch
    operators instead.  With none of the three given nothing changes."""
    return _task_head_loss("task_head_loss", emb, ffn, target, task, loss, dropout_p, n_rows, task_table, row_ids, sample_weight,
                           pos_weight, weight_table)


# ------------------------------------------------------------------- label-matrix head: labels [n, T] with holes --
def label_head_supported(T: int, H: int) -> bool:
    """The shapes ``mkgnn_label_head_*`` take (the task-indexed head's); anything else goes through ``label_head_reference`` on
    the GPU.  (A call must also keep ``n_rows * T`` below 2^31: the labelled-entry count is an exact int.)"""
    return task_head_supported(T, H)


# MKGNN_LABEL_HEAD=0 (A/B, diagnostics): the label-matrix loss runs its definition (label_head_reference) in torch operators on
# the GPU instead of the kernels
_LABEL_HEAD = os.environ.get("MKGNN_LABEL_HEAD", "1") != "0"


def _row_labels(labels, label_table, row_ids, n_rows: int) -> torch.Tensor:
    """The label row of each of the leading ``n_rows`` rows ``[n_rows, T]``: ``labels`` itself, or ``label_table[row_ids]`` with an
    id outside the table read as a row of NaN."""
    if labels is not None:
        return labels[:n_rows]
    ids = row_ids.reshape(-1)[:n_rows].long().to(label_table.device)
    m = label_table.shape[0]
    inside = (ids >= 0) & (ids < m)
    rows = label_table[ids.clamp(0, max(m - 1, 0))]
    return torch.where(inside[:, None], rows, torch.full_like(rows, float("nan")))


def label_head_reference(emb: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor], labels: Optional[torch.Tensor],
                         loss: str = "bce", keep: Optional[torch.Tensor] = None, n_rows: Optional[int] = None,
                         label_table: Optional[torch.Tensor] = None, row_ids: Optional[torch.Tensor] = None,
                         sample_weight: Optional[torch.Tensor] = None, pos_weight: Optional[torch.Tensor] = None,
                         weight_table: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """``(loss, pred [n_rows, T])`` of the label-matrix head in torch operators, in the dtype of ``emb``, differentiable: the
    DEFINITION of ``label_head_loss`` (and what it runs outside the kernels' limits).

    Row ``i < n_rows`` has the labels ``labels[i, :]`` (float, ``[>= n_rows, T]``), or ``label_table[row_ids[i], :]`` with an id
    outside the table read as "no label in any task".  Entry ``(i, t)`` is labelled iff its label is not NaN -- only NaN means
    missing, an infinite label is a label.  ``pred[i, t] = (keep_i * emb_i) . weight[t] + bias[t]`` for EVERY ``(i, t)``, labelled
    or not; a labelled entry's term is ``task_head_reference``'s for that kind -- ``"bce"`` (with ``pos_weight[t]``: ``(1 - y) x + L
    log(1 + e^-x)``, ``L = 1 + (p_t - 1) y``), ``"mse"``, ``"mse_sum"`` -- multiplied by the row's sample weight (``sample_weight[i]``,
    or ``weight_table[row_ids[i]]`` with an id outside the table read as +0.0); ``loss`` is the sum of the labelled terms over
    ``max(n_labelled_entries, 1)`` (``"mse_sum"``: not divided; never the sum of the weights).  An unlabelled entry is removed by a
    select, not by a product: its label, and the weight of a row without labels, reach neither the value nor any gradient.  Rows
    from ``n_rows`` on take no part.  Weights are constants (one that requires a gradient raises ``ValueError``).  With exactly one
    labelled entry per row this is ``task_head_reference`` with that task; with ``T == 1`` and no NaN the single-task head's
    definition."""
    loss_kind(loss)
    n = emb.shape[0] if n_rows is None else int(n_rows)
    T = weight.shape[0]
    if (labels is None) == (label_table is None):
        raise ValueError("label_head_reference needs either labels, or label_table together with row_ids")
    if label_table is not None and row_ids is None:
        raise ValueError("label_table needs row_ids")
    _check_loss_weights(loss, T, sample_weight, pos_weight, weight_table, row_ids)
    e = emb[:n]
    if keep is not None:
        e = e * keep[:n].to(e.dtype)
    pred = e @ weight.t()
    if bias is not None:
        pred = pred + bias
    yl = _row_labels(labels, label_table, row_ids, n).to(device=pred.device)
    lab = ~torch.isnan(yl)
    zero = torch.zeros((), dtype=pred.dtype, device=pred.device)
    y = torch.where(lab, yl.to(pred.dtype), zero)
    x = torch.where(lab, pred, zero)                      # (an unlabelled entry's logit takes no part: selected out before the term)
    if loss == "bce" and pos_weight is not None:
        L = 1 + (pos_weight.detach().reshape(-1).to(device=pred.device, dtype=pred.dtype) - 1) * y
        term = (1 - y) * x + L * torch.logaddexp(-x, torch.zeros_like(x))
    elif loss == "bce":
        term = torch.logaddexp(x, torch.zeros_like(x)) - x * y
    else:
        term = (x - y) ** 2
    s = _row_weights(sample_weight, weight_table, row_ids, n)
    if s is not None:
        # (the weight of an unlabelled entry is not used: zeroed BEFORE the product, so a NaN there reaches nothing)
        term = torch.where(lab, s.to(device=pred.device, dtype=pred.dtype)[:, None].expand_as(term), zero) * term
    total = torch.where(lab, term, zero).sum()
    if loss != "mse_sum":
        total = total / lab.sum().clamp(min=1).to(pred.dtype)
    return total, pred


class _LabelHeadFn(_HeadFnBase):
    """``mkgnn_label_head_*`` on the ``_HeadFnBase`` pattern: the fused entry when a gradient will be asked for, the forward /
    backward pair otherwise, the unit-seed shortcut.  Returns ``(loss, pred [n_rows, T])``; ``pred`` carries no gradient."""
    SYMS = ("mkgnn_label_head_fused", "mkgnn_label_head_forward", "mkgnn_label_head_backward")

    @classmethod
    def _launch(cls, which: int, kind, emb, B, w, y, ids, weights, before: tuple, after: tuple) -> None:
        """``SYMS[which](kind, emb, stride, B, H, T, w, *before, labels, T, ids, rows, *after, weights, workspace, stream)``."""
        lib, dev, (T, H) = _lib.load(), emb.device, w.shape
        with torch.cuda.device(dev):
            ws = _head_workspace(dev, int(lib.mkgnn_label_head_workspace_bytes(B, H, T)))
            _lib.check(getattr(lib, cls.SYMS[which])(int(kind), emb.data_ptr(), _stride0(emb), B, H, T, w.data_ptr(), *before,
                                                     y.data_ptr(), T, _lib.ptr(ids), y.numel() // T, *after,
                                                     ctypes.byref(_loss_weights(*weights)), ws.data_ptr(), ws.numel(),
                                                     _lib.stream_ptr(dev)), cls.SYMS[which])

    @staticmethod
    def forward(ctx, emb, weight, bias, labels, ids, sw, wids, pw, p_drop, n_rows, kind):
        cls = _LabelHeadFn
        emb = _row_major(emb if emb.dtype == torch.float32 else emb.float())
        w, y = weight.contiguous(), _f32(labels)
        ids, weights = _i32(ids), (_f32(sw), _i32(wids), _f32(pw))
        B, dev, T = int(n_rows), emb.device, weight.shape[0]
        ctx.family, ctx.kind, ctx.n_rows = cls, kind, B
        ctx.wshape, ctx.has_bias, ctx.p_drop = weight.shape, bias is not None, float(p_drop)
        pred = torch.empty((B, T), dtype=torch.float32, device=dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        rng = head_rng_state(dev) if p_drop > 0.0 else None
        used = torch.empty(2, dtype=torch.int64, device=dev) if p_drop > 0.0 else None
        after = (ctx.p_drop, _lib.ptr(rng), _lib.ptr(used), pred.data_ptr(), T, loss.data_ptr())
        ctx.unit = None
        if any(ctx.needs_input_grad[:3]) and not _SPLIT_HEAD:
            ctx.unit, gargs = cls._grads(ctx, emb, w)
            cls._launch(0, kind, emb, B, w, y, ids, weights, (_lib.ptr(bias),), after + gargs)
        else:
            cls._launch(1, kind, emb, B, w, y, ids, weights, (_lib.ptr(bias),), after)
        ctx.save_for_backward(emb, w, y, pred, used, ids, *weights)
        ctx.mark_non_differentiable(pred)
        return loss, pred

    @staticmethod
    def backward(ctx, grad_loss, _grad_pred=None):
        if ctx.unit is not None:
            grads, ctx.unit = ctx.unit, None
            if not _is_unit_seed(grad_loss):                 # d loss is not the registered 1: scale
                gl = grad_loss.reshape(()).float()
                grads = tuple(None if g is None else g * gl for g in grads)
        else:
            emb, w, y, pred, used, ids, *weights = ctx.saved_tensors
            gl = grad_loss.reshape(1).float().contiguous()
            grads, gargs = ctx.family._grads(ctx, emb, w)
            ctx.family._launch(2, ctx.kind, emb, ctx.n_rows, w, y, ids, weights, (),
                               (pred.data_ptr(), w.shape[0], gl.data_ptr(), ctx.p_drop, _lib.ptr(used)) + gargs)
        gemb, gw, gb = grads
        return (gemb, gw, gb) + (None,) * (len(ctx.needs_input_grad) - 3)


def label_head_loss(emb: torch.Tensor, ffn: torch.nn.Linear, labels: Optional[torch.Tensor] = None, loss: str = "bce",
                    dropout_p: float = 0.0, n_rows: Optional[int] = None, label_table: Optional[torch.Tensor] = None,
                    row_ids: Optional[torch.Tensor] = None, sample_weight: Optional[torch.Tensor] = None,
                    pos_weight: Optional[torch.Tensor] = None, weight_table: Optional[torch.Tensor] = None,
                    return_pred: bool = False):
    """The multi-label loss of a ``T``-output ``ffn`` on a label matrix with holes: ``label_head_reference(dropout(emb), ffn.weight,
    ffn.bias, labels, ...)[0]`` as two launches each way (``_LabelHeadFn``, ``mkgnn_label_head_*``).  Every row carries a row of
    labels -- ``labels [>= n_rows, T]`` (float32, NaN: not measured), or ``label_table [M, T]`` with ``row_ids [>= n_rows]`` (int32,
    on the device; both may be static buffers a captured step refills) -- so the network runs once per molecule, not once per
    (molecule, assay) pair as with ``task_head_loss``.  ``dropout_p``, its generator (``head_rng_state``) and mask, ``n_rows``, the
    loss kinds and the weights (``sample_weight [>= n_rows]``, or ``weight_table [M]`` read through the same ``row_ids``; ``pos_weight
    [T]``, ``"bce"`` only) are ``task_head_loss``'s.  ``return_pred``: ``(loss, pred [n_rows, T])``, ``pred`` without a gradient and,
    on the kernels, bit for bit ``task_scores`` at dropout 0.  Outside ``label_head_supported`` (or ``n_rows * T >= 2^31``), and with
    ``MKGNN_LABEL_HEAD=0``, the definition runs in torch operators on the GPU."""
    who = "label_head_loss"
    _lib.require_gpu_tensor(emb, "graph_embedding")
    kind = loss_kind(loss)
    n_rows = emb.shape[0] if n_rows is None else int(n_rows)
    T, H = ffn.weight.shape
    if (labels is None) == (label_table is None):
        raise ValueError(f"{who} needs either labels, or label_table together with row_ids")
    if label_table is not None and (row_ids is None or label_table.dim() != 2 or label_table.shape[0] < 1):
        raise ValueError(f"{who}: label_table [M, T] needs row_ids and at least one row")
    mat = labels if labels is not None else label_table
    if mat.dim() != 2 or mat.shape[1] != T or not mat.is_floating_point():
        raise ValueError(f"{who}: the labels must be a float [rows, {T}] matrix for a {T}-output linear layer, not {tuple(mat.shape)}")
    _check_loss_weights(loss, T, sample_weight, pos_weight, weight_table, row_ids)
    per_row = [t for t in (sample_weight, row_ids if (label_table is not None or weight_table is not None) else None)
               if t is not None]
    if emb.dim() != 2 or ffn.in_features != emb.shape[1] or n_rows <= 0 or n_rows > emb.shape[0] \
            or (labels is not None and labels.shape[0] < n_rows) or any(t.numel() < n_rows for t in per_row):
        raise ValueError(f"{who} needs an [n, H] embedding, an H-input linear layer and a label row, a weight (or a row id) per "
                         "(leading) row")
    if not 0.0 <= dropout_p < 1.0:
        raise ValueError(f"dropout probability {dropout_p} outside [0, 1)")
    for name, t in (("labels", labels), ("label_table", label_table), ("row_ids", row_ids), ("sample_weight", sample_weight),
                    ("pos_weight", pos_weight), ("weight_table", weight_table)):
        if t is not None:
            _lib.require_gpu_tensor(t, name)
    if not label_head_supported(T, H) or n_rows * T >= 2 ** 31 or not _LABEL_HEAD:
        keep = None
        if dropout_p > 0.0:
            keep = torch.empty((n_rows, H), dtype=emb.dtype, device=emb.device).bernoulli_(1.0 - dropout_p).mul_(1.0 / (1.0 - dropout_p))
        out, pred = label_head_reference(emb, ffn.weight, ffn.bias, labels, loss, keep, n_rows, label_table, row_ids,
                                         sample_weight, pos_weight, weight_table)
        return (out, pred.detach()) if return_pred else out
    sw = sample_weight if sample_weight is not None else weight_table
    out, pred = _LabelHeadFn.apply(emb, ffn.weight, ffn.bias, mat, row_ids if label_table is not None else None, sw,
                                   row_ids if weight_table is not None else None, pos_weight, float(dropout_p), n_rows, kind)
    return (out, pred) if return_pred else out


def task_scores(emb: torch.Tensor, ffn: torch.nn.Linear, n_rows: Optional[int] = None, out: Optional[torch.Tensor] = None,
                task_major: bool = False) -> torch.Tensor:
    """``pred [n_rows, T]`` (``task_major``: ``[T, n_rows]``): EVERY output of a ``T``-output ``ffn`` for the leading ``n_rows`` rows of
    a float32 CUDA ``emb [n, H]`` -- ``emb_i . ffn.weight[t] + ffn.bias[t]`` as one launch (``mkgnn_task_scores``), and bit for bit
    the ``pred`` the task-indexed head (``task_head_loss``, dropout 0) gives row ``i`` when it is labelled with task ``t``.  ``out``: a
    float32 tensor of that shape on the device to write into (its strides are passed on; elements it holds beyond that shape are
    not touched).  More than 32 tasks or an embedding wider than 64: the same expression through torch operators on the GPU.
    It has no autograd node: called where a gradient is being recorded for one of its inputs it raises instead of dropping it
    (``task_head_loss`` is the operator with gradients)."""
    _lib.require_gpu_tensor(emb, "graph_embedding")
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (emb, ffn.weight, ffn.bias)):
        raise RuntimeError("task_scores is forward only: call it under torch.no_grad() (or on detached inputs); "
                           "task_head_loss is the operator with gradients")
    if emb.dim() != 2 or emb.dtype != torch.float32 or ffn.in_features != emb.shape[1]:
        raise ValueError("task_scores needs a float32 [n, H] embedding and an H-input linear layer")
    n = emb.shape[0] if n_rows is None else int(n_rows)
    if not 0 <= n <= emb.shape[0]:
        raise ValueError(f"n_rows = {n_rows} outside [0, {emb.shape[0]}]")
    T, H = ffn.weight.shape
    dev = emb.device
    shape = (T, n) if task_major else (n, T)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=dev)
    elif out.dtype != torch.float32 or out.device != dev or tuple(out.shape) != shape:
        raise ValueError(f"out: a float32 tensor of shape {shape} on {dev}")
    if n == 0:
        return out
    w = ffn.weight.detach()
    b = None if ffn.bias is None else ffn.bias.detach()
    if not task_head_supported(T, H):
        pred = (emb[:n, None, :] * w[None]).sum(dim=2)
        if b is not None:
            pred = pred + b
        out.copy_(pred.t() if task_major else pred)
        return out
    emb, w = _row_major(emb), w.contiguous()
    rs, ts = (out.stride(1), out.stride(0)) if task_major else (out.stride(0), out.stride(1))
    with torch.cuda.device(dev):
        _lib.check(_lib.load().mkgnn_task_scores(emb.data_ptr(), _stride0(emb), n, H, T, w.data_ptr(), _lib.ptr(b), out.data_ptr(),
                                                 rs, ts, _lib.stream_ptr(dev)), "mkgnn_task_scores")
    return out


COSINE_EPS = 1e-8                     # MKGNN_EPS: the clamp of each norm (float32(1e-8) where it is applied)


def embedding_cosine_supported(Q: int, H: int) -> bool:
    """The shapes ``mkgnn_embed_cosine`` takes; anything else goes through torch operators on the GPU."""
    return 1 <= Q <= _lib.EMBED_COSINE_MAX_QUERIES and 1 <= H <= _lib.EMBED_COSINE_MAX_H


def embedding_cosine(emb: torch.Tensor, queries: torch.Tensor, n_rows: Optional[int] = None, out: Optional[torch.Tensor] = None,
                     query_major: bool = False) -> torch.Tensor:
    """``sim [n_rows, Q]`` (``query_major``: ``[Q, n_rows]``): the cosine similarity of the leading ``n_rows`` rows of a float32 CUDA
    ``emb [n, H]`` with every row of a float32 CUDA ``queries [Q, H]`` -- ``(e . q) / (max(||e||, eps) * max(||q||, eps))``, ``eps =
    1e-8``, each vector clamped on its own (``torch.nn.functional.cosine_similarity``; ``screening.cosine_reference`` is the
    definition in float64) -- as one launch (``mkgnn_embed_cosine``).  The queries are read raw: nothing is prepared ahead, so a
    captured call follows the contents of both tensors.  A zero row or query gives +0.0, a NaN its own row or column of NaN.  The
    bits of an element depend on its row's and its query's values alone.  ``out``: a float32 tensor of that shape on the device to
    write into (its strides are passed on; elements it holds beyond that shape are not touched).  More than 32 queries or an
    embedding wider than 64: the same definition through torch operators on the GPU.  It has no autograd node: called where a
    gradient is being recorded for one of its inputs it raises instead of dropping it."""
    if not (torch.is_tensor(emb) and torch.is_tensor(queries)) or emb.dim() != 2 or queries.dim() != 2 \
            or emb.dtype != torch.float32 or queries.dtype != torch.float32 or queries.shape[1] != emb.shape[1]:
        raise ValueError("embedding_cosine needs a float32 [n, H] embedding and float32 [Q, H] queries")
    Q, H = queries.shape
    if Q < 1 or H < 1:
        raise ValueError(f"embedding_cosine needs at least one query and one column, not {Q} x {H}")
    if not emb.is_cuda or queries.device != emb.device:
        raise ValueError(f"embedding_cosine runs on the GPU: emb is on {emb.device}, queries on {queries.device} (there is no CPU "
                         "path; screening.cosine_reference is the host form)")
    if torch.is_grad_enabled() and (emb.requires_grad or queries.requires_grad):
        raise RuntimeError("embedding_cosine is forward only: call it under torch.no_grad() (or on detached inputs)")
    n = emb.shape[0] if n_rows is None else int(n_rows)
    if not 0 <= n <= emb.shape[0]:
        raise ValueError(f"n_rows = {n_rows} outside [0, {emb.shape[0]}]")
    dev = emb.device
    shape = (Q, n) if query_major else (n, Q)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=dev)
    elif out.dtype != torch.float32 or out.device != dev or tuple(out.shape) != shape:
        raise ValueError(f"out: a float32 tensor of shape {shape} on {dev}")
    if n == 0:
        return out
    if not embedding_cosine_supported(Q, H):
        # (in float64, rounded once at the end: well inside the float32 bound, and no product of float32 values underflows there)
        e, q = emb[:n].detach().double(), queries.detach().double()
        eps = float(torch.tensor(COSINE_EPS, dtype=torch.float32))
        ie = 1.0 / e.square().sum(dim=1).sqrt().clamp_min(eps)
        iq = 1.0 / q.square().sum(dim=1).sqrt().clamp_min(eps)
        sim = ((e @ q.t() + 0.0) * ie[:, None] * iq[None, :]).float()
        out.copy_(sim.t() if query_major else sim)
        return out
    emb, queries = _row_major(emb.detach()), _row_major(queries.detach())
    rs, qs = (out.stride(1), out.stride(0)) if query_major else (out.stride(0), out.stride(1))
    with torch.cuda.device(dev):
        _lib.check(_lib.load().mkgnn_embed_cosine(emb.data_ptr(), _stride0(emb), n, H, queries.data_ptr(), _stride0(queries), Q,
                                                  out.data_ptr(), rs, qs, _lib.stream_ptr(dev)), "mkgnn_embed_cosine")
    return out


def embedding_max_cosine_supported(R: int, H: int) -> bool:
    """The shapes ``mkgnn_embed_max_cosine`` takes; anything else goes through torch operators on the GPU."""
    return 1 <= R <= _lib.MAX_COSINE_MAX_REFS and 1 <= H <= _lib.MAX_COSINE_MAX_H


MAX_COSINE_TORCH_CHUNK = 4096         # references per step of the torch route: no [n, R] matrix beyond [n, 4096] exists


def _first_max(sim: torch.Tensor):
    """``(value, index)`` per row of ``sim [n, c]`` by the order of ``screening.max_cosine_reference``: non-NaN before NaN, larger
    first, the lower index among equals (``-0.0 == +0.0``); an all-NaN row gives ``(NaN, 0)``."""
    c = sim.shape[1]
    nan = torch.isnan(sim)
    clean = torch.where(nan, torch.full_like(sim, float("-inf")), sim)
    best = clean.max(dim=1, keepdim=True).values
    col = torch.arange(c, device=sim.device)[None, :].expand_as(sim)
    arg = torch.where((clean == best) & ~nan, col, torch.full_like(col, c)).min(dim=1).values
    none = arg == c
    arg = torch.where(none, torch.zeros_like(arg), arg)
    value = sim.gather(1, arg[:, None])[:, 0]
    return torch.where(none, torch.full_like(value, float("nan")), value), arg


_MAX_COSINE_WS: dict = {}


def _max_cosine_workspace(dev, nbytes: int, given: Optional[torch.Tensor]) -> torch.Tensor:
    """The scratch of one ``mkgnn_embed_max_cosine``: the caller's ``workspace`` when given (uint8, on the device, large enough); a
    fresh buffer inside a capture (the graph's pool keeps it, and no other graph shares it); otherwise one buffer per device that
    only grows, so an eager loop over batches allocates once (eager calls on one stream are ordered; callers on several streams pass
    their own)."""
    if given is not None:
        if not torch.is_tensor(given) or given.dtype != torch.uint8 or given.device != dev or not given.is_contiguous() \
                or given.numel() < nbytes:
            raise ValueError(f"workspace: a contiguous uint8 tensor of at least {nbytes} bytes on {dev}")
        return given
    if torch.cuda.is_current_stream_capturing():
        return torch.empty(nbytes, dtype=torch.uint8, device=dev)
    held = _MAX_COSINE_WS.get(str(dev))
    if held is None or held.numel() < nbytes:
        held = _MAX_COSINE_WS[str(dev)] = torch.empty(max(nbytes, 1 << 16), dtype=torch.uint8, device=dev)
    return held


def embedding_max_cosine(emb: torch.Tensor, refs: torch.Tensor, n_rows: Optional[int] = None, out=None,
                         workspace: Optional[torch.Tensor] = None):
    """``(max_sim float32 [n_rows], arg_ref int32 [n_rows])``: for each of the leading ``n_rows`` rows of a float32 CUDA ``emb [n, H]``
    its nearest row of a float32 CUDA ``refs [R, H]`` by cosine similarity -- the similarity ``embedding_cosine`` gives for the pair,
    BIT FOR BIT, and the winner the first ``r`` in the order of ``screening.topk_update_reference``: non-NaN before NaN, larger
    first with ``-0.0 == +0.0``, then the lower ``r`` (``screening.max_cosine_reference`` is the definition in float64).  One
    ``mkgnn_embed_max_cosine``: the references are read raw, their norms are taken inside the call, so a captured call follows the
    contents of both tensors; no ``[n, R]`` matrix exists.  A row of NaN, or references that are all NaN, give ``(NaN, 0)``.  ``out``:
    a pair of contiguous tensors ``(float32 [n_rows], int32 [n_rows])`` on the device to write into.  ``workspace``: a uint8 device
    tensor of at least ``mkgnn_embed_max_cosine_workspace_bytes(n_rows, R)`` bytes to use as scratch; without it a per-device buffer
    that only grows serves eager calls, and a call inside a capture allocates its own.  More than 2^20 references or an
    embedding wider than 64: the same definition through torch operators on the GPU, ``MAX_COSINE_TORCH_CHUNK`` references at a time
    (float64 products, rounded once: inside ``screening.cosine_bound``, not the kernel's bits).  It has no autograd node: called where
    a gradient is being recorded for one of its inputs it raises instead of dropping it."""
    if not (torch.is_tensor(emb) and torch.is_tensor(refs)) or emb.dim() != 2 or refs.dim() != 2 \
            or emb.dtype != torch.float32 or refs.dtype != torch.float32 or refs.shape[1] != emb.shape[1]:
        raise ValueError("embedding_max_cosine needs a float32 [n, H] embedding and float32 [R, H] references")
    R, H = refs.shape
    if R < 1 or H < 1:
        raise ValueError(f"embedding_max_cosine needs at least one reference and one column, not {R} x {H}")
    if not emb.is_cuda or refs.device != emb.device:
        raise ValueError(f"embedding_max_cosine runs on the GPU: emb is on {emb.device}, refs on {refs.device} (there is no CPU "
                         "path; screening.max_cosine_reference is the host form)")
    if torch.is_grad_enabled() and (emb.requires_grad or refs.requires_grad):
        raise RuntimeError("embedding_max_cosine is forward only: call it under torch.no_grad() (or on detached inputs)")
    n = emb.shape[0] if n_rows is None else int(n_rows)
    if not 0 <= n <= emb.shape[0]:
        raise ValueError(f"n_rows = {n_rows} outside [0, {emb.shape[0]}]")
    dev = emb.device
    if out is None:
        out = (torch.empty(n, dtype=torch.float32, device=dev), torch.empty(n, dtype=torch.int32, device=dev))
    else:
        ok = isinstance(out, (tuple, list)) and len(out) == 2 and all(torch.is_tensor(o) for o in out)
        if not ok or out[0].dtype != torch.float32 or out[1].dtype != torch.int32 \
                or any(o.device != dev or tuple(o.shape) != (n,) or not o.is_contiguous() for o in out):
            raise ValueError(f"out: a pair of contiguous tensors (float32 [{n}], int32 [{n}]) on {dev}")
    max_sim, arg_ref = out
    if n == 0:
        return max_sim, arg_ref
    if not embedding_max_cosine_supported(R, H):
        e, eps = emb[:n].detach().double(), float(torch.tensor(COSINE_EPS, dtype=torch.float32))
        ie = 1.0 / e.square().sum(dim=1).sqrt().clamp_min(eps)
        best = arg = None
        for a in range(0, R, MAX_COSINE_TORCH_CHUNK):
            q = refs[a:a + MAX_COSINE_TORCH_CHUNK].detach().double()
            iq = 1.0 / q.square().sum(dim=1).sqrt().clamp_min(eps)
            value, index = _first_max(((e @ q.t() + 0.0) * ie[:, None] * iq[None, :]).float())
            if best is None:
                best, arg = value, index
            else:                                        # (the earlier chunk keeps a tie: it holds the lower indices)
                take = ~torch.isnan(value) & (torch.isnan(best) | (value > best))
                best, arg = torch.where(take, value, best), torch.where(take, index + a, arg)
        max_sim.copy_(best)
        arg_ref.copy_(arg)
        return max_sim, arg_ref
    emb, refs = _row_major(emb.detach()), _row_major(refs.detach())
    lib = _lib.load()
    ws = _max_cosine_workspace(dev, int(lib.mkgnn_embed_max_cosine_workspace_bytes(n, R)), workspace)
    with torch.cuda.device(dev):
        _lib.check(lib.mkgnn_embed_max_cosine(emb.data_ptr(), _stride0(emb), n, H, refs.data_ptr(), _stride0(refs), R,
                                              max_sim.data_ptr(), arg_ref.data_ptr(), ws.data_ptr(), ws.numel(),
                                              _lib.stream_ptr(dev)), "mkgnn_embed_max_cosine")
    return max_sim, arg_ref


def embedding_count_within_supported(R: int, H: int) -> bool:
    """The shapes ``mkgnn_embed_count_within`` takes; anything else goes through torch operators on the GPU."""
    return 1 <= R <= _lib.MAX_COSINE_MAX_REFS and 1 <= H <= _lib.MAX_COSINE_MAX_H


def embedding_count_within(emb: torch.Tensor, refs: torch.Tensor, min_sim: float, n_rows: Optional[int] = None,
                           out: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``counts int32 [n_rows]``: for each of the leading ``n_rows`` rows of a float32 CUDA ``emb [n, H]`` the number of rows ``r`` of a
    float32 CUDA ``refs [R, H]`` with ``S[i, r] > min_sim`` -- ``S[i, r]`` the similarity ``embedding_cosine`` gives for the pair
    (row ``i`` as the row, ``refs[r]`` as the query), BIT FOR BIT, which is also what ``diverse_pick`` compares; the comparison is
    strict and a NaN never counts (``screening.count_within_reference`` is the definition over a given matrix).  There is no
    "self": with ``refs`` the tensor ``emb`` itself the diagonal is a pair like any other.  One ``mkgnn_embed_count_within``: both
    tensors are read raw, so a captured call follows their contents; no ``[n, R]`` matrix exists; a count is a sum of integers and
    depends neither on the order of the references nor on how a launch splits them.  ``min_sim`` is finite.  ``out``: a contiguous
    int32 ``[n_rows]`` tensor on the device to write into (not a view of ``emb`` or ``refs``).  ``workspace``: a uint8 device tensor
    of at least ``mkgnn_embed_count_within_workspace_bytes(n_rows, R)`` bytes to use as scratch; without it a per-device buffer that
    only grows serves eager calls, and a call inside a capture allocates its own.  More than 2^20 references or an embedding
    wider than 64: the same definition through torch operators on the GPU, ``MAX_COSINE_TORCH_CHUNK`` references at a time
    (float64 products, rounded once: inside ``screening.cosine_bound``, not the kernel's bits).  It has no autograd node: called
    where a gradient is being recorded for one of its inputs it raises instead of dropping it."""
    if not (torch.is_tensor(emb) and torch.is_tensor(refs)) or emb.dim() != 2 or refs.dim() != 2 \
            or emb.dtype != torch.float32 or refs.dtype != torch.float32 or refs.shape[1] != emb.shape[1]:
        raise ValueError("embedding_count_within needs a float32 [n, H] embedding and float32 [R, H] references")
    R, H = refs.shape
    if R < 1 or H < 1:
        raise ValueError(f"embedding_count_within needs at least one reference and one column, not {R} x {H}")
    min_sim = float(min_sim)
    if min_sim != min_sim or min_sim in (float("inf"), float("-inf")):
        raise ValueError(f"embedding_count_within: min_sim = {min_sim} is not a finite threshold")
    if not emb.is_cuda or refs.device != emb.device:
        raise ValueError(f"embedding_count_within runs on the GPU: emb is on {emb.device}, refs on {refs.device} (there is no CPU "
                         "path; screening.count_within_reference is the host form)")
    if torch.is_grad_enabled() and (emb.requires_grad or refs.requires_grad):
        raise RuntimeError("embedding_count_within is forward only: call it under torch.no_grad() (or on detached inputs)")
    n = emb.shape[0] if n_rows is None else int(n_rows)
    if not 0 <= n <= emb.shape[0]:
        raise ValueError(f"n_rows = {n_rows} outside [0, {emb.shape[0]}]")
    dev = emb.device
    if out is None:
        out = torch.empty(n, dtype=torch.int32, device=dev)
    elif not torch.is_tensor(out) or out.dtype != torch.int32 or out.device != dev or tuple(out.shape) != (n,) \
            or not out.is_contiguous():
        raise ValueError(f"out: a contiguous int32 [{n}] tensor on {dev}")
    if n == 0:
        return out
    if not embedding_count_within_supported(R, H):
        e, eps = emb[:n].detach().double(), float(torch.tensor(COSINE_EPS, dtype=torch.float32))
        ie = 1.0 / e.square().sum(dim=1).sqrt().clamp_min(eps)
        total = torch.zeros(n, dtype=torch.int64, device=dev)
        bound = torch.tensor(min_sim, dtype=torch.float32, device=dev)     # (rounded to float32, as the kernel's argument is)
        for a in range(0, R, MAX_COSINE_TORCH_CHUNK):
            q = refs[a:a + MAX_COSINE_TORCH_CHUNK].detach().double()
            iq = 1.0 / q.square().sum(dim=1).sqrt().clamp_min(eps)
            sim = ((e @ q.t() + 0.0) * ie[:, None] * iq[None, :]).float()
            total += (sim > bound).sum(dim=1)                    # (strict; a NaN compares False)
        out.copy_(total)
        return out
    emb, refs = _row_major(emb.detach()), _row_major(refs.detach())
    lib = _lib.load()
    ws = _max_cosine_workspace(dev, int(lib.mkgnn_embed_count_within_workspace_bytes(n, R)), workspace)
    with torch.cuda.device(dev):
        _lib.check(lib.mkgnn_embed_count_within(emb.data_ptr(), _stride0(emb), n, H, refs.data_ptr(), _stride0(refs), R, min_sim,
                                                out.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_ptr(dev)),
                   "mkgnn_embed_count_within")
    return out


def embedding_neighbours_within_supported(R: int, H: int) -> bool:
    """The shapes ``mkgnn_embed_neighbours_within`` takes; anything else goes through torch operators on the GPU."""
    return 1 <= R <= _lib.MAX_COSINE_MAX_REFS and 1 <= H <= _lib.MAX_COSINE_MAX_H


def _neighbours_by_torch(emb, refs, min_sim: float, counts: torch.Tensor):
    """``(nbr int32 [nnz], nbr_sim float32 [nnz])`` of the torch route, rows ascending and references ascending inside a row: the
    similarities of ``embedding_count_within``'s torch route, chunk by chunk, ``nonzero`` of the comparison, then the chunks'
    pairs brought into row order by one stable sort."""
    dev = emb.device
    e, eps = emb.double(), float(torch.tensor(COSINE_EPS, dtype=torch.float32))
    ie = 1.0 / e.square().sum(dim=1).sqrt().clamp_min(eps)
    bound = torch.tensor(min_sim, dtype=torch.float32, device=dev)
    rows, cols, sims = [], [], []
    for a in range(0, refs.shape[0], MAX_COSINE_TORCH_CHUNK):
        q = refs[a:a + MAX_COSINE_TORCH_CHUNK].double()
        iq = 1.0 / q.square().sum(dim=1).sqrt().clamp_min(eps)
        sim = ((e @ q.t() + 0.0) * ie[:, None] * iq[None, :]).float()
        hit = (sim > bound).nonzero()                            # (row-major: by row, then by reference)
        rows.append(hit[:, 0])
        cols.append(hit[:, 1] + a)
        sims.append(sim[hit[:, 0], hit[:, 1]])
    rows, cols, sims = torch.cat(rows), torch.cat(cols), torch.cat(sims)
    order = torch.sort(rows, stable=True).indices                # (the chunks come in reference order: stable keeps it inside a row)
    if not torch.equal(torch.bincount(rows, minlength=counts.numel()), counts.long()):
        raise RuntimeError("embedding_neighbours_within: the torch route's lists and counts disagree")
    return cols[order].to(torch.int32), sims[order]


def embedding_neighbours_within(emb: torch.Tensor, refs: torch.Tensor, min_sim: float, max_pairs: int = 1 << 28,
                                n_rows: Optional[int] = None, row_ptr: Optional[torch.Tensor] = None, out=None,
                                found: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None):
    """``(row_ptr int64 [n_rows + 1], nbr int32 [nnz], nbr_sim float32 [nnz])``: WHICH rows ``r`` of a float32 CUDA ``refs [R, H]``
    ``embedding_count_within`` counts for each of the leading ``n_rows`` rows of a float32 CUDA ``emb [n, H]`` -- those with ``S[i, r] >
    min_sim``, strict, a NaN never -- as CSR lists: row ``i`` owns the slots ``row_ptr[i] .. row_ptr[i + 1]``, ``nbr`` holds its
    references in ASCENDING ``r`` and ``nbr_sim`` their similarities, the bits of ``embedding_cosine`` (``screening.neighbours_reference``
    is the definition over a given matrix).  There is no "self": with ``refs`` the tensor ``emb`` itself the diagonal is a pair like any
    other.  No ``[n, R]`` matrix exists.

    Without ``row_ptr``: ``embedding_count_within``, a ``cumsum``, ONE host read (``nnz``, to allocate the lists), then one
    ``mkgnn_embed_neighbours_within``; ``nnz > max_pairs`` raises ``ValueError`` naming it before anything of that size is allocated;
    that the fill found what the count counted is asserted on the device.  ``nnz == 0`` gives empty lists.

    With ``row_ptr`` (int64 ``[n_rows + 1]`` on the device) the raw form, which reads nothing back and can be captured: ``out`` is the
    pair ``(int32 [capacity], float32 [capacity])`` to write into and ``found`` an int32 ``[n_rows]`` tensor that receives every row's
    number of pairs, written or not; a row writes only inside ``[row_ptr[i], min(row_ptr[i + 1], capacity))`` whatever ``row_ptr``
    holds, and pairs that do not fit are counted in ``found`` and dropped.  ``workspace``: as for the count
    (``mkgnn_embed_neighbours_within_workspace_bytes``).  Returns ``(row_ptr, out[0], out[1])``.

    More than 2^20 references or an embedding wider than 64 (``embedding_neighbours_within_supported``): the same definition through
    torch operators, ``MAX_COSINE_TORCH_CHUNK`` references at a time (float64 products, rounded once: inside
    ``screening.cosine_bound``, not the kernel's bits); that route has no raw form.  It has no autograd node: called where a gradient
    is being recorded for one of its inputs it raises instead of dropping it."""
    who = "embedding_neighbours_within"
    if not (torch.is_tensor(emb) and torch.is_tensor(refs)) or emb.dim() != 2 or refs.dim() != 2 \
            or emb.dtype != torch.float32 or refs.dtype != torch.float32 or refs.shape[1] != emb.shape[1]:
        raise ValueError(f"{who} needs a float32 [n, H] embedding and float32 [R, H] references")
    R, H = refs.shape
    if R < 1 or H < 1:
        raise ValueError(f"{who} needs at least one reference and one column, not {R} x {H}")
    min_sim = float(min_sim)
    if min_sim != min_sim or min_sim in (float("inf"), float("-inf")):
        raise ValueError(f"{who}: min_sim = {min_sim} is not a finite threshold")
    max_pairs = int(max_pairs)
    if max_pairs < 0:
        raise ValueError(f"{who}: max_pairs = {max_pairs} is negative")
    if torch.is_grad_enabled() and (emb.requires_grad or refs.requires_grad):
        raise RuntimeError(f"{who} is forward only: call it under torch.no_grad() (or on detached inputs)")
    if row_ptr is None and (out is not None or found is not None):
        raise ValueError(f"{who}: out and found belong to the raw form, which takes row_ptr")
    if not emb.is_cuda or refs.device != emb.device:
        raise ValueError(f"{who} runs on the GPU: emb is on {emb.device}, refs on {refs.device} (there is no CPU path; "
                         "screening.neighbours_reference is the host form)")
    n = emb.shape[0] if n_rows is None else int(n_rows)
    if not 0 <= n <= emb.shape[0]:
        raise ValueError(f"n_rows = {n_rows} outside [0, {emb.shape[0]}]")
    dev = emb.device
    raw = row_ptr is not None
    if raw:
        if not torch.is_tensor(row_ptr) or row_ptr.dtype != torch.int64 or row_ptr.device != dev or tuple(row_ptr.shape) != (n + 1,) \
                or not row_ptr.is_contiguous():
            raise ValueError(f"row_ptr: a contiguous int64 [{n + 1}] tensor on {dev}")
        ok = isinstance(out, (tuple, list)) and len(out) == 2 and all(torch.is_tensor(o) for o in out)
        if not ok or out[0].dtype != torch.int32 or out[1].dtype != torch.float32 or out[0].dim() != 1 \
                or any(o.device != dev or o.shape != out[0].shape or not o.is_contiguous() for o in out):
            raise ValueError(f"out: a pair of contiguous tensors (int32 [capacity], float32 [capacity]) on {dev}")
        if not torch.is_tensor(found) or found.dtype != torch.int32 or found.device != dev or tuple(found.shape) != (n,) \
                or not found.is_contiguous():
            raise ValueError(f"found: a contiguous int32 [{n}] tensor on {dev}")
        if not embedding_neighbours_within_supported(R, H):
            raise ValueError(f"{who}: the raw form needs a shape the kernel takes (at most {_lib.MAX_COSINE_MAX_REFS} references "
                             f"of at most {_lib.MAX_COSINE_MAX_H} columns), not {R} x {H}")
        nbr, nbr_sim = out
        if n == 0:
            return row_ptr, nbr, nbr_sim
    else:
        counts = embedding_count_within(emb, refs, min_sim, n_rows=n, workspace=workspace)
        row_ptr = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        row_ptr[1:] = torch.cumsum(counts, dim=0, dtype=torch.int64)
        nnz = int(row_ptr[n])                                    # the one host read: the size of the lists
        if nnz > max_pairs:
            raise ValueError(f"{who}: nnz = {nnz} pairs lie above min_sim = {min_sim}, more than max_pairs = {max_pairs}")
        if nnz == 0:
            return row_ptr, torch.empty(0, dtype=torch.int32, device=dev), torch.empty(0, dtype=torch.float32, device=dev)
        if not embedding_neighbours_within_supported(R, H):
            nbr, nbr_sim = _neighbours_by_torch(emb[:n].detach(), refs.detach(), min_sim, counts)
            return row_ptr, nbr, nbr_sim
        nbr = torch.empty(nnz, dtype=torch.int32, device=dev)
        nbr_sim = torch.empty(nnz, dtype=torch.float32, device=dev)
        found = torch.empty(n, dtype=torch.int32, device=dev)
    emb, refs = _row_major(emb.detach()), _row_major(refs.detach())
    lib = _lib.load()
    ws = _max_cosine_workspace(dev, int(lib.mkgnn_embed_neighbours_within_workspace_bytes(n, R)), workspace)
    with torch.cuda.device(dev):
        _lib.check(lib.mkgnn_embed_neighbours_within(emb.data_ptr(), _stride0(emb), n, H, refs.data_ptr(), _stride0(refs), R, min_sim,
                                                     row_ptr.data_ptr(), nbr.numel(), _lib.ptr(nbr), _lib.ptr(nbr_sim),
                                                     found.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_ptr(dev)),
                   "mkgnn_embed_neighbours_within")
    if not raw:
        torch._assert_async((found == counts).all())             # (on the device: the fill found what the count counted)
    return row_ptr, nbr, nbr_sim


_COMPONENTS_WS: dict = {}


def graph_components(row_ptr: torch.Tensor, col: torch.Tensor, n: int, return_rounds: bool = False, out: Optional[torch.Tensor] = None,
                     state: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None, resume: bool = False,
                     _max_rounds: Optional[int] = None):
    """``labels int32 [n]``: for every vertex the smallest vertex of its connected component, in the graph where ``u`` and ``v`` are
    linked if the CSR lists ``(row_ptr int64 [n + 1], col int32 [row_ptr[n]])`` on the GPU hold ``v`` in ``u``'s segment OR ``u`` in
    ``v``'s (``mkgnn_graph_components``; ``screening.components_reference`` is the definition) -- the single-linkage clusters of a
    threshold when the lists are ``embedding_neighbours_within``'s self-join.  Self-loops and duplicate edges are harmless.  One
    call enqueues ``_lib.components_rounds(n)`` hook-and-compress rounds without a host round trip; this function then reads the
    operator's ``state`` ONCE, goes on with ``resume = 1`` while it says "not converged" (every such call lowers a label or
    converges), and raises ``ValueError`` if a column outside ``[0, n)`` or a segment outside ``0 <= row_ptr[v] <= row_ptr[v + 1] <=
    row_ptr[n]`` was met (they are skipped, never used as an index); before the launch it reads ``row_ptr[n]`` and refuses lists
    longer than ``col``.  ``return_rounds=True``: ``(labels, rounds)``, the rounds that changed a label.

    ``state`` (an int32 ``[4]`` device tensor) selects the raw form, which reads nothing back and can be captured: ONE call, after
    which ``state`` holds (changing rounds, converged, skipped input, 0) for the caller to look at, and ``col`` must hold
    ``row_ptr[n]`` entries.  ``out``: a contiguous int32 ``[n]`` tensor for the labels.  ``resume=True`` (with ``out``): go on from the
    labels an earlier call on the same graph left in ``out`` -- what the raw form's caller does while ``state[1] == 0``.
    ``workspace``: an int32 device tensor of at least ``mkgnn_graph_components_workspace_bytes(n)`` bytes.  ``_max_rounds`` is for the
    tests: fewer rounds per call."""
    who = "graph_components"
    n = int(n)
    if not 0 <= n <= _lib.COMPONENTS_MAX_VERTICES:
        raise ValueError(f"{who}: n = {n} outside [0, {_lib.COMPONENTS_MAX_VERTICES}]")
    if not (torch.is_tensor(row_ptr) and torch.is_tensor(col)) or row_ptr.dtype != torch.int64 or col.dtype != torch.int32 \
            or tuple(row_ptr.shape) != (n + 1,) or col.dim() != 1 or not row_ptr.is_contiguous() or not col.is_contiguous():
        raise ValueError(f"{who} needs a contiguous int64 [{n + 1}] row_ptr and a contiguous int32 [nnz] col")
    dev = row_ptr.device
    if dev.type != "cuda" or col.device != dev:
        raise ValueError(f"{who} runs on the GPU: row_ptr is on {dev}, col on {col.device} (there is no CPU path; "
                         "screening.components_reference is the host form)")
    if out is None:
        if resume:
            raise ValueError(f"{who}: resume=True goes on from the labels in out, which was not given")
        out = torch.empty(n, dtype=torch.int32, device=dev)
    elif not torch.is_tensor(out) or out.dtype != torch.int32 or out.device != dev or tuple(out.shape) != (n,) or not out.is_contiguous():
        raise ValueError(f"out: a contiguous int32 [{n}] tensor on {dev}")
    raw = state is not None
    if raw and (not torch.is_tensor(state) or state.dtype != torch.int32 or state.device != dev or tuple(state.shape) != (4,)
                or not state.is_contiguous()):
        raise ValueError(f"state: a contiguous int32 [4] tensor on {dev}")
    cap = 0 if _max_rounds is None else int(_max_rounds)
    if not 0 <= cap <= 63:
        raise ValueError(f"{who}: _max_rounds = {_max_rounds} outside [1, 63]")
    lib = _lib.load()
    need = int(lib.mkgnn_graph_components_workspace_bytes(n))
    if workspace is not None:
        if not torch.is_tensor(workspace) or workspace.dtype != torch.int32 or workspace.device != dev \
                or not workspace.is_contiguous() or 4 * workspace.numel() < need:
            raise ValueError(f"workspace: a contiguous int32 tensor of at least {need} bytes on {dev}")
    elif torch.cuda.is_current_stream_capturing():
        workspace = torch.empty(need // 4, dtype=torch.int32, device=dev)
    else:
        workspace = _COMPONENTS_WS.get(str(dev))
        if workspace is None or 4 * workspace.numel() < need:
            workspace = _COMPONENTS_WS[str(dev)] = torch.empty(max(need // 4, 1 << 14), dtype=torch.int32, device=dev)
    if not raw:
        nnz = int(row_ptr[n])                                    # (the operator takes col's length from row_ptr[n]: checked here)
        if not 0 <= nnz <= col.numel():
            raise ValueError(f"{who}: row_ptr[n] = {nnz} outside [0, {col.numel()}], the length of col")
        state = torch.empty(4, dtype=torch.int32, device=dev)

    def call(resume: int) -> None:
        with torch.cuda.device(dev):
            _lib.check(lib.mkgnn_graph_components(row_ptr.data_ptr(), _lib.ptr(col), n, _lib.ptr(out), state.data_ptr(),
                                                  resume | (cap << 8), workspace.data_ptr(), 4 * workspace.numel(),
                                                  _lib.stream_ptr(dev)), "mkgnn_graph_components")

    call(1 if resume else 0)
    if raw:
        return (out, None) if return_rounds else out
    rounds, converged, skipped, _ = state.tolist()
    while not converged and not skipped:
        call(1)
        more, converged, skipped, _ = state.tolist()
        rounds += more
    if skipped:
        raise ValueError(f"{who}: the lists hold a column outside [0, {n}) or a segment outside 0 <= row_ptr[v] <= row_ptr[v + 1] "
                         "<= row_ptr[n]; they were skipped and the labels are not the components")
    return (out, rounds) if return_rounds else out


def select_rows(scores: torch.Tensor, ids: torch.Tensor, key: torch.Tensor, n_valid, bounds: torch.Tensor, out=None):
    """``(out_scores float32 [B], out_ids int32 [B], n_kept int32 [1])``: the stable compaction ``mkgnn_select_rows`` -- the slots
    ``i < min(max(n_valid, 0), B)`` with ``bounds[0] <= key[i] <= bounds[1]`` (a NaN key is never kept), in order, at the head of the
    outputs, score bits carried over; slots from ``n_kept`` on are not written (``screening.select_rows_reference`` is the
    definition).  ``scores``, ``key`` float32 and ``ids`` int32, contiguous ``[B]`` on the GPU; ``bounds`` a float32 ``[2]`` device
    tensor (lo, hi) and ``n_valid`` a one-element int32 device tensor, both read when the launch runs (an int ``n_valid`` is uploaded
    first), so a captured call follows them.  ``out``: the three tensors to write into, which must not alias the inputs.  What it
    returns is what ``TopK.update(out_scores, out_ids, n_valid=n_kept)`` takes."""
    tensors = (scores, ids, key, bounds)
    if not all(torch.is_tensor(t) for t in tensors) or scores.dtype != torch.float32 or key.dtype != torch.float32 \
            or ids.dtype != torch.int32 or bounds.dtype != torch.float32:
        raise ValueError("select_rows needs float32 scores and key, int32 ids and float32 bounds")
    B = scores.numel()
    if B < 1 or scores.dim() != 1 or tuple(ids.shape) != (B,) or tuple(key.shape) != (B,) or tuple(bounds.shape) != (2,) \
            or not all(t.is_contiguous() for t in tensors):
        raise ValueError("select_rows needs contiguous scores, ids and key of one length B >= 1 and bounds [2]")
    dev = scores.device
    if dev.type != "cuda" or any(t.device != dev for t in tensors):
        raise ValueError(f"select_rows runs on the GPU: scores are on {dev} (there is no CPU path; screening.select_rows_reference "
                         "is the host form)")
    if torch.is_tensor(n_valid):
        if n_valid.dtype != torch.int32 or n_valid.numel() != 1 or n_valid.device != dev:
            raise ValueError("n_valid: one int32 on the scores' device, or an int")
    else:
        n_valid = torch.tensor([int(n_valid)], dtype=torch.int32, device=dev)
    if out is None:
        out = (torch.empty(B, dtype=torch.float32, device=dev), torch.empty(B, dtype=torch.int32, device=dev),
               torch.empty(1, dtype=torch.int32, device=dev))
    else:
        ok = isinstance(out, (tuple, list)) and len(out) == 3 and all(torch.is_tensor(o) and o.device == dev and o.is_contiguous()
                                                                      for o in out)
        if not ok or out[0].dtype != torch.float32 or out[1].dtype != torch.int32 or out[2].dtype != torch.int32 \
                or tuple(out[0].shape) != (B,) or tuple(out[1].shape) != (B,) or out[2].numel() != 1:
            raise ValueError(f"out: contiguous (float32 [{B}], int32 [{B}], int32 [1]) on {dev}")
    with torch.cuda.device(dev):
        _lib.check(_lib.load().mkgnn_select_rows(scores.data_ptr(), ids.data_ptr(), key.data_ptr(), B, n_valid.data_ptr(),
                                                 bounds.data_ptr(), out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(),
                                                 _lib.stream_ptr(dev)), "mkgnn_select_rows")
    return tuple(out)


def embedding_knn_supported(H: int, K: int) -> bool:
    """The shapes ``mkgnn_embed_knn_update`` takes: an embedding of ``1 <= H <= 64`` columns and lists of ``1 <= K <= 64`` slots.  A
    wider embedding goes through torch operators on the GPU; longer lists are ``screening.rank_embeddings``'s."""
    return 1 <= H <= _lib.KNN_MAX_H and 1 <= K <= _lib.KNN_MAX_K


KNN_TORCH_CHUNK = 4096                # rows per step of the torch route: no similarity matrix beyond [4096, Q] exists


def _knn_scalar(value, name: str, dev) -> Optional[torch.Tensor]:
    if value is None:
        return None
    if torch.is_tensor(value):
        if value.dtype != torch.int32 or value.numel() != 1 or value.device != dev:
            raise ValueError(f"{name}: one int32 on the lists' device, or an int")
        return value
    return torch.tensor([int(value)], dtype=torch.int32, device=dev)


def _knn_rank(sim: torch.Tensor, shard: torch.Tensor, mol: torch.Tensor) -> torch.Tensor:
    """The similarity's rank of ``screening.topk_update_reference`` as an int64 key, smaller = earlier: non-NaN descending with
    ``-0.0`` as ``+0.0``, then NaN, then an empty slot ``(-inf, -1, -1)``."""
    bits = sim.view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    b = torch.where(bits == 0x80000000, torch.zeros_like(bits), bits)
    key = torch.where((b & 0x80000000) != 0, b, ~(b | 0x80000000) & 0xFFFFFFFF)
    key = torch.where(torch.isnan(sim), torch.full_like(key, 0xFFFFFFFE), key)
    empty = (bits == 0xFF800000) & (shard == -1) & (mol == -1)
    return torch.where(empty, torch.full_like(key, 0xFFFFFFFF), key)


def _knn_update_torch(emb, queries, top_sim, top_shard, top_mol, ids, n_valid, shard_tag) -> None:
    """``embedding_knn_update`` for an embedding wider than the kernel takes: ``embedding_cosine``'s torch route per chunk of
    ``KNN_TORCH_CHUNK`` rows, then the total order by three stable sorts (id, shard, rank) of ``[old list | chunk]`` per query.  No
    host round trip: a row at or behind ``n_valid`` gets a rank behind the empty slot's and leaves as an empty slot."""
    n, dev = emb.shape[0], emb.device
    Q, K = top_sim.shape
    for a in range(0, n, KNN_TORCH_CHUNK):
        b = min(a + KNN_TORCH_CHUNK, n)
        sim = embedding_cosine(emb[a:b], queries, query_major=True)                       # [Q, c]
        row = torch.arange(a, b, dtype=torch.int32, device=dev)
        mol = (row if ids is None else ids[a:b])[None, :].expand(Q, -1)
        tag = torch.zeros(1, dtype=torch.int32, device=dev) if shard_tag is None else shard_tag.reshape(1)
        shard = tag[None, :].expand(Q, b - a)
        s, h, m = torch.cat([top_sim, sim], 1), torch.cat([top_shard, shard], 1), torch.cat([top_mol, mol], 1)
        rank = _knn_rank(s, h, m)
        if n_valid is not None:
            out = torch.cat([torch.zeros(K, dtype=torch.bool, device=dev), row >= n_valid.reshape(1)])
            rank = torch.where(out[None, :], torch.full_like(rank, 1 << 32), rank)
        order = torch.sort(m, dim=1, stable=True).indices
        order = order.gather(1, torch.sort(h.gather(1, order), dim=1, stable=True).indices)
        order = order.gather(1, torch.sort(rank.gather(1, order), dim=1, stable=True).indices)[:, :K]
        gone = rank.gather(1, order) == (1 << 32)
        top_sim.copy_(torch.where(gone, torch.full_like(top_sim, float("-inf")), s.gather(1, order)))
        top_shard.copy_(torch.where(gone, torch.full_like(top_shard, -1), h.gather(1, order)))
        top_mol.copy_(torch.where(gone, torch.full_like(top_mol, -1), m.gather(1, order)))


def embedding_knn_update(emb: torch.Tensor, queries: torch.Tensor, top_sim: torch.Tensor, top_shard: torch.Tensor,
                         top_mol: torch.Tensor, ids: Optional[torch.Tensor] = None, n_valid=None, shard_tag=None,
                         workspace: Optional[torch.Tensor] = None) -> None:
    """Fused cosine and top-k for any number of queries: the running lists ``top_sim`` float32, ``top_shard`` int32, ``top_mol`` int32
    (``[Q, K]``, contiguous, on the GPU; an empty slot is ``(-inf, -1, -1)``) are updated IN PLACE -- list ``q`` becomes
    ``screening.topk_update_reference`` of itself and the entries ``(sim[i, q], shard_tag, ids[i])`` of the rows ``i < n_valid`` of a
    float32 CUDA ``emb [n, H]``, where ``sim[i, q]`` is what ``embedding_cosine`` gives for row ``i`` and row ``q`` of a float32 CUDA
    ``queries [Q, H]``, BIT FOR BIT.  One ``mkgnn_embed_knn_update``: both inputs are read raw, no ``[n, Q]`` matrix exists, and a
    captured call follows the contents of ``emb``, ``queries``, ``ids`` and the device scalars.  ``ids``: contiguous int32 ``[n]`` on the
    device (None: the row index).  ``n_valid`` / ``shard_tag``: one-element int32 device tensors read when the launch runs, or ints
    (uploaded first), or None (every row; tag 0).  ``workspace``: as in ``embedding_max_cosine``.  The list of a query depends on its
    old list, the candidates, the tag and the query's own values alone: not on ``Q``, the strides or how the launch splits the rows.

    An embedding wider than 64 runs the same definition through torch operators on the GPU, ``KNN_TORCH_CHUNK`` rows at a time
    (``embedding_cosine``'s float64 route: inside ``screening.cosine_bound``, not the kernel's bits).  ``K > 64`` raises: longer lists
    are ``screening.rank_embeddings``'s.  Every check raises ``ValueError`` before a launch.  It has no autograd node: called where a
    gradient is being recorded for one of its inputs it raises instead of dropping it."""
    if not (torch.is_tensor(emb) and torch.is_tensor(queries)) or emb.dim() != 2 or queries.dim() != 2 \
            or emb.dtype != torch.float32 or queries.dtype != torch.float32:
        raise ValueError("embedding_knn_update needs a float32 [n, H] embedding and float32 [Q, H] queries")
    if queries.shape[1] != emb.shape[1]:
        raise ValueError(f"embedding_knn_update: the queries are {int(queries.shape[1])} wide, the embedding is {int(emb.shape[1])} wide")
    (Q, H), n = queries.shape, emb.shape[0]
    if H < 1 or not 1 <= Q <= _lib.KNN_MAX_QUERIES:
        raise ValueError(f"embedding_knn_update needs 1 to {_lib.KNN_MAX_QUERIES} queries (MKGNN_KNN_MAX_QUERIES) and at least one "
                         f"column, not {Q} x {H}")
    lists = (top_sim, top_shard, top_mol)
    if not all(torch.is_tensor(t) and t.dim() == 2 for t in lists) or top_sim.dtype != torch.float32 \
            or top_shard.dtype != torch.int32 or top_mol.dtype != torch.int32:
        raise ValueError("embedding_knn_update: the lists are top_sim float32, top_shard int32, top_mol int32, each [Q, K]")
    K = int(top_sim.shape[1])
    if K > _lib.KNN_MAX_K:
        raise ValueError(f"embedding_knn_update: K = {K} above {_lib.KNN_MAX_K} (MKGNN_KNN_MAX_K: one slot per lane of a wave); longer "
                         "lists are screening.rank_embeddings's, per group of 32 queries")
    if K < 1:
        raise ValueError(f"embedding_knn_update: K = {K} outside [1, {_lib.KNN_MAX_K}] (MKGNN_KNN_MAX_K)")
    if any(tuple(t.shape) != (Q, K) for t in lists):
        raise ValueError(f"embedding_knn_update: the lists are [{Q}, {K}] each, one row per query")
    if not all(t.is_contiguous() for t in lists):
        raise ValueError("embedding_knn_update: the lists are contiguous")
    if n > _lib.KNN_MAX_ROWS:
        raise ValueError(f"embedding_knn_update: {n} rows above {_lib.KNN_MAX_ROWS} (MKGNN_KNN_MAX_ROWS): call per chunk of rows "
                         "(screening.nearest_embeddings does)")
    dev = emb.device
    if not emb.is_cuda or queries.device != dev or any(t.device != dev for t in lists):
        raise ValueError(f"embedding_knn_update runs on the GPU: emb is on {emb.device}, queries on {queries.device}, the lists on "
                         f"{top_sim.device} (there is no CPU path; screening.topk_update_tasks_reference is the host form)")
    if ids is not None and (not torch.is_tensor(ids) or ids.dtype != torch.int32 or ids.device != dev or tuple(ids.shape) != (n,)
                            or not ids.is_contiguous()):
        raise ValueError(f"embedding_knn_update: ids is a contiguous int32 [{n}] tensor on {dev}")
    if torch.is_grad_enabled() and (emb.requires_grad or queries.requires_grad):
        raise RuntimeError("embedding_knn_update is forward only: call it under torch.no_grad() (or on detached inputs)")
    n_valid, shard_tag = _knn_scalar(n_valid, "n_valid", dev), _knn_scalar(shard_tag, "shard_tag", dev)
    if n == 0:
        return
    emb, queries = emb.detach(), queries.detach()
    if not embedding_knn_supported(H, K):
        _knn_update_torch(emb, queries, top_sim, top_shard, top_mol, ids, n_valid, shard_tag)
        return
    emb, queries = _row_major(emb), _row_major(queries)
    lib = _lib.load()
    ws = _max_cosine_workspace(dev, int(lib.mkgnn_embed_knn_workspace_bytes(n, Q, K)), workspace)
    with torch.cuda.device(dev):
        _lib.check(lib.mkgnn_embed_knn_update(emb.data_ptr(), _stride0(emb), n, H, None if ids is None else ids.data_ptr(),
                                              None if n_valid is None else n_valid.data_ptr(),
                                              None if shard_tag is None else shard_tag.data_ptr(), queries.data_ptr(),
                                              _stride0(queries), Q, K, top_sim.data_ptr(), top_shard.data_ptr(), top_mol.data_ptr(),
                                              ws.data_ptr(), ws.numel(), _lib.stream_ptr(dev)), "mkgnn_embed_knn_update")


def diverse_pick_supported(n: int, H: int) -> bool:
    """The shapes ``mkgnn_diverse_pick`` takes; anything else goes through torch operators on the GPU."""
    return 1 <= n <= _lib.DIVERSE_MAX_ROWS and 1 <= H <= _lib.DIVERSE_MAX_H


def _diverse_pick_torch(emb: torch.Tensor, max_sim: float, k: int, picks, n_picks, leader, leader_sim) -> None:
    """The walk of ``screening.diverse_pick_reference`` through torch operators on the GPU, for the shapes the kernel does not take:
    the similarities are ``embedding_cosine(emb, emb[a:a + 32])`` -- group by group of 32 columns, so no ``[n, n]`` matrix exists --
    and every row is one step of dependent masked updates without a host round trip.  Two passes over the groups: the diagonal
    first (a row whose own similarity is NaN must not be covered by an earlier pick), then the walk."""
    n, dev = emb.shape[0], emb.device
    row = torch.arange(n, device=dev)
    slot = torch.arange(k, device=dev)
    diag = torch.empty(n, dtype=torch.float32, device=dev)
    for a in range(0, n, 32):
        b = min(a + 32, n)
        diag[a:b] = embedding_cosine(emb, emb[a:b])[a:b].diagonal()
    alive = ~torch.isnan(diag)
    lead = torch.full((n,), -1, dtype=torch.int64, device=dev)
    lsim = torch.full((n,), float("nan"), dtype=torch.float32, device=dev)
    chosen = torch.full((k,), -1, dtype=torch.int64, device=dev)
    count = torch.zeros((), dtype=torch.int64, device=dev)
    for a in range(0, n, 32):
        b = min(a + 32, n)
        cols = embedding_cosine(emb, emb[a:b])
        for i in range(a, b):
            s = cols[:, i - a]
            pick = alive[i] & (count < k)                        # (0-dim, on the device)
            took = pick & alive & (row >= i) & ((s > max_sim) | (row == i))
            lead = torch.where(took, i, lead)
            lsim = torch.where(took, s, lsim)
            chosen = torch.where(pick & (slot == count), i, chosen)
            alive = alive & ~took
            count = count + pick
    picks.copy_(chosen)
    n_picks.copy_(count.reshape(1))
    leader.copy_(lead)
    leader_sim.copy_(lsim)


_DIVERSE_WS: dict = {}


def diverse_pick(emb: torch.Tensor, max_sim: float, k: Optional[int] = None, out=None):
    """``(picks int32 [k], n_picks int32 [1], leader int32 [n], leader_sim float32 [n])``: leader clustering of the rows of a
    float32 CUDA ``emb [n, H]`` given in RANK ORDER, best first (``mkgnn_diverse_pick``; ``screening.diverse_pick_reference`` is the
    definition).  With ``S[i, p]`` the similarity ``embedding_cosine`` gives for row ``i`` and query row ``p``, BIT FOR BIT: row ``i``
    is covered by the FIRST pick so far with ``S[i, p] > max_sim`` (strict; a NaN never covers) -- ``leader[i] = p``, ``leader_sim[i] =
    S[i, p]`` -- and becomes a pick itself otherwise while fewer than ``k`` exist (``leader[i] = i``); a row whose own similarity
    ``S[i, i]`` is NaN, and a row nothing covers once the list is full, keep ``(-1, NaN)``.  ``picks`` holds the picks' row indices in
    pick order, unused slots ``-1``.  ``k`` defaults to ``n`` (no cap); ``1 <= k <= n``, ``max_sim`` finite.  ``out``: the four
    contiguous tensors to write into.  The launches read ``emb`` raw, so a captured call follows its contents; the scratch is a
    per-device buffer that only grows for eager calls, and a call inside a capture allocates its own.  More than 2^20 rows or an
    embedding wider than 64: the same definition through torch operators on the GPU (``embedding_cosine``'s own route and bits at
    that width, one step of masked updates per row).  It has no autograd node: called where a gradient is being recorded for
    ``emb`` it raises instead of dropping it."""
    if not torch.is_tensor(emb) or emb.dim() != 2 or emb.dtype != torch.float32 or emb.shape[1] < 1:
        raise ValueError("diverse_pick needs a float32 [n, H] embedding in rank order")
    max_sim = float(max_sim)
    if max_sim != max_sim or max_sim in (float("inf"), float("-inf")):
        raise ValueError(f"diverse_pick: max_sim = {max_sim} is not a finite threshold")
    if not emb.is_cuda:
        raise ValueError(f"diverse_pick runs on the GPU: emb is on {emb.device} (there is no CPU path; "
                         "screening.diverse_pick_reference is the host form)")
    if torch.is_grad_enabled() and emb.requires_grad:
        raise RuntimeError("diverse_pick is forward only: call it under torch.no_grad() (or on a detached input)")
    n, H = int(emb.shape[0]), int(emb.shape[1])
    k = n if k is None else int(k)
    if n > 0 and not 1 <= k <= n:
        raise ValueError(f"diverse_pick: k = {k} outside [1, {n}]")
    dev = emb.device
    if out is None:
        out = (torch.empty(k, dtype=torch.int32, device=dev), torch.empty(1, dtype=torch.int32, device=dev),
               torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.float32, device=dev))
    else:
        ok = isinstance(out, (tuple, list)) and len(out) == 4 and all(torch.is_tensor(o) and o.device == dev and o.is_contiguous()
                                                                      for o in out)
        if not ok or any(o.dtype != torch.int32 for o in out[:3]) or out[3].dtype != torch.float32 \
                or tuple(out[0].shape) != (k,) or out[1].numel() != 1 or tuple(out[2].shape) != (n,) or tuple(out[3].shape) != (n,):
            raise ValueError(f"out: contiguous (int32 [{k}], int32 [1], int32 [{n}], float32 [{n}]) on {dev}")
    picks, n_picks, leader, leader_sim = out
    if n == 0:
        n_picks.zero_()
        picks.fill_(-1)
        return tuple(out)
    emb = emb.detach()
    if not diverse_pick_supported(n, H):
        _diverse_pick_torch(emb, max_sim, k, picks, n_picks, leader, leader_sim)
        return tuple(out)
    emb = _row_major(emb)
    lib = _lib.load()
    nbytes = int(lib.mkgnn_diverse_pick_workspace_bytes(n))
    if torch.cuda.is_current_stream_capturing():
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    else:
        ws = _DIVERSE_WS.get(str(dev))
        if ws is None or ws.numel() < nbytes:
            ws = _DIVERSE_WS[str(dev)] = torch.empty(max(nbytes, 1 << 16), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.mkgnn_diverse_pick(emb.data_ptr(), _stride0(emb), n, H, max_sim, k, picks.data_ptr(), n_picks.data_ptr(),
                                          leader.data_ptr(), leader_sim.data_ptr(), ws.data_ptr(), ws.numel(),
                                          _lib.stream_ptr(dev)), "mkgnn_diverse_pick")
    return tuple(out)


def maxmin_pick_supported(n: int, H: int, k: int) -> bool:
    """The shapes ``mkgnn_maxmin_pick`` takes.  A wider embedding goes through torch operators on the GPU; more rows or more picks
    than the kernel's limits are refused by ``maxmin_pick``."""
    return 1 <= n <= _lib.MAXMIN_MAX_ROWS and 1 <= H <= _lib.MAXMIN_MAX_H and 1 <= k <= min(n, _lib.MAXMIN_MAX_PICKS)


def _maxmin_pick_torch(emb: torch.Tensor, k: int, stop_sim: float, start_sim, picks, pick_sim, n_picks, leader, leader_sim) -> None:
    """The rounds of ``screening.maxmin_pick_reference`` through torch operators on the GPU, for the widths the kernel does not
    take: round ``t`` asks ``embedding_cosine(emb, emb[i:i + 1])`` for ONE column -- the similarities of that route at that width, so
    no ``[n, n]`` matrix exists -- with ``i`` kept on the device (no host round trip inside the rounds; after the stop the rounds
    still run and change nothing).  A row is valid when all its values are finite: beyond 64 columns ``embedding_cosine`` forms its
    products in float64, where exactly those rows have a similarity to themselves that is not NaN."""
    n, dev = emb.shape[0], emb.device
    row = torch.arange(n, device=dev)
    nan = torch.full((n,), float("nan"), dtype=torch.float32, device=dev)
    valid = torch.isfinite(emb).all(dim=1)
    cur = torch.full((n,), float("-inf"), dtype=torch.float32, device=dev) if start_sim is None else start_sim.clone()
    candidate = valid & ~torch.isnan(cur)
    cur = torch.where(valid, cur, nan)
    picked = torch.zeros(n, dtype=torch.bool, device=dev)
    lead = torch.full((n,), -1, dtype=torch.int64, device=dev)
    chosen = torch.full((k,), -1, dtype=torch.int64, device=dev)
    taken_at = torch.full((k,), float("nan"), dtype=torch.float32, device=dev)
    done = torch.zeros((), dtype=torch.bool, device=dev)
    count = torch.zeros((), dtype=torch.int64, device=dev)
    for t in range(k):
        key = torch.where(candidate, cur, torch.full_like(cur, float("inf")))
        least = key.min()
        i = torch.where(candidate & (key == least), row, torch.full_like(row, n)).min()     # (the lower row among equals; n: none)
        go = (i < n) & (least < stop_sim) & ~done                # (0-dim, on the device)
        done = done | ~go
        i = i.clamp_max(n - 1)
        col = embedding_cosine(emb, emb.index_select(0, i.reshape(1)))[:, 0]
        it = go & (row == i)
        chosen[t] = torch.where(go, i, chosen[t])
        taken_at[t] = torch.where(go, cur.index_select(0, i.reshape(1))[0], taken_at[t])
        meet = go & valid & ~picked & ~it & ~torch.isnan(col) & (torch.isnan(cur) | (col > cur))
        cur = torch.where(it | meet, col, cur)
        lead = torch.where(it | meet, i, lead)
        picked = picked | it
        candidate = candidate & ~it
        count = count + go
    picks.copy_(chosen)
    pick_sim.copy_(taken_at)
    n_picks.copy_(count.reshape(1))
    leader.copy_(lead)
    leader_sim.copy_(cur)


_MAXMIN_WS: dict = {}


def maxmin_pick(emb: torch.Tensor, k: int, stop_sim: Optional[float] = None, start_sim: Optional[torch.Tensor] = None, out=None):
    """``(picks int32 [k], pick_sim float32 [k], n_picks int32 [1], leader int32 [n], leader_sim float32 [n])``: MaxMin picking --
    the farthest-first traversal, RDKit's ``MaxMinPicker`` -- over the rows of a float32 CUDA ``emb [n, H]`` (``mkgnn_maxmin_pick``;
    ``screening.maxmin_pick_reference`` is the definition).  With ``S[i, p]`` the similarity ``embedding_cosine`` gives for row ``i``
    and query row ``p``, BIT FOR BIT, and ``cur[i]`` the largest similarity of row ``i`` to the selection so far (``start_sim[i]``, or
    ``-inf`` without ``start_sim``, before anything nearer turns up): every round the candidate with the SMALLEST ``cur`` (``-0.0 ==
    +0.0``, then the lower row) becomes the next pick while ``cur < stop_sim`` (strict; ``None``: no stop), at most ``k`` of them, and
    every other valid row meets it -- a strictly larger similarity replaces ``cur`` and the row's leader.  ``picks`` holds the row
    indices in pick order (unused slots ``-1``), ``pick_sim[t]`` how close pick ``t`` was to everything chosen before it (unused
    slots NaN; non-decreasing), ``leader`` / ``leader_sim`` the nearest pick of every row and the similarity to it (a pick leads
    itself).  A row whose own similarity ``S[i, i]`` is NaN is never picked and keeps ``(-1, NaN)``; a row nothing came nearer to
    than its start value keeps ``-1`` and that value.  ``start_sim``: float32 ``[n]`` on the device, every row's similarity to what
    the caller already owns (``embedding_max_cosine``'s first output); a NaN there EXCLUDES the row: never picked, still assigned.
    ``1 <= k <= min(n, 4096)``, ``n <= 2^20``.  ``out``: the five contiguous tensors to write into.  The launches read ``emb`` and
    ``start_sim`` raw, so a captured call follows their contents; the scratch is a per-device buffer that only grows for eager
    calls, and a call inside a capture allocates its own.  An embedding wider than 64: the same definition through torch operators
    on the GPU (``embedding_cosine``'s own route and bits at that width, one column per round).  It has no autograd node: called
    where a gradient is being recorded for ``emb`` or ``start_sim`` it raises instead of dropping it."""
    if not torch.is_tensor(emb) or emb.dim() != 2 or emb.dtype != torch.float32 or emb.shape[1] < 1:
        raise ValueError("maxmin_pick needs a float32 [n, H] embedding")
    n, H = int(emb.shape[0]), int(emb.shape[1])
    k = int(k)
    stop_sim = float("inf") if stop_sim is None else float(stop_sim)
    if stop_sim != stop_sim:
        raise ValueError("maxmin_pick: stop_sim is NaN")
    if n > _lib.MAXMIN_MAX_ROWS:
        raise ValueError(f"maxmin_pick: {n} rows: at most {_lib.MAXMIN_MAX_ROWS} (MKGNN_MAXMIN_MAX_ROWS) in one call")
    if k > _lib.MAXMIN_MAX_PICKS or (n > 0 and not 1 <= k <= n) or k < 0:
        raise ValueError(f"maxmin_pick: k = {k} outside [1, {min(n, _lib.MAXMIN_MAX_PICKS)}] (at most MKGNN_MAXMIN_MAX_PICKS = "
                         f"{_lib.MAXMIN_MAX_PICKS} picks per call, and no more than there are rows)")
    if start_sim is not None and (not torch.is_tensor(start_sim) or start_sim.dtype != torch.float32 or tuple(start_sim.shape) != (n,)):
        raise ValueError(f"maxmin_pick: start_sim is a float32 [{n}] tensor, one value per row of emb")
    if not emb.is_cuda or (start_sim is not None and start_sim.device != emb.device):
        raise ValueError(f"maxmin_pick runs on the GPU: emb is on {emb.device}" +
                         ("" if start_sim is None else f", start_sim on {start_sim.device}") +
                         " (there is no CPU path; screening.maxmin_pick_reference is the host form)")
    if torch.is_grad_enabled() and (emb.requires_grad or (start_sim is not None and start_sim.requires_grad)):
        raise RuntimeError("maxmin_pick is forward only: call it under torch.no_grad() (or on detached inputs)")
    dev = emb.device
    if out is None:
        out = (torch.empty(k, dtype=torch.int32, device=dev), torch.empty(k, dtype=torch.float32, device=dev),
               torch.empty(1, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev),
               torch.empty(n, dtype=torch.float32, device=dev))
    else:
        ok = isinstance(out, (tuple, list)) and len(out) == 5 and all(torch.is_tensor(o) and o.device == dev and o.is_contiguous()
                                                                      for o in out)
        if not ok or any(out[j].dtype != torch.int32 for j in (0, 2, 3)) or any(out[j].dtype != torch.float32 for j in (1, 4)) \
                or tuple(out[0].shape) != (k,) or tuple(out[1].shape) != (k,) or out[2].numel() != 1 \
                or tuple(out[3].shape) != (n,) or tuple(out[4].shape) != (n,):
            raise ValueError(f"out: contiguous (int32 [{k}], float32 [{k}], int32 [1], int32 [{n}], float32 [{n}]) on {dev}")
    picks, pick_sim, n_picks, leader, leader_sim = out
    if n == 0:
        n_picks.zero_()
        picks.fill_(-1)
        pick_sim.fill_(float("nan"))
        return tuple(out)
    emb = emb.detach()
    if start_sim is not None:
        start_sim = start_sim.detach().contiguous()
    if not maxmin_pick_supported(n, H, k):
        _maxmin_pick_torch(emb, k, stop_sim, start_sim, picks, pick_sim, n_picks, leader, leader_sim)
        return tuple(out)
    emb = _row_major(emb)
    lib = _lib.load()
    nbytes = int(lib.mkgnn_maxmin_pick_workspace_bytes(n))
    if torch.cuda.is_current_stream_capturing():
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    else:
        ws = _MAXMIN_WS.get(str(dev))
        if ws is None or ws.numel() < nbytes:
            ws = _MAXMIN_WS[str(dev)] = torch.empty(max(nbytes, 1 << 16), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.mkgnn_maxmin_pick(emb.data_ptr(), _stride0(emb), n, H, None if start_sim is None else start_sim.data_ptr(),
                                         stop_sim, k, picks.data_ptr(), pick_sim.data_ptr(), n_picks.data_ptr(), leader.data_ptr(),
                                         leader_sim.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_ptr(dev)),
                   "mkgnn_maxmin_pick")
    return tuple(out)


# ------------------------------------------------------------------- the tail of a training step, fused --
# MKGNN_FUSED_TAIL=0: readout_blocks + bce_head_loss as separate operators (nine launches; A/B, diagnostics)
_FUSED_TAIL = os.environ.get("MKGNN_FUSED_TAIL", "1") != "0"
_TAIL_WS: dict = {}


def _tail_workspace(dev, nbytes: int) -> torch.Tensor:
    """Per-device scratch of the fused tail (z and d z rows, gradient slabs); never released (a captured graph has its address
    baked in)."""
    held = _TAIL_WS.setdefault(str(dev), [])
    if not held or held[-1].numel() < nbytes:
        held.append(torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8, device=dev))
    return held[-1]


def _tail_limits_ok(seg: "MoleculeSegments", plan) -> bool:
    """No molecule beyond a chunk of the fused tail (``MKGNN_TAIL_MAX_ATOMS`` atoms, ``MKGNN_TAIL_MAX_EDGES`` edges each way).
    Needs the molecule sizes on the host: one synchronisation the first time a batch is seen, remembered on its segments
    (``max_atoms`` / ``max_edges`` may also be handed over by a loader that knows them).  Inside a capture an unknown
    batch is answered with False: the separate operators take it."""
    ma, me = getattr(seg, "max_atoms", None), getattr(seg, "max_edges", None)
    if ma is None or me is None:
        if getattr(seg, "from_loader", False) or torch.cuda.is_current_stream_capturing():
            return False                                  # (refillable tensors without a loader's bound: never -- eager or captured)
        ptr = seg.mol_ptr.long()
        sizes = ptr[1:] - ptr[:-1]
        rin, rout = plan.csr_in[0].long(), plan.csr_out[0].long()
        ein, eout = rin[ptr[1:]] - rin[ptr[:-1]], rout[ptr[1:]] - rout[ptr[:-1]]
        ma, me = int(sizes.max().item()), int(torch.maximum(ein.max(), eout.max()).item())
        seg.max_atoms, seg.max_edges = ma, me
    return ma <= _lib.TAIL_MAX_ATOMS and me <= _lib.TAIL_MAX_EDGES


def tail_supported(K: int, H: int, G: int, blocks) -> bool:
    return bool(_lib.load().mkgnn_tail_supported(int(K), int(H), int(G), _lib.Int32x4(*[int(b) for b in blocks])))


# Round 6: inside ``deferred_tail_reduce()`` the fused tail leaves its last launch -- the fixed-order reduction that writes the loss
# and the six parameter gradients, which nothing before the optimiser reads -- to the kernel convolution's backward, which makes it
# on its helper stream in front of the bank kernel (``mkgnn_tail_args.defer_reduce``): 10 us off the chain the next layer's
# gradient waits for.  Only ``train.training_step`` / ``train.CapturedSteps`` / bench.py open such a region, around
# ``loss -> backward`` as ONE unit, and flush at its end; ``model.loss`` anywhere else returns a finished loss as before.
_DEFER_TAIL_REDUCE = False
_TAIL_PROJECT_NEXT = False   # the next _TailFn.forward may also leave its d sim projection to the last convolution's backward (tail_loss)
_TAIL_HELD: list = []        # every tensor a pending reduction still reads or writes: referenced until the flush (the reduction runs on
                             # another stream, later than the allocator's stream-ordered reuse of a freed block would allow)


def tail_flush(device) -> None:
    """``mkgnn_tail_flush``: what the fused tail left pending on this device -- a deferred projection, then the deferred reduction
    -- is launched on the current stream now."""
    try:
        with torch.cuda.device(device):
            _lib.check(_lib.load().mkgnn_tail_flush(_lib.stream_ptr(device)), "mkgnn_tail_flush")
    finally:
        _TAIL_HELD.clear()           # (launched, here or by the backward's helper stream which the caller's stream has joined)


class deferred_tail_reduce:
    """``with deferred_tail_reduce(device): loss = model.loss(batch); backward(loss)`` -- see ``_DEFER_TAIL_REDUCE``.  Leaving the
    block launches whatever is still pending, on the current stream: behind it the loss and every gradient are complete in
    stream order, exactly as without the block.  Inside it the loss tensor must not be read."""

    def __init__(self, device):
        self.device = device

    def __enter__(self):
        global _DEFER_TAIL_REDUCE
        self.prev, _DEFER_TAIL_REDUCE = _DEFER_TAIL_REDUCE, _TAIL_DEFER_ENABLED
        return self

    def __exit__(self, *exc):
        global _DEFER_TAIL_REDUCE
        _DEFER_TAIL_REDUCE = self.prev
        if not self.prev and self.device is not None and torch.device(self.device).type == "cuda":
            tail_flush(self.device)
        return False


_TAIL_DEFER_ENABLED = os.environ.get("MKGNN_TAIL_DEFER", "1") != "0"


def _tail_grads_adopted(params) -> bool:
    """Nothing reads a deferred tail gradient before the reduction has written it: no parameter has a tensor hook
    (``register_hook``) or a post-accumulate hook (``register_post_accumulate_grad_hook``), and every one is contiguous, so
    AccumulateGrad adopts the gradient tensor as ``.grad`` instead of copying it into the parameter's strides.  (A hook on the
    AccumulateGrad node itself is not visible from here: see ``train.training_step``.)"""
    return all(p is None or (not p._backward_hooks and not getattr(p, "_post_accumulate_grad_hooks", None) and p.is_contiguous())
               for p in params)


def _tail_args(sim, plan, blocks, seg, n_rows, w1c, b1, w2c, b2, whc, bh):
    """The ``mkgnn_tail_args`` fields the training tail and the scoring tail both set, and what they point at beyond the
    arguments (to be kept alive across the call).  Everything not set here stays NULL / 0: a call ignores what it does not need."""
    a = _lib.TailArgs()
    a.sim, a.sim_stride = sim.data_ptr(), _stride0(sim)
    for i, L in enumerate(blocks):
        a.num_kernels[i] = int(L)
    bk = _sel_buckets(plan)
    a.buckets = ctypes.cast(bk, ctypes.c_void_p)
    rin, cin = plan.csr_in
    a.in_rowptr, a.in_col = rin.data_ptr(), cin.data_ptr()
    a.mol_ptr, a.atom_mol = seg.mol_ptr.data_ptr(), seg.atom_mol.data_ptr()
    a.n_atoms, a.n_mols, a.n_loss_mols = sim.shape[0], seg.size, n_rows
    a.readout = _params(w1c, b1, w2c, b2)
    a.head_weight, a.head_bias = whc.data_ptr(), _lib.ptr(bh)
    return a, (bk,)


class _TailFn(torch.autograd.Function):
    """``BCEWithLogitsLoss()(ffn(dropout(readout(propagate(sim)))), y)`` with every gradient for d loss = 1 in the same launch
    (``mkgnn_tail_fused``); the backward hands them out (scaled, if the incoming gradient is not the registered unit seed)."""

    @staticmethod
    def forward(ctx, sim, w1, b1, w2, b2, wh, bh, target, seg, plan, blocks, p_drop, n_rows, kind=_lib.LOSS_BCE_MEAN, p_readout=0.0):
        return _TailFn._run(ctx, sim, w1, b1, w2, b2, wh, bh, target, seg, plan, blocks, p_drop, n_rows, kind, p_readout, None)

    @staticmethod
    def _run(ctx, sim, w1, b1, w2, b2, wh, bh, target, seg, plan, blocks, p_drop, n_rows, kind, p_readout, weights, labels=None):
        """The forward of ``_TailFn`` (``weights`` None) and of ``_WeightedTailFn`` (``weights``: (sw, wids, pw), float32 / int32
        contiguous device tensors or None each -- ``mkgnn_tail_fused_weighted``); ``labels``: ``_TailLabelsFn``'s (label matrix,
        task vector, row ids) -- ``mkgnn_tail_fused_labels``, a ``T``-output ``wh [T, G]`` with ``pred [n_rows, T]``."""
        global _TAIL_PROJECT_NEXT
        project, _TAIL_PROJECT_NEXT = _TAIL_PROJECT_NEXT, False         # (tail_loss's one-shot: see there)
        lib = _lib.load()
        _lib.require_gpu_tensor(sim, "sim_sc")
        n, K = sim.shape
        dev = sim.device
        w1c, w2c = w1.contiguous(), w2.contiguous()
        H, G = w1c.shape[0], w2c.shape[0]
        whc = wh.reshape(-1).contiguous()
        y = target.reshape(-1).float().contiguous() if target is not None else None
        B = int(n_rows)
        pred = torch.empty(B if labels is None else (B, wh.shape[0]), dtype=torch.float32, device=dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        K4 = K + (-K) % 4
        gsim = torch.empty((n, K4), dtype=torch.float32, device=dev)[:, :K]     # block rows: only every atom's own block is written
        gw1, gw2, gwh = torch.empty_like(w1c), torch.empty_like(w2c), torch.empty_like(whc)
        gb1 = torch.empty_like(b1) if b1 is not None else None
        gb2 = torch.empty_like(b2) if b2 is not None else None
        gbh = torch.empty(1 if labels is None else wh.shape[0], dtype=torch.float32, device=dev) if bh is not None else None
        # (one generator state for the head's dropout and the readout's: read once, advanced by one -- mkgnn_readout_dropout_mask
        # gives the readout's mask for the pair left in ctx.rng_used)
        drop = p_drop > 0.0 or p_readout > 0.0
        rng = head_rng_state(dev) if drop else None
        used = torch.empty(2, dtype=torch.int64, device=dev) if drop else None
        a, keep = _tail_args(sim, plan, blocks, seg, B, w1c, b1, w2c, b2, whc, bh)
        rout, cout = plan.csr_out
        a.out_rowptr, a.out_col = rout.data_ptr(), cout.data_ptr()
        a.target = _lib.ptr(y)
        a.dropout_p, a.rng_state, a.rng_used = float(p_drop), _lib.ptr(rng), _lib.ptr(used)
        a.pred, a.loss = pred.data_ptr(), loss.data_ptr()
        a.grad_sim, a.grad_sim_stride = gsim.data_ptr(), K4
        a.grad_lin1_weight, a.grad_lin1_bias = gw1.data_ptr(), _lib.ptr(gb1)
        a.grad_lin2_weight, a.grad_lin2_bias = gw2.data_ptr(), _lib.ptr(gb2)
        a.grad_head_weight, a.grad_head_bias = gwh.data_ptr(), _lib.ptr(gbh)
        # (deferred only where a backward will follow in the same region: the caller of deferred_tail_reduce promises it -- and only
        # where autograd hands the six gradients straight to .grad: see _tail_grads_adopted)
        ctx.deferred = bool(_DEFER_TAIL_REDUCE and ctx.needs_input_grad[0] and _tail_grads_adopted((w1, b1, w2, b2, wh, bh)))
        a.defer_reduce = 1 if ctx.deferred else 0
        a.loss_kind = int(kind)
        ctx.params = (w1, b1, w2, b2, wh, bh)
        ctx.dev = dev
        with torch.cuda.device(dev):
            if labels is None:
                ws = _tail_workspace(dev, int(lib.mkgnn_tail_workspace_bytes(K, H, G, n, seg.size)))
            else:
                ws = _tail_workspace(dev, int(lib.mkgnn_tail_labels_workspace_bytes(K, H, G, n, seg.size, wh.shape[0])))
            if ctx.deferred and project:
                # the projection d sim = d z . W1[:, block] too (one-shot; MKGNN_TAIL_PROJECT_IN_PREPASS=0: ignored): the last
                # convolution's backward, gsim's only reader, forms it in its coefficient pre-pass and gsim is never written --
                # anything else that comes first (tail_flush, tail_score, another loss) makes the launch that was left out
                _lib.check(lib.mkgnn_tail_defer_projection(1), "mkgnn_tail_defer_projection")
            if labels is not None:
                mat, task, ids = labels
                tl, T = _lib.TailLabels(), wh.shape[0]
                tl.n_tasks, tl.row_ids, tl.pred, tl.pred_stride = T, _lib.ptr(ids), pred.data_ptr(), T
                if mat is not None:
                    tl.labels, tl.label_stride, tl.n_label_rows = mat.data_ptr(), T, mat.numel() // T
                else:
                    tl.task, tl.n_task = task.data_ptr(), task.numel()
                lw = _loss_weights(*weights)
                _lib.check(lib.mkgnn_tail_fused_labels(ctypes.byref(a), float(p_readout), ctypes.byref(tl), ctypes.byref(lw),
                                                       ws.data_ptr(), ws.numel(), _lib.stream_ptr(dev)), "mkgnn_tail_fused_labels")
            elif weights is not None:
                lw = _loss_weights(*weights)
                _lib.check(lib.mkgnn_tail_fused_weighted(ctypes.byref(a), float(p_readout), ctypes.byref(lw), ws.data_ptr(),
                                                         ws.numel(), _lib.stream_ptr(dev)), "mkgnn_tail_fused_weighted")
            elif p_readout > 0.0:
                _lib.check(lib.mkgnn_tail_fused_readout_dropout(ctypes.byref(a), float(p_readout), ws.data_ptr(), ws.numel(),
                                                                _lib.stream_ptr(dev)), "mkgnn_tail_fused_readout_dropout")
            else:
                _lib.check(lib.mkgnn_tail_fused(ctypes.byref(a), ws.data_ptr(), ws.numel(), _lib.stream_ptr(dev)), "mkgnn_tail_fused")
        del keep
        if ctx.deferred:
            # (their STORAGES: a second reference to a gradient TENSOR would make autograd copy it into .grad instead of adopting
            # it -- a copy made before the reduction has written it)
            # (the pending projection: its late dW1 launch on the helper stream reads d z -- the workspace --, sim and W1, a
            # materialising one writes gsim; sim is the convolution node's, W1 a parameter -- held all the same)
            _TAIL_HELD.extend(t.untyped_storage() for t in (loss, gw1, gb1, gw2, gb2, gwh, gbh, rng, used, ws, gsim, sim, w1c)
                              if t is not None)
        ctx.unit = (gsim, gw1, gb1, gw2, gb2, gwh.reshape(wh.shape), gbh)
        ctx.pred, ctx.rng_used = pred, used
        return loss

    @staticmethod
    def backward(ctx, grad_loss):
        if ctx.unit is None:
            raise RuntimeError("the fused tail keeps its gradients for ONE backward (retain_graph is not supported: "
                               "MKGNN_FUSED_TAIL=0 runs the separate operators)")
        grads, ctx.unit = ctx.unit, None
        params, ctx.params = ctx.params, None
        # a deferred reduction has not written the parameter gradients yet: fine as long as nothing on this stream touches them
        # before the region's flush -- a scale by the incoming gradient or an accumulation into an existing .grad would
        # (the flush also materialises a pending projection: gsim is written before it is scaled or handed to anyone but the
        # last convolution's backward, which takes the projection over itself)
        if ctx.deferred and (not _is_unit_seed(grad_loss) or torch.is_grad_enabled()
                             or any(p is not None and p.grad is not None for p in params)):
            tail_flush(ctx.dev)
        if not _is_unit_seed(grad_loss):                     # d loss is not the registered 1: scale
            gl = grad_loss.reshape(()).float()
            grads = tuple(None if g is None else g * gl for g in grads)
        return (*grads, None, None, None, None, None, None, None, None)


class _WeightedTailFn(_TailFn):
    """``_TailFn`` with the weighted loss (``mkgnn_tail_fused_weighted``): a sample weight per molecule (``sw``, read directly or
    through ``wids``) and one positive weight (``pw [1]``).  Same deferral, hook and contiguity rules, same single backward."""

    @staticmethod
    def forward(ctx, sim, w1, b1, w2, b2, wh, bh, target, seg, plan, blocks, p_drop, n_rows, kind, p_readout, sw, wids, pw):
        weights = (_f32(sw), _i32(wids), _f32(pw))
        ctx.weights = weights                  # (a deferred launch order does not read them: the middle kernel has run)
        return _TailFn._run(ctx, sim, w1, b1, w2, b2, wh, bh, target, seg, plan, blocks, p_drop, n_rows, kind, p_readout, weights)

    @staticmethod
    def backward(ctx, grad_loss):
        return (*_TailFn.backward(ctx, grad_loss), None, None, None)


class _TailLabelsFn(_TailFn):
    """``_TailFn`` for a ``T``-output head (``mkgnn_tail_fused_labels``): a label matrix with holes (``mat [rows, T]``, NaN: not
    measured) or a task per molecule (``task``, its label in ``target``), either read directly or through ``ids``; sample weights
    and ``pw [T]`` as ``_WeightedTailFn``'s.  Same deferral, hook and contiguity rules, same single backward; ``ctx.pred`` is
    ``[n_rows, T]``."""

    @staticmethod
    def forward(ctx, sim, w1, b1, w2, b2, wh, bh, target, seg, plan, blocks, p_drop, n_rows, kind, p_readout, mat, task, ids, sw, wids, pw):
        weights = (_f32(sw), _i32(wids), _f32(pw))
        labels = (_f32(mat), _i32(task), _i32(ids))
        ctx.weights, ctx.labels = weights, labels           # (held for the launches in flight; a deferred launch order reads neither)
        return _TailFn._run(ctx, sim, w1, b1, w2, b2, wh, bh, target, seg, plan, blocks, p_drop, n_rows, kind, p_readout, weights, labels)

    @staticmethod
    def backward(ctx, grad_loss):
        return (*_TailFn.backward(ctx, grad_loss), None, None, None, None, None, None)


# MKGNN_MULTI_TAIL=1: GNNModel.loss takes the multi-output fused tail for label-matrix and task-indexed batches where
# GNNModel.multi_output_tail is None (the default: off)
_MULTI_TAIL = os.environ.get("MKGNN_MULTI_TAIL", "0") == "1"


def tail_labels_supported(T: int) -> bool:
    """The head widths ``mkgnn_tail_fused_labels`` takes (beside ``tail_supported`` and ``_tail_limits_ok``)."""
    return 1 <= int(T) <= _lib.TASK_HEAD_MAX_TASKS


def tail_labels_loss(sim: torch.Tensor, plan, blocks, lin1: torch.nn.Linear, lin2: torch.nn.Linear, ffn: torch.nn.Linear,
                     seg: "MoleculeSegments", labels: Optional[torch.Tensor] = None, label_table: Optional[torch.Tensor] = None,
                     task: Optional[torch.Tensor] = None, task_table: Optional[torch.Tensor] = None,
                     target: Optional[torch.Tensor] = None, row_ids: Optional[torch.Tensor] = None, loss: str = "bce",
                     dropout_p: float = 0.0, n_rows: Optional[int] = None, readout_dropout_p: float = 0.0,
                     sample_weight: Optional[torch.Tensor] = None, pos_weight: Optional[torch.Tensor] = None,
                     weight_table: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``label_head_loss(readout_blocks(sim, ...), ffn, labels, ...)`` or ``task_head_loss(readout_blocks(sim, ...), ffn, target,
    task, ...)`` -- the two multi-output heads' definitions (``label_head_reference`` / ``task_head_reference``) behind the tail's
    readout -- as ONE operator whose forward also takes every gradient (``_TailLabelsFn``, ``mkgnn_tail_fused_labels``).  Exactly
    one label source: ``labels [>= n_rows, T]`` (float32, NaN: not measured), ``label_table [M, T]`` with ``row_ids``, ``task
    [>= n_rows]`` (int32, -1: none) with ``target``, or ``task_table [M]`` with ``row_ids`` and ``target``.  ``weight_table`` is read
    through the same ``row_ids``.  ``pred [n_rows, T]`` (every entry) stays on the node (``loss.grad_fn.pred``), as ``_TailFn``'s.
    The caller has checked ``tail_supported``, ``tail_labels_supported`` and ``_tail_limits_ok``."""
    who = "tail_labels_loss"
    kind = loss_kind(loss)
    n_rows = seg.size if n_rows is None else int(n_rows)
    T = ffn.out_features
    if sum(t is not None for t in (labels, label_table, task, task_table)) != 1:
        raise ValueError(f"{who} needs exactly one of labels, label_table, task and task_table")
    table = label_table if label_table is not None else task_table
    if table is not None and (row_ids is None or table.shape[0] < 1):
        raise ValueError(f"{who}: a table needs row_ids and at least one row")
    mat = labels if labels is not None else label_table
    if mat is not None and (mat.dim() != 2 or mat.shape[1] != T or not mat.is_floating_point()):
        raise ValueError(f"{who}: the labels must be a float [rows, {T}] matrix for a {T}-output linear layer, not {tuple(mat.shape)}")
    tsk = task if task is not None else task_table
    if tsk is not None and (target is None or target.numel() < n_rows):
        raise ValueError(f"{who}: a task per molecule needs a target per (leading) molecule")
    if not tail_labels_supported(T) or n_rows * T >= 2 ** 31:
        raise ValueError(f"{who}: {T} outputs for {n_rows} molecules outside the multi-output tail")
    _check_loss_weights(loss, T, sample_weight, pos_weight, weight_table, row_ids)
    uses_ids = table is not None or weight_table is not None
    per_mol = [t for t in (labels, task, sample_weight, row_ids if uses_ids else None) if t is not None]
    if n_rows <= 0 or n_rows > seg.size or any(t.shape[0] < n_rows for t in per_mol):
        raise ValueError(f"{who} needs a label row or a task, a weight (or a row id) per (leading) molecule")
    if not 0.0 <= dropout_p < 1.0 or not 0.0 <= readout_dropout_p < 1.0:
        raise ValueError(f"dropout probabilities {dropout_p}, {readout_dropout_p} outside [0, 1)")
    for name, t in (("labels", labels), ("label_table", label_table), ("task", task), ("task_table", task_table),
                    ("target", target if tsk is not None else None), ("row_ids", row_ids if uses_ids else None),
                    ("sample_weight", sample_weight), ("pos_weight", pos_weight), ("weight_table", weight_table)):
        if t is not None:
            _lib.require_gpu_tensor(t, name)
    global _TAIL_PROJECT_NEXT
    _TAIL_PROJECT_NEXT = bool(_DEFER_TAIL_REDUCE and _sole_reader_is_the_convolution(sim))
    try:
        return _TailLabelsFn.apply(sim, lin1.weight, lin1.bias, lin2.weight, lin2.bias, ffn.weight, ffn.bias,
                                   target if tsk is not None else None, seg, plan, tuple(blocks), float(dropout_p), n_rows, kind,
                                   float(readout_dropout_p), mat, tsk, row_ids if table is not None else None,
                                   sample_weight if sample_weight is not None else weight_table,
                                   row_ids if weight_table is not None else None, pos_weight)
    finally:
        _TAIL_PROJECT_NEXT = False


def _sole_reader_is_the_convolution(sim: torch.Tensor) -> bool:
    """``sim`` comes straight out of a kernel convolution (its block rows, not propagated) and nothing is in the way of its
    gradient: no hook on it and no ``retain_grad`` -- the gradient the tail hands back goes to that convolution's backward and
    nowhere else, provided the caller (``MolKGNNNet.forward``) feeds ``sim`` to nothing but the tail."""
    fn = sim.grad_fn
    return (fn is not None and type(fn).__name__ == "_KernelSetConvFnBackward" and not sim._backward_hooks
            and not getattr(sim, "retains_grad", False))


def tail_loss(sim: torch.Tensor, plan, blocks, lin1: torch.nn.Linear, lin2: torch.nn.Linear, ffn: torch.nn.Linear,
              target: torch.Tensor, seg: "MoleculeSegments", dropout_p: float = 0.0, n_rows: Optional[int] = None,
              loss: str = "bce", readout_dropout_p: float = 0.0, sample_weight: Optional[torch.Tensor] = None,
              pos_weight: Optional[torch.Tensor] = None, weight_table: Optional[torch.Tensor] = None,
              row_ids: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``head_loss(readout_blocks(sim, ...), ffn, target, loss, dropout_p, n_rows)`` as ONE operator whose forward also takes
    every gradient (``_TailFn``).  ``readout_dropout_p``: the readout's own dropout (``MolKGNNNet``'s ``drop_ratio`` in training
    mode), its mask drawn in the kernels from ``head_rng_state`` as ``readout_dropout_mask`` gives it.  The caller has checked
    ``tail_supported`` and ``_tail_limits_ok``.  ``sample_weight`` (per molecule; or ``weight_table`` through ``row_ids``) and
    ``pos_weight [1]``: ``head_loss``'s weighted loss, on ``mkgnn_tail_fused_weighted`` (``_WeightedTailFn``)."""
    kind = loss_kind(loss)
    n_rows = seg.size if n_rows is None else int(n_rows)
    weighted = sample_weight is not None or pos_weight is not None or weight_table is not None
    if weighted:
        _check_loss_weights(loss, 1, sample_weight, pos_weight, weight_table, row_ids)
        per_mol = sample_weight if sample_weight is not None else (row_ids if weight_table is not None else None)
        if per_mol is not None and per_mol.numel() < n_rows:
            raise ValueError("tail_loss needs a weight (or a row id) per (leading) molecule")
        for name, t in (("sample_weight", sample_weight), ("pos_weight", pos_weight), ("weight_table", weight_table),
                        ("row_ids", row_ids if weight_table is not None else None)):
            if t is not None:
                _lib.require_gpu_tensor(t, name)
    if ffn.out_features != 1 or n_rows <= 0 or n_rows > seg.size or target.numel() != n_rows:
        raise ValueError("tail_loss needs a one-output linear layer and one target per (leading) molecule")
    if not 0.0 <= readout_dropout_p < 1.0:
        raise ValueError(f"readout dropout probability {readout_dropout_p} outside [0, 1)")
    # (what only this caller can see -- inside the operator `sim` has no history -- goes to the operator's forward beside its arguments)
    global _TAIL_PROJECT_NEXT
    _TAIL_PROJECT_NEXT = bool(_DEFER_TAIL_REDUCE and _sole_reader_is_the_convolution(sim))
    try:
        if weighted:
            return _WeightedTailFn.apply(sim, lin1.weight, lin1.bias, lin2.weight, lin2.bias, ffn.weight, ffn.bias, target, seg,
                                         plan, tuple(blocks), float(dropout_p), n_rows, kind, float(readout_dropout_p),
                                         sample_weight if sample_weight is not None else weight_table,
                                         row_ids if weight_table is not None else None, pos_weight)
        return _TailFn.apply(sim, lin1.weight, lin1.bias, lin2.weight, lin2.bias, ffn.weight, ffn.bias, target, seg, plan,
                             tuple(blocks), float(dropout_p), n_rows, kind, float(readout_dropout_p))
    finally:
        _TAIL_PROJECT_NEXT = False


# MKGNN_SCORE_TAIL=0: GNNModel.predict runs the separate operators (readout_blocks, dropout, head) as before it existed (A/B)
_SCORE_TAIL = os.environ.get("MKGNN_SCORE_TAIL", "1") != "0"


def tail_score(sim: torch.Tensor, plan, blocks, lin1: torch.nn.Linear, lin2: torch.nn.Linear, ffn: torch.nn.Linear,
               seg: "MoleculeSegments", n_rows: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """``(pred [n_rows], emb [seg.size, G])``: ``ffn(readout_blocks(sim, ...))`` in evaluation mode as two launches
    (``mkgnn_tail_score``) -- no dropout, no loss, no gradient, and bit for bit the ``pred`` / ``emb`` of the training tail
    (``tail_loss``) at dropout 0.  ``n_rows``: the leading molecules whose prediction is wanted (a padded batch's real ones).
    It has no autograd node: called where a gradient is being recorded for one of its inputs it raises instead of dropping
    it (``tail_loss`` is the differentiable operator).  The caller has checked ``tail_supported`` and ``_tail_limits_ok``."""
    params = (lin1.weight, lin1.bias, lin2.weight, lin2.bias, ffn.weight, ffn.bias)
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (sim, *params)):
        raise RuntimeError("tail_score is forward only: call it under torch.no_grad() (or on detached inputs); "
                           "tail_loss is the operator with gradients")
    lib = _lib.load()
    _lib.require_gpu_tensor(sim, "sim_sc")
    n_rows = seg.size if n_rows is None else int(n_rows)
    if ffn.out_features != 1 or n_rows <= 0 or n_rows > seg.size:
        raise ValueError("tail_score needs a one-output linear layer and 1 <= n_rows <= the batch's molecules")
    n, K = sim.shape
    dev = sim.device
    w1, b1, w2, b2, wh, bh = (None if t is None else t.detach() for t in params)
    w1c, w2c, whc = w1.contiguous(), w2.contiguous(), wh.reshape(-1).contiguous()
    H, G = w1c.shape[0], w2c.shape[0]
    pred = torch.empty(n_rows, dtype=torch.float32, device=dev)
    emb = torch.empty((seg.size, G), dtype=torch.float32, device=dev)
    a, keep = _tail_args(sim, plan, blocks, seg, n_rows, w1c, b1, w2c, b2, whc, bh)
    a.emb, a.emb_stride = emb.data_ptr(), G
    a.pred = pred.data_ptr()
    with torch.cuda.device(dev):
        # (the training tail's scratch: its first bytes are the z rows there too, and a reduction still pending on its slabs
        # is launched by the call before anything is overwritten)
        ws = _tail_workspace(dev, int(lib.mkgnn_tail_score_workspace_bytes(K, H, G, n, seg.size)))
        _lib.check(lib.mkgnn_tail_score(ctypes.byref(a), ws.data_ptr(), ws.numel(), _lib.stream_ptr(dev)), "mkgnn_tail_score")
    del keep
    return pred, emb


# ---------------------------------------------------------------- Monte Carlo dropout samples on the forward-only tail --
# MKGNN_SCORE_MC=0: GNNModel.predict_mc runs its PyTorch route (h once, S rounds of torch operators, torch's generator; A/B)
_SCORE_MC = os.environ.get("MKGNN_SCORE_MC", "1") != "0"


def mc_statistics_reference(samples, alpha: float = 1.0, beta: float = 0.0):
    """The definition of ``mkgnn_tail_score_mc``'s statistics: ``(mean, std, acq)`` of every row of ``samples [n, S]``, float32
    numpy arrays ``[n]``, in the kernel's own steps -- each ONE float32 round-to-nearest operation, in sample order:
    ``sum = +0; sum = sum + x_s``; ``mean = sum / S``; ``q = +0; d = x_s - mean; q = q + d * d``; ``std = sqrt(q / (S - 1))``
    (unbiased; exactly 0 for ``S = 1``); ``acq = alpha * mean + beta * std`` (two products, one sum).  The kernel's vectors equal
    these bit for bit.  A row holding a NaN gives NaN (its ``std`` too, unless ``S = 1``)."""
    import numpy as np
    x = samples.detach().cpu().numpy() if torch.is_tensor(samples) else np.asarray(samples)
    x = np.ascontiguousarray(x, dtype=np.float32)
    if x.ndim != 2 or x.shape[1] < 1:
        raise ValueError("mc_statistics_reference needs samples [n, S] with S >= 1")
    n, S = x.shape
    f32 = np.float32
    with np.errstate(invalid="ignore", over="ignore"):
        total = np.zeros(n, dtype=f32)
        for s in range(S):
            total = (total + x[:, s]).astype(f32)
        mean = (total / f32(S)).astype(f32)
        q = np.zeros(n, dtype=f32)
        for s in range(S):
            d = (x[:, s] - mean).astype(f32)
            q = (q + (d * d).astype(f32)).astype(f32)
        std = np.sqrt((q / f32(S - 1)).astype(f32)).astype(f32) if S > 1 else np.zeros(n, dtype=f32)
        acq = ((f32(alpha) * mean).astype(f32) + (f32(beta) * std).astype(f32)).astype(f32)
    return mean, std, acq


def _check_mc_samples(n_samples) -> int:
    S = int(n_samples)
    if S != n_samples or not 1 <= S <= _lib.TAIL_MC_MAX_SAMPLES:
        raise ValueError(f"n_samples = {n_samples} outside [1, {_lib.TAIL_MC_MAX_SAMPLES}] (MKGNN_TAIL_MC_MAX_SAMPLES)")
    return S


def tail_score_mc(sim: torch.Tensor, plan, blocks, lin1: torch.nn.Linear, lin2: torch.nn.Linear, ffn: torch.nn.Linear,
                  seg: "MoleculeSegments", n_samples: int, dropout_p: float, readout_dropout_p: float,
                  n_rows: Optional[int] = None, alpha: float = 1.0, beta: float = 0.0, rng_pair: Optional[torch.Tensor] = None,
                  return_samples: bool = False, return_pred: bool = False) -> dict:
    """Monte Carlo dropout behind the last convolution as two launches (``mkgnn_tail_score_mc``): ``n_samples`` stochastic
    predictions of every one of the ``n_rows`` leading molecules -- evaluation-mode inputs, the head's dropout ``dropout_p`` and
    the readout's ``readout_dropout_p`` left on -- reduced to ``mean``, ``std`` (unbiased) and ``acq = alpha * mean + beta * std``,
    ``[n_rows]`` each (``mc_statistics_reference`` is their definition).  Sample ``s`` is bit for bit the ``pred`` of the training
    tail (``tail_loss``) for generator state ``{seed, offset + s}``.  ``return_samples``: also ``samples [n_rows, n_samples]``
    (otherwise no such matrix exists anywhere); ``return_pred``: also ``pred [n_rows]`` and ``emb [seg.size, G]``, ``tail_score``'s
    bits.  ``rng_pair=None``: the pair is ``head_rng_state`` and its offset is advanced by ``n_samples`` behind the call, in place
    on the same stream -- capturable: every replay of a captured call draws fresh masks.  A pair given (int64 ``{seed, offset}``
    on the device) is read and nothing is advanced.  Forward only, as ``tail_score``: where a gradient is being recorded for one
    of its inputs it raises instead of dropping it.  The caller has checked ``tail_supported`` and ``_tail_limits_ok``."""
    params = (lin1.weight, lin1.bias, lin2.weight, lin2.bias, ffn.weight, ffn.bias)
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (sim, *params)):
        raise RuntimeError("tail_score_mc is forward only: call it under torch.no_grad() (or on detached inputs); "
                           "tail_loss is the operator with gradients")
    S = _check_mc_samples(n_samples)
    for name, p in (("dropout", dropout_p), ("readout dropout", readout_dropout_p)):
        if not 0.0 <= p < 1.0:
            raise ValueError(f"{name} probability {p} outside [0, 1)")
    lib = _lib.load()
    _lib.require_gpu_tensor(sim, "sim_sc")
    n_rows = seg.size if n_rows is None else int(n_rows)
    if ffn.out_features != 1 or n_rows <= 0 or n_rows > seg.size:
        raise ValueError("tail_score_mc needs a one-output linear layer and 1 <= n_rows <= the batch's molecules")
    n, K = sim.shape
    dev = sim.device
    advance = rng_pair is None
    if advance:
        rng_pair = head_rng_state(dev)
    elif rng_pair.dtype != torch.int64 or rng_pair.numel() != 2 or not rng_pair.is_contiguous() or rng_pair.device != dev:
        raise ValueError("rng_pair: two contiguous int64 values {seed, offset} on the batch's device")
    w1, b1, w2, b2, wh, bh = (None if t is None else t.detach() for t in params)
    w1c, w2c, whc = w1.contiguous(), w2.contiguous(), wh.reshape(-1).contiguous()
    H, G = w1c.shape[0], w2c.shape[0]
    result = {k: torch.empty(n_rows, dtype=torch.float32, device=dev) for k in ("mean", "std", "acq")}
    a, keep = _tail_args(sim, plan, blocks, seg, n_rows, w1c, b1, w2c, b2, whc, bh)
    a.dropout_p = float(dropout_p)
    if return_pred:
        result["pred"] = torch.empty(n_rows, dtype=torch.float32, device=dev)
        result["emb"] = torch.empty((seg.size, G), dtype=torch.float32, device=dev)
        a.pred, a.emb, a.emb_stride = result["pred"].data_ptr(), result["emb"].data_ptr(), G
    out = _lib.TailMcOut()
    out.mean, out.std, out.acq = (result[k].data_ptr() for k in ("mean", "std", "acq"))
    out.alpha, out.beta = float(alpha), float(beta)
    if return_samples:
        result["samples"] = torch.empty((n_rows, S), dtype=torch.float32, device=dev)
        out.samples, out.samples_stride = result["samples"].data_ptr(), S
    with torch.cuda.device(dev):
        # (the training tail's scratch, as tail_score: a reduction still pending on its slabs is launched by the call first)
        ws = _tail_workspace(dev, int(lib.mkgnn_tail_score_mc_workspace_bytes(K, H, G, n, seg.size)))
        _lib.check(lib.mkgnn_tail_score_mc(ctypes.byref(a), float(readout_dropout_p), S, rng_pair.data_ptr(), ctypes.byref(out),
                                           ws.data_ptr(), ws.numel(), _lib.stream_ptr(dev)), "mkgnn_tail_score_mc")
        if advance:
            rng_pair[1:].add_(S)                             # (behind the kernel on its stream; inside a capture: a graph node)
    del keep
    return result


# ------------------------------------------------------------- every atom's share of every logit (evaluation mode) --
# MKGNN_ATOM_CONTRIB=0: GNNModel.atom_contributions runs the PyTorch operators on a dense h (atom_contributions_torch; A/B)
_ATOM_CONTRIB = os.environ.get("MKGNN_ATOM_CONTRIB", "1") != "0"


def atom_contributions_reference(h, w1, b1, w2, b2, wh):
    """The definition, in float64 on the CPU and in the reference's own order: ``((swish(h W1^T + b1)) W2^T + b2) Wh^T`` --
    ``contrib [N, T]`` (a float64 numpy array), the share of every atom in every logit: a molecule's rows sum to its ``pred``
    minus the head's bias.  ``h [N, K]`` is the last layer's propagated output; tensors or arrays, either bias may be ``None``."""
    import numpy as np

    def f64(a):
        return None if a is None else (a.detach().cpu().double().numpy() if torch.is_tensor(a) else np.asarray(a, dtype=np.float64))

    h, w1, b1, w2, b2, wh = (f64(a) for a in (h, w1, b1, w2, b2, wh))
    wh = wh.reshape(-1, w2.shape[0])
    if h.ndim != 2 or w1.ndim != 2 or w2.ndim != 2 or h.shape[1] != w1.shape[1] or w2.shape[1] != w1.shape[0]:
        raise ValueError("atom_contributions_reference needs h [N, K], W1 [H, K], W2 [G, H] and Wh [T, G]")
    pre = h @ w1.T
    if b1 is not None:
        pre = pre + b1
    with np.errstate(over="ignore"):
        act = pre / (1.0 + np.exp(-pre))
    emb = act @ w2.T
    if b2 is not None:
        emb = emb + b2
    return emb @ wh.T


def atom_contributions_supported(K: int, H: int, G: int, blocks, T: int) -> bool:
    """The shapes ``mkgnn_atom_contributions`` takes: the fused tail's, and ``1 <= T <= 32`` tasks."""
    return 1 <= int(T) <= _lib.ATOM_CONTRIB_MAX_TASKS and tail_supported(K, H, G, blocks)


def atom_contributions(sim: torch.Tensor, plan, blocks, lin1: torch.nn.Linear, lin2: torch.nn.Linear, ffn: torch.nn.Linear,
                       out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``contrib [n_atoms, T]``: the exact share of every atom in every output of ``ffn(readout_blocks(sim, ...))`` in evaluation
    mode -- ``pred[g, t] = ffn.bias[t] + sum of contrib[n, t] over the atoms of g`` -- from the last convolution's block rows as
    two launches (``mkgnn_atom_contributions``; ``atom_contributions_reference`` is the definition).  Needs no molecule segments
    and knows no limit on a molecule's size.  ``out``: a float32 tensor ``[n_atoms, >= T]`` on the device whose leading ``T``
    columns are written (its row stride is passed on; the other columns are not touched) and returned as a view.  It has no
    autograd node: called where a gradient is being recorded for one of its inputs it raises instead of dropping it.  The caller
    has checked ``atom_contributions_supported``."""
    params = (lin1.weight, lin1.bias, lin2.weight, lin2.bias, ffn.weight)
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (sim, *params)):
        raise RuntimeError("atom_contributions is forward only: call it under torch.no_grad() (or on detached inputs)")
    lib = _lib.load()
    _lib.require_gpu_tensor(sim, "sim_sc")
    n, K = sim.shape
    dev = sim.device
    w1, b1, w2, b2, wh = (None if t is None else t.detach() for t in params)
    w1c, w2c = w1.contiguous(), w2.contiguous()
    whc = wh if wh.stride(1) == 1 else wh.contiguous()
    H, G, T = w1c.shape[0], w2c.shape[0], whc.shape[0]
    if whc.dim() != 2 or whc.shape[1] != G or not 1 <= T <= _lib.ATOM_CONTRIB_MAX_TASKS:
        raise ValueError(f"atom_contributions needs a head of 1 to {_lib.ATOM_CONTRIB_MAX_TASKS} outputs on the G = {G} embedding columns")
    if out is None:
        out = torch.empty((n, T), dtype=torch.float32, device=dev)
    elif (out.dtype != torch.float32 or out.device != dev or out.dim() != 2 or out.shape[0] != n or out.shape[1] < T
          or (n > 0 and out.stride(1) != 1)):
        raise ValueError(f"out: a float32 tensor [{n}, >= {T}] of rows on {dev}")
    if n == 0:
        return out[:, :T]
    a = _lib.AtomContribArgs()
    a.sim, a.sim_stride = sim.data_ptr(), _stride0(sim)
    for i, L in enumerate(blocks):
        a.num_kernels[i] = int(L)
    bk = _sel_buckets(plan)
    a.buckets = ctypes.cast(bk, ctypes.c_void_p)
    rin, cin = plan.csr_in
    a.in_rowptr, a.in_col, a.n_atoms = rin.data_ptr(), cin.data_ptr(), n
    a.readout = _params(w1c, b1, w2c, b2)
    a.head_weight, a.head_stride, a.T = whc.data_ptr(), (whc.stride(0) if T > 1 else G), T
    a.contrib, a.contrib_stride = out.data_ptr(), (out.stride(0) if n > 1 else out.shape[1])
    with torch.cuda.device(dev):
        # (the tail's scratch: its first bytes are the z rows there too, and a reduction still pending on its slabs is launched
        # by the call before anything is overwritten)
        ws = _tail_workspace(dev, int(lib.mkgnn_atom_contributions_workspace_bytes(K, H, G, n)))
        _lib.check(lib.mkgnn_atom_contributions(ctypes.byref(a), ws.data_ptr(), ws.numel(), _lib.stream_ptr(dev)),
                   "mkgnn_atom_contributions")
    del bk
    return out[:, :T]


def atom_contributions_torch(h: torch.Tensor, lin1: torch.nn.Linear, lin2: torch.nn.Linear, ffn: torch.nn.Linear) -> torch.Tensor:
    """``contrib [N, T]`` from a dense ``h`` (the last layer's propagated output) with float32 PyTorch operators, in the
    reference's order: ``ffn.weight`` applied to ``lin2(swish(lin1(h)))``, without the head's bias.  The route for shapes outside
    ``atom_contributions_supported`` and for ``MKGNN_ATOM_CONTRIB=0``; the readout's dropout is not applied (evaluation mode)."""
    return torch.nn.functional.linear(lin2(swish(lin1(h))), ffn.weight)


def readout_dropout_mask(rng_pair: torch.Tensor, n_rows: int, H: int, p: float, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The keep multipliers ``[n_rows, H]`` (0, or 1 / (1 - p)) of the readout's dropout that the fused tail and the
    molecule-resident step draw for the generator pair ``rng_pair`` (``{seed, offset}``, int64 on the device -- the ``rng_used``
    of a call, or ``head_rng_state`` before it): row r is the batch's atom r (``mkgnn_readout_dropout_mask``).  Fed to
    ``_ReadoutFn`` / ``_ReadoutBlocksFn`` as ``keep``, the separate operators apply the fused paths' mask."""
    if not 0.0 <= p < 1.0:
        raise ValueError(f"readout dropout probability {p} outside [0, 1)")
    _lib.require_gpu_tensor(rng_pair, "rng_pair")
    if rng_pair.dtype != torch.int64 or rng_pair.numel() != 2 or not rng_pair.is_contiguous():
        raise ValueError("rng_pair: two contiguous int64 values {seed, offset}")
    dev = rng_pair.device
    if out is None:
        out = torch.empty((int(n_rows), int(H)), dtype=torch.float32, device=dev)
    if out.shape != (n_rows, H) or out.dtype != torch.float32 or out.stride(1) != 1 or out.device != dev:
        raise ValueError("out: [n_rows, H] float32 rows on the generator's device")
    lib = _lib.load()
    with torch.cuda.device(dev):
        _lib.check(lib.mkgnn_readout_dropout_mask(rng_pair.data_ptr(), int(n_rows), int(H), float(p), out.data_ptr(),
                                                  _stride0(out) if n_rows > 0 else int(H), _lib.stream_ptr(dev)),
                   "mkgnn_readout_dropout_mask")
    return out


def bootstrap_roc_replicates_per_pass(n: int, n_boot: int) -> int:
    """The replicates ``bootstrap_roc`` keeps in flight when it sizes its own scratch: all ``n_boot`` where their multiplicities fit
    under ``_lib.BOOTSTRAP_WORKSPACE_CAP`` bytes (``4 * ceil4(n)`` each), otherwise as many as do, at least one."""
    per = 4 * ((int(n) + 3) // 4 * 4)
    return max(1, min(int(n_boot), _lib.BOOTSTRAP_WORKSPACE_CAP // per))


def _bootstrap_checked(who: str, rank, y_sorted, group_last, split, n_boot, seed, offset, lower, upper):
    """The checks ``bootstrap_roc`` and ``bootstrap_early`` share: ``(n, split, B, seed, offset, lower, upper)`` as Python numbers."""
    if not all(torch.is_tensor(x) and x.dim() == 1 for x in (rank, y_sorted, group_last)) or rank.dtype != torch.int32 \
            or y_sorted.dtype != torch.uint8 or group_last.dtype != torch.uint8 \
            or not (rank.numel() == y_sorted.numel() == group_last.numel()):
        raise ValueError(f"{who} needs rank int32 [n], y_sorted uint8 [n] and group_last uint8 [n]")
    if not rank.is_cuda or y_sorted.device != rank.device or group_last.device != rank.device:
        raise ValueError(f"{who} runs on the GPU: rank is on {rank.device}, y_sorted on {y_sorted.device}, group_last on "
                         f"{group_last.device} (there is no CPU path; evaluation.bootstrap_reference is the host form)")
    if torch.is_grad_enabled() and any(x.requires_grad for x in (rank, y_sorted, group_last)):
        raise RuntimeError(f"{who} is forward only: call it under torch.no_grad() (or on detached inputs)")
    n, split, B = rank.numel(), int(split), int(n_boot)
    if not 1 <= n <= _lib.BOOTSTRAP_MAX_ROWS:
        raise ValueError(f"{who}: {n} rows outside [1, {_lib.BOOTSTRAP_MAX_ROWS}]")
    if not 1 <= B <= _lib.BOOTSTRAP_MAX_REPLICATES:
        raise ValueError(f"{who}: n_boot = {n_boot} outside [1, {_lib.BOOTSTRAP_MAX_REPLICATES}] per call")
    if not 0 <= split <= n:
        raise ValueError(f"{who}: split = {split} outside [0, {n}]")
    lower, upper = float(lower), float(upper)
    if not (0.0 < lower < upper <= 1.0):
        raise ValueError(f"{who}: FPR window ({lower}, {upper}): 0 < lower < upper <= 1 is required")
    seed, offset = int(seed), int(offset)
    if not (0 <= seed < 1 << 64 and 0 <= offset and offset + B <= 1 << 64):
        raise ValueError(f"{who}: seed and offset .. offset + n_boot - 1 are unsigned 64-bit values")
    if not (rank.is_contiguous() and y_sorted.is_contiguous() and group_last.is_contiguous()):
        raise ValueError(f"{who} needs contiguous tensors")
    return n, split, B, seed, offset, lower, upper


def _bootstrap_scratch(lib, dev, n: int, B: int, workspace):
    """``(pointer, bytes)`` of the scratch of a bootstrap call: none up to ``_lib.BOOTSTRAP_LDS_MAX_N`` rows."""
    if n <= _lib.BOOTSTRAP_LDS_MAX_N:
        return None, 0
    want = workspace.numel() if workspace is not None else \
        int(lib.mkgnn_bootstrap_roc_workspace_bytes(n, bootstrap_roc_replicates_per_pass(n, B)))
    if workspace is not None and want < int(lib.mkgnn_bootstrap_roc_workspace_bytes(n, 1)):
        raise ValueError(f"workspace: at least {int(lib.mkgnn_bootstrap_roc_workspace_bytes(n, 1))} bytes (one replicate)")
    ws = _max_cosine_workspace(dev, want, workspace)
    return ws.data_ptr(), ws.numel()


def bootstrap_roc(rank: torch.Tensor, y_sorted: torch.Tensor, group_last: torch.Tensor, split: int, n_boot: int, seed: int,
                  offset: int, lower: float, upper: float, workspace: Optional[torch.Tensor] = None):
    """``(auc float64 [n_boot], logauc float64 [n_boot], two_u int64 [n_boot], n_pos int32 [n_boot])``: ``n_boot`` bootstrap replicates
    of the ROC curve of ``n`` rows whose scores were sorted ONCE (descending, stable) -- ``rank int32 [n]`` the rank of row ``i`` of the
    caller's or class-major order, ``y_sorted uint8 [n]`` the labels by rank, ``group_last uint8 [n]`` 1 where a rank ends its tie
    group, all contiguous CUDA tensors.  Replicate ``b`` draws with ``philox_word(seed, offset + b, i)``; ``split`` rows in front form
    one stratum, the rest another (``split = n``: unstratified).  ``evaluation.bootstrap_reference`` is the definition: ``two_u``,
    ``n_pos`` and ``auc`` agree with it exactly, ``logauc`` within the rounding of a float64 sum; a replicate with one class only has
    NaN in both.  One ``mkgnn_bootstrap_roc``: no sort, no host round trip, capturable; a replicate's outputs do not depend on
    ``n_boot``, on where the replicates start or on the scratch's size.  ``workspace``: a uint8 device tensor to use as scratch, at
    least ``mkgnn_bootstrap_roc_workspace_bytes(n, 1)`` bytes -- the call passes over the replicates as many at a time as it holds;
    without it a per-device buffer that only grows serves eager calls (sized for ``bootstrap_roc_replicates_per_pass``), and a call
    inside a capture allocates its own.  Up to ``_lib.BOOTSTRAP_LDS_MAX_N`` rows no scratch is used.  It has no autograd node: called
    where a gradient is being recorded for one of its inputs it raises."""
    n, split, B, seed, offset, lower, upper = _bootstrap_checked("bootstrap_roc", rank, y_sorted, group_last, split, n_boot, seed, offset,
                                                                 lower, upper)
    dev = rank.device
    auc = torch.empty(B, dtype=torch.float64, device=dev)
    logauc = torch.empty(B, dtype=torch.float64, device=dev)
    two_u = torch.empty(B, dtype=torch.int64, device=dev)
    n_pos = torch.empty(B, dtype=torch.int32, device=dev)
    lib = _lib.load()
    ws_ptr, ws_bytes = _bootstrap_scratch(lib, dev, n, B, workspace)
    with torch.cuda.device(dev):
        _lib.check(lib.mkgnn_bootstrap_roc(rank.data_ptr(), y_sorted.data_ptr(), group_last.data_ptr(), n, split, B, seed, offset,
                                           lower, upper, auc.data_ptr(), logauc.data_ptr(), two_u.data_ptr(), n_pos.data_ptr(),
                                           ws_ptr, ws_bytes, _lib.stream_ptr(dev)), "mkgnn_bootstrap_roc")
    return auc, logauc, two_u, n_pos


def _early_vector(who: str, what: str, values, dtype, limit: int, dev) -> torch.Tensor:
    """``cuts`` / ``alphas`` of ``bootstrap_early`` as a contiguous device vector: a tensor is taken as it is (no host read: a
    captured call re-reads it), a sequence is copied over."""
    if torch.is_tensor(values):
        if values.dim() != 1 or values.dtype != dtype or values.device != dev or not values.is_contiguous():
            raise ValueError(f"{who}: {what} as a tensor is a contiguous {dtype} vector on {dev}")
        v = values
    else:
        v = torch.tensor(list(values), dtype=dtype).reshape(-1).to(dev)
    if v.numel() > limit:
        raise ValueError(f"{who}: {v.numel()} {what}, at most {limit}")
    return v


def bootstrap_early(rank: torch.Tensor, y_sorted: torch.Tensor, group_last: torch.Tensor, split: int, n_boot: int, seed: int,
                    offset: int, lower: float, upper: float, cuts, alphas, workspace: Optional[torch.Tensor] = None):
    """``bootstrap_roc`` with the early-recognition sums of the same replicates, from the same walk behind the same draw (one
    ``mkgnn_bootstrap_early``): ``(auc, logauc, two_u, n_pos, ap float64 [n_boot], hits float64 [n_boot, J], rie float64 [n_boot,
    A])``.  ``cuts``: up to ``_lib.BOOTSTRAP_MAX_CUTS`` integers ``1 <= k <= n`` (an int32 device tensor, or a sequence) --
    ``hits[b, j]`` is the expected number of actives among the first ``cuts[j]`` drawn rows, a tie group's rows in random order;
    ``alphas``: up to ``_lib.BOOTSTRAP_MAX_ALPHAS`` values in ``(0, 500]`` (a float64 device tensor, or a sequence) -- ``rie[b, a]``
    is the sum over the drawn actives of ``exp(-alpha r / n)``; ``ap`` is the weighted average precision.  ``evaluation.
    early_reference_sorted`` is the definition (``hits`` agrees bit for bit, ``ap`` and ``rie`` within the rounding of a float64 sum)
    and ``evaluation.early_derived`` turns the sums into AP, EF and BEDROC.  The first four outputs are ``bootstrap_roc``'s bit for
    bit.  A cut or an alpha outside its range gives a NaN column and changes nothing else.  Checks, scratch and capture: as
    ``bootstrap_roc``."""
    who = "bootstrap_early"
    n, split, B, seed, offset, lower, upper = _bootstrap_checked(who, rank, y_sorted, group_last, split, n_boot, seed, offset, lower, upper)
    dev = rank.device
    cuts = _early_vector(who, "cuts", cuts, torch.int32, _lib.BOOTSTRAP_MAX_CUTS, dev)
    alphas = _early_vector(who, "alphas", alphas, torch.float64, _lib.BOOTSTRAP_MAX_ALPHAS, dev)
    J, A = cuts.numel(), alphas.numel()
    auc = torch.empty(B, dtype=torch.float64, device=dev)
    logauc = torch.empty(B, dtype=torch.float64, device=dev)
    two_u = torch.empty(B, dtype=torch.int64, device=dev)
    n_pos = torch.empty(B, dtype=torch.int32, device=dev)
    ap = torch.empty(B, dtype=torch.float64, device=dev)
    hits = torch.empty((B, J), dtype=torch.float64, device=dev)
    rie = torch.empty((B, A), dtype=torch.float64, device=dev)
    lib = _lib.load()
    ws_ptr, ws_bytes = _bootstrap_scratch(lib, dev, n, B, workspace)
    with torch.cuda.device(dev):
        _lib.check(lib.mkgnn_bootstrap_early(rank.data_ptr(), y_sorted.data_ptr(), group_last.data_ptr(), n, split, B, seed, offset,
                                             lower, upper, cuts.data_ptr() if J else None, J, alphas.data_ptr() if A else None, A,
                                             auc.data_ptr(), logauc.data_ptr(), two_u.data_ptr(), n_pos.data_ptr(), ap.data_ptr(),
                                             hits.data_ptr() if J else None, rie.data_ptr() if A else None, ws_ptr, ws_bytes,
                                             _lib.stream_ptr(dev)), "mkgnn_bootstrap_early")
    return auc, logauc, two_u, n_pos, ap, hits, rie


def bootstrap_regression_replicates_per_pass(n: int, n_boot: int) -> int:
    """The replicates ``bootstrap_regression`` keeps in flight when it sizes its own scratch: all ``n_boot`` where their two prefix-sum
    rows fit under ``_lib.BOOTSTRAP_WORKSPACE_CAP`` bytes (``2 * 4 * ceil4(n)`` each), otherwise as many as do, at least one."""
    per = 8 * ((int(n) + 3) // 4 * 4)
    return max(1, min(int(n_boot), _lib.BOOTSTRAP_WORKSPACE_CAP // per))


def bootstrap_regression(rank_p: torch.Tensor, first_p: torch.Tensor, last_p: torch.Tensor, cross: torch.Tensor, first_t: torch.Tensor,
                         last_t: torch.Tensor, p_sorted: torch.Tensor, t_by_prank: torch.Tensor, centre: torch.Tensor, cuts, n_boot: int,
                         seed: int, offset: int, workspace: Optional[torch.Tensor] = None):
    """``(mom float64 [n_boot, 7], rank_sums int64 [n_boot, 3], hits int64 [n_boot, J], n_drawn int32 [n_boot])``: the raw sums of the
    regression metrics of ``n_boot`` bootstrap replicates of ``n`` rows whose predictions and truths were each sorted ONCE (best
    first, stable; ``evaluation.regression_prepare`` builds the arguments) -- ``rank_p int32 [n]`` the prediction rank of row ``i``,
    ``first_p`` / ``last_p int32 [n]`` the ends of every prediction rank's tie group, ``cross int32 [n]`` the prediction rank of the row
    at every truth rank, ``first_t`` / ``last_t`` the tie groups by truth rank, ``p_sorted`` / ``t_by_prank float64 [n]`` the two values
    by prediction rank, ``centre float64 [2]`` the values the moments are centred on, all contiguous CUDA tensors; ``cuts``: up to
    ``_lib.BOOTSTRAP_MAX_CUTS`` top-k sizes ``1 <= k <= n`` (an int32 device tensor, or a sequence).  Replicate ``b`` draws as the
    unstratified ``bootstrap_roc`` does, with ``philox_word(seed, offset + b, i)``.  ``evaluation.regression_reference_sorted`` is the
    definition: ``rank_sums``, ``hits`` and ``n_drawn`` agree with it exactly, ``mom`` within the rounding of a float64 sum; a cut outside
    ``[1, n]`` gives a column of ``-1`` and changes nothing else; ``evaluation.regression_derived`` turns the sums into RMSE, MAE, R2,
    Pearson, Spearman and top-fraction recall.  One ``mkgnn_bootstrap_regression``: no sort, no host round trip, capturable (``centre``
    and a ``cuts`` tensor are re-read by a replay); a replicate's outputs do not depend on ``n_boot``, on where the replicates start
    or on the scratch's size.  ``workspace``: a uint8 device tensor to use as scratch, at least
    ``mkgnn_bootstrap_regression_workspace_bytes(n, 1)`` bytes -- the call passes over the replicates as many at a time as it holds;
    without it a per-device buffer that only grows serves eager calls (sized for ``bootstrap_regression_replicates_per_pass``), and a
    call inside a capture allocates its own.  At most ``_lib.BOOTSTRAP_REG_MAX_ROWS`` rows; there is no fallback beyond.  It has no
    autograd node: called where a gradient is being recorded for one of its inputs it raises."""
    who = "bootstrap_regression"
    ints, reals = (rank_p, first_p, last_p, cross, first_t, last_t), (p_sorted, t_by_prank)
    if not all(torch.is_tensor(x) and x.dim() == 1 for x in ints + reals) or any(x.dtype != torch.int32 for x in ints) \
            or any(x.dtype != torch.float64 for x in reals) or len({x.numel() for x in ints + reals}) != 1:
        raise ValueError(f"{who} needs rank_p, first_p, last_p, cross, first_t, last_t int32 [n] and p_sorted, t_by_prank float64 [n]")
    dev = rank_p.device
    if not rank_p.is_cuda or any(x.device != dev for x in ints + reals):
        raise ValueError(f"{who} runs on the GPU: rank_p is on {dev} and the other arrays on {sorted({str(x.device) for x in ints + reals})} "
                         f"(there is no CPU path; evaluation.regression_reference_sorted is the host form)")
    if not torch.is_tensor(centre) or centre.dtype != torch.float64 or centre.numel() != 2 or centre.device != dev \
            or not centre.is_contiguous():
        raise ValueError(f"{who}: centre is a contiguous float64 tensor of two values on {dev}")
    if torch.is_grad_enabled() and any(x.requires_grad for x in reals + (centre,)):
        raise RuntimeError(f"{who} is forward only: call it under torch.no_grad() (or on detached inputs)")
    n, B, seed, offset = rank_p.numel(), int(n_boot), int(seed), int(offset)
    if not 1 <= n <= _lib.BOOTSTRAP_REG_MAX_ROWS:
        raise ValueError(f"{who}: {n} rows outside [1, {_lib.BOOTSTRAP_REG_MAX_ROWS}]")
    if not 1 <= B <= _lib.BOOTSTRAP_MAX_REPLICATES:
        raise ValueError(f"{who}: n_boot = {n_boot} outside [1, {_lib.BOOTSTRAP_MAX_REPLICATES}] per call")
    if not (0 <= seed < 1 << 64 and 0 <= offset and offset + B <= 1 << 64):
        raise ValueError(f"{who}: seed and offset .. offset + n_boot - 1 are unsigned 64-bit values")
    if not all(x.is_contiguous() for x in ints + reals):
        raise ValueError(f"{who} needs contiguous tensors")
    cuts = _early_vector(who, "cuts", cuts, torch.int32, _lib.BOOTSTRAP_MAX_CUTS, dev)
    J = cuts.numel()
    mom = torch.empty((B, 7), dtype=torch.float64, device=dev)
    rank_sums = torch.empty((B, 3), dtype=torch.int64, device=dev)
    hits = torch.empty((B, J), dtype=torch.int64, device=dev)
    n_drawn = torch.empty(B, dtype=torch.int32, device=dev)
    lib = _lib.load()
    one = int(lib.mkgnn_bootstrap_regression_workspace_bytes(n, 1))
    if workspace is not None and workspace.numel() < one:
        raise ValueError(f"workspace: at least {one} bytes (one replicate)")
    want = workspace.numel() if workspace is not None else \
        int(lib.mkgnn_bootstrap_regression_workspace_bytes(n, bootstrap_regression_replicates_per_pass(n, B)))
    ws = _max_cosine_workspace(dev, want, workspace)
    with torch.cuda.device(dev):
        _lib.check(lib.mkgnn_bootstrap_regression(rank_p.data_ptr(), first_p.data_ptr(), last_p.data_ptr(), cross.data_ptr(),
                                                  first_t.data_ptr(), last_t.data_ptr(), p_sorted.data_ptr(), t_by_prank.data_ptr(),
                                                  centre.data_ptr(), cuts.data_ptr() if J else None, J, n, B, seed, offset,
                                                  mom.data_ptr(), rank_sums.data_ptr(), hits.data_ptr() if J else None,
                                                  n_drawn.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_ptr(dev)),
                   "mkgnn_bootstrap_regression")
    return mom, rank_sums, hits, n_drawn
