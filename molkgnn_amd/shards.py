"""Packed molecule shards: the pre-collated on-disk / in-memory format of SURVEY.md 8 f-2.

The reference stores one PyG ``Data`` object per molecule (``wrapper.py:362-460``, ``InMemoryDataset``) and lets
``DataLoader`` workers collate a batch from B Python objects with 20 extra per-degree tensors each
(``wrapper.py:559-672``).  At the ≥ 10^6 molecules/s the kernels run at, that loader is the bound.  A shard keeps the
molecules of a (pre-shuffled) part of the data set **already concatenated**, in the order they will be consumed:

* a batch is a contiguous molecule range, so collation is five slice copies into one pinned staging buffer and ONE
  host-to-device copy (the slices of ``x``, ``p``, ``edge_attr``, the bond endpoints and the molecule pointers);
* everything index-like is rebuilt on the device: batch-local atom ids (stored ids are shard-global int32: one
  subtraction), the ``batch`` vector, and then the degree buckets / index plan by the HIP builders
  (``receptive_field.attach_receptive_fields``, ``plan.BatchPlan.build_hip``);
* the file is a fixed header + 64-byte aligned little-endian arrays, read through ``numpy.memmap`` (no parsing, no
  pickling; a shard written on one box is mapped on another);
* data-parallel ranks take batches ``rank, rank + world, ...`` of the same shard sequence, so the union over
  ranks is the single-GPU stream.

Layout (version 2)::

    header   256 bytes: b"MKGS", u32 version, u64 n_molecules, u64 n_atoms, u64 n_bonds (directed edges),
                        u32 x_dim, u32 e_dim, u32 p_dim, u32 flags (bit 0: the compact wire form applies), then 10 x u64
                        array offsets in the order below
    mol_atom_ptr  i64 [M + 1]     first atom of every molecule
    mol_edge_ptr  i64 [M + 1]     first directed edge of every molecule
    y             f32 [M]         label (data.py:37 trains on one task)
    assay_id      i32 [M]         PubChem AID the molecule comes from (mixed nine-assay shards, BASELINE configs[4])
    x             f32 [A, x_dim]
    p             f32 [A, p_dim]
    edge_src      i32 [E]         shard-global atom ids; bonds as consecutive (i, j), (j, i) (wrapper.py:152-156)
    edge_dst      i32 [E]
    edge_attr     f32 [E, e_dim]
    mol_deg_ptr   i64 [M + 1, 5]  prefix sums over molecules of their atoms of degree 1, 2, 3, 4 and of any other degree:
                                  the degree histogram of a molecule range is one subtraction (fixed-shape padding)

Fixed-shape batches (``padding.py``: one captured graph serves every batch) come straight out of the loader:
``ShardLoader(..., fixed_shape=True)`` pads every batch ON THE HOST while staging it -- the padding atoms, their bonds
and molecules exactly as ``padding.pad_batch`` makes them -- directly in the layout of ``padding.StaticBatch``'s flat
buffer, so a batch reaches the static buffers by one host-to-device copy and one device copy, with no device-side
index work and no host synchronisation.
"""
from __future__ import annotations

import atexit
import os
import struct
import weakref
from queue import Queue
from typing import Iterable, Iterator, List, Optional, Sequence

import numpy as np
import torch

from .receptive_field import GraphBatch

MAGIC = b"MKGS"
VERSION = 2
HEADER_BYTES = 256
ALIGN = 64
_ARRAYS = ("mol_atom_ptr", "mol_edge_ptr", "y", "assay_id", "x", "p", "edge_src", "edge_dst", "edge_attr", "mol_deg_ptr")
_HEAD = struct.Struct("<4sIQQQIIII10Q")


def _align(n: int) -> int:
    return (n + ALIGN - 1) // ALIGN * ALIGN


def write_shard(path: str, batch: GraphBatch) -> None:
    """Write the molecules of a collated batch (``x``, ``p``, ``edge_index``, ``edge_attr``, ``batch``, ``y`` and
    optionally ``assay_id``) as one shard, in the batch's molecule order."""
    x = batch.x.detach().cpu().numpy().astype(np.float32, copy=False)
    p = batch.p.detach().cpu().numpy().astype(np.float32, copy=False)
    ei = batch.edge_index.detach().cpu().numpy()
    ea = batch.edge_attr.detach().cpu().numpy().astype(np.float32, copy=False)
    bvec = batch.batch.detach().cpu().numpy()
    y = batch.y.detach().cpu().numpy().astype(np.float32, copy=False).reshape(-1)
    m = int(y.shape[0])
    a, e = int(x.shape[0]), int(ei.shape[1])
    if a >= 2 ** 31 or e >= 2 ** 31:
        raise ValueError("a shard holds fewer than 2^31 atoms and directed edges (ids are int32)")
    if bvec.shape[0] != a or (a and (np.diff(bvec) < 0).any()):
        raise ValueError("`batch` must be sorted (atoms grouped by molecule), one entry per atom")
    edge_mol = bvec[ei[0]] if e else np.zeros(0, dtype=np.int64)
    if e and ((np.diff(edge_mol) < 0).any() or (bvec[ei[1]] != edge_mol).any()):
        raise ValueError("edges must be grouped by molecule and stay inside it")
    atom_ptr = np.zeros(m + 1, dtype=np.int64)
    atom_ptr[1:] = np.cumsum(np.bincount(bvec, minlength=m))
    edge_ptr = np.zeros(m + 1, dtype=np.int64)
    edge_ptr[1:] = np.cumsum(np.bincount(edge_mol, minlength=m))
    assay = getattr(batch, "assay_id", None)
    assay = np.zeros(m, dtype=np.int32) if assay is None else assay.detach().cpu().numpy().astype(np.int32)
    deg = np.bincount(ei[0], minlength=a) if e else np.zeros(a, dtype=np.int64)
    cls = np.where((deg >= 1) & (deg <= 4), deg - 1, 4)                 # 0..3: degree 1..4, 4: in no bucket
    per_mol = np.zeros((m, 5), dtype=np.int64)
    np.add.at(per_mol, (bvec, cls), 1)
    deg_ptr = np.zeros((m + 1, 5), dtype=np.int64)
    deg_ptr[1:] = np.cumsum(per_mol, axis=0)
    arrays = {"mol_atom_ptr": atom_ptr, "mol_edge_ptr": edge_ptr, "y": y, "assay_id": assay,
              "x": np.ascontiguousarray(x), "p": np.ascontiguousarray(p),
              "edge_src": ei[0].astype(np.int32), "edge_dst": ei[1].astype(np.int32), "edge_attr": np.ascontiguousarray(ea),
              "mol_deg_ptr": deg_ptr}
    offsets, off = [], HEADER_BYTES
    for name in _ARRAYS:
        offsets.append(off)
        off = _align(off + arrays[name].nbytes)
    # can the batches of this shard travel in the compact wire form (collate_compact)?  Bonds stored as consecutive
    # (i, j), (j, i) pairs with one attribute row for both directions, attributes byte-valued
    compact = e % 2 == 0 and (e == 0 or (
        np.array_equal(ei[0, 0::2], ei[1, 1::2]) and np.array_equal(ei[1, 0::2], ei[0, 1::2]) and
        np.array_equal(ea[0::2], ea[1::2]) and float(ea.min()) >= 0.0 and float(ea.max()) <= 255.0 and
        np.array_equal(ea, np.rint(ea))))
    head = _HEAD.pack(MAGIC, VERSION, m, a, e, x.shape[1], ea.shape[1] if ea.ndim == 2 else 0, p.shape[1], 1 if compact else 0,
                      *offsets)
    tmp = path + ".tmp"
    with open(tmp, "wb") as f:
        f.write(head.ljust(HEADER_BYTES, b"\0"))
        for name, o in zip(_ARRAYS, offsets):
            f.seek(o)
            f.write(arrays[name].tobytes())
        f.truncate(off)
    os.replace(tmp, path)


class Shard:
    """A memory-mapped shard; ``slices(m0, m1)`` are zero-copy views of a molecule range."""

    def __init__(self, path: str):
        self.path = path
        with open(path, "rb") as f:
            head = f.read(HEADER_BYTES)
        if len(head) < _HEAD.size:
            raise ValueError(f"{path}: not a molecule shard (short header)")
        magic, version, m, a, e, xd, ed, pd, flags, *offs = _HEAD.unpack(head[:_HEAD.size])
        if magic != MAGIC:
            raise ValueError(f"{path}: not a molecule shard (magic {magic!r})")
        if version != VERSION:
            raise ValueError(f"{path}: shard version {version}, this reader knows {VERSION}")
        self.n_molecules, self.n_atoms, self.n_edges = int(m), int(a), int(e)
        self.x_dim, self.e_dim, self.p_dim = int(xd), int(ed), int(pd)
        self.compact_ok = bool(flags & 1)    # bonds as reversed pairs with shared, byte-valued attributes: collate_compact applies
        shapes = {"mol_atom_ptr": (np.int64, (m + 1,)), "mol_edge_ptr": (np.int64, (m + 1,)), "y": (np.float32, (m,)),
                  "assay_id": (np.int32, (m,)), "x": (np.float32, (a, xd)), "p": (np.float32, (a, pd)),
                  "edge_src": (np.int32, (e,)), "edge_dst": (np.int32, (e,)), "edge_attr": (np.float32, (e, ed)),
                  "mol_deg_ptr": (np.int64, (m + 1, 5))}
        size = os.path.getsize(path)
        self._mm = np.memmap(path, dtype=np.uint8, mode="r")
        for name, o in zip(_ARRAYS, offs):
            dt, shp = shapes[name]
            nbytes = int(np.prod(shp)) * np.dtype(dt).itemsize
            if o % ALIGN or o + nbytes > size:
                raise ValueError(f"{path}: array {name} at {o} (+{nbytes}) does not fit the file ({size} bytes)")
            setattr(self, name, np.frombuffer(self._mm, dtype=dt, count=int(np.prod(shp)), offset=int(o)).reshape(shp))
        if self.mol_atom_ptr[-1] != a or self.mol_edge_ptr[-1] != e:
            raise ValueError(f"{path}: molecule pointers do not cover the arrays")

    def degree_histogram(self, m0: int, m1: int) -> List[int]:
        """``padding.degree_histogram`` of the molecules [m0, m1): [atoms, N_1, N_2, N_3, N_4, atoms in no bucket]."""
        d = (self.mol_deg_ptr[m1] - self.mol_deg_ptr[m0]).tolist()
        return [int(self.mol_atom_ptr[m1] - self.mol_atom_ptr[m0]), d[0], d[1], d[2], d[3], d[4]]

    def ranges(self, m0: int, m1: int):
        return (int(self.mol_atom_ptr[m0]), int(self.mol_atom_ptr[m1]), int(self.mol_edge_ptr[m0]), int(self.mol_edge_ptr[m1]))


def _stage_layout(n_mol: int, n_atoms: int, n_edges: int, xd: int, pd: int, ed: int):
    """Byte offsets of a batch's slices in the staging buffer (each 64-byte aligned) and the total."""
    parts = (("x", 4 * n_atoms * xd), ("p", 4 * n_atoms * pd), ("edge_attr", 4 * n_edges * ed), ("edge_src", 4 * n_edges),
             ("edge_dst", 4 * n_edges), ("atom_ptr", 8 * (n_mol + 1)), ("y", 4 * n_mol), ("assay_id", 4 * n_mol))
    out, off = {}, 0
    for name, nbytes in parts:
        out[name] = (off, nbytes)
        off = _align(off + nbytes)
    return out, off


def collate(shard: Shard, m0: int, m1: int, device, staging: Optional[torch.Tensor] = None,
            stream: Optional["torch.cuda.Stream"] = None) -> GraphBatch:
    """Molecules ``[m0, m1)`` of a shard as one collated batch on ``device``: slice copies into ONE staging buffer
    (pinned when the device is a GPU), one host-to-device copy, index arithmetic on the device."""
    device = torch.device(device)
    a0, a1, e0, e1 = shard.ranges(m0, m1)
    nm, na, ne = m1 - m0, a1 - a0, e1 - e0
    lay, total = _stage_layout(nm, na, ne, shard.x_dim, shard.p_dim, shard.e_dim)
    if staging is None or staging.numel() < total:
        staging = torch.empty(max(total, 1), dtype=torch.uint8, pin_memory=(device.type == "cuda"))
    host = staging.numpy()

    def put(name, arr):
        o, nbytes = lay[name]
        host[o:o + nbytes] = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)

    put("x", shard.x[a0:a1]); put("p", shard.p[a0:a1]); put("edge_attr", shard.edge_attr[e0:e1])
    put("edge_src", shard.edge_src[e0:e1]); put("edge_dst", shard.edge_dst[e0:e1])
    put("atom_ptr", shard.mol_atom_ptr[m0:m1 + 1]); put("y", shard.y[m0:m1]); put("assay_id", shard.assay_id[m0:m1])
    if device.type == "cuda":
        with torch.cuda.stream(stream) if stream is not None else _null():
            dev = staging[:total].to(device, non_blocking=True)
    else:
        dev = staging[:total].clone()

    def view(name, dtype, shape):
        o, nbytes = lay[name]
        return dev[o:o + nbytes].view(dtype).view(shape)

    with torch.cuda.stream(stream) if (stream is not None and device.type == "cuda") else _null():
        src = view("edge_src", torch.int32, (ne,)).long() - a0
        dst = view("edge_dst", torch.int32, (ne,)).long() - a0
        atom_ptr = view("atom_ptr", torch.int64, (nm + 1,)) - a0
        counts = atom_ptr[1:] - atom_ptr[:-1]
        batch_vec = torch.repeat_interleave(torch.arange(nm, device=device), counts, output_size=na)
        out = GraphBatch(x=view("x", torch.float32, (na, shard.x_dim)), p=view("p", torch.float32, (na, shard.p_dim)),
                         edge_index=torch.stack([src, dst]), edge_attr=view("edge_attr", torch.float32, (ne, shard.e_dim)),
                         batch=batch_vec, y=view("y", torch.float32, (nm,)), num_graphs=nm, smiles=None,
                         assay_id=view("assay_id", torch.int32, (nm,)).long(), mol_ptr=atom_ptr)
    out._staging = staging            # (the pinned buffer must outlive the asynchronous copy)
    return out


def padded_layout(shape, num_molecules: int, x_dim: int, p_dim: int, e_dim: int):
    """Field table of ``padding.StaticBatch``'s flat buffer for a fixed shape: (name, offset, shape, numpy dtype, bytes)."""
    from .padding import PAD_MOLECULES, StaticBatch
    A, Eg, G = shape["atoms"], shape["edges"], num_molecules + PAD_MOLECULES
    spec = {"x": ((A, x_dim), np.float32), "p": ((A, p_dim), np.float32), "edge_index": ((2, Eg), np.int64),
            "edge_attr": ((Eg, e_dim), np.float32), "batch": ((A,), np.int64), "y": ((num_molecules,), np.float32),
            "mol_ptr": ((G + 1,), np.int32), "atom_mol": ((A,), np.int32), "n_valid_atoms": ((1,), np.int64)}
    table, off = [], 0
    for k in StaticBatch.FIELDS:
        shp, dt = spec[k]
        nbytes = int(np.prod(shp)) * np.dtype(dt).itemsize
        table.append((k, off, shp, dt, nbytes))
        off += (nbytes + 255) // 256 * 256
    return table, off


def collate_padded(shard: Shard, m0: int, m1: int, shape, host: np.ndarray) -> None:
    """Molecules ``[m0, m1)`` padded to ``shape`` (``padding.fixed_shape``), written into ``host`` (uint8, the flat
    layout of ``padded_layout``): what ``padding.pack(padding.pad_batch(collate(...), shape, m1 - m0))`` holds, made on
    the host with slice copies and a few small index fills."""
    from .padding import PAD_MOLECULES
    nm = m1 - m0
    a0, a1, e0, e1 = shard.ranges(m0, m1)
    na, ne = a1 - a0, e1 - e0
    h = shard.degree_histogram(m0, m1)
    need = [shape[f"n{d}"] - h[d] for d in range(1, 5)]
    if min(need) < 0 or h[5]:
        raise ValueError(f"molecules [{m0}, {m1}) with degree histogram {h[1:5]} (+{h[5]} in no bucket) do not fit the shape {shape}")
    n_pad = sum(need)
    table, total = padded_layout(shape, nm, shard.x_dim, shard.p_dim, shard.e_dim)
    if host.shape[0] < total:
        raise ValueError("staging buffer too small")
    f = {k: host[off:off + nbytes].view(dt).reshape(shp) for k, off, shp, dt, nbytes in table}
    f["x"][:na] = shard.x[a0:a1]; f["x"][na:] = 0.0
    f["p"][:na] = shard.p[a0:a1]; f["p"][na:] = 0.0
    f["edge_attr"][:ne] = shard.edge_attr[e0:e1]
    f["edge_attr"][ne:] = 0.0
    f["edge_attr"][ne:, 0] = 1.0
    ei = f["edge_index"]
    np.subtract(shard.edge_src[e0:e1], a0, out=ei[0, :ne], casting="unsafe")
    np.subtract(shard.edge_dst[e0:e1], a0, out=ei[1, :ne], casting="unsafe")
    # padding atoms in degree order, their bond stubs paired off in sequence (padding.pad_batch)
    deg_of = np.repeat(np.arange(1, 5), need)
    stubs = np.repeat(np.arange(n_pad, dtype=np.int64), deg_of) + na
    if stubs.shape[0] % 2 or stubs.shape[0] != shape["edges"] - ne:
        raise ValueError("padding bond stubs do not pair up: the shape does not come from fixed_shape() over these batches")
    a, b = stubs[0::2], stubs[1::2]
    ei[0, ne::2] = a; ei[0, ne + 1::2] = b
    ei[1, ne::2] = b; ei[1, ne + 1::2] = a
    atom_ptr = shard.mol_atom_ptr[m0:m1 + 1] - a0
    counts = np.diff(atom_ptr)
    bt = f["batch"]
    bt[:na] = np.repeat(np.arange(nm, dtype=np.int64), counts)
    bt[na:] = nm + (np.arange(n_pad, dtype=np.int64) * PAD_MOLECULES) // max(n_pad, 1)
    f["atom_mol"][:] = bt
    f["y"][:] = shard.y[m0:m1]
    mp = f["mol_ptr"]
    mp[0] = 0
    mp[1:nm + 1] = atom_ptr[1:]
    pad_counts = np.bincount(bt[na:] - nm, minlength=PAD_MOLECULES)
    mp[nm + 1:] = na + np.cumsum(pad_counts)
    f["n_valid_atoms"][0] = na


def compact_layout(shape, num_molecules: int, x_dim: int, p_dim: int, e_dim: int):
    """Field table of the compact wire form of a fixed-shape batch (``padding.CompactStaticBatch``): what has to cross
    PCIe and nothing derived -- features and coordinates as they are, every bond once as an int32 pair with byte-valued
    attributes, labels, molecule pointers; ``mkgnn_expand_batch`` rebuilds ``edge_index`` (int64, both directions),
    ``edge_attr`` (fp32, both directions), ``batch`` and ``atom_mol`` on the device.  14.5 MB instead of 23.8 MB for 4096
    molecules."""
    from .padding import PAD_MOLECULES
    A, B2, G = shape["atoms"], shape["edges"] // 2, num_molecules + PAD_MOLECULES
    spec = (("x", (A, x_dim), np.float32), ("p", (A, p_dim), np.float32), ("bond_ij", (B2, 2), np.int32),
            ("bond_attr", (B2, e_dim), np.uint8), ("y", (num_molecules,), np.float32), ("mol_ptr", (G + 1,), np.int32),
            ("n_valid_atoms", (1,), np.int64))
    table, off = [], 0
    for k, shp, dt in spec:
        nbytes = int(np.prod(shp)) * np.dtype(dt).itemsize
        table.append((k, off, shp, dt, nbytes))
        off += (nbytes + 255) // 256 * 256
    return table, off


def collate_compact(shard: Shard, m0: int, m1: int, shape, host: np.ndarray) -> None:
    """Molecules ``[m0, m1)`` padded to ``shape`` in the compact wire form (``compact_layout``); expands (``mkgnn_expand_batch``)
    to exactly what ``collate_padded`` writes.  Needs ``shard.compact_ok``."""
    from .padding import PAD_MOLECULES
    if not shard.compact_ok:
        raise ValueError(f"{shard.path}: bonds are not reversed pairs with shared byte-valued attributes: no compact form")
    nm = m1 - m0
    a0, a1, e0, e1 = shard.ranges(m0, m1)
    na, ne = a1 - a0, e1 - e0
    h = shard.degree_histogram(m0, m1)
    need = [shape[f"n{d}"] - h[d] for d in range(1, 5)]
    if min(need) < 0 or h[5]:
        raise ValueError(f"molecules [{m0}, {m1}) with degree histogram {h[1:5]} (+{h[5]} in no bucket) do not fit the shape {shape}")
    n_pad = sum(need)
    table, total = compact_layout(shape, nm, shard.x_dim, shard.p_dim, shard.e_dim)
    if host.shape[0] < total:
        raise ValueError("staging buffer too small")
    f = {k: host[off:off + nbytes].view(dt).reshape(shp) for k, off, shp, dt, nbytes in table}
    nb = ne // 2
    f["x"][:na] = shard.x[a0:a1]; f["x"][na:] = 0.0
    f["p"][:na] = shard.p[a0:a1]; f["p"][na:] = 0.0
    f["bond_attr"][:nb] = shard.edge_attr[e0:e1:2]           # (float -> uint8: exact, the shard checked the values)
    f["bond_attr"][nb:] = 0
    f["bond_attr"][nb:, 0] = 1
    ij = f["bond_ij"]
    np.subtract(shard.edge_src[e0:e1:2], a0, out=ij[:nb, 0], casting="unsafe")
    np.subtract(shard.edge_dst[e0:e1:2], a0, out=ij[:nb, 1], casting="unsafe")
    deg_of = np.repeat(np.arange(1, 5), need)
    stubs = np.repeat(np.arange(n_pad, dtype=np.int64), deg_of) + na
    if stubs.shape[0] % 2 or stubs.shape[0] != shape["edges"] - ne:
        raise ValueError("padding bond stubs do not pair up: the shape does not come from fixed_shape() over these batches")
    ij[nb:, 0] = stubs[0::2]
    ij[nb:, 1] = stubs[1::2]
    atom_ptr = shard.mol_atom_ptr[m0:m1 + 1] - a0
    f["y"][:] = shard.y[m0:m1]
    mp = f["mol_ptr"]
    mp[0] = 0
    mp[1:nm + 1] = atom_ptr[1:]
    pad_mol = (np.arange(n_pad, dtype=np.int64) * PAD_MOLECULES) // max(n_pad, 1)
    mp[nm + 1:] = na + np.cumsum(np.bincount(pad_mol, minlength=PAD_MOLECULES))
    f["n_valid_atoms"][0] = na


def gather_compact(shard: Shard, ids, shape, host: np.ndarray) -> None:
    """The molecules ``ids`` of a shard -- any integer sequence: repeats allowed, order kept -- padded to ``shape`` in the
    compact wire form (``compact_layout(shape, len(ids), ...)``): exactly what ``collate_compact`` writes for a shard that
    holds those molecules in that order as its range ``[0, len(ids))``.  The definition ``mkgnn_gather_compact`` (the gather
    from a device-resident shard) is tested against, and the CPU path of ``ResidentLoader``."""
    from .padding import PAD_MOLECULES
    if not shard.compact_ok:
        raise ValueError(f"{shard.path}: bonds are not reversed pairs with shared byte-valued attributes: no compact form")
    ids = np.asarray(ids if isinstance(ids, np.ndarray) else list(ids), dtype=np.int64).reshape(-1)
    nm = int(ids.shape[0])
    if nm and (int(ids.min()) < 0 or int(ids.max()) >= shard.n_molecules):
        raise ValueError(f"molecule ids outside [0, {shard.n_molecules})")
    a_first, e_first = shard.mol_atom_ptr[ids], shard.mol_edge_ptr[ids]
    cnt_a, cnt_b = shard.mol_atom_ptr[ids + 1] - a_first, (shard.mol_edge_ptr[ids + 1] - e_first) // 2
    atom_ptr = np.zeros(nm + 1, dtype=np.int64)
    atom_ptr[1:] = np.cumsum(cnt_a)
    bond_ptr = np.zeros(nm + 1, dtype=np.int64)
    bond_ptr[1:] = np.cumsum(cnt_b)
    na, nb = int(atom_ptr[-1]), int(bond_ptr[-1])
    d = (shard.mol_deg_ptr[ids + 1] - shard.mol_deg_ptr[ids]).sum(axis=0).tolist() if nm else [0] * 5
    h = [na, d[0], d[1], d[2], d[3], d[4]]
    need = [shape[f"n{k}"] - h[k] for k in range(1, 5)]
    if min(need) < 0 or h[5]:
        raise ValueError(f"{nm} gathered molecules with degree histogram {h[1:5]} (+{h[5]} in no bucket) do not fit the shape {shape}")
    n_pad = sum(need)
    table, total = compact_layout(shape, nm, shard.x_dim, shard.p_dim, shard.e_dim)
    if host.shape[0] < total:
        raise ValueError("staging buffer too small")
    f = {k: host[off:off + nbytes].view(dt).reshape(shp) for k, off, shp, dt, nbytes in table}
    # output atom r of slot s comes from shard atom (first atom of molecule ids[s]) + (r - atom_ptr[s]); bonds likewise
    src_atom = np.repeat(a_first - atom_ptr[:-1], cnt_a) + np.arange(na, dtype=np.int64)
    src_edge = np.repeat(e_first - 2 * bond_ptr[:-1], cnt_b) + 2 * np.arange(nb, dtype=np.int64)
    shift = np.repeat(atom_ptr[:-1] - a_first, cnt_b)
    f["x"][:na] = shard.x[src_atom]; f["x"][na:] = 0.0
    f["p"][:na] = shard.p[src_atom]; f["p"][na:] = 0.0
    f["bond_attr"][:nb] = shard.edge_attr[src_edge]
    f["bond_attr"][nb:] = 0
    f["bond_attr"][nb:, 0] = 1
    ij = f["bond_ij"]
    ij[:nb, 0] = shard.edge_src[src_edge] + shift
    ij[:nb, 1] = shard.edge_dst[src_edge] + shift
    deg_of = np.repeat(np.arange(1, 5), need)
    stubs = np.repeat(np.arange(n_pad, dtype=np.int64), deg_of) + na
    if stubs.shape[0] % 2 or stubs.shape[0] != shape["edges"] - 2 * nb:
        raise ValueError("padding bond stubs do not pair up: the shape does not come from fixed_shape() over these batches")
    ij[nb:, 0] = stubs[0::2]
    ij[nb:, 1] = stubs[1::2]
    f["y"][:] = shard.y[ids]
    mp = f["mol_ptr"]
    mp[0] = 0
    mp[1:nm + 1] = atom_ptr[1:]
    pad_mol = (np.arange(n_pad, dtype=np.int64) * PAD_MOLECULES) // max(n_pad, 1)
    mp[nm + 1:] = na + np.cumsum(np.bincount(pad_mol, minlength=PAD_MOLECULES))
    f["n_valid_atoms"][0] = na


def collate_compact_native(shard: Shard, m0: int, m1: int, shape, host: np.ndarray) -> None:
    """``collate_compact`` by ONE call into the library (``mkgnn_collate_compact``, host code): byte for byte the same buffer
    (tested), and the interpreter lock is released for the whole batch -- the numpy form holds it through a dozen small array
    operations per batch, which with three loader threads kept the thread that replays the training graph waiting (0.2 ms of
    idle GPU per step of a shard-fed epoch)."""
    from . import _lib
    from .padding import PAD_MOLECULES
    lib = _lib.load()
    view = getattr(shard, "_view", None)
    if view is None:
        if not shard.compact_ok:
            raise ValueError(f"{shard.path}: bonds are not reversed pairs with shared byte-valued attributes: no compact form")
        view = _lib.ShardView()
        for name in ("x", "p", "edge_src", "edge_dst", "edge_attr", "y", "mol_atom_ptr", "mol_edge_ptr", "mol_deg_ptr"):
            setattr(view, name, getattr(shard, name).ctypes.data)
        view.n_molecules, view.x_dim, view.p_dim, view.e_dim = shard.n_molecules, shard.x_dim, shard.p_dim, shard.e_dim
        shard._view = view
    sh = _lib.Int64x6(shape["atoms"], shape["edges"], shape["n1"], shape["n2"], shape["n3"], shape["n4"])
    _lib.check(lib.mkgnn_collate_compact(view, int(m0), int(m1), sh, PAD_MOLECULES, host.ctypes.data, host.shape[0]),
               "mkgnn_collate_compact")


class CompactBatch:
    """A fixed-shape batch in the compact wire form on the device (``padding.CompactStaticBatch.load`` takes it)."""

    def __init__(self, flat, shape, num_molecules: int):
        self.flat, self.shape, self.n_valid_molecules = flat, dict(shape), num_molecules
        self.bucket_sizes = [shape["n1"], shape["n2"], shape["n3"], shape["n4"]]


class PackedBatch:
    """A fixed-shape batch as one flat device buffer in ``padding.StaticBatch``'s layout (``StaticBatch.load`` takes it)."""

    def __init__(self, flat, shape, num_molecules: int):
        from .padding import PAD_MOLECULES
        self.flat = flat
        self.bucket_sizes = [shape["n1"], shape["n2"], shape["n3"], shape["n4"]]
        self.n_valid_molecules, self.num_graphs = num_molecules, num_molecules + PAD_MOLECULES

    def unpack(self, shard_dims) -> GraphBatch:
        """The fields as views of the flat buffer (a ``padding.pad_batch`` result)."""
        x_dim, p_dim, e_dim = shard_dims
        shape = {"n1": self.bucket_sizes[0], "n2": self.bucket_sizes[1], "n3": self.bucket_sizes[2], "n4": self.bucket_sizes[3]}
        shape["atoms"] = sum(self.bucket_sizes)
        shape["edges"] = sum((d + 1) * self.bucket_sizes[d] for d in range(4))
        table, _ = padded_layout(shape, self.n_valid_molecules, x_dim, p_dim, e_dim)
        out = GraphBatch()
        tdt = {np.float32: torch.float32, np.int64: torch.int64, np.int32: torch.int32}
        for k, off, shp, dt, nbytes in table:
            setattr(out, k, self.flat[off:off + nbytes].view(tdt[dt]).view(shp))
        out.flat = self.flat
        out.bucket_sizes, out.n_valid_molecules, out.num_graphs = self.bucket_sizes, self.n_valid_molecules, self.num_graphs
        return out


class _null:
    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


_LOADERS: "weakref.WeakSet" = weakref.WeakSet()


def _release_all() -> None:
    """Pinned staging and device landing buffers of loaders that are still alive go BEFORE the interpreter tears the GPU
    runtime down (a pinned buffer freed after that aborts the process)."""
    for ld in list(_LOADERS):
        ld.close()


atexit.register(_release_all)


class ShardLoader:
    """Batches of ``batch_size`` consecutive molecules from a sequence of shards, for rank ``rank`` of ``world``.

    Batch k of the global sequence (shard after shard, a shard's tail batch may be short) goes to rank ``k % world``
    (SURVEY 8e).  ``workers`` background threads stage the next batches into pinned buffers and issue their
    host-to-device copies on a copy stream, ``prefetch`` batches ahead, handed over in order; the consumer's stream waits
    for the copy's event, not for the host.
    """

    def __init__(self, paths: Sequence[str], batch_size: int, device="cpu", rank: int = 0, world: int = 1,
                 prefetch: int = 2, drop_last: bool = False, workers: int = 2, fixed_shape: bool = False,
                 compact: bool = False):
        if not (0 <= rank < world):
            raise ValueError(f"rank {rank} of world {world}")
        self.paths, self.batch_size, self.device = list(paths), int(batch_size), torch.device(device)
        self.rank, self.world, self.prefetch, self.drop_last = rank, world, max(1, int(prefetch)), drop_last
        self.workers = max(1, int(workers))
        self.shards = [Shard(p) for p in self.paths]
        # fixed_shape: every batch padded on the host to the common shape of this rank's batches (padding.fixed_shape) and
        # handed over as a PackedBatch; short tail batches are dropped (the static buffers hold exactly batch_size molecules)
        self._pinned: list = []                          # (pinned staging buffer, event of its last host-to-device copy)
        self._landing: list = []
        self._consumed: list = []                        # per landing buffer: the consumer's stream has passed its last use
        self._copy_stream = None
        _LOADERS.add(self)
        self.shape = None
        # compact (with fixed_shape): batches travel in the compact wire form (collate_compact) and come out as CompactBatch
        self.compact = bool(compact)
        if self.compact and not fixed_shape:
            raise ValueError("the compact wire form is a fixed-shape form: fixed_shape=True is required")
        if self.compact and not all(sh.compact_ok for sh in self.shards):
            raise ValueError("a shard's bonds do not allow the compact wire form")
        if fixed_shape:
            from .padding import fixed_shape as _fixed_shape
            self.drop_last = True
            work = self.plan()
            if not work:
                raise ValueError("no full batch for this rank")
            self.shape = _fixed_shape([self.shards[si].degree_histogram(m0, m1) for si, m0, m1 in work])

    def close(self) -> None:
        """Drop the pinned staging and device landing buffers (they are re-made on the next epoch)."""
        if self._copy_stream is not None:
            try:
                self._copy_stream.synchronize()          # no copy may still be reading a pinned buffer that is about to go
            except Exception:                            # (interpreter shutdown: the runtime may be gone already)
                pass
        self._pinned, self._landing, self._consumed = [], [], []

    def plan(self) -> List[tuple]:
        """``(shard index, m0, m1)`` of this rank's batches, in order."""
        out, k = [], 0
        for si, sh in enumerate(self.shards):
            for m0 in range(0, sh.n_molecules, self.batch_size):
                m1 = min(m0 + self.batch_size, sh.n_molecules)
                if self.drop_last and m1 - m0 < self.batch_size:
                    continue
                if k % self.world == self.rank:
                    out.append((si, m0, m1))
                k += 1
        return out

    def __len__(self):
        return len(self.plan())

    def __iter__(self) -> Iterator[GraphBatch]:
        work = self.plan()
        if self.device.type != "cuda":
            for si, m0, m1 in work:
                if self.shape is None:
                    yield collate(self.shards[si], m0, m1, self.device)
                else:
                    sh = self.shards[si]
                    layout, fill, make = (compact_layout, collate_compact, CompactBatch) if self.compact else \
                        (padded_layout, collate_padded, PackedBatch)
                    _, total = layout(self.shape, m1 - m0, sh.x_dim, sh.p_dim, sh.e_dim)
                    flat = torch.empty(total, dtype=torch.uint8)
                    fill(sh, m0, m1, self.shape, flat.numpy())
                    yield make(flat, self.shape, m1 - m0)
            return
        from concurrent.futures import ThreadPoolExecutor
        # One copy stream for the loader's life, and every buffer keeps the event that guards its reuse ACROSS epochs: a
        # pinned staging buffer the event of its last host-to-device copy, a landing buffer the event the consumer's stream
        # recorded after its last use.  (A fresh stream and forgotten events per epoch let a new epoch's workers overwrite
        # buffers whose copies -- or whose consumer -- of the previous epoch's tail had not run yet whenever the GPU lagged
        # the host by a batch or more.)
        if getattr(self, "_copy_stream", None) is None:
            self._copy_stream = torch.cuda.Stream(device=self.device)
        copy_stream = self._copy_stream
        depth = self.prefetch + self.workers
        free: Queue = Queue()                            # pinned staging buffers with the event of their last copy
        for k in range(depth + 1):                       # (kept across epochs: pinning memory costs milliseconds)
            free.put(self._pinned[k] if k < len(self._pinned) else (None, None))
        self._pinned = []
        # fixed-shape batches land in a ring of device buffers that is allocated once: a fresh device tensor per batch
        # would have the allocator wait for (or grow past) blocks the consumer's stream has not released yet.  A landing
        # buffer is reused only after the consumer's stream has passed the use of the batch it held (event recorded when
        # the consumer asks for the next batch), so a batch's ``flat`` is valid until the loader has handed out
        # ``prefetch + workers + 1`` more batches.
        K = depth + 2
        if len(self._landing) != K:
            self._landing = [None] * K
            self._consumed = [None] * K
        consumed = self._consumed

        def stage(i, si, m0, m1):
            staging, last = free.get()
            if last is not None:
                last.synchronize()                       # the buffer's previous copy has left the host
            with torch.cuda.device(self.device):
                if self.shape is None:
                    b = collate(self.shards[si], m0, m1, self.device, staging, copy_stream)
                else:
                    sh = self.shards[si]
                    layout, fill, make = (compact_layout, collate_compact_native, CompactBatch) if self.compact else \
                        (padded_layout, collate_padded, PackedBatch)
                    _, total = layout(self.shape, m1 - m0, sh.x_dim, sh.p_dim, sh.e_dim)
                    if staging is None or staging.numel() < total:
                        staging = torch.empty(total, dtype=torch.uint8, pin_memory=True)
                    fill(sh, m0, m1, self.shape, staging.numpy())
                    k = i % K
                    if self._landing[k] is None or self._landing[k].numel() < total:
                        self._landing[k] = torch.empty(total, dtype=torch.uint8, device=self.device)
                    with torch.cuda.stream(copy_stream):
                        if consumed[k] is not None:
                            copy_stream.wait_event(consumed[k])
                        dst = self._landing[k][:total]
                        dst.copy_(staging[:total], non_blocking=True)
                        b = make(dst, self.shape, m1 - m0)
                    b._staging, b._slot = staging, k
                ev = torch.cuda.Event()
                ev.record(copy_stream)
            return b, ev

        with ThreadPoolExecutor(self.workers) as pool:   # (numpy's slice copies release the GIL: the workers overlap)
            pending = []
            it = iter(enumerate(work))
            for i, w in it:
                pending.append(pool.submit(stage, i, *w))
                if len(pending) >= depth:
                    break
            while pending:
                b, ev = pending.pop(0).result()
                nxt = next(it, None)
                if nxt is not None:
                    pending.append(pool.submit(stage, nxt[0], *nxt[1]))
                cur = torch.cuda.current_stream(self.device)
                cur.wait_event(ev)
                slot = getattr(b, "_slot", None)
                if slot is None:                         # (per-batch device tensors: keep the allocator informed)
                    for v in b.__dict__.values():
                        if torch.is_tensor(v) and v.is_cuda:
                            v.record_stream(cur)
                free.put((b._staging, ev))
                self._pinned = [(t, e) for t, e in self._pinned if t is not b._staging] + [(b._staging, ev)]
                yield b
                if slot is not None:                     # the consumer has enqueued its use of the landing buffer
                    done = torch.cuda.Event()
                    done.record(torch.cuda.current_stream(self.device))
                    consumed[slot] = done


def classify_x_columns(x) -> np.ndarray:
    """``bool[x_dim]``: column ``c`` of ``x`` (float32 ``[A, x_dim]``) is a BYTE column iff every value ``v`` in it is an integer
    (``v == rint(v)``: NaN fails), lies in ``[-128, 127]`` (the infinities fail) and is not ``-0.0`` (bits ``0x80000000``: an int8
    zero would come back as ``+0.0``).  Such a column survives the trip through int8 bit for bit; any other stays fp32."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    if x.ndim != 2:
        raise ValueError("x must be [atoms, x_dim]")
    ok = (x == np.rint(x)) & (x >= -128.0) & (x <= 127.0) & (x.view(np.uint32) != 0x80000000)
    return ok.all(axis=0)


def packed_x_layout(byte_cols):
    """``(x_col int32[x_dim], rec_bytes)`` of the packed record for the byte-column mask ``byte_cols``: first the ``nf`` fp32
    columns in column order, then the ``nq`` int8 columns in column order, then zero bytes to a multiple of 4
    (``rec_bytes = 4 nf + 4 ceil(nq / 4)``).  ``x_col[c] >= 0``: fp32 at that byte offset; ``x_col[c] < 0``: int8 at byte offset
    ``-x_col[c] - 1``."""
    byte_cols = np.asarray(byte_cols, dtype=bool).reshape(-1)
    nq = int(byte_cols.sum())
    nf = int(byte_cols.shape[0]) - nq
    x_col = np.empty(byte_cols.shape[0], dtype=np.int32)
    x_col[~byte_cols] = 4 * np.arange(nf, dtype=np.int32)
    x_col[byte_cols] = -(4 * nf + np.arange(nq, dtype=np.int32)) - 1
    return x_col, 4 * nf + 4 * ((nq + 3) // 4)


def pack_x(x, byte_cols=None):
    """``(records uint8[A, rec_bytes], x_col)``: ``x`` with its byte columns (``classify_x_columns``; or a GIVEN mask ``byte_cols``,
    e.g. to pack the shards of one library alike -- a column forced to byte that does not pass the rule raises) held as int8 and
    the others as fp32, one contiguous record per atom (``packed_x_layout``).  Together with ``unpack_x`` the definition of what
    ``mkgnn_gather_compact_packed`` decodes."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    fits = classify_x_columns(x)
    if byte_cols is None:
        byte_cols = fits
    else:
        byte_cols = np.asarray(byte_cols, dtype=bool).reshape(-1)
        if byte_cols.shape[0] != x.shape[1]:
            raise ValueError(f"byte_cols has {byte_cols.shape[0]} entries, x has {x.shape[1]} columns")
        bad = np.nonzero(byte_cols & ~fits)[0]
        if bad.size:
            raise ValueError(f"columns {bad.tolist()} hold values that an int8 does not carry bit for bit")
    x_col, rec_bytes = packed_x_layout(byte_cols)
    nf = int((~byte_cols).sum())
    nq = x.shape[1] - nf
    records = np.zeros((x.shape[0], rec_bytes), dtype=np.uint8)
    records[:, :4 * nf] = np.ascontiguousarray(x[:, ~byte_cols]).view(np.uint8).reshape(x.shape[0], 4 * nf)
    records[:, 4 * nf:4 * nf + nq] = x[:, byte_cols].astype(np.int8).view(np.uint8)
    return records, x_col


def unpack_x(records, x_col, x_dim: int) -> np.ndarray:
    """``float32[A, x_dim]`` out of packed records: fp32 columns bit for bit, int8 columns converted."""
    records = np.ascontiguousarray(records, dtype=np.uint8)
    x_col = np.asarray(x_col, dtype=np.int64).reshape(-1)
    if x_col.shape[0] != x_dim:
        raise ValueError(f"the column table has {x_col.shape[0]} entries for x_dim {x_dim}")
    out = np.empty((records.shape[0], x_dim), dtype=np.float32)
    for c, e in enumerate(x_col.tolist()):
        if e >= 0:
            out[:, c] = np.ascontiguousarray(records[:, e:e + 4]).view(np.float32)[:, 0]
        else:
            out[:, c] = records[:, -e - 1].view(np.int8)
    return out


class ResidentShard:
    """One ``compact_ok`` shard held in device memory in the layout of ``mkgnn_resident_shard``: features and coordinates as
    they are, every bond once (the even-indexed directed edges) as shard-global int32 endpoints with uint8 attributes, labels,
    per-molecule atom / bond pointers and per-degree atom counts.  ``padding.CompactStaticBatch.gather`` forms a batch from
    ANY list of its molecules on the device (``mkgnn_gather_compact``), so the only per-batch traffic from the host is the
    id list.  The host keeps the per-molecule counts (``mol_atoms``, ``mol_bonds``, ``mol_deg``) for planning and ``y`` for a
    sampler: ``sampling.oversampling_sampler(resident.y, seed)``.  With ``device="cpu"`` nothing is uploaded (the loader's CPU
    path gathers with ``gather_compact``).

    ``packed=True`` holds ``x`` as packed records (``pack_x``: the columns whose values are byte-sized integers over the whole
    shard as int8, the others as fp32) in the layout of ``mkgnn_resident_shard_packed``; the gather decodes them
    (``mkgnn_gather_compact_packed``) into the same wire bytes, so everything downstream is unchanged.  ``x_col``, ``rec_bytes``
    and ``byte_columns`` (the column numbers held as int8) say what was done, ``byte_cols`` forces a mask (``pack_x``), and
    ``nbytes()`` is the device footprint of this form.  The host-side records stay in ``x_rec`` (on the CPU, too, where the loader
    still gathers from the shard itself).

    ``assays`` (a list of assay ids: the tasks of a mixed-assay model, in output order) keeps ``task`` -- every molecule's task
    index on the host, ``sampling.task_index(shard.assay_id, assays)`` -- and uploads it as ``tensors["task"]`` (int32 ``[M]``):
    ``CompactStaticBatch.gather`` hands it to the batch as the task table of the masked multi-task loss.

    ``weights`` (a float ``[M]`` tensor or array: one loss weight per molecule -- importance weights that undo an oversampling
    draw, label confidence, down-weighted inactives) is kept as ``weight`` (float32, on the host) and uploaded as
    ``tensors["weight"]``: ``CompactStaticBatch.gather`` hands it to the batch as the weight table of the weighted loss.

    ``labels`` (a float ``[M, T]`` tensor or array, NaN for "not measured": the label matrix of a multi-label model, every molecule
    once with all its assays) is kept as ``labels`` (float32, on the host) and uploaded as ``tensors["labels"]``:
    ``CompactStaticBatch.gather`` hands it to the batch as the label table of ``readout.label_head_loss``.  Not together with
    ``assays``: a molecule names one task, or carries a row of labels."""

    def __init__(self, shard_or_path, device="cpu", packed: bool = False, byte_cols=None, assays=None, weights=None, labels=None):
        sh = shard_or_path if isinstance(shard_or_path, Shard) else Shard(str(shard_or_path))
        if not sh.compact_ok:
            raise ValueError(f"{sh.path}: bonds are not reversed pairs with shared byte-valued attributes: no compact form")
        if int(sh.mol_deg_ptr[-1, 4]):
            raise ValueError(f"{sh.path}: {int(sh.mol_deg_ptr[-1, 4])} atoms of degree 0 or > 4 are in no bucket")
        self.shard, self.device = sh, torch.device(device)
        self.n_molecules, self.x_dim, self.p_dim, self.e_dim = sh.n_molecules, sh.x_dim, sh.p_dim, sh.e_dim
        self.mol_atoms = np.diff(sh.mol_atom_ptr)
        self.mol_bonds = np.diff(sh.mol_edge_ptr) // 2
        self.mol_deg = np.ascontiguousarray(np.diff(sh.mol_deg_ptr, axis=0)[:, :4])
        self.y = torch.from_numpy(np.array(sh.y))
        self.tensors, self.view = {}, None
        # assays: every molecule's task, the position of its assay_id in the list (-1: not listed) -- sampling.task_index
        self.assays, self.task = None, None
        if assays is not None:
            from .sampling import task_index
            self.assays = tuple(int(a) for a in assays)
            self.task = task_index(torch.from_numpy(np.array(sh.assay_id)), self.assays)
        self.weight = None
        if weights is not None:
            self.weight = torch.as_tensor(np.asarray(weights) if not torch.is_tensor(weights) else weights.detach().cpu()) \
                .reshape(-1).to(torch.float32).contiguous()
            if self.weight.numel() != sh.n_molecules:
                raise ValueError(f"weights holds {self.weight.numel()} entries for {sh.n_molecules} molecules")
        self.labels = None
        if labels is not None:
            if assays is not None:
                raise ValueError("labels (a label matrix) and assays (one task per molecule) exclude each other")
            self.labels = torch.as_tensor(np.asarray(labels) if not torch.is_tensor(labels) else labels.detach().cpu()) \
                .to(torch.float32).contiguous()
            if self.labels.dim() != 2 or self.labels.shape[0] != sh.n_molecules or self.labels.shape[1] < 1:
                raise ValueError(f"labels must be [{sh.n_molecules}, T], not {tuple(self.labels.shape)}")
        self.packed = bool(packed)
        self.x_col = self.x_rec = self.rec_bytes = self.byte_columns = None
        if byte_cols is not None and not self.packed:
            raise ValueError("byte_cols is the column mask of the packed form: packed=True is required")
        if self.packed:
            from . import _lib
            if sh.x_dim > _lib.PACKED_MAX_X_DIM:
                raise ValueError(f"{sh.path}: a packed shard holds at most {_lib.PACKED_MAX_X_DIM} feature columns, not {sh.x_dim}")
            self.x_rec, self.x_col = pack_x(sh.x, byte_cols)
            self.rec_bytes = int(self.x_rec.shape[1])
            self.byte_columns = np.nonzero(self.x_col < 0)[0].tolist()
        if self.device.type == "cuda":
            from . import _lib
            host = {"x": sh.x, "p": sh.p, "bond_ij": np.stack([sh.edge_src[0::2], sh.edge_dst[0::2]], axis=1),
                    "bond_attr": sh.edge_attr[0::2].astype(np.uint8), "y": sh.y,
                    "mol_atom_ptr": sh.mol_atom_ptr.astype(np.int32), "mol_bond_ptr": (sh.mol_edge_ptr // 2).astype(np.int32),
                    "mol_deg": self.mol_deg.astype(np.int32)}
            if self.packed:
                del host["x"]
                host["x_rec"] = self.x_rec
            self.tensors = {k: torch.from_numpy(np.array(v)).to(self.device) for k, v in host.items()}     # (np.array: a writable copy of the map)
            self.view = _lib.ResidentShardPackedView() if self.packed else _lib.ResidentShardView()
            for k, t in self.tensors.items():
                setattr(self.view, k, t.data_ptr())
            self.view.n_molecules, self.view.x_dim, self.view.p_dim, self.view.e_dim = sh.n_molecules, sh.x_dim, sh.p_dim, sh.e_dim
            if self.packed:
                self.view.x_col, self.view.rec_bytes = self.x_col.ctypes.data, self.rec_bytes       # (a host pointer: self.x_col lives as long)
            if self.task is not None:                        # (not a field of the view: the gather does not read it)
                self.tensors["task"] = self.task.to(self.device)
            if self.weight is not None:                      # (nor this one)
                self.tensors["weight"] = self.weight.to(self.device)
            if self.labels is not None:                      # (nor this one)
                self.tensors["labels"] = self.labels.to(self.device)

    def nbytes(self) -> int:
        """Bytes of device memory the shard takes (0 for an unpacked shard on the CPU, which uploads nothing; the packed form
        reports its device footprint wherever it is)."""
        if self.packed:
            sh = self.shard
            m, a, nb = sh.n_molecules, sh.n_atoms, sh.n_edges // 2
            return a * self.rec_bytes + 4 * a * sh.p_dim + 8 * nb + nb * sh.e_dim + 4 * m + 2 * 4 * (m + 1) + 16 * m
        return sum(t.numel() * t.element_size() for t in self.tensors.values())


class ResidentLoader:
    """One epoch of batches drawn from a ``ResidentShard`` by an arbitrary index stream ``indices`` (a
    ``WeightedRandomSampler``, a permutation, a tensor ...): the stream is cut into pieces of ``batch_size`` (a short tail is
    dropped, as ``ShardLoader(fixed_shape=True)`` does), pieces ``rank, rank + world, ...`` are this rank's.  Everything is
    planned on the host from the per-molecule counts before anything is launched: ids out of range, every batch's degree
    histogram, the common ``shape`` (``padding.fixed_shape`` over the plan, the four per-degree targets scaled up by
    ``headroom`` before the parity fix; or a GIVEN shape -- e.g. the first epoch's, so that a captured graph survives a new
    draw -- which every batch must fit) and ``max_mol_atoms`` / ``max_mol_edges``, the largest molecule of the plan with the
    padding molecules included (what ``padding.pad_batch`` reports, maximised over the batches).

    The epoch's ids are uploaded once; iterating yields one device int32 view per batch for
    ``padding.CompactStaticBatch.gather``.  On the CPU it yields ``CompactBatch``es filled by ``gather_compact``.

    ``drop_last=False`` (``world == 1`` only) keeps the short tail: the last piece is filled up to ``batch_size`` by repeating
    its last real id, and ``n_live`` (host int32 array; ``n_live_dev``, a device int32 vector, on a GPU) holds every batch's
    count of real molecules.  The filler molecules are planned like any other (shape fit, ``max_mol_atoms``,
    ``max_mol_edges``).  This is for SCORING (``screening.score_resident``): in evaluation mode the batch norm uses its running
    statistics, so a molecule's score does not depend on its neighbours in the batch and the filler cannot change the real
    molecules' scores; the consumer ignores the slots from ``n_live`` on.  In training the filler would enter the batch
    statistics and the loss a second time, which is why a training draw drops the tail (the default)."""

    def __init__(self, resident: ResidentShard, batch_size: int, indices, device="cpu", rank: int = 0, world: int = 1,
                 shape=None, headroom: float = 0.0, drop_last: bool = True):
        if not (0 <= rank < world):
            raise ValueError(f"rank {rank} of world {world}")
        if not drop_last and world != 1:
            raise ValueError("drop_last=False keeps the tail of ONE stream of batches: it exists for world == 1")
        self.drop_last = bool(drop_last)
        if headroom < 0:
            raise ValueError("headroom is a non-negative fraction")
        self.resident, self.batch_size, self.device = resident, int(batch_size), torch.device(device)
        self.rank, self.world, self.headroom = rank, world, float(headroom)
        self.shape = None if shape is None else dict(shape)
        self._ids_host = self._ids_dev = None
        self.set_epoch(indices)

    def set_epoch(self, indices) -> None:
        """Plan a new epoch from a new index stream; ``shape`` is kept (a batch that does not fit it raises)."""
        from .padding import PAD_MOLECULES, fixed_shape
        r, bs = self.resident, self.batch_size
        ids = np.asarray(indices.tolist() if torch.is_tensor(indices) else list(indices), dtype=np.int64).reshape(-1)
        if ids.size and (int(ids.min()) < 0 or int(ids.max()) >= r.n_molecules):
            raise ValueError(f"molecule ids outside [0, {r.n_molecules})")
        n_all, tail = divmod(ids.shape[0], bs)
        if tail and not self.drop_last:                                         # the tail, filled up with its last real id
            ids = np.concatenate([ids, np.full(bs - tail, ids[-1], dtype=np.int64)])
            n_all += 1
        else:
            tail = 0
        batches = ids[:n_all * bs].reshape(n_all, bs)[self.rank::self.world]
        if batches.shape[0] == 0:
            raise ValueError("no full batch for this rank")
        self.n_live = np.full(batches.shape[0], bs, dtype=np.int32)
        if tail:
            self.n_live[-1] = tail
        atoms = r.mol_atoms[batches].sum(axis=1)
        deg = r.mol_deg[batches].sum(axis=1)                                    # [batches, 4]
        if self.shape is None:
            shape = fixed_shape([[int(a), *map(int, d), 0] for a, d in zip(atoms, deg)])
            if self.headroom > 0:
                t = [int(np.ceil(shape[f"n{k}"] * (1.0 + self.headroom))) for k in range(1, 5)]
                if sum((k + 1) * t[k] for k in range(4)) % 2:
                    t[0] += 1
                shape = {"n1": t[0], "n2": t[1], "n3": t[2], "n4": t[3], "atoms": sum(t), "edges": sum((k + 1) * t[k] for k in range(4))}
            self.shape = shape
        target = np.array([self.shape[f"n{k}"] for k in range(1, 5)], dtype=np.int64)
        need = target[None, :] - deg
        if self.shape["atoms"] != int(target.sum()) or self.shape["edges"] != int((target * np.arange(1, 5)).sum()) or self.shape["edges"] % 2:
            raise ValueError(f"the shape {self.shape} is not a bucket shape (padding.fixed_shape)")
        short = np.nonzero((need < 0).any(axis=1))[0]
        if short.size:
            k = int(short[0])
            raise ValueError(f"batch {k} of this rank's plan, with degree histogram {deg[k].tolist()}, does not fit the shape {self.shape}")
        # the largest molecule of the plan, padding molecules included (padding.pad_batch's figures, maximised): the padding atoms
        # come in degree order and are dealt to the padding molecules in runs; an atom of degree d has d edges each way
        pad_atoms = pad_edges = 0
        for nd in {tuple(row) for row in need.tolist()}:
            n_pad = sum(nd)
            if n_pad:
                mol = (np.arange(n_pad, dtype=np.int64) * PAD_MOLECULES) // n_pad
                deg_of = np.repeat(np.arange(1, 5), nd)
                pad_atoms = max(pad_atoms, int(np.bincount(mol).max()))
                pad_edges = max(pad_edges, int(np.bincount(mol, weights=deg_of).max()))
        self.max_mol_atoms = max(int(r.mol_atoms[batches].max()), pad_atoms)
        self.max_mol_edges = max(2 * int(r.mol_bonds[batches].max()), pad_edges)
        self._batches = batches
        self._ids_dev = self.n_live_dev = None
        if self.device.type == "cuda":
            self.n_live_dev = torch.from_numpy(self.n_live).to(self.device, non_blocking=True)
            # (through pinned memory, without waiting: the host plans the next epoch while the device still works on this one)
            self._ids_host = torch.from_numpy(batches.astype(np.int32)).pin_memory()
            self._ids_dev = self._ids_host.to(self.device, non_blocking=True)

    def plan(self) -> np.ndarray:
        """This rank's batches, in order: ``[batches, batch_size]`` molecule ids."""
        return self._batches

    def __len__(self):
        return int(self._batches.shape[0])

    def __iter__(self):
        if self._ids_dev is not None:
            for k in range(len(self)):
                yield self._ids_dev[k]
            return
        sh = self.resident.shard
        _, total = compact_layout(self.shape, self.batch_size, sh.x_dim, sh.p_dim, sh.e_dim)
        for row in self._batches:
            flat = torch.empty(total, dtype=torch.uint8)
            gather_compact(sh, row, self.shape, flat.numpy())
            yield CompactBatch(flat, self.shape, self.batch_size)


def write_shards(directory: str, batches: Iterable[GraphBatch], prefix: str = "shard") -> List[str]:
    """One shard per collated batch of ``batches`` (e.g. a few hundred thousand molecules each); returns the paths."""
    os.makedirs(directory, exist_ok=True)
    paths = []
    for i, b in enumerate(batches):
        path = os.path.join(directory, f"{prefix}-{i:05d}.mkgs")
        write_shard(path, b)
        paths.append(path)
    return paths
