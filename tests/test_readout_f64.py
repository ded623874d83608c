"""The separate readout operators -- ``readout()`` / ``_ReadoutFn`` (``mkgnn_readout_forward`` / ``_backward``) and
``readout_blocks()`` / ``_ReadoutBlocksFn`` (``mkgnn_readout_blocks_forward`` / ``_backward``), what a training step runs when the
fused tail declines a batch -- against float64 at every grid cap, width boundary, alignment and molecule-size edge of
``csrc/kgnn_readout.hip``.  Rows, references and the predicates that prove a row reaches its edge: ``tests/_readout_f64.py``
(pinned without a GPU by ``tests/test_readout_reference_cpu.py``).  ``pytest -m gpu``.

Bound: ``tests/_f64.check`` with its constants as they stand, the yardstick being the reference's own float32 leg; applied per
tensor AND per slice (a degree's column block of grad W1 / grad sim, the rows of the last partial 16-atom tile, the first and
last molecule's output rows), so an edge element cannot hide under an unrelated maximum.
"""
import pytest
import torch

from tests import _f64 as F64
from tests import _readout_f64 as RF
from tests import _topologies as T

pytestmark = pytest.mark.gpu


def _dev():
    assert torch.cuda.is_available(), "pytest -m gpu needs the MI355X"
    return torch.device("cuda:0")


def _padded_rows(t: torch.Tensor, dev) -> torch.Tensor:
    """``t`` [n, W] as the leading W columns of NaN-filled 16-byte rows [n, W4] on the device: nothing may read the padding."""
    n, W = t.shape
    store = torch.full((n, W + (-W) % 4), float("nan"))
    store[:, :W] = t
    return store.to(dev)[:, :W]


def _linear(w, b, dev) -> torch.nn.Linear:
    lin = torch.nn.Linear(w.shape[1], w.shape[0], bias=b is not None)
    with torch.no_grad():
        lin.weight.copy_(w)
        if b is not None:
            lin.bias.copy_(b)
    return lin.to(dev)


def _molecule_slices(sizes):
    """(name, row) of the first and the last molecule, and of the first and last molecule that has atoms."""
    full = [m for m, s in enumerate(sizes) if s > 0]
    return {"first": 0, "last": len(sizes) - 1, "first_with_atoms": full[0], "last_with_atoms": full[-1]}


def _finite(tag, **tensors):
    for nm, t in tensors.items():
        if t is not None:
            assert bool(torch.isfinite(t).all()), (tag, nm, "NaN / inf: poisoned padding or an unwritten buffer was read")


def _sliced(d, key, name, index):
    """Add ``d[key][index]`` to the dict under ``name`` (the per-slice leg of the bound)."""
    if key in d and d[key] is not None:
        d[name] = d[key][index]


# ------------------------------------------------------------------------------------------ dense readout --
def _run_dense(name, bias, keep):
    from molkgnn_amd import readout as R
    dev = _dev()
    c = RF.DENSE_CASES[name]
    assert R.readout_supported(c.F, c.H, c.G)
    i = RF.dense_inputs(name, bias, keep)
    f32, f64 = (dict(d) for d in RF.dense_reference(name, bias, keep))      # (copies: the slices below are added to them)
    tag = f"dense:{name}:bias{int(bias)}:keep{int(keep)}"
    n, size = i["h"].shape[0], i["size"]
    lin1, lin2 = _linear(i["w1"], i["b1"], dev), _linear(i["w2"], i["b2"], dev)
    keep_d = None if i["keep"] is None else i["keep"].to(dev)
    batch_d, cot = i["batch"].to(dev), i["cot"].to(dev)
    seg = R.molecule_segments(batch_d, size)
    assert seg.sorted
    sizes = RF.T.molecule_sizes(RF.batch(c.mols))

    def run(h_grad):
        h = _padded_rows(i["h"], dev).requires_grad_(h_grad)
        out = R._ReadoutFn.apply(h, lin1.weight, lin1.bias, lin2.weight, lin2.bias, keep_d, seg)
        pooled = out.grad_fn.saved_tensors[-1]
        leaves = ([h] if h_grad else []) + [p for p in (lin1.weight, lin1.bias, lin2.weight, lin2.bias) if p is not None]
        grads = torch.autograd.grad((out * cot).sum(), leaves)
        names = (["h"] if h_grad else []) + [nm for nm, p in zip(("w1", "b1", "w2", "b2"), (lin1.weight, lin1.bias, lin2.weight, lin2.bias))
                                             if p is not None]
        return dict(zip(names, grads), out=out.detach()), pooled, h

    got, pooled, h = run(True)
    torch.cuda.synchronize()
    _finite(tag, pooled=pooled, **got)
    assert got["h"].shape == (n, c.F) and got["w1"].shape == (c.H, c.F) and got["out"].shape == (size, c.G)
    # through the module-level entry point (its dispatch on the path): the same launches, the same bits
    if keep_d is None:
        with torch.no_grad():
            assert torch.equal(R.readout(h.detach(), lin1, lin2, torch.nn.Dropout(0.25).eval(), batch_d, size), got["out"]), tag
            assert torch.equal(R.readout(h.detach(), lin1, lin2, None, batch_d, size, segments=seg), got["out"]), tag
    # an input that needs no gradient (grad_h == nullptr): the parameter gradients to the bit
    got_ng, _, _ = run(False)
    for nm, t in got_ng.items():
        assert torch.equal(t, got[nm]), (tag, nm, "changes when h needs no gradient")
    # an empty molecule: output row and pooled row exactly zero
    for m, s in enumerate(sizes):
        if s == 0:
            assert float(got["out"][m].abs().max()) == 0.0 and float(pooled[m].abs().max()) == 0.0, (tag, "empty molecule", m)
    # the bound, per tensor and per slice
    ms = _molecule_slices(sizes)
    last_tile = slice(RF.TILE * ((n - 1) // RF.TILE), n)
    for d in (got, f32, f64):
        for nm, m in ms.items():
            _sliced(d, "out", f"out[{nm} molecule]", m)
        _sliced(d, "h", "h[last tile]", last_tile)
        _sliced(d, "h", "h[first tile]", slice(0, min(n, RF.TILE)))
        _sliced(d, "w1", "w1[last column]", (slice(None), slice(c.F - 1, c.F)))
        _sliced(d, "w1", "w1[last row]", slice(c.H - 1, c.H))
    assert F64.check(got, f32, f64, tag) >= 10


@pytest.mark.parametrize("keep", [False, True], ids=["nokeep", "keep"])
@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("name", [c.name for c in RF.DENSE_WIDTHS])
def test_dense_readout_widths(name, bias, keep):
    """(F, H, G) on both sides of NU, HP / groups and at G = 1 | 64; h stored [n, F4] with NaN padding; with and without biases,
    dropout multipliers and an input gradient."""
    _run_dense(name, bias, keep)


@pytest.mark.parametrize("full", [False, True], ids=["plain", "bias+keep"])
@pytest.mark.parametrize("name", [c.name for c in RF.DENSE_SIZES if not c.name.startswith("many_small")])
def test_dense_readout_sizes(name, full):
    """Atom counts around the 16-atom tile, the molecule-size edges (empty, one atom, 7 8 9, 15 16 17, 300) and slab counts
    1, 7, 8, 9 of the fixed-order reduction."""
    _run_dense(name, full, full)


@pytest.mark.parametrize("name", ["many_small_h20", "many_small_h40"])
def test_dense_readout_past_every_grid_cap(name):
    """10 000 molecules of 4 .. 8 atoms, 67 500 atoms: the grid-stride loops of the pre, pool, atoms and molecule kernels all take
    more than one round, the MC chunk loop iterates and the reduction sums 256 slabs."""
    _run_dense(name, True, True)


# -------------------------------------------------------------------------------------- block-row readout --
def _run_blocks(name, H, full):
    from molkgnn_amd import readout as R
    from molkgnn_amd.plan import plan_from_data
    dev = _dev()
    c = RF.BLOCK_CASES[name]
    i = RF.block_inputs(name, H, full)
    f32, f64 = RF.block_reference(name, H, full)
    tag = f"blocks:{name}:H{H}:full{int(full)}"
    counts, K, G = c.counts, sum(c.counts), i["G"]
    assert R.readout_blocks_supported(K, H, G, counts)
    b = RF.batch(c.mols)
    bd = b.to(dev)
    plan = plan_from_data(bd)
    n, size = i["sim"].shape[0], i["size"]
    mask = i["mask"]
    lin1, lin2 = _linear(i["w1"], i["b1"], dev), _linear(i["w2"], i["b2"], dev)
    keep_d = None if i["keep"] is None else i["keep"].to(dev)
    cot = i["cot"].to(dev)
    seg = R.molecule_segments(bd.batch, size)
    assert seg.sorted
    sizes = RF.T.molecule_sizes(b)
    # NaN everywhere outside every atom's own block, and in the alignment padding
    stored = torch.where(mask, i["sim"], torch.full((), float("nan")))

    def run(sim_grad):
        sim = _padded_rows(stored, dev).requires_grad_(sim_grad)
        out = R._ReadoutBlocksFn.apply(sim, lin1.weight, lin1.bias, lin2.weight, lin2.bias, keep_d, seg, plan, tuple(counts))
        pooled = out.grad_fn.saved_tensors[-1]
        params = [p for p in (lin1.weight, lin1.bias, lin2.weight, lin2.bias) if p is not None]
        grads = torch.autograd.grad((out * cot).sum(), ([sim] if sim_grad else []) + params)
        names = (["sim"] if sim_grad else []) + [nm for nm, p in zip(("w1", "b1", "w2", "b2"), (lin1.weight, lin1.bias, lin2.weight, lin2.bias))
                                                 if p is not None]
        return dict(zip(names, grads), out=out.detach()), pooled, sim

    got, pooled, sim = run(True)
    torch.cuda.synchronize()
    # inference (gsum == nullptr: pre is not overwritten with the gate): the same output bit for bit, also through the wrapper
    with torch.no_grad():
        out_ng = R._ReadoutBlocksFn.apply(sim, lin1.weight, lin1.bias, lin2.weight, lin2.bias, keep_d, seg, plan, tuple(counts))
        assert torch.equal(out_ng, got["out"]), (tag, "no_grad output differs")
        if keep_d is None:
            assert torch.equal(R.readout_blocks(sim, plan, counts, lin1, lin2, torch.nn.Dropout(0.25).eval(), seg), got["out"]), tag
    got_ng, _, _ = run(False)
    for nm, t in got_ng.items():
        assert torch.equal(t, got[nm]), (tag, nm, "changes when sim needs no gradient")
    gsim = got.pop("sim").cpu()
    assert gsim.shape == (n, K) and got["w1"].shape == (H, K)          # (a degree with L_d = 0 has no columns)
    _finite(tag, pooled=pooled, **got)
    assert bool(torch.isfinite(gsim[mask]).all()), (tag, "grad sim inside the blocks")
    for m, s in enumerate(sizes):
        if s == 0:
            assert float(got["out"][m].abs().max()) == 0.0 and float(pooled[m].abs().max()) == 0.0, (tag, "empty molecule", m)
    # the bound, per tensor and per slice
    deg = RF.bucket_of_atom(c.mols)
    legs = ({k: v.cpu() for k, v in got.items()}, dict(f32), dict(f64))
    for d in legs:
        d.pop("h_value", None)
    ref_sims = (gsim, f32["sim"], f64["sim"])
    for d, s in zip(legs, ref_sims):
        d.pop("sim", None)
        off = 0
        for k in range(1, 5):
            L = counts[k - 1]
            sel = getattr(b, f"selected_index_deg{k}")
            cols = slice(off, off + L)
            if L > 0:
                d[f"w1[degree {k}]"] = d["w1"][:, cols]
                if sel.numel():
                    d[f"sim[degree {k}]"] = s[sel][:, cols]
                    d[f"sim[degree {k}, last tile]"] = s[sel[RF.TILE * ((sel.numel() - 1) // RF.TILE):]][:, cols]
                    d[f"sim[degree {k}, last column]"] = s[sel][:, off + L - 1:off + L]
            off += L
        for nm, m in _molecule_slices(sizes).items():
            _sliced(d, "out", f"out[{nm} molecule]", m)
    # a degree with kernels but no atoms: its columns of grad W1 are exactly zero
    off = 0
    for k in range(1, 5):
        if counts[k - 1] > 0 and int((deg == k).sum()) == 0:
            assert float(got["w1"][:, off:off + counts[k - 1]].abs().max()) == 0.0, (tag, "absent degree", k)
        off += counts[k - 1]
    assert F64.check(legs[0], legs[1], legs[2], tag) >= 8


@pytest.mark.parametrize("full", [False, True], ids=["plain", "bias+keep"])
@pytest.mark.parametrize("name,H", [(c.name, H) for c in RF.BLOCK_CASES_LIST if len(c.hidden) > 1 for H in c.hidden])
def test_block_row_readout_edges(name, H, full):
    """Kernel counts for every alignment of a block's first column, partial last chunks, L = 1 .. 64, absent degrees on either
    side (atoms without kernels, kernels without atoms), atoms in no bucket with up to nine neighbours, a batch that needs no
    memset of z; sim stored [n, K4] with NaN outside every atom's own block."""
    _run_blocks(name, H, full)


@pytest.mark.parametrize("name,H", [(c.name, c.hidden[0]) for c in RF.BLOCK_CASES_LIST if len(c.hidden) == 1])
def test_block_row_readout_past_every_grid_cap(name, H):
    """67 500 atoms at H <= 32 and 33 750 at H > 32: more than one tile per wave in the backward projection, the d z gather past
    DZ_BLOCKS, the pool and molecule kernels past their caps."""
    _run_blocks(name, H, True)


@pytest.mark.parametrize("name,H", [("hubs", 5), ("hubs", 32), ("hubs", 33), ("hubs", 64), ("c10_20_30_50", 32), ("all_bucketed", 33)])
def test_block_row_backward_writes_every_dz_row(name, H):
    """``mkgnn_readout_blocks_backward``'s ``dz`` rows (d loss / d z = propagate^T(d pre), an output of the C ABI) for EVERY atom.
    The operator reads them only for atoms in a bucket, and those have at most four neighbours: the serial tail of
    ``readout_dz_gather_kernel`` (a fifth neighbour and beyond) shows nowhere but in the rows of the hubs, so the ABI is called
    directly with a buffer the test owns.  The gradients of that call are the operator's, bit for bit."""
    from molkgnn_amd import _lib
    from molkgnn_amd import readout as R
    from molkgnn_amd.functional import _stride0
    from molkgnn_amd.plan import plan_from_data
    dev = _dev()
    c = RF.BLOCK_CASES[name]
    i = RF.block_inputs(name, H, True)
    f32, f64 = RF.block_reference(name, H, True)
    tag = f"blocks-dz:{name}:H{H}"
    counts, K = c.counts, sum(c.counts)
    b = RF.batch(c.mols)
    bd = b.to(dev)
    plan = plan_from_data(bd)
    n, size = i["sim"].shape[0], i["size"]
    lin1, lin2 = _linear(i["w1"], i["b1"], dev), _linear(i["w2"], i["b2"], dev)
    keep_d, cot = i["keep"].to(dev), i["cot"].to(dev).contiguous()
    seg = R.molecule_segments(bd.batch, size)
    sim = _padded_rows(torch.where(i["mask"], i["sim"], torch.full((), float("nan"))), dev).requires_grad_(True)
    out = R._ReadoutBlocksFn.apply(sim, lin1.weight, lin1.bias, lin2.weight, lin2.bias, keep_d, seg, plan, tuple(counts))
    _, w1, b1, w2, b2, gate, gsum, pooled = out.grad_fn.saved_tensors
    want = torch.autograd.grad((out * cot).sum(), [sim, lin1.weight, lin1.bias, lin2.weight, lin2.bias], retain_graph=True)
    lib = _lib.load()
    hs = gate.shape[1]
    K4 = K + (-K) % 4
    dz = torch.full((n, hs), float("nan"), device=dev)
    gsim = torch.full((n, K4), float("nan"), device=dev)
    gw1, gb1, gw2, gb2 = (torch.full_like(t, float("nan")) for t in (w1, b1, w2, b2))
    rowptr, col = plan.csr_out
    with torch.cuda.device(dev):
        ws_bytes = int(lib.mkgnn_readout_blocks_workspace_bytes(K, H, w2.shape[0], size))
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        _lib.check(lib.mkgnn_readout_blocks_backward(
            R._params(w1, b1, w2, b2), sim.data_ptr(), _stride0(sim), _lib.Int32x4(*counts), R._sel_buckets(plan), n, rowptr.data_ptr(),
            col.data_ptr(), seg.mol_ptr.data_ptr(), seg.atom_mol.data_ptr(), size, gate.data_ptr(), gsum.data_ptr(), pooled.data_ptr(),
            cot.data_ptr(), _stride0(cot), dz.data_ptr(), gsim.data_ptr(), K4, gw1.data_ptr(), gb1.data_ptr(), gw2.data_ptr(),
            gb2.data_ptr(), ws.data_ptr(), ws_bytes, _lib.stream_ptr(dev)), "mkgnn_readout_blocks_backward")
    torch.cuda.synchronize()
    for a, w in zip((gw1, gb1, gw2, gb2), want[1:]):
        assert torch.equal(a, w), (tag, "the direct call is not the operator's backward")
    mask = i["mask"].to(dev)
    assert torch.equal(gsim[:, :K][mask], want[0][mask]), tag
    assert bool(torch.isfinite(dz).all()), (tag, "a d z row was not written")
    assert float(dz[:, H:].abs().max()) == 0.0 if hs > H else True, (tag, "d z beyond H")
    many = T.degrees(b) > 4
    got = {"dz": dz[:, :H].cpu()}
    legs = [got, {"dz": f32["dz"]}, {"dz": f64["dz"]}]
    for d in legs:
        d["dz[atoms in no bucket]"] = d["dz"][RF.bucket_of_atom(c.mols) == 0]
        d["dz[more than four neighbours]"] = d["dz"][many]
    assert c.name != "hubs" or int(many.sum()) == 2
    assert F64.check(*legs, tag) >= (3 if bool(many.any()) else 1)
