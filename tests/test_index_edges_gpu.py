"""The receptive-field builder (kgnn_rf.hip), the plan builder (kgnn_plan.hip) and the one-pass index builder (kgnn_index.hip)
at their dispatch edges, against the torch definitions ``receptive_field.build_receptive_fields`` and the ``BatchPlan`` properties
under ``MKGNN_TORCH_PLAN=1`` -- ``torch.equal`` on integers and on float bit patterns, no tolerance anywhere.

Where the sizes come from:

* the receptive-field passes and every pass of the one-pass builder work on chunks of 256 atoms (one block each; bucket ranks and
  row pointers of a chunk start from the sums over the chunks before it); the plan builder scans in blocks of 2048 elements
  (eight sub-chunks of 256).  So: 1 atom, 255, 256 (exactly one chunk), 257 (a second chunk of one atom), 2048 (eight full
  chunks, exactly one scan block), 2049 (a ninth chunk and a second scan block of one atom) -- built with the isolated atoms IN
  FRONT, so that the last atom is bucketed, has in-edges and sits where the boundary falls.
* the one-pass builder's fill kernel has ``max(atoms, edges)`` threads: mostly isolated atoms (atoms > edges) and the hand-made
  stars and chains of tests/_batch_cases.py (edges > atoms) take one arm each; a batch without an edge launches no edge kernel.
* unit-normalised bond rows ride along for ``E <= 8`` only: E = 1, 8 (the last with), 9 (the first without), 12.
* capacities that differ from the batch are a documented error state: zero rows (atom 0, zero attributes) behind the real ones,
  atoms beyond a capacity dropped in atom order and counted in ``rf_counts[4]``.
"""
import os

import pytest
import torch

from molkgnn_amd.synthetic import make_batch
from tests import _batch_cases as C

pytestmark = pytest.mark.gpu
NAMES = ("selected_index", "nei_index", "p_focal", "nei_p", "nei_edge_attr")


def _dev():
    return torch.device("cuda:0")


def _first_molecules(b, max_atoms):
    """The leading molecules of a collated batch that fit ``max_atoms`` atoms: ``(p, edge_index, edge_attr)``."""
    n_mol = int((torch.bincount(b.batch).cumsum(0) <= max_atoms).sum())
    a = int((b.batch < n_mol).sum())
    keep = b.edge_index[0] < a
    return b.p[:a], b.edge_index[:, keep], b.edge_attr[keep]


def _with_isolated_in_front(n, parts):
    """``n`` atoms: isolated ones first, then the atoms of ``parts`` (edge list shifted); new coordinates for all of them."""
    p, ei, ea = parts
    k = n - p.shape[0]
    assert k >= 0
    g = torch.Generator().manual_seed(n)
    return torch.randn(n, 3, generator=g), (ei + k).contiguous(), ea.contiguous()


def _custom(e_dim):
    b = C.collate(C.molecules(4, 3, e_dim, seed=e_dim))
    return b.p, b.edge_index, b.edge_attr


def _cases():
    """``{name: (p, edge_index, edge_attr)}`` on the host."""
    out = {}
    synth = make_batch(110, seed=31, with_receptive_fields=False)                 # about 2 700 atoms
    few = _first_molecules(synth, 80)
    for n in (255, 256, 257, 2048, 2049):
        out[f"{n} atoms, mostly isolated"] = _with_isolated_in_front(n, few)
    for n in (2048, 2049):                                                        # molecules on both sides of every boundary
        out[f"{n} atoms, dense"] = _with_isolated_in_front(n, _first_molecules(synth, n))
    out["past one scan block"] = (synth.p, synth.edge_index, synth.edge_attr)
    none = (torch.zeros((2, 0), dtype=torch.int64), torch.zeros((0, 7)))
    out["5 atoms, no edge"] = (torch.randn(5, 3, generator=torch.Generator().manual_seed(5)), *none)
    out["1 atom"] = (torch.randn(1, 3, generator=torch.Generator().manual_seed(1)), *none)
    for e_dim in (1, 8, 9, 12):
        out[f"stars and chains, E = {e_dim}"] = _custom(e_dim)
    # the two directions of a bond with DIFFERENT attributes (in this copy only): both take the row of edge 2 * (e // 2)
    p, ei, ea = _custom(8)
    ea = ea.clone()
    ea[1::2] += 1.0
    out["attributes of the odd edges differ"] = (p, ei, ea)
    return out


CASES = _cases()


def _torch_plan(n, lists, edge_index):
    from molkgnn_amd.plan import plan_from_lists
    ref = plan_from_lists(n, *lists, edge_index)
    os.environ["MKGNN_TORCH_PLAN"] = "1"
    try:
        return [ref.scatter, ref.deg8] + ([ref.csr_in, ref.csr_out, ref.csr_in_packed] if edge_index is not None else [])
    finally:
        del os.environ["MKGNN_TORCH_PLAN"]


def _assert_plan(got, want, what):
    assert len(got) == len(want)
    for gi, (gv, wv) in enumerate(zip(got, want)):
        if isinstance(gv, tuple):
            assert torch.equal(gv[0], wv[0]) and torch.equal(gv[1], wv[1]), (what, gi)
        else:
            assert torch.equal(gv, wv), (what, gi)


def _unit_rows(raw, E):
    from molkgnn_amd import _lib
    raw = raw.reshape(-1, E).contiguous()
    unit = torch.empty((raw.shape[0], 8), dtype=torch.float32, device=raw.device)
    _lib.check(_lib.load().mkgnn_unit_rows8(raw.data_ptr(), raw.shape[0], E, unit.data_ptr(), _lib.stream_ptr(raw.device)), "unit")
    return unit


def _assert_fields(rf, f, sizes, E, what):
    for d in range(1, 5):
        for nm in NAMES:
            got, want = rf[f"{nm}_deg{d}"], f[f"{nm}_deg{d}"]
            assert got.dtype == want.dtype and got.numel() == want.numel(), (what, nm, d)
            assert torch.equal(got.reshape(-1), want.reshape(-1)), (what, nm, d)
            if got.is_floating_point():
                assert torch.equal(got.reshape(-1).view(torch.int32), want.reshape(-1).view(torch.int32)), (what, nm, d)
        unit = rf.get(f"nei_edge_unit_deg{d}")
        if E <= 8 and sizes[d - 1]:
            assert unit is not None and torch.equal(unit.view(torch.int32), _unit_rows(f[f"nei_edge_attr_deg{d}"], E).view(torch.int32)), (what, d)
        else:
            assert unit is None, (what, d)


@pytest.mark.parametrize("name", list(CASES))
def test_builders_equal_the_definitions(name):
    from molkgnn_amd.plan import plan_from_lists
    from molkgnn_amd.receptive_field import build_index_hip, build_receptive_fields, build_receptive_fields_hip, check_sizes
    dev = _dev()
    p, edge_index, edge_attr = (t.to(dev) for t in CASES[name])
    n, m, E = p.shape[0], edge_index.shape[1], edge_attr.shape[1]
    x = torch.zeros((n, 1), device=dev)                     # (the builders read the atom count off x, nothing else)
    f = build_receptive_fields(x, p, edge_index, edge_attr)
    sizes = [int(f[f"selected_index_deg{d}"].numel()) for d in range(1, 5)]
    if m == 0:                                              # the definitions of an edge-free batch: empty fields, zero row pointers
        assert sizes == [0, 0, 0, 0]
    elif "isolated" in name or "dense" in name:             # the last atom is bucketed and has in-edges
        assert int((edge_index[1] == n - 1).sum()) >= 1 and int((edge_index[0] == n - 1).sum()) in (1, 2, 3, 4)
    if "isolated" in name:
        assert n > m
    if name.startswith("stars"):
        assert m > n
    # the receptive-field builder: sizes read back, and sizes given
    _assert_fields(build_receptive_fields_hip(x, p, edge_index, edge_attr), f, sizes, E, (name, "rf"))
    rf = build_receptive_fields_hip(x, p, edge_index, edge_attr, sizes=sizes)
    check_sizes(rf)
    assert rf["rf_counts"].tolist() == sizes
    _assert_fields(rf, f, sizes, E, (name, "rf, sizes given"))
    # the plan builder, with and without the edge list
    lists = [[f[f"{nm}_deg{d}"] for d in range(1, 5)] for nm in ("p_focal", "nei_p", "nei_edge_attr", "selected_index", "nei_index")]
    for ei in (edge_index, None):
        hip = plan_from_lists(n, *lists, ei)
        assert hip.build_hip()
        got = [hip.scatter, hip.deg8] + ([hip.csr_in, hip.csr_out, hip.csr_in_packed] if ei is not None else [])
        want = _torch_plan(n, lists, ei)
        _assert_plan(got, want, (name, "plan", ei is not None))
        if m == 0:
            assert all(int(w[0].abs().sum()) == 0 and w[0].numel() == n + 1 for w in want if isinstance(w, tuple))
    # the one-pass builder
    rf, parts = build_index_hip(x, p, edge_index, edge_attr, sizes)
    check_sizes(rf)
    assert rf["rf_counts"].tolist() == sizes + [0, 0]
    _assert_fields(rf, f, sizes, E, (name, "one pass"))
    got = [parts["scatter"], parts["deg8"], parts["csr_in"], parts["csr_out"], parts["csr_in_packed"]]
    _assert_plan(got, _torch_plan(n, lists, edge_index), (name, "one pass"))


# ---------------------------------------------------------------------------------------------------------------------------
# capacities that differ from the batch, through the C entry points on buffers of the test's own

I64_FILL, GUARD = -7, 5                                      # what every output starts out as (floats: NaN); guard rows behind it


class _Outputs:
    """Per-degree output buffers of ``caps`` rows plus ``GUARD`` rows behind them, every entry a sentinel, and the bucket table
    that points at them."""

    def __init__(self, caps, E, dev):
        from molkgnn_amd import _lib
        self.caps, self.E = list(caps), E
        self.buckets = _lib.Buckets4()
        self.t = {}
        for d in range(1, 5):
            rows = caps[d - 1] + GUARD
            i64 = lambda *s: torch.full(s, I64_FILL, dtype=torch.int64, device=dev)                    # noqa: E731
            f32 = lambda *s: torch.full(s, float("nan"), dtype=torch.float32, device=dev)               # noqa: E731
            t = {"selected_index": i64(rows, 1), "nei_index": i64(rows, d), "nei_edge_attr": f32(rows, d * E), "p_focal": f32(rows, 3),
                 "nei_p": f32(rows, d * 3), "nei_edge_unit": f32(rows, d * 8) if E <= 8 else None}
            self.t[d] = t
            b = self.buckets[d - 1]
            b.count = caps[d - 1]
            for k, v in t.items():
                setattr(b, k, _lib.ptr(v))

    def rows(self, d, k, lo, hi):
        return self.t[d][k][lo:hi]

    def assert_guards(self, what):
        for d in range(1, 5):
            for k, v in self.t[d].items():
                if v is None:
                    continue
                tail, body = v[self.caps[d - 1]:], v[:self.caps[d - 1]]
                if v.is_floating_point():
                    assert bool(torch.isnan(tail).all()), (what, d, k, "written past the capacity")
                    assert not bool(torch.isnan(body).any()), (what, d, k, "left as allocated")
                else:
                    assert bool((tail == I64_FILL).all()), (what, d, k, "written past the capacity")
                    assert not bool((body == I64_FILL).any()), (what, d, k, "left as allocated")


def _run_rf(p, edge_index, edge_attr, caps):
    """``mkgnn_rf_count`` + ``mkgnn_rf_fill`` as ``build_receptive_fields_hip(sizes=caps)`` calls them."""
    from molkgnn_amd import _lib
    lib, dev = _lib.load(), p.device
    n, m, E = p.shape[0], edge_index.shape[1], edge_attr.shape[1]
    ws = torch.full((int(lib.mkgnn_rf_workspace_bytes(n)),), 0xFF, dtype=torch.uint8, device=dev)
    counts = torch.full((4,), I64_FILL, dtype=torch.int64, device=dev)
    out = _Outputs(caps, E, dev)
    st = _lib.stream_ptr(dev)
    _lib.check(lib.mkgnn_rf_count(edge_index.data_ptr(), n, m, ws.data_ptr(), ws.numel(), counts.data_ptr(), st), "mkgnn_rf_count")
    _lib.check(lib.mkgnn_rf_fill(edge_index.data_ptr(), p.data_ptr(), edge_attr.data_ptr(), n, m, E, ws.data_ptr(), out.buckets, st),
               "mkgnn_rf_fill")
    torch.cuda.synchronize()
    return out, counts


def _run_index(p, edge_index, edge_attr, caps):
    """``mkgnn_index_build`` as ``build_index_hip(sizes=caps)`` calls it."""
    from molkgnn_amd import _lib
    lib, dev = _lib.load(), p.device
    n, m, E = p.shape[0], edge_index.shape[1], edge_attr.shape[1]
    r = sum(c * (d + 1) for d, c in zip(range(1, 5), caps))
    out = _Outputs(caps, E, dev)
    counts = torch.full((6,), I64_FILL, dtype=torch.int64, device=dev)
    i32 = lambda k: torch.full((max(k, 1),), -1, dtype=torch.int32, device=dev)                         # noqa: E731
    s_ptr, s_rows = i32(n + 1), i32(r)
    in_ptr, in_col, in_pk, out_ptr, out_col = i32(n + 1), i32(m), i32(m), i32(n + 1), i32(m)
    deg8 = torch.full((n,), -1, dtype=torch.int8, device=dev)
    nbytes = int(lib.mkgnn_index_workspace_bytes(n, m, r))
    ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=dev)
    _lib.check(lib.mkgnn_index_build(edge_index.data_ptr(), p.data_ptr(), edge_attr.data_ptr(), n, m, E, out.buckets, s_ptr.data_ptr(),
                                     s_rows.data_ptr(), in_ptr.data_ptr(), in_col.data_ptr(), in_pk.data_ptr(), out_ptr.data_ptr(),
                                     out_col.data_ptr(), deg8.data_ptr(), counts.data_ptr(), ws.data_ptr(), nbytes, None,
                                     _lib.stream_ptr(dev)), "mkgnn_index_build")
    torch.cuda.synchronize()
    return out, counts


@pytest.mark.parametrize("builder", ["rf", "one pass"])
@pytest.mark.parametrize("degree", [2, 4])
def test_capacities_that_differ_from_the_batch(builder, degree):
    """One degree three rows over (the real rows exact, the extra rows atom 0 with zero attributes) and three rows under (the rows
    kept are the first ``cap`` atoms of the degree in atom order; the one-pass builder counts the three dropped atoms); the real
    sizes are reported, ``check_sizes`` raises, nothing is left as allocated and nothing is written behind a capacity.  Only
    the receptive fields are compared: this is an error state, and the plan arrays of the two builders legitimately differ in it
    (the one-pass builder plans the rows it kept, ``BatchPlan.build_hip`` the lists it is handed)."""
    from molkgnn_amd.receptive_field import build_receptive_fields, check_sizes
    dev = _dev()
    p, edge_index, edge_attr = (t.to(dev).contiguous() for t in _custom(7))
    n, E = p.shape[0], 7
    f = build_receptive_fields(torch.zeros((n, 1), device=dev), p, edge_index, edge_attr)
    sizes = [int(f[f"selected_index_deg{d}"].numel()) for d in range(1, 5)]
    assert sizes == [124, 371, 0, 5] and n > 256            # (more than one 256-atom chunk; degree 4: five atoms in all)
    run = _run_rf if builder == "rf" else _run_index
    for delta in (3, -3):
        caps = list(sizes)
        caps[degree - 1] += delta
        out, counts = run(p, edge_index, edge_attr, caps)
        what = (builder, degree, delta)
        assert counts.tolist()[:4] == sizes, what
        if builder == "one pass":
            assert counts.tolist()[4:] == [3 if delta < 0 else 0, 0], what
        with pytest.raises(ValueError):
            check_sizes({"rf_counts": counts, "rf_sizes": tuple(caps)})
        out.assert_guards(what)
        for d in range(1, 5):
            kept = min(caps[d - 1], sizes[d - 1])
            nd = sizes[d - 1]
            want = {"selected_index": f[f"selected_index_deg{d}"].reshape(nd, 1), "nei_index": f[f"nei_index_deg{d}"].reshape(nd, d),
                    "nei_edge_attr": f[f"nei_edge_attr_deg{d}"].reshape(nd, d * E), "p_focal": f[f"p_focal_deg{d}"].reshape(nd, 3),
                    "nei_p": f[f"nei_p_deg{d}"].reshape(nd, d * 3)}
            if nd:
                want["nei_edge_unit"] = _unit_rows(f[f"nei_edge_attr_deg{d}"], E).reshape(nd, d * 8)
            for k, w in want.items():
                g = out.rows(d, k, 0, kept)
                assert torch.equal(g, w[:kept]), (what, d, k)
                if g.is_floating_point():
                    assert torch.equal(g.view(torch.int32), w[:kept].contiguous().view(torch.int32)), (what, d, k)
                extra = out.rows(d, k, kept, caps[d - 1])
                assert extra.shape[0] == max(caps[d - 1] - sizes[d - 1], 0)
                assert int(extra.view(torch.int32 if extra.is_floating_point() else torch.int64).abs().sum()) == 0, (what, d, k, "extra rows")
