"""``mkgnn_gather_compact`` and ``mkgnn_expand_batch`` at their dispatch edges, against their numpy definitions
(``shards.gather_compact``; ``tests/test_shards.py::_expand_on_host``), field by field and bit for bit -- no tolerance anywhere.

Where the sizes come from (molkgnn_amd/csrc/kgnn_gather.hip, kgnn_plan.hip):

* ``gather_scan_kernel`` is ONE workgroup of 1024 threads (16 waves); a thread owns ``ceil(n / 1024)`` consecutive slots.  Up to
  n = 1024 that is one slot: the loop over a thread's slots, the exclusive offset ``v - mine`` and a scan whose 16 waves all
  carry data only run beyond.  n = 1023 (the last size with one slot and an idle thread), 1024, 1025 (two slots: 513 threads
  busy, the last of them with one slot), 2049 (three), 4096 (four: the workload's batch).
* ``gather_fill_kernel``: a wave owns 64 output rows, a block 256.  The hand-made molecules of tests/_batch_cases.py put whole
  tiles inside one molecule (a 300-atom chain: in two blocks) and tiles across 32 two-atom molecules.
* rows of ``p`` travel in 16-byte pieces when ``p_dim`` is a multiple of 4 (``vec_p``); the attribute bytes of a tile are put
  together four to a dword, bytes of up to four bonds in one dword and a partial last dword when ``(bonds * e_dim) % 4 != 0``.
* the padding's closed forms with no padding atom at all and with fewer padding atoms than the 64 padding molecules.
* ``expand_batch_kernel`` finds an atom's molecule by bisection of ``mol_ptr``: runs of EMPTY padding molecules are runs of
  equal pointers.
"""
import numpy as np
import pytest
import torch

from molkgnn_amd import padding as P
from molkgnn_amd import shards as S
from molkgnn_amd.synthetic import make_batch
from tests import _batch_cases as C
from tests import test_shards as _host

gpu = pytest.mark.gpu
_TORCH = {np.float32: torch.float32, np.int64: torch.int64, np.int32: torch.int32, np.uint8: torch.uint8}
E_DIMS, P_DIMS, WIDTH_N, HEADROOMS = (1, 4, 5, 12), (3, 4), (1, 57, 200), (0.0, 0.5)
X_DIM = 6
CANARY = 4096


def _dev():
    return torch.device("cuda:0")


def _shape_for(shard, ids, headroom=0.0):
    return S.ResidentLoader(S.ResidentShard(shard, "cpu"), len(ids), ids, "cpu", headroom=headroom).shape


def _gather_raw(res, ids, shape, packed=False):
    """One call of the C entry point as tests/test_gather_gpu.py makes it: a fresh wire buffer of 0xA5 bytes with a canary of
    4 KB behind it, a workspace of 0xFF bytes.  Returns ``(rc, buffer, status, bytes of the wire form)``."""
    from molkgnn_amd import _lib
    lib = _lib.load()
    n = len(ids)
    ids_dev = torch.from_numpy(np.asarray(ids).astype(np.int32)).to(_dev())
    _, total = S.compact_layout(shape, n, res.x_dim, res.p_dim, res.e_dim)
    buf = torch.full((total + CANARY,), 0xA5, dtype=torch.uint8, device=_dev())
    ws = torch.full((lib.mkgnn_gather_compact_workspace_bytes(n),), 0xFF, dtype=torch.uint8, device=_dev())
    sh = _lib.Int64x6(shape["atoms"], shape["edges"], shape["n1"], shape["n2"], shape["n3"], shape["n4"])
    fn = lib.mkgnn_gather_compact_packed if packed else lib.mkgnn_gather_compact
    rc = fn(res.view, ids_dev.data_ptr(), n, sh, P.PAD_MOLECULES, buf.data_ptr(), total, ws.data_ptr(), _lib.stream_ptr(_dev()))
    torch.cuda.synchronize()
    return rc, buf, int(ws[:4].view(torch.int32)[0]), total


def _numpy_wire(shard, ids, shape):
    _, total = S.compact_layout(shape, len(ids), shard.x_dim, shard.p_dim, shard.e_dim)
    want = np.full(total, 0xA5, dtype=np.uint8)
    S.gather_compact(shard, ids, shape, want)
    return want


def _assert_wire(buf, total, shard, ids, shape, what):
    """Every field against the definition, the alignment gaps and the canary still 0xA5; returns the definition's fields."""
    want = torch.from_numpy(_numpy_wire(shard, ids, shape))
    got = buf.cpu()
    table, _ = S.compact_layout(shape, len(ids), shard.x_dim, shard.p_dim, shard.e_dim)
    for k, off, shp, dt, nbytes in table:
        g, w = got[off:off + nbytes].view(_TORCH[dt]).view(shp), want[off:off + nbytes].view(_TORCH[dt]).view(shp)
        assert torch.equal(g, w), (what, k)
    assert torch.equal(got[:total], want), (what, "alignment gaps")
    assert bool((got[total:] == 0xA5).all()), (what, "canary")
    return {k: want[off:off + nbytes].view(_TORCH[dt]).view(shp) for k, off, shp, dt, nbytes in table}


def _assert_expansion(buf, total, shape, n, dims, what):
    """``mkgnn_expand_batch`` on the gathered wire buffer, into outputs that start out as -1 / NaN, against the numpy expansion."""
    from molkgnn_amd import _lib
    e_dim = dims[2]
    table, _ = S.compact_layout(shape, n, *dims)
    at = {k: (off, nbytes) for k, off, shp, dt, nbytes in table}
    A, E2, G = shape["atoms"], shape["edges"], n + P.PAD_MOLECULES
    dev = _dev()
    edge_index = torch.full((2, E2), -1, dtype=torch.int64, device=dev)
    edge_attr = torch.full((E2, e_dim), float("nan"), dtype=torch.float32, device=dev)
    batch = torch.full((A,), -1, dtype=torch.int64, device=dev)
    atom_mol = torch.full((A,), -1, dtype=torch.int32, device=dev)
    base = buf.data_ptr()
    _lib.check(_lib.load().mkgnn_expand_batch(base + at["bond_ij"][0], base + at["bond_attr"][0], E2 // 2, e_dim, base + at["mol_ptr"][0],
                                              G, A, edge_index.data_ptr(), edge_attr.data_ptr(), batch.data_ptr(),
                                              atom_mol.data_ptr(), _lib.stream_ptr(dev)), "mkgnn_expand_batch")
    torch.cuda.synchronize()
    want = _host._expand_on_host(S.CompactBatch(buf[:total], shape, n), dims)
    got = {"edge_index": edge_index, "edge_attr": edge_attr, "batch": batch, "atom_mol": atom_mol}
    for k, g in got.items():
        g, w = g.cpu().numpy(), want[k]
        assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), (what, k)
    return want


# ---------------------------------------------------------------------------------------------------------------------------
# slots per scan thread

@pytest.fixture(scope="module")
def synthetic(tmp_path_factory):
    """The 300 synthetic molecules of tests/test_gather_gpu.py narrowed to five feature columns (small buffers), the first three
    of them byte-valued so that the packed form holds both kinds of column."""
    whole = make_batch(300, seed=12, assay="all9", with_receptive_fields=False)
    whole.y = (torch.arange(300) % 7 == 0).to(whole.y.dtype)
    x = whole.x[:, :5].contiguous()
    x[:, :3] = torch.clamp(torch.round(8.0 * x[:, :3]), -128, 127) + 0.0       # (+ 0.0: no -0.0, which an int8 would not carry)
    whole.x = x
    path = str(tmp_path_factory.mktemp("scan") / "x5.mkgs")
    S.write_shard(path, whole)
    return S.Shard(path)


@gpu
@pytest.mark.parametrize("n", [1023, 1024, 1025, 2049, 4096])
def test_several_slots_per_scan_thread(synthetic, n):
    """1, 1, 2, 3 and 4 slots per thread of the one-workgroup scan (1024 threads): random ids with repeats, one molecule repeated
    (every slot the same size: offsets are a multiple of it) and descending ids; at 4096 the wire form is expanded as well."""
    shard = synthetic
    res = S.ResidentShard(shard, _dev())
    assert (res.x_dim, res.p_dim, res.e_dim) == (5, 3, 7)
    assert -(-n // 1024) == {1023: 1, 1024: 1, 1025: 2, 2049: 3, 4096: 4}[n]
    for name, ids in C.id_lists(n, shard.n_molecules).items():
        shape = _shape_for(shard, ids)
        rc, buf, status, total = _gather_raw(res, ids, shape)
        assert rc == 0 and status == 0, (name, rc, status)
        _assert_wire(buf, total, shard, ids, shape, name)
        if n == 4096 and name == "repeats":
            _assert_expansion(buf, total, shape, n, (5, 3, 7), name)


@gpu
def test_two_slots_per_scan_thread_from_a_packed_shard(synthetic):
    """n = 1025 through ``mkgnn_gather_compact_packed`` (the scan kernel is shared, the id list and the workspace are its own):
    the packed gather, the unpacked gather and the numpy definition agree on the whole wire buffer."""
    shard = synthetic
    packed, plain = S.ResidentShard(shard, _dev(), packed=True), S.ResidentShard(shard, _dev())
    assert packed.byte_columns == [0, 1, 2] and packed.rec_bytes == 12
    for name, ids in C.id_lists(1025, shard.n_molecules).items():
        shape = _shape_for(shard, ids)
        rc_p, wire_p, st_p, total = _gather_raw(packed, ids, shape, packed=True)
        rc_u, wire_u, st_u, _ = _gather_raw(plain, ids, shape)
        assert (rc_p, st_p, rc_u, st_u) == (0, 0, 0, 0), name
        assert torch.equal(wire_p, wire_u), name
        assert torch.equal(wire_p[:total].cpu(), torch.from_numpy(_numpy_wire(shard, ids, shape))), name
        assert bool((wire_p[total:] == 0xA5).all()), name


# ---------------------------------------------------------------------------------------------------------------------------
# widths, on the hand-made molecules

def _custom_shard(directory, p_dim, e_dim):
    """The hand-made molecules with these widths as a shard, and the molecules themselves."""
    mols = C.molecules(X_DIM, p_dim, e_dim, seed=10 * e_dim + p_dim)
    path = str(directory / f"p{p_dim}e{e_dim}.mkgs")
    S.write_shard(path, C.collate(mols))
    return S.Shard(path), mols


def _width_ids(n):
    return np.arange(57) if n == 57 else C.id_lists(n, 57, seed=3)["repeats"]


def test_the_width_cases_cover_what_they_are_for(tmp_path):
    """The shapes of ``test_feature_widths`` between them: the attribute field ends on every byte of a dword
    (``(bonds * e_dim) % 4`` in {0, 1, 2, 3}), and some shape has a last atom tile and a last bond tile that are partial."""
    left, partial = set(), False
    for e_dim in E_DIMS:
        shard, _ = _custom_shard(tmp_path, 3, e_dim)
        for n in WIDTH_N:
            for headroom in HEADROOMS:
                shape = _shape_for(shard, _width_ids(n), headroom)
                left.add((shape["edges"] // 2 * e_dim) % 4)
                partial |= shape["atoms"] % 64 != 0 and (shape["edges"] // 2) % 64 != 0
    assert left == {0, 1, 2, 3} and partial


@gpu
@pytest.mark.parametrize("p_dim", P_DIMS)
@pytest.mark.parametrize("e_dim", E_DIMS)
def test_feature_widths(tmp_path, e_dim, p_dim):
    """1, 4, 5 and 12 attribute bytes per bond (a dword holds the bytes of four bonds / one bond / parts of two; a tile's 64 bonds
    take 16, 64, 80 and 192 dwords: one, one, two and three trips of the wave), ``p`` rows of 12 bytes (element-wise) and of 16
    (``vec_p``), one id, all 57 molecules in order and 200 ids with repeats, minimum padding and headroom 0.5; every wire buffer is
    expanded as well."""
    shard, _ = _custom_shard(tmp_path, p_dim, e_dim)
    res = S.ResidentShard(shard, _dev())
    dims = (X_DIM, p_dim, e_dim)
    assert (res.x_dim, res.p_dim, res.e_dim) == dims
    if p_dim == 4:                                          # the conditions under which the entry point sets vec_p
        assert res.p_dim % 4 == 0 and res.tensors["p"].data_ptr() % 16 == 0
    for n in WIDTH_N:
        ids = _width_ids(n)
        for headroom in HEADROOMS:
            shape = _shape_for(shard, ids, headroom)
            what = (n, headroom)
            rc, buf, status, total = _gather_raw(res, ids, shape)
            assert rc == 0 and status == 0, (what, rc, status)
            _assert_wire(buf, total, shard, ids, shape, what)
            _assert_expansion(buf, total, shape, n, dims, what)


# ---------------------------------------------------------------------------------------------------------------------------
# padding extremes

@gpu
@pytest.mark.parametrize("need", [(0, 0, 0, 0), (1, 0, 1, 0), (2, 1, 0, 0), (0, 0, 0, 1), (20, 20, 20, 3)],
                         ids=lambda need: "-".join(map(str, need)))
def test_padding_extremes(tmp_path, need):
    """No padding atom at all (all 64 padding molecules empty: ``mol_ptr`` repeats the atom count, and the expansion puts no atom
    into a padding molecule), and a whole padding of 2, 3, 1 and 63 atoms -- fewer than the 64 padding molecules, so most of
    them are empty and the others hold one atom."""
    dims = (X_DIM, 4, 5)
    shard, mols = _custom_shard(tmp_path, 4, 5)
    res = S.ResidentShard(shard, _dev())
    n_pad = sum(need)
    assert n_pad < P.PAD_MOLECULES
    for n in (57, 200):
        ids = _width_ids(n)
        shape = C.shape_with_padding(C.degree_counts([mols[int(m)] for m in ids]), need)
        rc, buf, status, total = _gather_raw(res, ids, shape)
        assert rc == 0 and status == 0, (n, rc, status)
        f = _assert_wire(buf, total, shard, ids, shape, n)
        na = int(f["n_valid_atoms"][0])
        assert shape["atoms"] - na == n_pad
        pad_sizes = np.diff(f["mol_ptr"].numpy()[n:])
        assert pad_sizes.shape[0] == P.PAD_MOLECULES and int(pad_sizes.sum()) == n_pad and int(pad_sizes.max(initial=0)) <= 1
        got = _assert_expansion(buf, total, shape, n, dims, n)
        assert int((got["batch"] >= n).sum()) == n_pad
        if n_pad == 0:
            assert bool((f["mol_ptr"][n:] == na).all()) and int(got["batch"].max()) == n - 1


# ---------------------------------------------------------------------------------------------------------------------------
# the checked error paths (safe by the kernel's own clamps; not faults)

@gpu
def test_negative_ids_set_the_flag_and_read_molecule_zero(tmp_path):
    """An id of -1 and an id of INT32_MIN: ``MKGNN_GATHER_BAD_ID``, and apart from the flag the batch with id 0 in their place."""
    from molkgnn_amd import _lib
    shard, _ = _custom_shard(tmp_path, 4, 5)
    res = S.ResidentShard(shard, _dev())
    good = _width_ids(200).copy()
    good[[3, 150]] = 0
    shape = _shape_for(shard, good, 0.5)
    bad = good.copy()
    bad[3], bad[150] = -1, np.iinfo(np.int32).min
    rc, buf, status, total = _gather_raw(res, bad, shape)
    assert rc == 0 and status == _lib.GATHER_BAD_ID
    _assert_wire(buf, total, shard, good, shape, "clamped")


@gpu
def test_a_shape_of_half_the_atoms_sets_the_flag_and_stays_in_bounds(tmp_path):
    """The offsets saturate by hundreds of atoms and bonds, not by one: ``MKGNN_GATHER_MISFIT``, the call returns 0, the canary
    behind the wire buffer is intact, and what was written are indices of the shape (``bond_ij`` in [0, atoms), ``mol_ptr``
    non-decreasing up to atoms)."""
    from molkgnn_amd import _lib
    shard, mols = _custom_shard(tmp_path, 4, 5)
    res = S.ResidentShard(shard, _dev())
    ids = _width_ids(200)
    counts = C.degree_counts([mols[int(m)] for m in ids])
    half = [c // 2 for c in counts]
    half[0] += sum((d + 1) * half[d] for d in range(4)) % 2                     # (an even number of directed edges)
    shape = C.shape_with_padding(half)
    assert shape["atoms"] < 0.51 * sum(counts)
    rc, buf, status, total = _gather_raw(res, ids, shape)
    assert rc == 0 and status & _lib.GATHER_MISFIT and not status & _lib.GATHER_BAD_ID
    host = buf.cpu()
    assert bool((host[total:] == 0xA5).all())
    table, _ = S.compact_layout(shape, 200, X_DIM, 4, 5)
    f = {k: host[off:off + nbytes].view(_TORCH[dt]).view(shp) for k, off, shp, dt, nbytes in table}
    A = shape["atoms"]
    assert int(f["bond_ij"].min()) >= 0 and int(f["bond_ij"].max()) < A
    mp = f["mol_ptr"].numpy()
    assert mp[0] == 0 and (np.diff(mp) >= 0).all() and mp[-1] <= A and int(f["n_valid_atoms"][0]) == A
    # ... and the next gather with a fitting shape is exact again
    shape = _shape_for(shard, ids)
    rc, buf, status, total = _gather_raw(res, ids, shape)
    assert rc == 0 and status == 0
    _assert_wire(buf, total, shard, ids, shape, "after the misfit")
