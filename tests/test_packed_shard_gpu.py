"""``mkgnn_gather_compact_packed`` on the GPU: the gather from a resident shard whose byte-valued feature columns are held as
int8 writes, byte for byte, the wire buffer of ``mkgnn_gather_compact`` on the same shard held unpacked and of the numpy
definition ``shards.gather_compact``; scoring, evaluation and training fed from the packed shard give the same bits.  Every
comparison is ``torch.equal`` -- on the WHOLE wire buffer where one is compared (all buffers start out as 0xA5 bytes, so the
alignment gaps that no gather writes agree as well)."""
import copy

import numpy as np
import pytest
import torch

from molkgnn_amd import padding as P
from molkgnn_amd import shards as S
from molkgnn_amd.synthetic import make_batch, with_reference_features

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
N_MOL = 150
FILL = 0xA5


@pytest.fixture(scope="module")
def base():
    b = make_batch(N_MOL, seed=21, assay="all9", with_receptive_fields=False)
    b.y = (torch.arange(N_MOL) % 5 == 0).to(b.y.dtype)
    return b


def _shard_with_x(base, x, path):
    b = copy.copy(base)
    b.x = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
    S.write_shard(str(path), b)
    return S.Shard(str(path))


@pytest.fixture(scope="module")
def reference(base, tmp_path_factory):
    """The shard with the reference's column pattern, resident both ways."""
    b = with_reference_features(copy.copy(base), seed=2)
    shard = _shard_with_x(base, b.x.numpy(), tmp_path_factory.mktemp("packed") / "reference.mkgs")
    packed, plain = S.ResidentShard(shard, DEV, packed=True), S.ResidentShard(shard, DEV)
    assert packed.rec_bytes == 52 and list(packed.byte_columns) == list(range(20))
    assert packed.nbytes() == sum(t.numel() * t.element_size() for t in packed.tensors.values())
    assert plain.nbytes() - packed.nbytes() == 60 * shard.n_atoms           # 112 -> 52 bytes of x per atom
    assert "x" not in packed.tensors and "x_rec" not in plain.tensors
    return shard, packed, plain


def _shape_for(shard, ids, headroom=0.0):
    return S.ResidentLoader(S.ResidentShard(shard, "cpu"), len(ids), ids, "cpu", headroom=headroom).shape


def _gather_raw(res, ids, shape):
    """One call of the C entry point that belongs to ``res`` into a fresh wire buffer of 0xA5 bytes; ``(rc, wire, status)``."""
    from molkgnn_amd import _lib
    lib = _lib.load()
    n = len(ids)
    ids_dev = torch.from_numpy(np.asarray(ids).astype(np.int32)).to(DEV)
    _, total = S.compact_layout(shape, n, res.x_dim, res.p_dim, res.e_dim)
    buf = torch.full((total,), FILL, dtype=torch.uint8, device=DEV)
    ws = torch.full((lib.mkgnn_gather_compact_workspace_bytes(n),), 0xFF, dtype=torch.uint8, device=DEV)
    sh = _lib.Int64x6(shape["atoms"], shape["edges"], shape["n1"], shape["n2"], shape["n3"], shape["n4"])
    fn = lib.mkgnn_gather_compact_packed if res.packed else lib.mkgnn_gather_compact
    rc = fn(res.view, ids_dev.data_ptr(), n, sh, P.PAD_MOLECULES, buf.data_ptr(), total, ws.data_ptr(), _lib.stream_ptr(DEV))
    torch.cuda.synchronize()
    return rc, buf, int(ws[:4].view(torch.int32)[0])


def _numpy_wire(shard, ids, shape):
    _, total = S.compact_layout(shape, len(ids), shard.x_dim, shard.p_dim, shard.e_dim)
    want = np.full(total, FILL, dtype=np.uint8)
    S.gather_compact(shard, ids, shape, want)
    return torch.from_numpy(want)


def _check_three_ways(shard, packed, plain, ids, shape, what):
    rc_p, wire_p, st_p = _gather_raw(packed, ids, shape)
    rc_u, wire_u, st_u = _gather_raw(plain, ids, shape)
    assert (rc_p, st_p, rc_u, st_u) == (0, 0, 0, 0), what
    assert torch.equal(wire_p, wire_u), what
    assert torch.equal(wire_p.cpu(), _numpy_wire(shard, ids, shape)), what


def _id_lists(n, mol_atoms):
    rng = np.random.default_rng(300 + n)
    M = len(mol_atoms)
    repeats = rng.integers(0, M, size=n)
    repeats[n // 2:] = repeats[: n - n // 2]                                 # (every id of the second half is a repeat)
    return {"repeats": repeats, "shuffled": rng.permutation(M)[np.arange(n) % M],
            "one id": np.full(n, int(np.argmin(mol_atoms))), "last id": np.full(n, M - 1)}


@pytest.mark.parametrize("n", [7, 64, 130])
def test_packed_gather_equals_both_definitions(reference, n):
    """7 ids (a few tiles at most; the smallest molecule repeated is about one 64-row tile), 64 ids, 130 ids (some 3 000 atoms:
    many 64-row tiles in more than one 256-row block, tile boundaries inside molecules), with the padding at its minimum
    (headroom 0) and with whole tiles of padding rows (headroom 0.5)."""
    shard, packed, plain = reference
    for name, ids in _id_lists(n, packed.mol_atoms).items():
        for headroom in (0.0, 0.5):
            shape = _shape_for(shard, ids, headroom)
            if n == 130 and name != "one id":
                assert shape["atoms"] > 2 * 256
            _check_three_ways(shard, packed, plain, ids, shape, (name, headroom))


def _byte_columns(x_dim, pattern):
    if pattern == "reference":
        return set(range({28: 20, 30: 20, 5: 3}[x_dim]))
    if pattern == "all byte":
        return set(range(x_dim))
    if pattern == "all float":
        return set()
    if pattern == "one byte":
        return {x_dim // 2}
    assert pattern == "21 bytes"                                            # record padding in play: nq = 21 (3 where x_dim = 5)
    return set(np.random.default_rng(x_dim).permutation(x_dim)[:21].tolist()) if x_dim >= 21 else {0, 2, 4}


def _matrix(rows, x_dim, byte_cols, seed):
    """``x`` whose byte columns are exactly ``byte_cols``: integers with -128 and 127 among them; the float columns are normal
    draws with a NaN payload, -0.0 and a denormal among them, each at rows of their own."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((rows, x_dim)).astype(np.float32)
    bits = x.view(np.uint32)
    for c in range(x_dim):
        at = rng.choice(rows, size=24, replace=False)
        if c in byte_cols:
            x[:, c] = rng.integers(-128, 128, size=rows)
            x[at[:12], c], x[at[12:], c] = -128, 127
        else:
            bits[at[:8], c], bits[at[8:16], c], bits[at[16:], c] = 0x7FC00000 | (c + 1), 0x80000000, 0x00000001 + c
    return x


@pytest.mark.parametrize("pattern", ["reference", "all byte", "all float", "one byte", "21 bytes"])
@pytest.mark.parametrize("x_dim", [28, 30, 5])
def test_shape_matrix(base, tmp_path, x_dim, pattern):
    """16-byte stores (x_dim 28), plain stores (30: not a multiple of 4), an odd width (5), against every column pattern."""
    cols = _byte_columns(x_dim, pattern)
    x = _matrix(int(base.x.shape[0]), x_dim, cols, seed=17 * x_dim + len(cols))
    shard = _shard_with_x(base, x, tmp_path / "case.mkgs")
    packed, plain = S.ResidentShard(shard, DEV, packed=True), S.ResidentShard(shard, DEV)
    nq, nf = len(cols), x_dim - len(cols)
    assert sorted(packed.byte_columns) == sorted(cols) and packed.rec_bytes == 4 * nf + 4 * ((nq + 3) // 4)
    rng = np.random.default_rng(x_dim)
    for n in (64, 130):
        ids = rng.integers(0, N_MOL, size=n)
        ids[n // 2:] = ids[: n - n // 2]
        rng.shuffle(ids)
        _check_three_ways(shard, packed, plain, ids, _shape_for(shard, ids), (x_dim, pattern, n))
    # the specials were in what was gathered: all of the shard's atoms, so every NaN payload, -0.0 and denormal, -128 and 127
    ids = np.arange(N_MOL)
    shape = _shape_for(shard, ids)
    rc, wire, status = _gather_raw(packed, ids, shape)
    assert rc == 0 and status == 0
    got = wire[:4 * shard.n_atoms * x_dim].view(torch.int32).view(shard.n_atoms, x_dim).cpu().numpy()
    assert np.array_equal(got, np.array(shard.x).view(np.int32))
    assert torch.equal(wire.cpu(), _numpy_wire(shard, ids, shape))


def test_bad_ids_set_the_flag_and_clamp_alike(reference):
    from molkgnn_amd import _lib
    shard, packed, plain = reference
    ids = np.random.default_rng(4).integers(0, N_MOL, size=64)
    ids[5], ids[40] = -1, N_MOL
    clamped = ids.copy()
    clamped[5], clamped[40] = 0, N_MOL - 1
    shape = _shape_for(shard, clamped, 0.5)
    rc_p, wire_p, st_p = _gather_raw(packed, ids, shape)
    rc_u, wire_u, st_u = _gather_raw(plain, ids, shape)
    assert rc_p == 0 and rc_u == 0
    assert st_p == st_u == _lib.GATHER_BAD_ID
    assert torch.equal(wire_p, wire_u)
    assert torch.equal(wire_p.cpu(), _numpy_wire(shard, clamped, shape))


def test_misfit_sets_the_flag_and_the_next_gather_is_right(reference):
    """A checked error path, not a fault: a shape one degree-2 atom short sets MKGNN_GATHER_MISFIT as the unpacked gather does
    (the clamped contents need not agree); the call returns, and the next gather with a fitting shape is byte-equal again."""
    from molkgnn_amd import _lib
    shard, packed, plain = reference
    ids = np.arange(40, 104)
    shape = _shape_for(shard, ids)
    tight = dict(shape)
    tight["n2"] = int(packed.mol_deg[ids, 1].sum()) - 1
    tight["atoms"] = sum(tight[f"n{d}"] for d in range(1, 5))
    tight["edges"] = sum(d * tight[f"n{d}"] for d in range(1, 5))
    tight["edges"] -= tight["edges"] % 2
    rc_p, _, st_p = _gather_raw(packed, ids, tight)
    rc_u, _, st_u = _gather_raw(plain, ids, tight)
    assert rc_p == 0 and rc_u == 0
    assert st_p & _lib.GATHER_MISFIT and st_p == st_u
    _check_three_ways(shard, packed, plain, ids, shape, "after the misfit")


def test_one_captured_gather_serves_every_id_list(reference):
    shard, packed, plain = reference
    lists = np.random.default_rng(8).integers(0, N_MOL, size=(4, 96))       # list 0 warms up, lists 1..3 are replayed
    loader = S.ResidentLoader(packed, 96, lists.reshape(-1), DEV)
    assert loader.resident is packed and len(loader) == 4
    batches = list(loader)
    dims = (28, 3, 7)
    csb_p = P.CompactStaticBatch(loader.shape, 96, *dims, DEV, max_mol_atoms=loader.max_mol_atoms, max_mol_edges=loader.max_mol_edges)
    csb_u = P.CompactStaticBatch(loader.shape, 96, *dims, DEV, max_mol_atoms=loader.max_mol_atoms, max_mol_edges=loader.max_mol_edges)
    csb_p.wire.fill_(FILL)
    csb_u.wire.fill_(FILL)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        csb_p.gather(packed, batches[0])                                    # (allocates the static id buffer and fills it)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            csb_p.gather(packed)
        for k in range(1, 4):
            csb_p.ids.copy_(batches[k])
            g.replay()
            csb_u.gather(plain, batches[k])
            assert torch.equal(csb_p.wire, csb_u.wire), k
            assert torch.equal(csb_p.wire.cpu(), _numpy_wire(shard, lists[k], loader.shape)), k
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert csb_p.gather_status() == 0 and csb_u.gather_status() == 0


def _model(**kw):
    from molkgnn_amd.train import GNNModel
    torch.manual_seed(0)
    return GNNModel(num_layers=2, **kw).to(DEV)


def test_scoring_from_the_packed_shard_gives_the_same_bits(tmp_path):
    """100 molecules at batch 32 (three full batches and a tail of 4): score_resident, screen and evaluate_resident."""
    from molkgnn_amd.screening import score_resident, screen
    from molkgnn_amd.train import evaluate_resident
    b = with_reference_features(make_batch(100, seed=33, assay="all9", with_receptive_fields=False), seed=3)
    b.y = (torch.arange(100) % 3 == 0).float()
    S.write_shard(str(tmp_path / "lib.mkgs"), b)
    shard = S.Shard(str(tmp_path / "lib.mkgs"))
    packed, plain = S.ResidentShard(shard, DEV, packed=True), S.ResidentShard(shard, DEV)
    assert packed.rec_bytes == 52
    model = _model()
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, torch.nn.modules.batchnorm._BatchNorm):
                m.running_mean.uniform_(-0.2, 0.2)
                m.running_var.uniform_(0.5, 1.5)
    model.eval()
    s_p, s_u = score_resident(model, packed, 32), score_resident(model, plain, 32)
    assert s_p.shape == (100,) and not bool(torch.isnan(s_p).any())
    assert torch.equal(s_p.view(torch.int32), s_u.view(torch.int32))
    r_p, r_u = screen(model, [packed], 16, 32), screen(model, [plain], 16, 32)
    assert r_p["n_scored"] == r_u["n_scored"] == 100 and r_p["top_score"].shape == (16,)
    for k in ("top_score", "top_shard", "top_mol"):
        assert torch.equal(r_p[k], r_u[k]), k
    e_p, e_u = evaluate_resident(model, packed, 32), evaluate_resident(model, plain, 32)
    assert torch.equal(e_p["loss"], e_u["loss"]) and not bool(torch.isnan(e_p["loss"]))
    assert torch.equal(e_p["pred_y"], s_p) and torch.equal(e_u["pred_y"], s_u)


def test_two_training_steps_from_the_packed_shard_give_the_same_bits(reference):
    from molkgnn_amd.receptive_field import attach_receptive_fields
    from molkgnn_amd.train import configure_optimizer, training_step
    _, packed, plain = reference
    ids = np.random.default_rng(11).integers(0, N_MOL, size=2 * 64)
    runs = []
    for res in (packed, plain):
        model = _model(ffn_dropout_rate=0.0, dropout_ratio=0.0)
        opt = configure_optimizer(model, lr=1e-3, capturable=True)
        loader = S.ResidentLoader(res, 64, ids, DEV)
        csb = P.CompactStaticBatch(loader.shape, 64, 28, 3, 7, DEV, max_mol_atoms=loader.max_mol_atoms,
                                   max_mol_edges=loader.max_mol_edges)
        losses = []
        for ids_dev in loader:
            csb.gather(res, ids_dev)
            csb.expand()
            attach_receptive_fields(csb.data, sizes=csb.data.bucket_sizes, overlap=True)
            losses.append(training_step(model, csb.data, opt).detach().clone())
        torch.cuda.synchronize()
        assert len(losses) == 2 and csb.gather_status() == 0
        runs.append((losses, model))
    (l_p, m_p), (l_u, m_u) = runs
    for k in range(2):
        assert torch.equal(l_p[k], l_u[k]), (k, float(l_p[k]), float(l_u[k]))
    assert float(l_p[0]) != float(l_p[1])
    for (name, a), (_, b) in zip(m_p.named_parameters(), m_u.named_parameters()):
        assert torch.equal(a, b), name
