"""The packed form of a resident shard's atom features on the host: the column classification, ``pack_x`` / ``unpack_x`` (the
definition the device decode is tested against), the footprint of ``ResidentShard(..., packed=True)`` and the C ABI of
``mkgnn_gather_compact_packed``.  Everything is compared as bits."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from molkgnn_amd import shards as S
from molkgnn_amd.synthetic import REFERENCE_BYTE_COLUMNS, make_batch, with_reference_features

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _f32(bits):
    return np.array([bits], dtype=np.uint32).view(np.float32)[0]


def test_classification_column_by_column():
    n = 6
    cols = {
        "flags": ([0, 1, 1, 0, 1, 0], True),
        "byte ends": ([-128, 127, 0, 5, -7, 100], True),
        "128": ([0, 128, 1, 2, 3, 4], False),
        "-129": ([0, -129, 1, 2, 3, 4], False),
        "half": ([0, 1, 0.5, 2, 3, 4], False),
        "one negative zero": ([0, 1, -0.0, 2, 3, 4], False),
        "nan payload": ([0, 1, _f32(0x7FC0BEEF), 2, 3, 4], False),
        "plus inf": ([0, 1, np.inf, 2, 3, 4], False),
        "minus inf": ([0, 1, -np.inf, 2, 3, 4], False),
        "all zero": ([0] * n, True),
    }
    x = np.stack([np.array(v, dtype=np.float32) for v, _ in cols.values()], axis=1)
    assert x.view(np.uint32)[2, 5] == 0x80000000 and x.view(np.uint32)[2, 6] == 0x7FC0BEEF      # (the specials got there)
    got = S.classify_x_columns(x)
    assert got.dtype == np.bool_ and got.shape == (len(cols),)
    for k, (name, (_, want)) in enumerate(cols.items()):
        assert bool(got[k]) == want, name
    assert S.classify_x_columns(np.zeros((0, 3), dtype=np.float32)).tolist() == [True, True, True]


def _matrix(rows, x_dim, byte_cols, seed):
    """``x`` whose byte columns are exactly ``byte_cols``: those hold integers with -128 and 127 among them, the others
    normal draws with a NaN payload, -0.0, a denormal and an infinity among them."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((rows, x_dim)).astype(np.float32)
    bits = x.view(np.uint32)
    for c in range(x_dim):
        if c in byte_cols:
            x[:, c] = rng.integers(-128, 128, size=rows)
            x[0, c], x[1, c] = -128, 127
        else:
            bits[0, c], bits[1, c], bits[2, c] = 0x7FC00000 | (c + 1), 0x80000000, 0x00000001 + c
            x[3, c] = np.inf if c % 2 else -np.inf
    return x


def _byte_sets(x_dim):
    """Byte-column sets with nq in {0, 1, 3, 20, 21, x_dim} (where x_dim allows), scattered over the columns."""
    out = []
    for nq in sorted({0, 1, 3, 20, 21, x_dim}):
        if nq <= x_dim:
            out.append(sorted(np.random.default_rng(1000 * x_dim + nq).permutation(x_dim)[:nq].tolist()))
    return out


@pytest.mark.parametrize("x_dim", [28, 5, 30, 1])
def test_round_trip_layout_and_table(x_dim):
    for cols in _byte_sets(x_dim):
        x = _matrix(37, x_dim, set(cols), seed=x_dim + len(cols))
        mask = S.classify_x_columns(x)
        assert np.nonzero(mask)[0].tolist() == cols
        rec, x_col = S.pack_x(x)
        nq, nf = len(cols), x_dim - len(cols)
        rec_bytes = 4 * nf + 4 * ((nq + 3) // 4)
        assert rec.dtype == np.uint8 and rec.shape == (37, rec_bytes) and rec.flags["C_CONTIGUOUS"]
        assert x_col.dtype == np.int32 and x_col.shape == (x_dim,)
        # the table: floats first in column order, then the bytes in column order
        floats = [c for c in range(x_dim) if c not in cols]
        assert [int(x_col[c]) for c in floats] == [4 * k for k in range(nf)]
        assert [-int(x_col[c]) - 1 for c in cols] == [4 * nf + k for k in range(nq)]
        assert (rec[:, 4 * nf + nq:] == 0).all()                                   # the padding of the record
        for k, c in enumerate(floats):                                              # the record's own bytes
            assert np.array_equal(rec[:, 4 * k:4 * k + 4].copy().view(np.uint32)[:, 0], x.view(np.uint32)[:, c])
        for k, c in enumerate(cols):
            assert np.array_equal(rec[:, 4 * nf + k].view(np.int8), x[:, c].astype(np.int8))
        back = S.unpack_x(rec, x_col, x_dim)
        assert back.dtype == np.float32 and np.array_equal(back.view(np.uint32), x.view(np.uint32))
        assert (S.packed_x_layout(mask)[0] == x_col).all() and S.packed_x_layout(mask)[1] == rec_bytes


def test_given_byte_columns():
    x = _matrix(20, 8, {1, 2, 6}, seed=3)
    # fewer byte columns than would fit: legal (a library's common mask), and still exact
    mask = np.zeros(8, dtype=bool)
    mask[[2]] = True
    rec, x_col = S.pack_x(x, mask)
    assert rec.shape[1] == 4 * 7 + 4 and (x_col < 0).tolist() == mask.tolist()
    assert np.array_equal(S.unpack_x(rec, x_col, 8).view(np.uint32), x.view(np.uint32))
    # a column forced to byte that does not pass the rule
    mask[0] = True
    with pytest.raises(ValueError):
        S.pack_x(x, mask)
    with pytest.raises(ValueError):
        S.pack_x(x, np.zeros(7, dtype=bool))
    with pytest.raises(ValueError):
        S.unpack_x(rec, x_col[:-1], 8)


@pytest.fixture(scope="module")
def reference_shard(tmp_path_factory):
    b = with_reference_features(make_batch(40, seed=5, with_receptive_fields=False), seed=1)
    path = str(tmp_path_factory.mktemp("packed") / "ref.mkgs")
    S.write_shard(path, b)
    return b, S.Shard(path)


def test_reference_pattern_features(reference_shard):
    b, shard = reference_shard
    plain = make_batch(40, seed=5, with_receptive_fields=False)
    for k in ("p", "edge_index", "edge_attr", "batch", "y"):                        # nothing but x changed
        assert torch.equal(getattr(b, k), getattr(plain, k)), k
    x = b.x.numpy()
    assert x.shape[1] == 28 and REFERENCE_BYTE_COLUMNS == 20
    assert (x[:, :12].sum(axis=1) == 1).all() and set(np.unique(x[:, :12])) == {0.0, 1.0}
    deg = np.bincount(b.edge_index[0].numpy(), minlength=x.shape[0])
    assert np.array_equal(np.argmax(x[:, 12:16], axis=1) + 1, deg) and (x[:, 12:16].sum(axis=1) == 1).all()
    assert set(np.unique(x[:, 16])) <= {-1.0, 0.0, 1.0} and set(np.unique(x[:, 17:19])) <= {0.0, 1.0}
    assert x[:, 19].min() >= 1 and x[:, 19].max() <= 6
    assert S.classify_x_columns(x).tolist() == [True] * 20 + [False] * 8
    assert torch.equal(with_reference_features(make_batch(40, seed=5, with_receptive_fields=False), seed=1).x, b.x)


def test_footprint_of_a_packed_resident_shard(reference_shard):
    _, shard = reference_shard
    res = S.ResidentShard(shard, "cpu", packed=True)
    assert res.packed and res.rec_bytes == 52 and list(res.byte_columns) == list(range(20))
    assert res.x_col.dtype == np.int32
    assert res.x_col.tolist() == [-(32 + k) - 1 for k in range(20)] + [4 * k for k in range(8)]
    assert res.x_rec.shape == (shard.n_atoms, 52) and res.view is None
    assert np.array_equal(S.unpack_x(res.x_rec, res.x_col, 28).view(np.uint32), np.array(shard.x).view(np.uint32))
    m, a, nb = shard.n_molecules, shard.n_atoms, shard.n_edges // 2
    # records + p + bond endpoints + bond attributes + y + the two pointer arrays + the degree counts
    assert res.nbytes() == 52 * a + 12 * a + 8 * nb + 7 * nb + 4 * m + 8 * (m + 1) + 16 * m
    # atom data: 124 -> 64 bytes per atom
    unpacked_atoms, packed_atoms = (4 * 28 + 12) * a, (52 + 12) * a
    assert unpacked_atoms - packed_atoms == 60 * a
    # the unpacked form is what it was: nothing of the packed form, nothing uploaded on the CPU
    plain = S.ResidentShard(shard, "cpu")
    assert plain.packed is False and plain.x_col is None and plain.rec_bytes is None and plain.byte_columns is None
    assert plain.nbytes() == 0 and plain.tensors == {} and plain.view is None
    # the CPU loader path goes on gathering from the shard itself
    ids = [3, 3, 0, 39, 7, 12, 1, 1]
    got = next(iter(S.ResidentLoader(res, 8, ids, "cpu")))
    want = next(iter(S.ResidentLoader(plain, 8, ids, "cpu")))
    for k, off, _, _, nbytes in S.compact_layout(got.shape, 8, 28, 3, 7)[0]:        # (the gaps between the fields are not written)
        assert torch.equal(got.flat[off:off + nbytes], want.flat[off:off + nbytes]), k
    with pytest.raises(ValueError):
        S.ResidentShard(shard, "cpu", packed=True, byte_cols=[True] * 28)           # the float columns do not fit a byte
    with pytest.raises(ValueError):
        S.ResidentShard(shard, "cpu", byte_cols=[False] * 28)                       # a mask without packed=True


def test_library_exports_and_header_declares_the_packed_gather(tmp_path):
    from molkgnn_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "mkgnn_gather_compact_packed")
    assert "mkgnn_gather_compact_packed" in _lib.EXPORTS
    text = open(os.path.join(REPO, "include", "molkgnn_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+mkgnn_gather_compact_packed\s*\(\s*const\s+mkgnn_resident_shard_packed\s*\*", code)
    body = re.search(r"typedef\s+struct\s+mkgnn_resident_shard_packed\s*\{(.*?)\}\s*mkgnn_resident_shard_packed\s*;", code, flags=re.S)
    assert body is not None
    for field in ("x_rec", "x_col", "rec_bytes", "p", "bond_ij", "bond_attr", "y", "mol_atom_ptr", "mol_bond_ptr", "mol_deg",
                  "n_molecules", "x_dim", "p_dim", "e_dim"):
        assert re.search(rf"\b{field}\b", body.group(1)), field
    assert not re.search(r"\bx\s*;", body.group(1))                                  # no fp32 x in the packed struct
    assert re.search(r"#define\s+MKGNN_PACKED_MAX_X_DIM\s+160\b", code) and _lib.PACKED_MAX_X_DIM == 160
    assert _lib.ABI_VERSION == 8
    # the ctypes view has the header's size and field offsets (a C compile of the header)
    import shutil
    import subprocess
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    src = tmp_path / "sz.c"
    src.write_text('#include "molkgnn_hip.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void){printf("%zu %zu %zu %zu\\n", '
                   'sizeof(mkgnn_resident_shard_packed), offsetof(mkgnn_resident_shard_packed, x_col), '
                   'offsetof(mkgnn_resident_shard_packed, n_molecules), offsetof(mkgnn_resident_shard_packed, rec_bytes));return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)], check=True)
    sizes = [int(v) for v in subprocess.run([str(exe)], check=True, stdout=subprocess.PIPE, text=True).stdout.split()]
    V = _lib.ResidentShardPackedView
    assert sizes == [ctypes.sizeof(V), V.x_col.offset, V.n_molecules.offset, V.rec_bytes.offset]


def test_entry_point_rejects_a_bad_table_before_any_launch():
    """Host-side validation only (no GPU is touched: every case returns before the first launch)."""
    from molkgnn_amd import _lib
    lib = _lib.load()
    shape = _lib.Int64x6(64, 128, 16, 16, 16, 16)

    def call(x_dim, table, rec_bytes, x_rec=4096):
        v = _lib.ResidentShardPackedView()
        tab = np.asarray(table, dtype=np.int32)
        for k in ("p", "bond_ij", "bond_attr", "y", "mol_atom_ptr", "mol_bond_ptr", "mol_deg"):
            setattr(v, k, 4096)
        v.x_rec, v.x_col, v.n_molecules, v.x_dim, v.p_dim, v.e_dim, v.rec_bytes = x_rec, tab.ctypes.data, 10, x_dim, 3, 7, rec_bytes
        rc = lib.mkgnn_gather_compact_packed(v, 4096, 4, shape, 4, None, 0, None, None)      # (wire = null: the last thing checked)
        return rc, lib.mkgnn_last_error().decode()

    rc, msg = call(3, [0, 4, -9], 12)
    assert rc != 0 and "null pointer" in msg                                        # a good table gets through to the other checks
    for table, rec_bytes, what in (([0, 6, -9], 12, "x_col[1]"),                    # a float off its dword
                                   ([0, 12, -9], 12, "x_col[1]"),                   # a float past the record
                                   ([0, 4, -13], 12, "x_col[2]"),                   # a byte past the record
                                   ([0, 4, -9], 16, "rec_bytes"),                   # a record longer than the layout
                                   ([0, 4, -9], 10, "rec_bytes")):                  # and one that is no multiple of 4
        rc, msg = call(3, table, rec_bytes)
        assert rc != 0 and what in msg, (table, rec_bytes, msg)
    rc, msg = call(161, [0] * 161, 4 * 161)
    assert rc != 0 and "x_dim" in msg
    rc, msg = call(3, [0, 4, -9], 12, x_rec=4098)
    assert rc != 0 and "4-byte aligned" in msg
