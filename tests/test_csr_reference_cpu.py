"""The references of ``tests/_csr_reference.py`` checked WITHOUT a GPU: a wrong reference would bless a wrong kernel.  The float64
sum against ``index_add_``, the sequential fp32 sum against a per-row Python loop and against its own rounding bound, the pre-split
decoder against a plain numpy fp16 split, the block mask against the one ``test_block_row_propagate_matches_dense_bitwise`` builds."""
import numpy as np
import pytest
import torch

from tests import _csr_reference as R


def _rows(n, w, seed):
    return np.random.default_rng(seed).standard_normal((n, w)).astype(np.float32)


def _topologies(n, rpw):
    return [("mixed", R.mixed(n, rpw))] + [(f"uniform{L}", R.uniform(n, L)) for L in range(6)] + [("empty", R.empty(n))]


@pytest.mark.parametrize("n,w", [(1, 3), (7, 5), (33, 28), (257, 110)])
def test_sum_f64_equals_index_add_and_seq_sum_f32_is_within_its_bound(n, w):
    v = _rows(n, w, n + w)
    for name, (rowptr, col) in _topologies(n, R.rows_per_wave(w)):
        assert rowptr.dtype == np.int32 and col.dtype == np.int32 and rowptr.shape == (n + 1,), name
        dst = torch.from_numpy(np.repeat(np.arange(n), np.diff(rowptr)))
        ref = torch.zeros(n, w, dtype=torch.float64).index_add_(0, dst, torch.from_numpy(v).double()[torch.from_numpy(col).long()])
        s64 = R.sum_f64(rowptr, col, v)
        # (index_add_ adds in the same order here -- one thread, ascending k -- but nothing promises it: a float64 rounding of slack)
        assert np.abs(s64 - ref.numpy()).max(initial=0.0) <= 2.0 ** -50 * max(1.0, np.abs(ref.numpy()).max(initial=0.0)), name
        s32 = R.seq_sum_f32(rowptr, col, v)
        assert s32.dtype == np.float32
        bound = R.seq_sum_bound(rowptr, col, v)
        assert (np.abs(s32.astype(np.float64) - s64) <= bound).all(), name
        lens = np.diff(rowptr)
        assert (s32[lens == 0] == 0).all() and (bound[lens <= 1] == 0).all(), name


def test_seq_sum_f32_equals_a_per_row_loop():
    n, w = 41, 6
    v = _rows(n, w, 3)
    rowptr, col = R.mixed(n, 8)
    want = np.zeros((n, w), dtype=np.float32)
    for i in range(n):
        for c in range(w):
            acc = np.float32(0)
            for t, k in enumerate(range(rowptr[i], rowptr[i + 1])):
                acc = v[col[k], c] if t == 0 else np.float32(acc + v[col[k], c])
            want[i, c] = acc
    assert np.array_equal(R.seq_sum_f32(rowptr, col, v), want)
    # the order matters at this precision: the reversed sum differs somewhere, so equality with the kernel is a statement
    rev = np.zeros_like(want)
    for i in range(n):
        for k in range(rowptr[i + 1] - 1, rowptr[i] - 1, -1):
            rev[i] = rev[i] + v[col[k]]
    assert not np.array_equal(rev, want)


@pytest.mark.parametrize("rpw", [1, 2, 4, 8])
def test_mixed_topology_has_what_it_promises(rpw):
    for n in (rpw + 1, 16 * rpw + 1, 257, 20 * rpw + 3):
        rowptr, col = R.mixed(n, rpw)
        lens = np.diff(rowptr)
        assert lens[0] == 0 and lens[-1] == 0 and set(lens.tolist()) <= set(R.MIXED_LENGTHS)
        assert col.size == 0 or (col.min() >= 0 and col.max() < n)
    rowptr, col = R.mixed(257, rpw)
    lens = np.diff(rowptr)
    assert set(lens.tolist()) == set(R.MIXED_LENGTHS)
    row_of = np.repeat(np.arange(257), lens)
    assert (col == row_of).any()                                         # self references
    assert any(len(set(col[rowptr[i]:rowptr[i + 1]].tolist())) < lens[i] for i in range(257))     # repeated entries
    longest = {int(lens[g:g + rpw].max()) for g in range(0, 257, rpw)}
    assert {1, 2, 3, 4} <= longest and max(longest) > 4                  # every arm of the kernel's switch, and the long loop
    t_rowptr, t_col = R.tile_to(rowptr, col, 1000)
    assert np.array_equal(np.diff(t_rowptr)[:257], lens) and np.array_equal(np.diff(t_rowptr)[257:514], lens)
    assert t_col.max() < 1000 and t_rowptr[-1] == t_col.shape[0]
    for L in range(6):
        u_rowptr, u_col = R.uniform(13, L)
        assert (np.diff(u_rowptr) == L).all() and u_col.shape == (13 * L,)


@pytest.mark.parametrize("width", [1, 3, 4, 5, 28, 110, 255])
def test_decode_split_inverts_a_numpy_fp16_split(width):
    rng = np.random.default_rng(width)
    x = (rng.standard_normal((50, width)) * np.exp2(rng.integers(-20, 20, size=(50, 1)))).astype(np.float32)
    inv = (1.0 / np.maximum(np.linalg.norm(x.astype(np.float64), axis=1), 1e-8)).astype(np.float32)
    store = R.split_rows_numpy(x, inv)
    back = R.decode_split(torch.from_numpy(store), width, torch.from_numpy(inv)).double().numpy()
    # two fp16 roundings of the scaled value: 2^-22 of the element, or (lo subnormal) 2^-25 scaled, the scaled norm in (128, 256]
    norm = np.linalg.norm(x.astype(np.float64), axis=1)[:, None]
    assert (np.abs(back - x) <= 2.0 ** -22 * np.abs(x) + 2.0 ** -32 * norm).all()
    assert float(np.abs(back - x).max()) > 0.0                           # (it is a rounding, not a copy)
    w4 = (width + 3) // 4 * 4
    halves = R.split_halves(torch.from_numpy(store), width).float().numpy()
    hi = halves[:, :, 0, :].reshape(50, w4)
    assert (hi[:, width:] == 0).all()
    e = ((inv.view(np.int32) >> 23) & 0xFF) - 127 + 8
    assert np.array_equal(hi[:, :width], (x * np.exp2(e.astype(np.float32))[:, None]).astype(np.float16).astype(np.float32))


@pytest.mark.parametrize("Ls", [(10, 20, 30, 50), (3, 0, 7, 6), (16, 16, 16, 16), (1, 0, 0, 1), (0, 0, 0, 9)])
def test_block_helpers_agree_with_the_inline_mask_of_the_parity_test(Ls):
    n = 64
    deg_np = R.degrees(n)
    assert set(deg_np.tolist()) == {0, 1, 2, 3, 4}
    # (the mask as tests/test_hip_parity.py::test_block_row_propagate_matches_dense_bitwise builds it)
    K = sum(Ls)
    offs = [0, Ls[0], Ls[0] + Ls[1], Ls[0] + Ls[1] + Ls[2]]
    deg = torch.from_numpy(deg_np).long()
    col = torch.arange(K)[None, :]
    lo = torch.tensor([0] + offs)[deg][:, None]
    ln = torch.tensor([0] + list(Ls))[deg][:, None]
    inblock = (col >= lo) & (col < lo + ln)
    mask = R.block_mask(deg_np, Ls)
    assert np.array_equal(mask, inblock.numpy())
    dense = _rows(n, K, 5)
    store = R.block_store(dense, mask, K + (-K) % 4 + 4)
    assert np.array_equal(store[:, :K][mask], dense[mask]) and np.isnan(store[:, :K][~mask]).all() and np.isnan(store[:, K:]).all()
    rowptr, c = R.mixed(n, 8)
    packed = R.pack_col(c, deg_np)
    assert packed.dtype == np.int32
    assert np.array_equal(packed & 0x0FFFFFFF, c) and np.array_equal((packed >> 28) & 7, deg_np[c].astype(np.int32))
