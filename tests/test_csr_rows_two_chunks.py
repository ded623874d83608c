"""``csr_rows_kernel`` with two sixteen-byte chunks per lane (csrc/kgnn_csr.hip, template parameter ``CPL = 2``: lane l of a row's
LPR lanes holds columns 4 l and 4 (l + LPR), a wave works on twice the rows), forced for every launch of this module by
``mkgnn_debug_set_csr_chunks(2)`` whatever the dispatch takes by default -- dense sums, block-row modes 1, 2, 3 and the backward
gather, against the plain references of ``tests/_csr_reference.py``.  ``pytest -m gpu``.  Nothing here compares one form of the
kernel with another; ``tests/test_csr_rows_exact.py`` holds whatever the default dispatch launches to the same references.

Held EXACTLY, as in that module: sums equal ``seq_sum_f32``; alignment padding is written as zero; guard floats and, in mode 2,
every float outside the destination's own block keep their sentinel bits; NaN in the inputs' padding and outside the source
blocks reaches no result; handed norms are ``mkgnn_row_inv_norm`` of the written rows bit for bit (that kernel holds a row in
twice the lanes, one chunk each: the two-chunk form adds a lane's two partial sums first, which is that tree's first step);
mode 3's bytes are ``mkgnn_rows_presplit`` of mode 1's output.

Shapes: widths on both sides of every boundary of the two-chunk lane assignment -- 1 .. 5 (the second chunk of every lane idle),
16 | 17 (first second chunk at LPR = 4), 32 | 33 (LPR 4 -> 8), 64 | 65 (8 -> 16), 128 | 129 (16 -> 32), 255, 256, every residue
mod 4 among them; row counts around the two-chunk rows-per-wave count; the uniform topologies (one arm of the K = 1..4 switch per
launch, 5 the long-segment loop), ``mixed``, and ``uneven``: groups of rows with lengths (1, .., 1, 5) and (0, 4, 0, ..), so that
the wave-uniform K is set by a row other than the first and the long-segment loop runs for one row of the group.

The gather's bound is derived at ``test_gather_two_chunks_is_within_the_derived_bound``.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import _csr_child as D
from tests import _csr_reference as R

pytestmark = pytest.mark.gpu

WIDTHS = [1, 3, 4, 5, 16, 17, 28, 31, 32, 33, 63, 64, 65, 110, 112, 127, 128, 129, 255, 256]
CLAMP_INV = np.float32(1) / np.float32(1e-8)
NORM_BOUND = 2.0 ** -20          # tests/test_csr_rows_exact.py derives it: 7.5 roundings of 2^-24, a factor two on top
U = 2.0 ** -24


def rows_per_wave2(width: int) -> int:
    """Rows a wave works on with two chunks per lane: twice ``R.rows_per_wave``."""
    return 2 * R.rows_per_wave(width)


@pytest.fixture(scope="module", autouse=True)
def two_chunks():
    from molkgnn_amd import _lib
    lib = _lib.load()
    assert lib.mkgnn_debug_set_csr_chunks(2) == 0
    yield
    lib.mkgnn_debug_set_csr_chunks(0)


def uneven(n: int, rpw: int, seed: int = 0):
    """Groups of ``rpw`` rows, alternately (1, .., 1, 5) and (0, 4, 0, ..) -- for rpw = 4: (1, 1, 1, 5) and (0, 4, 0, 0)."""
    a = np.ones(rpw, dtype=np.int64)
    a[-1] = 5
    b = np.zeros(rpw, dtype=np.int64)
    b[min(1, rpw - 1)] = 4
    groups = (n + rpw - 1) // rpw
    lens = np.concatenate([a if g % 2 == 0 else b for g in range(groups)])[:n]
    rowptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(lens, out=rowptr[1:])
    col = np.random.default_rng(31 * n + rpw + seed).integers(0, n, size=int(rowptr[-1]))
    return rowptr.astype(np.int32), col.astype(np.int32)


def _topologies(n, rpw):
    return [("mixed", R.mixed(n, rpw)), ("uneven", uneven(n, rpw))] + [(f"uniform{L}", R.uniform(n, L)) for L in range(6)]


def _row_counts(rpw):
    return sorted({1, rpw - 1, rpw, rpw + 1, 16 * rpw + 1, 257} - {0})


def _w4(w):
    return w + (-w) % 4


def _f32(t, n, stride):
    return t[:n * stride].view(n, stride)


def _guards_intact(buf, n, stride, first):
    return bool((D.bits(_f32(buf, n, stride))[:, first:] == D.SENTINEL).all())


def _col_dev(col):
    return D.up(col) if col.size else torch.zeros(1, dtype=torch.int32, device=D.dev())      # never null: the pipelined kernel


def _norm_error(inv, rows):
    norm = np.linalg.norm(rows.astype(np.float64), axis=1)
    return np.abs(inv.astype(np.float64) * np.maximum(norm, 1e-8) - 1.0)


def _check_sum(tag, out, n, w, os_, w4, rowptr, col, v):
    got = _f32(out, n, os_)
    g = got[:, :w].cpu().numpy()
    ref = R.seq_sum_f32(rowptr, col, v)
    assert np.array_equal(g, ref), (tag, float(np.abs(g - ref).max()))
    assert bool((D.bits(got)[:, w:w4] == 0).all()), tag
    assert _guards_intact(out, n, os_, w4), tag
    return g


def _check_norms(tag, inv, out, os_, n, w, rows, rowptr):
    again = D.sentinel(n)
    assert D.row_inv_norm(out, os_, n, w, again) == 0, tag
    assert torch.equal(D.bits(inv), D.bits(again)), tag
    got = inv.cpu().numpy()
    err = _norm_error(got, rows)
    assert (err <= NORM_BOUND).all(), (tag, float(err.max()))
    assert (got[np.diff(rowptr) == 0] == CLAMP_INV).all(), tag
    return float(err.max())


# ---------------------------------------------------------------------------------------------- dense sums --
@pytest.mark.parametrize("width", WIDTHS)
def test_dense_sum_two_chunks_equals_the_csr_order_sum(width):
    """mkgnn_segment_sum_rows: out == seq_sum_f32, padding zero, guards intact, NaN input padding unseen, the handed norms
    mkgnn_row_inv_norm's on ``out`` bit for bit and within the norm bound."""
    rpw, w4 = rows_per_wave2(width), _w4(width)
    os_ = w4 + 4
    rng = np.random.default_rng(500 + width)
    worst = 0.0
    for n in _row_counts(rpw):
        v = rng.standard_normal((n, width)).astype(np.float32)
        src = D.up(D.padded(v, w4))
        for name, (rowptr, col) in _topologies(n, rpw):
            tag = (width, n, name)
            out, inv = D.sentinel(n * os_), D.sentinel(n)
            assert D.segment_sum(src, w4, D.up(rowptr), _col_dev(col), n, width, out, os_, inv) == 0, (tag, D.last_error())
            g = _check_sum(tag, out, n, width, os_, w4, rowptr, col, v)
            worst = max(worst, _check_norms(tag, inv, out, os_, n, width, g, rowptr))
    print(f"CSR-WORST two-chunk fused-norm width={width} {worst:.3e} bound={NORM_BOUND:.3e}")


# ------------------------------------------------------------------------------------------------ block rows --
# 10 | 20 | 30 | 50 at LPR = 16: lanes straddle the block edges at columns 10 and 30 (chunks 2 and 7), the edge at 60 is
# aligned, block 4 spans both chunks of most lanes; 66 | 2 | 0 | 42: block 2 = columns 66, 67 lies inside the second chunk of
# lane 0 only, block 3 is absent; 5 | 11 | 0 | 12 (K = 28, LPR = 4): edges inside the first and the second chunk of a lane;
# 0 | 0 | 0 | 130 (LPR = 32): one block over both chunks of every lane, the others absent
LAYOUTS = [(10, 20, 30, 50), (66, 2, 0, 42), (5, 11, 0, 12), (0, 0, 0, 130)]


@pytest.mark.parametrize("Ls", LAYOUTS, ids=lambda L: "-".join(map(str, L)))
def test_block_rows_two_chunks_are_exact_and_touch_nothing_else(Ls):
    """mkgnn_segment_sum_block_rows, NaN outside every source's own block.  Mode 1: out == seq_sum_f32 of the zero-filled dense
    input, padding zero, guards intact, norms mkgnn_row_inv_norm's bit for bit.  Mode 2: the destination's own block ==
    seq_sum_f32 restricted to it, every other float of the buffer keeps its sentinel.  Mode 3: the bytes of mkgnn_rows_presplit
    on mode 1's output, and its norms."""
    K = sum(Ls)
    w4 = _w4(K)
    os_ = w4 + 4
    rpw = rows_per_wave2(K)
    rng = np.random.default_rng(700 + K + Ls[0])
    for n in _row_counts(rpw):
        deg = R.degrees(n)
        mask = R.block_mask(deg, Ls)
        full = rng.standard_normal((n, K)).astype(np.float32)
        masked = np.where(mask, full, np.float32(0))
        blocks = D.up(R.block_store(full, mask, w4))
        dense = D.up(D.padded(full, w4))
        for name, (rowptr, col) in (("mixed", R.mixed(n, rpw)), ("uneven", uneven(n, rpw)), ("uniform4", R.uniform(n, 4))):
            tag = (Ls, n, name)
            rowptr_d, col_d = D.up(rowptr), _col_dev(col)
            packed = D.up(R.pack_col(col, deg)) if col.size else col_d
            out1, inv1 = D.sentinel(n * os_), D.sentinel(n)
            assert D.block_sum(blocks, w4, rowptr_d, packed, None, n, Ls, 1, out1, os_, inv1) == 0, (tag, D.last_error())
            g = _check_sum(tag + (1,), out1, n, K, os_, w4, rowptr, col, masked)
            _check_norms(tag + (1,), inv1, out1, os_, n, K, g, rowptr)
            out2 = D.sentinel(n * os_)
            assert D.block_sum(dense, w4, rowptr_d, col_d, D.up(deg), n, Ls, 2, out2, os_, None) == 0, (tag, D.last_error())
            got = D.bits(_f32(out2, n, os_)).cpu().numpy()
            m = np.zeros((n, os_), dtype=bool)
            m[:, :K] = mask
            assert np.array_equal(got[m].view(np.float32), R.seq_sum_f32(rowptr, col, full)[mask]), tag
            assert (got[~m] == D.SENTINEL).all(), tag
            out3, inv3 = D.sentinel(n * os_), D.sentinel(n)
            assert D.block_sum(blocks, w4, rowptr_d, packed, None, n, Ls, 3, out3, os_, inv3) == 0, (tag, D.last_error())
            outs, invs = D.sentinel(n * os_), D.sentinel(n)
            assert D.presplit(out1, os_, n, K, invs, outs, os_) == 0, (tag, D.last_error())
            assert torch.equal(D.bits(out3), D.bits(outs)), tag
            assert torch.equal(D.bits(inv3), D.bits(inv1)) and torch.equal(D.bits(invs), D.bits(inv1)), tag


# ---------------------------------------------------------------------------------------------------- gather --
def _gather(contrib, cs, rowptr, rows, x, xs, inv, n, F, gx, gxs, x_split) -> int:
    """mkgnn_debug_backward_gather: the pipelined gather on buffers the caller owns."""
    from molkgnn_amd import _lib
    fn = _lib.load().mkgnn_debug_backward_gather
    P, I64, I32 = C.c_void_p, C.c_int64, C.c_int32
    fn.restype, fn.argtypes = C.c_int, [P, I64, P, P, P, I64, P, I64, I32, P, I64, I32, P]
    return fn(contrib.data_ptr(), cs, rowptr.data_ptr(), rows.data_ptr(), x.data_ptr(), xs, inv.data_ptr(), n, F, gx.data_ptr(), gxs,
              x_split, _lib.stream_ptr(D.dev()))


def _gather_reference(rowptr, rows, contrib, x, dtype):
    """d/dx of x / max(|x|, eps) applied to the segment sum, evaluated in ``dtype`` from the fp32 inputs."""
    acc = R.sum_f64(rowptr, rows, contrib) if dtype == np.float64 else R.seq_sum_f32(rowptr, rows, contrib)
    xd = x.astype(dtype)
    norm = np.sqrt((xd * xd).sum(axis=1, dtype=dtype)).astype(dtype)
    inv = (dtype(1) / np.maximum(norm, dtype(1e-8))).astype(dtype)
    xh = xd * inv[:, None]
    dot = (acc * xh).sum(axis=1, dtype=dtype).astype(dtype)
    full = (acc - dot[:, None] * xh) * inv[:, None]
    clamped = norm < dtype(1e-8)
    return np.where(clamped[:, None], acc * inv[:, None], full).astype(dtype), xh.astype(np.float64), inv.astype(np.float64)


@pytest.mark.parametrize("x_split", [0, 1], ids=["rows_fp32", "rows_presplit"])
@pytest.mark.parametrize("width", [28, 110])
def test_gather_two_chunks_is_within_the_derived_bound(width, x_split):
    """The backward gather gx_j = J(x_j) A_j, A_j = sum_k contrib[rows[k]] in CSR order, J the Jacobian of x / max(|x|, eps):
    (A - (A . xh) xh) inv with xh = x inv, inv = 1 / max(|x|, eps), or A inv where the clamp is active -- against the same formula
    in float64 on the float64 segment sum.  With u = 2^-24, len the segment's length, S_c = sum_k |contrib[rows[k], c]| and
    M = sum_c S_c |xh_c| (both in float64; |A_c| <= S_c, |A . xh| <= M):

    * A_c carries (len - 1) u S_c (seq_sum_bound);
    * the handed inv is within 2^-20 = 16 u of 1 / max(|x|, eps) (the norm bound), xh_c = fl(x_c inv) adds one rounding: 17 u |xh_c|;
      pre-split rows add two fp16 roundings, 4 u |xh_c|, and at most 2^-32 absolute (call it e);
    * the dot product is one product, three fused steps and at most 6 tree adds -- 10 roundings of partial sums bounded by M --
      on operands carrying the errors above: (len - 1 + 17 + 4 + 10) u M + e T with T = sum_c S_c;
    * r_c = fl(fl(A_c - dot xh_c) inv): the fused step rounds once, u (S_c + M |xh_c|); dot xh_c carries the dot product's error
      times |xh_c| plus M (17 + 4) u |xh_c| + M e; the final product one rounding and inv's 16 u.

    Summed, first order: |gx_c - ref_c| <= inv u ((len + 17) S_c + (len + 69) M |xh_c|) + inv e (T |xh_c| + M), e = 0 without
    pre-split rows; asserted with len + 20 and len + 72 (the two spare counts cover the second-order terms).  A clamped row is
    A_c inv: len u S_c inv, inside the same form.  The fp32 evaluation of the reference on the CPU (numpy: CSR-order sum, plain
    products, pairwise row sums) is held to the same bound and its worst ratio printed beside the kernel's: the yardstick for
    what fp32 gives on these inputs.  Padding of gx is written as zero; guards keep their sentinel."""
    rpw, w4 = rows_per_wave2(width), _w4(width)
    os_ = w4 + 4
    rng = np.random.default_rng(900 + width)
    worst_k = worst_c = 0.0
    for n in (1, rpw + 1, 257):
        contrib = rng.standard_normal((n, width)).astype(np.float32)
        x = (rng.standard_normal((n, width)) * np.exp2(rng.integers(-3, 4, size=(n, 1)))).astype(np.float32)
        x[n // 2] = np.float32(1e-10)                                   # one clamped row: |x| < eps, inv = 1 / eps
        src = D.up(D.padded(contrib, w4))
        xrows = D.up(D.padded(x, w4))
        inv = D.sentinel(n)
        if x_split:
            xd = D.sentinel(n * w4)
            assert D.presplit(xrows, w4, n, width, inv, xd, w4) == 0, D.last_error()
        else:
            xd = xrows
            assert D.row_inv_norm(xrows, w4, n, width, inv) == 0, D.last_error()
        assert inv.cpu().numpy()[n // 2] == CLAMP_INV
        for name, (rowptr, rows) in _topologies(n, rpw):
            tag = (width, x_split, n, name)
            gx = D.sentinel(n * os_)
            rc = _gather(src, w4, D.up(rowptr), _col_dev(rows), xd, w4, inv, n, width, gx, os_, x_split)
            assert rc == 0, (tag, rc)
            got = _f32(gx, n, os_)
            assert bool((got[:, width:w4] == 0).all()), tag
            assert _guards_intact(gx, n, os_, w4), tag
            g = got[:, :width].cpu().numpy().astype(np.float64)
            ref, xh, inv64 = _gather_reference(rowptr, rows, contrib, x, np.float64)
            S = R.abs_sum_f64(rowptr, rows, contrib)
            M = (S * np.abs(xh)).sum(axis=1)[:, None]
            T = S.sum(axis=1)[:, None]
            ln = np.diff(rowptr.astype(np.int64))[:, None]
            e = 2.0 ** -32 if x_split else 0.0
            bound = inv64[:, None] * (U * ((ln + 20) * S + (ln + 72) * M * np.abs(xh)) + e * (T * np.abs(xh) + M))
            err = np.abs(g - ref)
            assert (err <= bound).all(), (tag, float((err / np.maximum(bound, 1e-300)).max()))
            cpu32, _, _ = _gather_reference(rowptr, rows, contrib, x, np.float32)
            err_c = np.abs(cpu32.astype(np.float64) - ref)
            assert (err_c <= bound).all(), (tag, "fp32 on the CPU")
            nz = bound > 0
            if nz.any():
                worst_k = max(worst_k, float((err[nz] / bound[nz]).max()))
                worst_c = max(worst_c, float((err_c[nz] / bound[nz]).max()))
            assert (err[~nz] == 0).all(), tag                        # empty segments: exact zeros
    print(f"CSR-WORST two-chunk gather width={width} x_split={x_split} error / bound: kernel {worst_k:.3f}, fp32 on the CPU {worst_c:.3f}")
