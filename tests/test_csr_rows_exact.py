"""Exact leg of the CSR row passes: ``csr_rows_kernel`` (dense sums, block-row modes 1, 2, 3), ``row_inv_norm_aligned_kernel``,
``row_presplit_kernel`` (csrc/kgnn_csr.hip) and their one-row-per-wave fallbacks (csrc/kgnn_generic.hip), as operators on buffers
this file owns, against the plain references of ``tests/_csr_reference.py``.  ``pytest -m gpu``.

What is held EXACTLY (the kernels' headers promise CSR-order sums and fixed reduction trees):

* every segment sum equals ``seq_sum_f32`` -- the fp32 sum in CSR order -- on every element (numerically: the kernels add masked
  terms as +0, so a sum may be +0 where the reference has -0), in the pipelined kernel and in both forms of the fallback, whose
  order is the CSR order too (``acc = 0; acc += in[col[k]]`` for ascending k, eight per round);
* alignment padding of ``out`` is written as zero by the pipelined kernel; guard floats behind every row, and in mode 2 every
  float outside the destination's own block, keep their sentinel bits; NaN in the inputs' padding and outside the source blocks
  reaches no result;
* block rows mode 1 equals the dense sum of the zero-filled input, mode 3 is ``mkgnn_rows_presplit`` of mode 1's output byte for
  byte, handed norms are bit-identical to ``mkgnn_row_inv_norm`` on the written rows; results do not depend on the grid.

What is held to a DERIVED bound (nothing below is taken from a run):

* sums against float64: ``|out - sum_f64| <= (len - 1) * 2^-24 * sum_k |in[col[k]]|`` (len - 1 adds, half an ulp each, of partial
  sums no larger than the sum of magnitudes) -- implied by the equality above, asserted as the floor should equality ever go;
* norms: ``|inv * max(||x||_64, 1e-8) - 1| <= 2^-20``.  The sum of squares is one product, three fused steps and log2(LPR) <= 6 tree
  adds of non-negative terms: at most 10 roundings of 2^-24, halved by the square root; the correctly rounded square root, the
  division and fp32(1e-8) add 2.5 more: 7.5 * 2^-24 < 2^-21, the bound carries a factor two.  The fallback's chain at width 300 is
  6 fused steps per lane (three pairs) and 6 tree adds: 12 roundings halved, plus 2.5: 8.5 * 2^-24 < 2^-20 as well;
* pre-split rows: ``|x_i - decode_i| <= 2^-22 |x_i| + 2^-32 * max(||x||, 1e-8)``: two fp16 roundings give 2^-22 of an element while
  ``lo`` is normal, else 2^-25 in scaled units where the scaled row norm lies in (128, 256].

The worst figures seen are printed (``pytest -s``) as ``CSR-WORST`` lines; DESIGN.md section 0 records them.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import _csr_child as D
from tests import _csr_reference as R

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDTHS = [1, 3, 4, 5, 28, 32, 33, 64, 65, 110, 128, 129, 200, 255, 256]
CLAMP_INV = np.float32(1) / np.float32(1e-8)
NORM_BOUND = 2.0 ** -20


def _dev():
    return D.dev()


def _topologies(n, rpw):
    return [("mixed", R.mixed(n, rpw))] + [(f"uniform{L}", R.uniform(n, L)) for L in range(6)]


def _w4(w):
    return w + (-w) % 4


def _f32(t, n, stride):
    return t[:n * stride].view(n, stride)


def _guards_intact(buf, n, stride, first):
    """Columns ``first`` .. of every row of the flat buffer still hold the sentinel bits."""
    return bool((D.bits(_f32(buf, n, stride))[:, first:] == D.SENTINEL).all())


def _norm_error(inv: np.ndarray, rows: np.ndarray) -> np.ndarray:
    """|inv * max(||x||_64, 1e-8) - 1| per row, the rows fp32 values read in float64."""
    norm = np.linalg.norm(rows.astype(np.float64), axis=1)
    return np.abs(inv.astype(np.float64) * np.maximum(norm, 1e-8) - 1.0)


def _check_sum(tag, out, n, w, os_, first_guard, rowptr, col, v, pad_zero):
    """out (flat device buffer, row stride os_) against the references of the sum of the rows v (numpy [*, w])."""
    got = _f32(out, n, os_)
    ref32 = R.seq_sum_f32(rowptr, col, v)
    g = got[:, :w].cpu().numpy()
    assert np.array_equal(g, ref32), (tag, float(np.abs(g - ref32).max()))
    if pad_zero:
        assert bool((D.bits(got)[:, w:first_guard] == 0).all()), tag
    assert _guards_intact(out, n, os_, first_guard), tag
    assert (np.abs(g.astype(np.float64) - R.sum_f64(rowptr, col, v)) <= R.seq_sum_bound(rowptr, col, v)).all(), tag
    return g


# ---------------------------------------------------------------------------------------------- dense sums --
@pytest.mark.parametrize("width", WIDTHS)
def test_dense_segment_sum_equals_the_csr_order_sum(width):
    """mkgnn_segment_sum_rows on aligned storage (the pipelined kernel): every uniform topology (one arm of the K = 1..4 switch per
    launch, L = 5 the long-segment loop, L = 0 an index list that is never dereferenced) and ``mixed``, at row counts around the
    rows-per-wave count: out == seq_sum_f32, padding zero, guards intact, NaN input padding unseen, handed norms bit-identical to
    mkgnn_row_inv_norm on out and within the norm bound."""
    rpw, w4 = R.rows_per_wave(width), _w4(width)
    os_ = w4 + 4
    rng = np.random.default_rng(width)
    worst = 0.0
    for n in sorted({1, rpw - 1, rpw, rpw + 1, 16 * rpw + 1, 257} - {0}):
        v = rng.standard_normal((n, width)).astype(np.float32)
        src = D.up(D.padded(v, w4))
        for name, (rowptr, col) in _topologies(n, rpw):
            tag = (width, n, name)
            col_d = D.up(col) if col.size else torch.zeros(1, dtype=torch.int32, device=_dev())     # never null here: the pipelined kernel
            out, inv = D.sentinel(n * os_), D.sentinel(n)
            assert D.segment_sum(src, w4, D.up(rowptr), col_d, n, width, out, os_, inv) == 0, (tag, D.last_error())
            g = _check_sum(tag, out, n, width, os_, w4, rowptr, col, v, pad_zero=True)
            again = D.sentinel(n)
            assert D.row_inv_norm(out, os_, n, width, again) == 0, tag
            assert torch.equal(D.bits(inv), D.bits(again)), tag
            err = _norm_error(inv.cpu().numpy(), g)
            assert (err <= NORM_BOUND).all(), (tag, float(err.max()))
            assert (inv.cpu().numpy()[np.diff(rowptr) == 0] == CLAMP_INV).all(), tag
            worst = max(worst, float(err.max()))
    print(f"CSR-WORST fused-norm width={width} {worst:.3e} bound={NORM_BOUND:.3e}")


FALLBACKS = {
    # name: (width, in stride, out stride, base offset in floats)          which kernel takes it
    "odd_stride": (28, 29, 29, 0),                                       # scalar form
    "offset_4_bytes": (28, 32, 32, 1),                                   # scalar form (bases 4 bytes off)
    "offset_8_bytes": (28, 32, 32, 2),                                   # VEC2 form (8-byte aligned only)
    "width_257": (257, 260, 260, 0),                                     # scalar form, three column rounds
    "width_300": (300, 300, 304, 0),                                     # VEC2 form, three column rounds
    "even_stride": (30, 30, 34, 0),                                      # VEC2 form
    "odd_width": (7, 7, 9, 0),                                           # scalar form
}


@pytest.mark.parametrize("case", sorted(FALLBACKS))
def test_fallback_segment_sum_equals_the_csr_order_sum(case):
    """segment_sum_rows_kernel<VEC2> (one row per wave): its order IS the CSR order -- ``acc = 0`` then ``acc += in[col[k]]`` for
    ascending k in rounds of eight -- so equality with seq_sum_f32 is asserted, not the bound alone.  It writes the width only:
    everything else of ``out`` keeps its sentinel.  The handed norms are mkgnn_row_inv_norm's on ``out``, bit for bit."""
    width, is_, os_, off = FALLBACKS[case]
    rng = np.random.default_rng(len(case))
    for n in (1, 5, 257):
        v = rng.standard_normal((n, width)).astype(np.float32)
        src = torch.cat([D.sentinel(off), D.up(D.padded(v, is_)).reshape(-1)])[off:] if off else D.up(D.padded(v, is_)).reshape(-1)
        for name, (rowptr, col) in _topologies(n, 1):
            tag = (case, n, name)
            buf, inv, again = D.sentinel(n * os_ + off), D.sentinel(n), D.sentinel(n)
            out = buf[off:]
            assert src.data_ptr() % 16 == 4 * off % 16 and out.data_ptr() % 16 == 4 * off % 16
            rc = D.segment_sum(src, is_, D.up(rowptr), D.up(col) if col.size else None, n, width, out, os_, inv)
            assert rc == 0, (tag, D.last_error())
            g = _check_sum(tag, out, n, width, os_, width, rowptr, col, v, pad_zero=False)
            assert bool((D.bits(buf)[:off] == D.SENTINEL).all()), tag
            assert D.row_inv_norm(out, os_, n, width, again) == 0, tag
            assert torch.equal(D.bits(inv), D.bits(again)), tag
            err = _norm_error(inv.cpu().numpy(), g)
            assert (err <= NORM_BOUND).all(), (tag, float(err.max()))


@pytest.mark.parametrize("width", [28, 110])
def test_empty_topology_takes_the_fallback_and_gives_zero_rows(width):
    """No entries at all and a null index pointer (what ``functional._segment_sum`` passes for an empty list): the pipelined
    kernel declines, the fallback writes zero rows of the width and clamped norms."""
    w4 = _w4(width)
    for n in (1, 9, 257):
        rowptr, col = R.empty(n)
        src = D.up(D.padded(np.ones((n, width), dtype=np.float32), w4))
        out, inv = D.sentinel(n * (w4 + 4)), D.sentinel(n)
        assert D.segment_sum(src, w4, D.up(rowptr), None, n, width, out, w4 + 4, inv) == 0, D.last_error()
        assert bool((D.bits(_f32(out, n, w4 + 4))[:, :width] == 0).all())
        assert _guards_intact(out, n, w4 + 4, w4)
        assert (inv.cpu().numpy() == CLAMP_INV).all()


# ------------------------------------------------------------------------------- steady state of the pipeline --
STEADY = [(200, 40_000), (110, 70_000), (60, 140_000), (28, 270_000)]


@pytest.fixture(scope="module", params=STEADY, ids=lambda p: f"w{p[0]}_n{p[1]}")
def steady(request):
    """One case per lanes-per-row variant with more than two loop iterations per wave at the default grid (16 384 waves): the
    mixed topology tiled to size, the CPU references and every pass's output, built once and shared by the four mode tests."""
    width, n = request.param
    assert n > 2 * 16384 * R.rows_per_wave(width)
    c = D.case_inputs(width, n)
    refs = dict(full=R.seq_sum_f32(c["rowptr"], c["col"], c["full"]), masked=R.seq_sum_f32(c["rowptr"], c["col"], c["masked"]))
    return width, n, c, refs, D.run_case(width, n, c)


def _rows_of(a, n, stride):
    return a.reshape(n, stride)


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_pipeline_steady_state_is_exact(steady, mode):
    """Row pointers two groups ahead, indices one group ahead (and the destination degree of mode 2) for waves that walk three and
    more groups: the same exact assertions as the small cases."""
    width, n, c, refs, res = steady
    w4 = _w4(width)
    os_ = w4 + 4
    if mode in (0, 1):
        out = _rows_of(res["dense" if mode == 0 else "mode1"], n, os_)
        ref = refs["full" if mode == 0 else "masked"]
        assert np.array_equal(out[:, :width].view(np.float32), ref)
        assert (out[:, width:w4] == 0).all() and (out[:, w4:] == D.SENTINEL).all()
        inv = res["dense_inv" if mode == 0 else "mode1_inv"].view(np.float32)
        err = _norm_error(inv, ref)
        assert (err <= NORM_BOUND).all(), float(err.max())
        if mode == 1:
            assert np.array_equal(res["norm"], res["mode1_inv"])
    elif mode == 2:
        out = _rows_of(res["mode2"], n, os_)
        mask = np.zeros((n, os_), dtype=bool)
        mask[:, :width] = c["mask"]
        assert np.array_equal(out[mask].view(np.float32), refs["full"][c["mask"]])
        assert (out[~mask] == D.SENTINEL).all()
    else:
        assert np.array_equal(res["mode3"], res["split"])
        assert np.array_equal(res["mode3_inv"], res["mode1_inv"]) and np.array_equal(res["split_inv"], res["mode1_inv"])


# --------------------------------------------------------------------------------------- grid independence --
def test_results_do_not_depend_on_the_grid(tmp_path):
    """Per-row sums in a fixed order: one block (four waves, each walking five or more groups) and three blocks must give the bits
    the default grid gives.  MKGNN_CSR_BLOCKS is read once per process: a fresh child per value, this process leaves it unset."""
    assert "MKGNN_CSR_BLOCKS" not in os.environ
    cases = [[w, 4 * R.rows_per_wave(w) * 5 + 3] for w in (28, 60, 110, 200)]
    want = D.run_cases(cases)
    for blocks in ("1", "3"):
        path = tmp_path / f"blocks{blocks}.npz"
        env = dict(os.environ, MKGNN_CSR_BLOCKS=blocks)
        done = subprocess.run([sys.executable, "-m", "tests._csr_child", json.dumps(cases), str(path)], cwd=REPO, env=env,
                              capture_output=True, text=True, timeout=120)
        assert done.returncode == 0, (blocks, done.returncode, done.stderr[-2000:])
        with np.load(path) as got:
            assert sorted(got.files) == sorted(want)
            for k in want:
                assert np.array_equal(got[k], want[k]), (blocks, k)


# ------------------------------------------------------------------------------------------------ block rows --
LAYOUTS = [(10, 20, 30, 50), (5, 10, 15, 25), (1, 1, 1, 1), (3, 0, 7, 6), (1, 0, 0, 1), (2, 3, 0, 0), (16, 32, 48, 64),
           (63, 64, 64, 64), (0, 0, 0, 9)]


@pytest.mark.parametrize("Ls", LAYOUTS, ids=lambda L: "-".join(map(str, L)))
def test_block_rows_are_exact_and_touch_nothing_else(Ls):
    """mkgnn_segment_sum_block_rows: blocks that start and end inside one float4, blocks shorter than 4, absent blocks, K < 4 and
    K = 255.  Mode 1: NaN outside the source blocks, out == seq_sum_f32 of the zero-filled dense input, padding zero, guards intact,
    norms bit-identical to the dense call's.  Mode 2: every destination's own block == seq_sum_f32 restricted to it and EVERY other
    float of the buffer keeps its sentinel.  Mode 3: the bytes of mkgnn_rows_presplit on mode 1's output, the same norms."""
    K = sum(Ls)
    w4 = _w4(K)
    os_ = w4 + 4
    rpw = R.rows_per_wave(K)
    rng = np.random.default_rng(K + Ls[0])
    for n in (rpw + 1, 257):
        rowptr, col = R.mixed(n, rpw)
        deg = R.degrees(n)
        dst_deg = deg[np.diff(rowptr) > 0]
        if n == 257:
            assert set(deg[col].tolist()) == {0, 1, 2, 3, 4} and set(dst_deg.tolist()) == {0, 1, 2, 3, 4} and (deg == 0).any()
        mask = R.block_mask(deg, Ls)
        full = rng.standard_normal((n, K)).astype(np.float32)
        masked = np.where(mask, full, np.float32(0))
        if col.size:
            rowptr_d, col_d, packed = D.up(rowptr), D.up(col), D.up(R.pack_col(col, deg))
        else:                                        # (two rows, both empty: the entry wants a pointer, the kernel never follows it)
            rowptr_d, col_d, packed = D.up(rowptr), torch.zeros(1, dtype=torch.int32, device=_dev()), torch.zeros(1, dtype=torch.int32, device=_dev())
        blocks = D.up(R.block_store(full, mask, w4))
        # mode 1 against the reference and the dense call
        out1, inv1 = D.sentinel(n * os_), D.sentinel(n)
        assert D.block_sum(blocks, w4, rowptr_d, packed, None, n, Ls, 1, out1, os_, inv1) == 0, D.last_error()
        _check_sum((Ls, n, 1), out1, n, K, os_, w4, rowptr, col, masked, pad_zero=True)
        outd, invd = D.sentinel(n * os_), D.sentinel(n)
        assert D.segment_sum(D.up(D.padded(masked, w4)), w4, rowptr_d, col_d, n, K, outd, os_, invd) == 0, D.last_error()
        assert torch.equal(D.bits(inv1), D.bits(invd))
        assert torch.equal(_f32(out1, n, os_)[:, :K], _f32(outd, n, os_)[:, :K])
        # mode 2
        out2 = D.sentinel(n * os_)
        assert D.block_sum(D.up(D.padded(full, w4)), w4, rowptr_d, col_d, D.up(deg), n, Ls, 2, out2, os_, None) == 0, D.last_error()
        got = D.bits(_f32(out2, n, os_)).cpu().numpy()
        m = np.zeros((n, os_), dtype=bool)
        m[:, :K] = mask
        assert np.array_equal(got[m].view(np.float32), R.seq_sum_f32(rowptr, col, full)[mask]), (Ls, n)
        assert (got[~m] == D.SENTINEL).all(), (Ls, n)
        # mode 3
        out3, inv3 = D.sentinel(n * os_), D.sentinel(n)
        assert D.block_sum(blocks, w4, rowptr_d, packed, None, n, Ls, 3, out3, os_, inv3) == 0, D.last_error()
        outs, invs = D.sentinel(n * os_), D.sentinel(n)
        assert D.presplit(out1, os_, n, K, invs, outs, os_) == 0, D.last_error()
        assert torch.equal(D.bits(out3), D.bits(outs)), (Ls, n)
        assert torch.equal(D.bits(inv3), D.bits(inv1)) and torch.equal(D.bits(invs), D.bits(inv1))


def test_block_rows_refusals_write_nothing():
    """K = 256 (the packed column tables hold 6-bit float4 indices and byte offsets: 255 is the limit), a stride that is no multiple
    of 4 and mode 3 without norms return an error code before any launch; the Python wrapper refuses blocks that do not add up."""
    from molkgnn_amd import _lib
    from molkgnn_amd import functional as Fn
    n = 33
    rowptr, col = R.mixed(n, 1)
    deg = R.degrees(n)
    rowptr_d, col_d, packed = D.up(rowptr), D.up(col), D.up(R.pack_col(col, deg))

    def refused(Ls, in_stride, os_, mode, with_inv):
        src = D.up(np.ones((n, in_stride), dtype=np.float32))
        out, inv = D.sentinel(n * os_), D.sentinel(n)
        rc = D.block_sum(src, in_stride, rowptr_d, col_d if mode == 2 else packed, D.up(deg), n, Ls, mode, out, os_,
                         inv if with_inv else None)
        torch.cuda.synchronize()
        assert rc != 0 and D.last_error(), (Ls, mode)
        assert bool((D.bits(out) == D.SENTINEL).all()) and bool((D.bits(inv) == D.SENTINEL).all()), (Ls, mode)

    for mode in (1, 2, 3):
        refused((64, 64, 64, 64), 256, 256, mode, True)
        refused((10, 20, 30, 50), 111, 112, mode, True)
        refused((10, 20, 30, 50), 112, 114, mode, True)
    refused((10, 20, 30, 50), 112, 112, 3, False)
    refused((10, 20, 30, 50), 112, 112, 4, True)
    refused((10, 20, 300, 50), 380, 380, 1, True)
    v = torch.zeros(n, 112, device=_dev())[:, :110]
    with pytest.raises(_lib.MolKGNNLibraryError):
        Fn._segment_sum_blocks(v, (rowptr_d, packed), None, (10, 20, 30, 49), 1, 2, torch.empty(n, device=_dev()))


# ------------------------------------------------------------------------------------------------- row norms --
def _scaled(rng, n, w, norm):
    x = rng.standard_normal((n, w))
    x[:, 0] += 0.25                                                      # (a row of width 1 is never zero)
    return (x * (norm / np.linalg.norm(x, axis=1))[:, None]).astype(np.float32)


FAMILIES = {
    "unit": lambda rng, n, w: (rng.standard_normal((n, w)) / np.sqrt(w)).astype(np.float32),
    "norm_1e-30": lambda rng, n, w: _scaled(rng, n, w, 1e-30),
    "norm_1e-9": lambda rng, n, w: _scaled(rng, n, w, 1e-9),
    "clamp_below": lambda rng, n, w: _scaled(rng, n, w, 1e-8 * (1 - 2.0 ** -20)),
    "clamp_above": lambda rng, n, w: _scaled(rng, n, w, 1e-8 * (1 + 2.0 ** -20)),
    "norm_1e-4": lambda rng, n, w: _scaled(rng, n, w, 1e-4),
    "norm_300": lambda rng, n, w: _scaled(rng, n, w, 300.0),
    "norm_1e18": lambda rng, n, w: _scaled(rng, n, w, 1e18),
    "spread_2^20": lambda rng, n, w: (rng.standard_normal((n, w)) * np.exp2(rng.integers(0, 21, size=(n, w)))).astype(np.float32),
    "zero": lambda rng, n, w: np.zeros((n, w), dtype=np.float32),
}
# below the clamp by more than the computed norm's error (2^-21 relative at most, see the module docstring): exactly 1 / fp32(1e-8)
CLAMPED = ("norm_1e-30", "norm_1e-9", "clamp_below", "zero")


def _check_norms(tag, family, inv, x):
    err = _norm_error(inv, x)
    assert (err <= NORM_BOUND).all(), (tag, family, float(err.max()))
    if family in CLAMPED:
        assert (inv == CLAMP_INV).all(), (tag, family)
    return float(err.max())


@pytest.mark.parametrize("width", WIDTHS)
def test_row_inv_norm_is_within_its_derived_bound(width):
    """row_inv_norm_aligned_kernel at row counts around the rows-per-wave count, every input family; NaN in the padding unseen."""
    rpw, w4 = R.rows_per_wave(width), _w4(width)
    rng = np.random.default_rng(100 + width)
    worst = {}
    for n in sorted({1, rpw - 1, rpw + 1, 8 * rpw + 1} - {0}):
        for family, make in FAMILIES.items():
            x = make(rng, n, width)
            inv = D.sentinel(n + 4)
            assert D.row_inv_norm(D.up(D.padded(x, w4)), w4, n, width, inv) == 0, D.last_error()
            assert bool((D.bits(inv)[n:] == D.SENTINEL).all())
            worst[family] = max(worst.get(family, 0.0), _check_norms((width, n), family, inv[:n].cpu().numpy(), x))
    print(f"CSR-WORST row_inv_norm_aligned width={width} " + " ".join(f"{k}={v:.3e}" for k, v in worst.items()))


def _family_rows(rng, n, w):
    """Rows of every family interleaved (row i: family i mod 10), and the family index per row."""
    names = list(FAMILIES)
    x = np.empty((n, w), dtype=np.float32)
    fam = np.arange(n) % len(names)
    for f, name in enumerate(names):
        x[fam == f] = FAMILIES[name](rng, int((fam == f).sum()), w)
    return x, fam, names


@pytest.mark.parametrize("width,n", [(132, 40_000), (110, 70_000), (60, 140_000), (4, 300_000)])
def test_row_inv_norm_second_loop_iteration(width, n):
    """More than 2 * 16 384 waves' worth of row groups: the two-groups-per-iteration loop of every lanes-per-row variant runs again."""
    assert n > 2 * 16384 * R.rows_per_wave(width)
    w4 = _w4(width)
    x, fam, names = _family_rows(np.random.default_rng(width), n, width)
    inv = D.sentinel(n + 4)
    assert D.row_inv_norm(D.up(D.padded(x, w4)), w4, n, width, inv) == 0, D.last_error()
    assert bool((D.bits(inv)[n:] == D.SENTINEL).all())
    got = inv[:n].cpu().numpy()
    for f, name in enumerate(names):
        _check_norms((width, n), name, got[fam == f], x[fam == f])


NORM_FALLBACKS = {"odd_stride": (28, 29, 0), "offset_4_bytes": (28, 32, 1), "offset_8_bytes": (28, 32, 2), "width_257": (257, 260, 0),
                  "width_300": (300, 300, 0), "even_stride": (30, 30, 0), "odd_width": (7, 7, 0)}


@pytest.mark.parametrize("case", sorted(NORM_FALLBACKS))
def test_row_inv_norm_fallback_is_within_the_same_bound(case):
    """row_inv_norm_kernel<VEC2> (one row per wave, two floats per lane and 128-column round): at width 300 a lane chains 6 fused
    steps, the wave tree adds 6 more roundings: 12 * 2^-24 halved by the square root, plus 2.5 for the square root, the division
    and fp32(1e-8): 8.5 * 2^-24, inside 2^-20 = 16 * 2^-24 -- the aligned kernel's bound holds here unchanged."""
    width, stride, off = NORM_FALLBACKS[case]
    rng = np.random.default_rng(len(case) + width)
    worst = {}
    for n in (1, 5, 257):
        for family, make in FAMILIES.items():
            x = make(rng, n, width)
            src = torch.cat([D.sentinel(off), D.up(D.padded(x, stride)).reshape(-1)])[off:] if off else D.up(D.padded(x, stride))
            inv = D.sentinel(n + 4)
            assert D.row_inv_norm(src, stride, n, width, inv) == 0, D.last_error()
            assert bool((D.bits(inv)[n:] == D.SENTINEL).all())
            worst[family] = max(worst.get(family, 0.0), _check_norms((case, n), family, inv[:n].cpu().numpy(), x))
    print(f"CSR-WORST row_inv_norm_fallback case={case} " + " ".join(f"{k}={v:.3e}" for k, v in worst.items()))


# -------------------------------------------------------------------------------------------- pre-split rows --
@pytest.mark.parametrize("width", WIDTHS)
def test_presplit_rows_decode_within_the_derived_bound(width):
    """mkgnn_rows_presplit: |x_i - decode_i| <= 2^-22 |x_i| + 2^-32 max(||x||, 1e-8) in every family up to norm 1e18; the norms are
    mkgnn_row_inv_norm's bit for bit; the half-words of a partial last chunk beyond the width are zero; guards are intact."""
    rpw, w4 = R.rows_per_wave(width), _w4(width)
    os_ = w4 + 4
    rng = np.random.default_rng(200 + width)
    worst = {}
    for n in (1, rpw + 1, 8 * rpw + 1):
        for family, make in FAMILIES.items():
            x = make(rng, n, width)
            src = D.up(D.padded(x, w4))
            out, inv, again = D.sentinel(n * os_), D.sentinel(n), D.sentinel(n)
            assert D.presplit(src, w4, n, width, inv, out, os_) == 0, D.last_error()
            assert D.row_inv_norm(src, w4, n, width, again) == 0
            assert torch.equal(D.bits(inv), D.bits(again)), (width, n, family)
            assert _guards_intact(out, n, os_, w4), (width, n, family)
            rows = _f32(out, n, os_)
            back = R.decode_split(rows, width, inv).double().cpu().numpy()
            x64 = x.astype(np.float64)
            norm = np.maximum(np.linalg.norm(x64, axis=1), 1e-8)[:, None]
            err = np.abs(back - x64)
            assert (err <= 2.0 ** -22 * np.abs(x64) + 2.0 ** -32 * norm).all(), (width, n, family, float((err / norm).max()))
            halves = R.split_halves(rows, width).view(torch.int16).cpu().numpy().reshape(n, w4 // 4, 2, 4)
            tail = halves.transpose(0, 2, 1, 3).reshape(n, 2, w4)[:, :, width:]
            assert (tail == 0).all(), (width, n, family)
            worst[family] = max(worst.get(family, 0.0), float(((err - 2.0 ** -22 * np.abs(x64)) / norm).max()))
    print(f"CSR-WORST presplit width={width} (err - 2^-22|x|)/norm, bound {2.0 ** -32:.3e}: " + " ".join(f"{k}={v:.3e}" for k, v in worst.items()))


def test_presplit_refusals_write_nothing():
    """Width 257 and an unaligned stride or base return the documented error and launch nothing."""
    n = 9
    for width, xs, os_, off in ((257, 260, 260, 0), (28, 30, 32, 0), (28, 32, 30, 0), (28, 32, 32, 1)):
        src = D.up(np.ones((n * xs + 4,), dtype=np.float32))[off:]
        out, inv = D.sentinel(n * os_), D.sentinel(n)
        rc = D.presplit(src, xs, n, width, inv, out, os_)
        torch.cuda.synchronize()
        assert rc != 0 and "16-byte aligned" in D.last_error(), (width, xs, os_, off)
        assert bool((D.bits(out) == D.SENTINEL).all()) and bool((D.bits(inv) == D.SENTINEL).all())
