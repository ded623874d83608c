"""Plain references for the CSR row passes (csrc/kgnn_csr.hip, and their one-row-per-wave fallbacks in csrc/kgnn_generic.hip):
what ``mkgnn_segment_sum_rows`` / ``mkgnn_segment_sum_block_rows`` / ``mkgnn_row_inv_norm`` / ``mkgnn_rows_presplit`` are documented
to compute, written with numpy on the CPU.  Nothing here imports the library; ``tests/test_csr_reference_cpu.py`` pins these
helpers without a GPU, ``tests/test_csr_rows_exact.py`` holds the kernels to them.

The segment sum ``out[i] = sum_k in[col[k]]`` over ``k in [rowptr[i], rowptr[i + 1])`` runs in CSR order in both kernels (the
pipelined one adds the first four terms left to right and then four more per round; the fallback starts from +0 and adds eight per
round), every add a plain fp32 add: ``seq_sum_f32`` is that sum, and the kernels must EQUAL it.
"""
import numpy as np
import torch

MAX_DEGREE = 4
MIXED_LENGTHS = (0, 1, 2, 3, 4, 5, 8, 9, 13)


def rows_per_wave(width: int) -> int:
    """Rows a wave of the pipelined kernels works on at once: a row of ``width`` floats is held by 8 / 16 / 32 / 64 lanes."""
    return 8 if width <= 32 else 4 if width <= 64 else 2 if width <= 128 else 1


# ------------------------------------------------------------------------------------------------------ sums --
def _seq_sum(rowptr, col, v, dtype, magnitude=False):
    rowptr = np.asarray(rowptr, dtype=np.int64)
    col = np.asarray(col, dtype=np.int64)
    v = np.asarray(v)
    assert v.ndim == 2 and rowptr.ndim == 1 and rowptr[0] == 0 and rowptr[-1] == col.shape[0]
    n = rowptr.shape[0] - 1
    lens = rowptr[1:] - rowptr[:-1]
    assert (lens >= 0).all() and (col.size == 0 or (col.min() >= 0 and col.max() < v.shape[0]))
    src = v.astype(dtype)
    if magnitude:
        src = np.abs(src)
    acc = np.zeros((n, v.shape[1]), dtype=dtype)
    for t in range(int(lens.max()) if n else 0):
        rows = np.nonzero(lens > t)[0]
        term = src[col[rowptr[rows] + t]]
        if t == 0:
            acc[rows] = term                       # a segment's first term is taken as it is
        else:
            acc[rows] = acc[rows] + term           # one rounded add per term (numpy: no fused operations)
    return acc


def seq_sum_f32(rowptr, col, v) -> np.ndarray:
    """The fp32 sum in CSR order, one position of every segment at a time; empty segments give 0."""
    assert np.asarray(v).dtype == np.float32
    return _seq_sum(rowptr, col, v, np.float32)


def sum_f64(rowptr, col, v) -> np.ndarray:
    """The same sum in float64 (of fp32 inputs: exact to 2^-53 per add)."""
    return _seq_sum(rowptr, col, v, np.float64)


def abs_sum_f64(rowptr, col, v) -> np.ndarray:
    """sum_k |in[col[k]]| in float64: the scale of the rounding bound of a segment sum."""
    return _seq_sum(rowptr, col, v, np.float64, magnitude=True)


def seq_sum_bound(rowptr, col, v) -> np.ndarray:
    """|fp32 sum in any order - float64 sum| <= (len - 1) * 2^-24 * sum_k |in[col[k]]|: len - 1 adds, each rounded to nearest (half an
    ulp, 2^-24 of a partial sum that is at most the sum of magnitudes).  Rows of length 0 and 1 are exact."""
    lens = np.diff(np.asarray(rowptr, dtype=np.int64))
    return np.maximum(lens - 1, 0)[:, None] * 2.0 ** -24 * abs_sum_f64(rowptr, col, v)


# ------------------------------------------------------------------------------------------------ block rows --
def block_offsets(num_kernels):
    offs = [0]
    for L in num_kernels:
        offs.append(offs[-1] + int(L))
    return offs                                        # block d = columns [offs[d - 1], offs[d]); offs[4] = K


def block_mask(deg, num_kernels) -> np.ndarray:
    """[n, K] bool: column c of row i lies in the block of atom i's degree (degree 0, or an empty block: no column)."""
    deg = np.asarray(deg, dtype=np.int64)
    offs = block_offsets(num_kernels)
    lo = np.array([0] + offs[:MAX_DEGREE])[deg][:, None]
    ln = np.array([0] + [int(L) for L in num_kernels])[deg][:, None]
    c = np.arange(offs[MAX_DEGREE])[None, :]
    return (c >= lo) & (c < lo + ln)


def block_store(dense, mask, stride: int) -> np.ndarray:
    """[n, stride] fp32 storage of block rows: the dense values inside the blocks, NaN outside them and in the padding."""
    n, K = mask.shape
    assert stride >= K
    store = np.full((n, stride), np.nan, dtype=np.float32)
    store[:, :K] = np.where(mask, np.asarray(dense, dtype=np.float32)[:, :K], np.float32(np.nan))
    return store


def pack_col(col, deg) -> np.ndarray:
    """Index entries of a block-row source list: the source row in bits 0..27, its degree in bits 28..30."""
    col = np.asarray(col, dtype=np.int64)
    d = np.asarray(deg, dtype=np.int64)[col] if col.size else col
    assert col.size == 0 or (col.max() < (1 << 28) and d.min() >= 0 and d.max() <= MAX_DEGREE)
    return (col | (d << 28)).astype(np.int32)


# --------------------------------------------------------------------------------------------- pre-split rows --
def decode_split(store: torch.Tensor, width: int, inv: torch.Tensor) -> torch.Tensor:
    """fp32 values of pre-split rows: ``(hi + lo) / 2^(exponent(inv) + 8)``.  ``store`` is the [n, >= width] tensor the producer
    wrote (or a column slice of it: its row stride says where the rows are); four floats are the fp16 halves hi(0..3) | lo(0..3)."""
    n = store.shape[0]
    raw = torch.as_strided(store, (n, store.stride(0)), (store.stride(0), 1))
    w4 = (width + 3) // 4 * 4
    halves = raw[:, :w4].contiguous().view(torch.float16).view(n, w4 // 4, 2, 4).float()      # [n, granule, hi|lo, 4]
    vals = (halves[:, :, 0, :] + halves[:, :, 1, :]).reshape(n, w4)[:, :width]                # exact in fp32
    e = (inv.view(torch.int32) >> 23) & 0xFF
    scale = torch.exp2((e - 127 + 8).float())
    return vals / scale[:, None]


def split_halves(store: torch.Tensor, width: int) -> torch.Tensor:
    """[n, chunks, 2, 4] fp16: the hi | lo half-words of every sixteen-byte chunk of the rows."""
    n = store.shape[0]
    w4 = (width + 3) // 4 * 4
    return store[:, :w4].contiguous().view(torch.float16).view(n, w4 // 4, 2, 4)


def split_rows_numpy(x: np.ndarray, inv: np.ndarray) -> np.ndarray:
    """A straightforward fp16 split of fp32 rows (numpy): [n, width rounded up to 4] fp32 storage holding hi = fp16(x s),
    lo = fp16(x s - hi), s = 2^(exponent(inv) + 8), as hi(0..3) | lo(0..3) per four values; zeros beyond the width."""
    x = np.asarray(x, dtype=np.float32)
    n, w = x.shape
    w4 = (w + 3) // 4 * 4
    e = ((np.asarray(inv, dtype=np.float32).view(np.int32) >> 23) & 0xFF).astype(np.int64)
    s = np.ldexp(np.float32(1), (e - 127 + 8).astype(np.int32)).astype(np.float32)[:, None]
    xs = np.zeros((n, w4), dtype=np.float32)
    xs[:, :w] = x * s
    hi = xs.astype(np.float16)
    lo = (xs - hi.astype(np.float32)).astype(np.float16)
    out = np.empty((n, w4 // 4, 2, 4), dtype=np.float16)
    out[:, :, 0, :] = hi.reshape(n, w4 // 4, 4)
    out[:, :, 1, :] = lo.reshape(n, w4 // 4, 4)
    return out.reshape(n, 2 * w4).view(np.float32)


# ------------------------------------------------------------------------------------------------ topologies --
def _csr(lens, col):
    rowptr = np.zeros(len(lens) + 1, dtype=np.int64)
    np.cumsum(lens, out=rowptr[1:])
    assert rowptr[-1] == len(col) < 2 ** 31
    return rowptr.astype(np.int32), np.asarray(col, dtype=np.int32)


def uniform(n: int, L: int):
    """Every segment has length ``L``: L = 0 no entries, 1 a matching (i <-> i ^ 1), 2 a cycle, 3 a cubic circulant, 4 and 5 the
    next circulants -- one launch on it runs one arm of the kernel's K = 1..4 switch (and for L = 5 the long-segment loop) in
    every wave.  (On fewer rows than offsets the entries repeat and refer to the row itself.)"""
    i = np.arange(n, dtype=np.int64)
    if L == 1:
        col = np.minimum(i ^ 1, n - 1)[:, None]
    else:
        offs = np.array([1, -1, n // 2 if n > 4 else 2, 2, -2][:L], dtype=np.int64)
        col = (i[:, None] + offs[None, :]) % max(n, 1)
    return _csr(np.full(n, L, dtype=np.int64), col.reshape(-1))


def empty(n: int):
    """No entries at all."""
    return uniform(n, 0)


def mixed(n: int, rpw: int, seed: int = 0):
    """Every group of ``rpw`` consecutive rows holds lengths drawn from MIXED_LENGTHS (a different draw per group, so waves meet
    short rows beside a long one and every value of the wave-uniform ``need``); the first and the last row are empty; some rows
    repeat a column entry, some refer to themselves."""
    rng = np.random.default_rng(1000 * seed + 17 * n + rpw)
    pool = np.array(MIXED_LENGTHS, dtype=np.int64)
    groups = (n + rpw - 1) // rpw
    # two pool entries per group, its rows draw from the two: groups whose longest row is 0, 1, 2, 3, 4 and > 4 all occur
    a = pool[rng.integers(0, len(pool), size=groups)]
    b = pool[rng.integers(0, len(pool), size=groups)]
    pick = rng.integers(0, 2, size=(groups, rpw)).astype(bool)
    lens = np.where(pick, a[:, None], b[:, None]).reshape(-1)[:n].copy()
    lens[0] = 0
    lens[n - 1] = 0
    rowptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(lens, out=rowptr[1:])
    col = rng.integers(0, n, size=int(rowptr[-1]), dtype=np.int64)
    row_of = np.repeat(np.arange(n, dtype=np.int64), lens)
    pos = np.arange(col.shape[0], dtype=np.int64) - rowptr[row_of]
    selfref = (row_of % 5 == 1) & (pos == 0)
    col[selfref] = row_of[selfref]
    rep = np.nonzero((row_of % 3 == 0) & (pos == 1))[0]
    col[rep] = col[rep - 1]                              # a repeated column entry
    return _csr(lens, col)


def tile_to(rowptr, col, n: int):
    """The graph repeated (column entries shifted by the base size, wrapped into range) and cut to ``n`` rows."""
    rowptr = np.asarray(rowptr, dtype=np.int64)
    col = np.asarray(col, dtype=np.int64)
    base = rowptr.shape[0] - 1
    reps = (n + base - 1) // base
    lens = np.tile(np.diff(rowptr), reps)[:n]
    cols = (np.tile(col, reps) + np.repeat(np.arange(reps, dtype=np.int64) * base, col.shape[0]))[:int(lens.sum())] % n
    return _csr(lens, cols)


def degrees(n: int, seed: int = 0) -> np.ndarray:
    """[n] int8 degrees 0..4, every value present once n >= 5."""
    rng = np.random.default_rng(77 + seed)
    d = rng.integers(0, MAX_DEGREE + 1, size=n)
    d[:min(n, 5)] = np.arange(min(n, 5))
    return d.astype(np.int8)
