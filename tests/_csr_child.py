"""Driver of the CSR row passes for ``tests/test_csr_rows_exact.py``: thin calls of the C entries on buffers the caller owns
(sentinels, guards, odd strides), and ``run_cases`` -- the dense sum, the block-row modes 1, 2 and 3, the row norms and the pre-split
rows of a list of (width, n) cases, every output as its bit pattern.

As a program (``python -m tests._csr_child '<json list of [width, n]>' out.npz``) it writes those outputs to an ``.npz``: the grid
cap ``MKGNN_CSR_BLOCKS`` is read once per process, so the grid-independence test runs this in a fresh child per value and compares
with its own default-grid results bit for bit.
"""
import json
import sys

import numpy as np
import torch

from tests import _csr_reference as R

SENTINEL = 0x7FC5A5A5                      # a quiet NaN with a payload: nothing computes it, and added into a result it shows
GRID_BLOCKS = {28: (3, 5, 8, 12), 60: (5, 10, 15, 30), 110: (10, 20, 30, 50), 200: (20, 40, 60, 80)}


def dev():
    assert torch.cuda.is_available(), "pytest -m gpu needs the MI355X"
    return torch.device("cuda:0")


def up(a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def sentinel(numel: int) -> torch.Tensor:
    """A flat fp32 buffer (256-byte aligned: a fresh allocation) filled with SENTINEL."""
    return torch.full((max(int(numel), 1),), SENTINEL, dtype=torch.int32, device=dev()).view(torch.float32)


def bits(t: torch.Tensor) -> torch.Tensor:
    return t.view(torch.int32)


def padded(v: np.ndarray, stride: int, fill=np.nan) -> np.ndarray:
    """[n, stride] fp32 storage of the rows ``v``; what lies beyond the width holds ``fill`` (NaN: nothing may read it into a result)."""
    n, w = v.shape
    store = np.full((n, stride), fill, dtype=np.float32)
    store[:, :w] = v
    return store


def _p(t):
    return None if t is None else t.data_ptr()


def _lib():
    from molkgnn_amd import _lib as L
    return L, L.load()


def segment_sum(inp, in_stride, rowptr, col, n, w, out, out_stride, inv) -> int:
    L, lib = _lib()
    return lib.mkgnn_segment_sum_rows(_p(inp), in_stride, _p(rowptr), _p(col), n, w, _p(out), out_stride, _p(inv), L.stream_ptr(dev()))


def block_sum(inp, in_stride, rowptr, col, deg8, n, Ls, mode, out, out_stride, inv) -> int:
    L, lib = _lib()
    return lib.mkgnn_segment_sum_block_rows(_p(inp), in_stride, _p(rowptr), _p(col), _p(deg8), n, L.Int32x4(*Ls), mode, _p(out),
                                            out_stride, _p(inv), L.stream_ptr(dev()))


def row_inv_norm(x, stride, n, w, inv) -> int:
    L, lib = _lib()
    return lib.mkgnn_row_inv_norm(_p(x), stride, n, w, _p(inv), L.stream_ptr(dev()))


def presplit(x, xs, n, w, inv, out, out_stride) -> int:
    L, lib = _lib()
    return lib.mkgnn_rows_presplit(_p(x), xs, n, w, _p(inv), _p(out), out_stride, L.stream_ptr(dev()))


def last_error() -> str:
    _, lib = _lib()
    msg = lib.mkgnn_last_error()
    return msg.decode() if msg else ""


def case_inputs(width: int, n: int, seed: int = 0):
    """The inputs of one (width, n) case of ``run_cases`` (numpy): mixed topology, degrees, a dense input and its block rows."""
    rpw = R.rows_per_wave(width)
    base = R.mixed(min(n, 4099), rpw, seed)
    rowptr, col = base if n <= 4099 else R.tile_to(*base, n)
    deg = R.degrees(n, seed)
    Ls = GRID_BLOCKS[width]
    rng = np.random.default_rng(9 * width + seed)
    full = rng.standard_normal((n, width)).astype(np.float32)
    mask = R.block_mask(deg, Ls)
    return dict(rowptr=rowptr, col=col, deg=deg, Ls=Ls, full=full, mask=mask, masked=np.where(mask, full, np.float32(0)))


def run_case(width: int, n: int, inputs=None):
    """Every pass on one case; outputs as int32 bit patterns (numpy), whole buffers (padding and guard floats included)."""
    c = inputs if inputs is not None else case_inputs(width, n)
    w4 = width + (-width) % 4
    os_ = w4 + 4
    rowptr, col, deg8 = up(c["rowptr"]), up(c["col"]), up(c["deg"])
    packed = up(R.pack_col(c["col"], c["deg"]))
    full = up(padded(c["full"], w4))
    blocks = up(R.block_store(c["full"], c["mask"], w4))
    res = {}

    def keep(name, t):
        res[name] = bits(t).cpu().numpy().copy()

    def run(name, rc, out, inv=None):
        assert rc == 0, (name, last_error())
        keep(name, out)
        if inv is not None:
            keep(name + "_inv", inv)

    out, inv = sentinel(n * os_), sentinel(n)
    run("dense", segment_sum(full, w4, rowptr, col, n, width, out, os_, inv), out, inv)
    out, inv = sentinel(n * os_), sentinel(n)
    run("mode1", block_sum(blocks, w4, rowptr, packed, None, n, c["Ls"], 1, out, os_, inv), out, inv)
    m1 = out
    out = sentinel(n * os_)
    run("mode2", block_sum(full, w4, rowptr, col, deg8, n, c["Ls"], 2, out, os_, None), out)
    out, inv = sentinel(n * os_), sentinel(n)
    run("mode3", block_sum(blocks, w4, rowptr, packed, None, n, c["Ls"], 3, out, os_, inv), out, inv)
    inv = sentinel(n)
    run("norm", row_inv_norm(m1, os_, n, width, inv), inv)
    out, inv = sentinel(n * os_), sentinel(n)
    run("split", presplit(m1, os_, n, width, inv, out, os_), out, inv)
    torch.cuda.synchronize()
    return res


def run_cases(cases):
    res = {}
    for width, n in cases:
        for k, v in run_case(int(width), int(n)).items():
            res[f"w{width}_n{n}_{k}"] = v
    return res


if __name__ == "__main__":
    np.savez(sys.argv[2], **run_cases(json.loads(sys.argv[1])))
