"""A numpy mirror of the kernels' dropout generator (``csrc/kgnn_philox.h``): Philox4x32-10 (Salmon et al., SC'11) keyed by
``seed``, counter ``(element / 4, offset)``, word ``element % 4``; the keep rule of ``keep_scale_of``; the readout's element map
(``element = 2^62 + atom * H + h``, include/molkgnn_hip.h)."""
import numpy as np

_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
_LO = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)
READOUT_BASE = 1 << 62


def philox4x32_10(counter, key):
    """The four output words of one Philox4x32-10 block for ``counter`` = (c0, c1, c2, c3), ``key`` = (k0, k1), each an array
    (or scalar) of 32-bit values; returns four uint64 arrays holding 32-bit words."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & _LO for c in counter)
    k0, k1 = (np.asarray(k, dtype=np.uint64) & _LO for k in key)
    for _ in range(10):
        p0, p1 = _M0 * c0, _M1 * c2                  # (< 2^64: no wrap)
        c0, c1, c2, c3 = ((p1 >> _S32) ^ c1 ^ k0, p1 & _LO, (p0 >> _S32) ^ c3 ^ k1, p0 & _LO)
        k0, k1 = (k0 + _W0) & _LO, (k1 + _W1) & _LO
    return c0, c1, c2, c3


def philox_word(seed: int, offset: int, element):
    """``philox_word(seed, offset, element)`` of kgnn_philox.h for an array of elements (uint64)."""
    e = np.asarray(element, dtype=np.uint64)
    w = philox4x32_10((e >> np.uint64(2), e >> np.uint64(34), np.uint64(offset & 0xFFFFFFFF), np.uint64(offset >> 32)),
                      (np.uint64(seed & 0xFFFFFFFF), np.uint64(seed >> 32)))
    sel = (e & np.uint64(3)).astype(np.int64)
    return np.choose(sel, w).astype(np.uint32)


def keep_scale(words, p: float):
    """``keep_scale_of``: 0 where the 24-bit uniform is below p, else 1 / (1 - p), in float32 as the kernels compute it."""
    u = (np.asarray(words, dtype=np.uint32) >> np.uint32(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)
    pf = np.float32(p)
    scale = np.float32(1.0) / (np.float32(1.0) - pf)
    return np.where(u >= pf, scale, np.float32(0.0)).astype(np.float32)


def readout_mask(seed: int, offset: int, n_rows: int, H: int, p: float, row0: int = 0):
    """The readout's keep multipliers ``[n_rows, H]`` for batch atoms ``row0 .. row0 + n_rows - 1``."""
    atoms = np.arange(row0, row0 + n_rows, dtype=np.uint64)[:, None]
    hs = np.arange(H, dtype=np.uint64)[None, :]
    e = np.uint64(READOUT_BASE) + atoms * np.uint64(H) + hs
    return keep_scale(philox_word(seed, offset, e.reshape(-1)), p).reshape(n_rows, H)


def head_mask(seed: int, offset: int, n_rows: int, G: int, p: float):
    """The head's keep multipliers ``[n_rows, G]`` (element mol * G + j)."""
    e = np.arange(n_rows * G, dtype=np.uint64)
    return keep_scale(philox_word(seed, offset, e), p).reshape(n_rows, G)
