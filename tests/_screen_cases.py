"""Inputs shared by the screening tests (CPU and GPU): score vectors with the special values and ties the ranking's order is
about, and a brute-force ranking by the order as it is written down in include/molkgnn_hip.h."""
import struct

import numpy as np


def f32(bits: int) -> np.float32:
    return np.array([bits], dtype=np.uint32).view(np.float32)[0]


NEG_ZERO, NAN_A, NAN_B = f32(0x80000000), f32(0x7FC00001), f32(0xFFC12345)       # (two NaNs with different payloads and signs)


def bits(a) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.int32)


def special_scores(n: int, seed: int) -> np.ndarray:
    """``n`` scores: normal values with -0.0, +0.0, NaNs, +inf and REAL -inf entries sprinkled in."""
    rng = np.random.default_rng(seed)
    s = rng.standard_normal(n).astype(np.float32)
    pool = np.array([NEG_ZERO, np.float32(0.0), NAN_A, NAN_B, np.float32(np.inf), np.float32(-np.inf), np.float32(1.5)], dtype=np.float32)
    pool_bits = pool.view(np.int32)
    at = rng.random(n) < 0.4
    out = s.view(np.int32).copy()
    out[at] = pool_bits[rng.integers(0, len(pool), int(at.sum()))]
    return out.view(np.float32)


def quantised_scores(n: int, seed: int, levels: int = 8) -> np.ndarray:
    rng = np.random.default_rng(seed)
    return (rng.integers(0, levels, n).astype(np.float32) - np.float32(levels // 2)) * np.float32(0.25)


def case_inputs(kind: str, n: int, seed: int):
    """``(scores float32[n], ids int32[n])`` of a named case."""
    rng = np.random.default_rng(seed + 1000)
    ids = rng.permutation(n).astype(np.int32)
    if kind == "special":
        return special_scores(n, seed), ids
    if kind == "equal":
        return np.full(n, np.float32(0.75)), ids
    if kind == "quantised":
        return quantised_scores(n, seed), ids
    if kind == "repeated_ids":
        return quantised_scores(n, seed, 4), rng.integers(0, max(n // 8, 1), n).astype(np.int32)
    if kind == "normal":
        return rng.standard_normal(n).astype(np.float32), ids
    raise KeyError(kind)


CASES = ("special", "equal", "quantised", "repeated_ids", "normal")


def brute_force_update(top, scores, ids, n_valid, shard_tag):
    """The written order, entry by entry in Python: a tuple key per entry and ``sorted`` (stable)."""
    ts, th, tm = top
    K = len(ts)
    n = min(max(int(n_valid), 0), len(scores))
    entries = [(np.float32(ts[j]), int(th[j]), int(tm[j])) for j in range(K)]
    entries += [(np.float32(scores[i]), int(shard_tag), int(ids[i])) for i in range(n)]

    def key(e):
        s, h, m = e
        raw = struct.unpack("<I", struct.pack("<f", s))[0]
        empty = raw == 0xFF800000 and h == -1 and m == -1
        nan = s != s
        # (score descending; Python compares -0.0 == 0.0; a NaN's score takes no part)
        return (1 if empty else 0, 1 if nan else 0, 0.0 if nan else -float(s), h, m)

    best = sorted(entries, key=key)[:K]
    return (np.array([e[0] for e in best], dtype=np.float32), np.array([e[1] for e in best], dtype=np.int32),
            np.array([e[2] for e in best], dtype=np.int32))


def same_list(a, b) -> bool:
    """Bit equality of two lists: the scores as int32 views."""
    return (np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(np.asarray(a[1], dtype=np.int32), np.asarray(b[1], dtype=np.int32))
            and np.array_equal(np.asarray(a[2], dtype=np.int32), np.asarray(b[2], dtype=np.int32)))
