"""The convolution's dispatch as the two launch-free queries of the C ABI see it (csrc/kgnn_capi.hip ``plan_conv_forward`` /
``plan_conv_backward`` behind ``mkgnn_backward_streams`` and ``mkgnn_rows_split_supported``), and the table of ``MKGNN_*``
environment switches in INTEGRATION.md.  No GPU: the queries look at shapes, null-ness and alignment only, so fake non-null
integers serve as pointers.

The expected answers were recorded from the library as it was BEFORE the dispatch was gathered into the two plan functions
(one decision spread over the entry points and two hand-written predictions of it): a change of an answer here is a change of
which kernels a training step runs."""
import json
import os
import re
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(REPO, "molkgnn_amd", "libmolkgnn_hip.so")

REF = (10, 20, 30, 50)
ALL, NO_DEG3, NONE = 0, 1, 2          # which degree buckets hold atoms
# (kernel counts, F, E, buckets, unit bond rows present, x misaligned by 4 bytes, x stride padded to 4 floats, atoms, switch)
#   -> (mkgnn_backward_streams, mkgnn_rows_split_supported)
ROWS = [
    ((REF, 28, 7, ALL, 1, 0, 1, 500, None), (1, 1)),
    ((REF, 110, 7, ALL, 1, 0, 1, 500, None), (1, 1)),
    ((REF, 112, 7, ALL, 1, 0, 1, 500, None), (1, 1)),                   # 112 / 113: the widest rows of the split-fp16 products
    ((REF, 113, 7, ALL, 1, 0, 1, 500, None), (1, 0)),
    ((REF, 137, 7, ALL, 1, 0, 1, 500, None), (1, 0)),
    ((REF, 160, 7, ALL, 1, 0, 1, 500, None), (1, 0)),                   # 160 / 161: the widest rows of the streamed kernels
    ((REF, 161, 7, ALL, 1, 0, 1, 500, None), (0, 0)),
    ((REF, 200, 7, ALL, 1, 0, 1, 500, None), (0, 0)),
    ((REF, 27, 7, ALL, 1, 0, 1, 500, None), (1, 1)),
    ((REF, 27, 7, ALL, 1, 0, 0, 500, None), (0, 0)),                    # rows of 27 floats: not 16-byte rows
    ((REF, 4, 7, ALL, 1, 0, 1, 500, None), (1, 1)),
    ((REF, 28, 9, ALL, 1, 0, 1, 500, None), (0, 0)),                    # bond attributes wider than the 8-float unit rows
    ((REF, 28, 7, ALL, 0, 0, 1, 500, None), (0, 0)),
    ((REF, 28, 7, ALL, 1, 1, 1, 500, None), (0, 1)),                    # (the rows-split query takes no x)
    ((REF, 28, 7, ALL, 1, 0, 1, 1 << 26, None), (0, 0)),                # 32-bit element offsets
    ((REF, 28, 7, NO_DEG3, 1, 0, 1, 500, None), (1, 1)),
    ((REF, 28, 7, NONE, 1, 0, 1, 500, None), (0, 0)),
    (((5, 10, 15, 25), 137, 7, ALL, 1, 0, 1, 500, None), (1, 0)),
    (((1, 1, 1, 1), 28, 7, ALL, 1, 0, 1, 500, None), (1, 1)),
    (((16, 32, 48, 64), 160, 7, ALL, 1, 0, 1, 500, None), (1, 0)),
    (((16, 32, 48, 64), 110, 7, ALL, 1, 0, 1, 500, None), (1, 1)),
    (((10, 20, 30, 100), 28, 7, ALL, 1, 0, 1, 500, None), (0, 0)),      # degree 4's sign table: 64 kernels pass, 100 do not
    (((40, 70, 100, 64), 28, 7, ALL, 1, 0, 1, 500, None), (1, 1)),
    (((100, 100, 100, 64), 28, 7, ALL, 1, 0, 1, 500, None), (0, 0)),    # 7 + 4 + 4 + 2 = 17 column groups, the table holds 16
    (((100, 100, 100, 64), 28, 7, NO_DEG3, 1, 0, 1, 500, None), (1, 1)),
    (((10, 0, 30, 50), 28, 7, ALL, 1, 0, 1, 500, None), (1, 1)),
    (((10, 0, 30, 50), 110, 7, ALL, 1, 0, 1, 500, None), (1, 1)),
    ((REF, 28, 7, ALL, 1, 0, 1, 500, "MKGNN_ROWS_STREAM=0"), (0, 0)),
    ((REF, 28, 7, ALL, 1, 0, 1, 500, "MKGNN_BANK_STREAM=0"), (0, 0)),
    ((REF, 28, 7, ALL, 1, 0, 1, 500, "MKGNN_BANK_FUSED=0"), (0, 0)),
    ((REF, 28, 7, ALL, 1, 0, 1, 500, "MKGNN_NO_MFMA_BWD=1"), (0, 0)),
    ((REF, 28, 7, ALL, 1, 0, 1, 500, "MKGNN_FWD_STREAM=0"), (1, 0)),
    ((REF, 28, 7, ALL, 1, 0, 1, 500, "MKGNN_ROWS_SPLIT=0"), (1, 0)),
    ((REF, 28, 7, ALL, 1, 0, 1, 500, "MKGNN_FWD_PP=1"), (1, 0)),
    ((REF, 28, 7, ALL, 1, 0, 1, 500, "MKGNN_FWD_SPLIT=0"), (1, 0)),
    ((REF, 28, 7, ALL, 1, 0, 1, 500, "MKGNN_BWD_SPLIT=0"), (1, 0)),
    ((REF, 110, 7, ALL, 1, 0, 1, 500, "MKGNN_FWD_PP=0"), (1, 1)),
    ((REF, 110, 7, ALL, 1, 0, 1, 500, "MKGNN_BANK_FUSED=1"), (1, 1)),
    ((REF, 137, 7, ALL, 1, 0, 1, 500, "MKGNN_BANK_STREAM=0"), (0, 0)),
    ((REF, 110, 7, ALL, 1, 0, 1, 500, "MKGNN_BWD_SPLIT=0"), (1, 0)),
]

_WORKER = r"""
import ctypes, json, sys
lib = ctypes.CDLL(sys.argv[1])
P = ctypes.c_void_p
class Bank(ctypes.Structure):
    _fields_ = [("num_kernels", ctypes.c_int32), ("reserved", ctypes.c_int32)] + [("p%d" % k, P) for k in range(7)]
class Bucket(ctypes.Structure):
    _fields_ = [("count", ctypes.c_int64)] + [("p%d" % k, P) for k in range(5)] + [("nei_edge_unit", P)]
lib.mkgnn_backward_streams.argtypes = [P, P, P, ctypes.c_int64, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32]
lib.mkgnn_rows_split_supported.argtypes = [P, P, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32]
out = []
for ks, F, E, present, unit, misaligned, padded, n in json.loads(sys.argv[2]):
    banks, buckets = (Bank * 4)(), (Bucket * 4)()
    for i in range(4):
        banks[i].num_kernels = ks[i]
        for k in range(7): setattr(banks[i], "p%d" % k, 0x1000)
        buckets[i].count = 0 if present == 2 or (present == 1 and i == 2) else n // 5
        for k in range(5): setattr(buckets[i], "p%d" % k, 0x2000)
        buckets[i].nei_edge_unit = 0x3000 if unit else None
    xs = (F + 3) // 4 * 4 if padded else F
    out_stride = (sum(ks) + 3) // 4 * 4
    out.append([lib.mkgnn_backward_streams(ctypes.addressof(banks), ctypes.addressof(buckets), 0x10000 + 4 * misaligned, xs, n, F, E),
                lib.mkgnn_rows_split_supported(ctypes.addressof(banks), ctypes.addressof(buckets), xs, out_stride, n, F, E)])
print(json.dumps(out))
"""


def answers(rows, lib=LIB):
    """The two queries' answers for ``rows``: one fresh child process per switch setting (the library reads its switches once)."""
    got = {}
    for switch in sorted({r[-1] for r in rows}, key=str):
        env = {k: v for k, v in os.environ.items() if not k.startswith("MKGNN_")}
        if switch:
            env.update([switch.split("=")])
        mine = [r for r in rows if r[-1] == switch]
        res = subprocess.run([sys.executable, "-c", _WORKER, lib, json.dumps([r[:-1] for r in mine])], env=env, check=True,
                             capture_output=True, text=True)
        got.update(zip(mine, (tuple(a) for a in json.loads(res.stdout))))
    return [got[r] for r in rows]


def test_queries_answer_as_before_the_dispatch_was_gathered():
    rows = [r for r, _ in ROWS]
    wrong = [(r, g, e) for r, g, (_, e) in zip(rows, answers(rows), ROWS) if g != e]
    assert not wrong, wrong
    assert {r[-1] for r in rows} >= {"MKGNN_ROWS_STREAM=0", "MKGNN_BANK_STREAM=0", "MKGNN_BANK_FUSED=0", "MKGNN_NO_MFMA_BWD=1",
                                     "MKGNN_FWD_STREAM=0", "MKGNN_ROWS_SPLIT=0", "MKGNN_FWD_PP=1", "MKGNN_FWD_SPLIT=0",
                                     "MKGNN_BWD_SPLIT=0"}


def _sources(top, suffixes):
    for base, _, names in os.walk(top):
        for n in names:
            if n.endswith(suffixes):
                yield os.path.join(base, n), open(os.path.join(base, n), encoding="utf-8").read()


def test_every_environment_switch_has_a_row_in_the_integration_table():
    """Every ``MKGNN_*`` name the C side passes to ``getenv`` (one file does) or the package reads from ``os.environ``."""
    csrc = os.path.join(REPO, "molkgnn_amd", "csrc")
    readers = [(p, s) for p, s in _sources(csrc, (".hip", ".h", ".cpp")) if "getenv" in s]
    assert [os.path.basename(p) for p, _ in readers] == ["kgnn_switches.h"]
    names = set(re.findall(r'"(MKGNN_[A-Z0-9_]+)"', readers[0][1]))
    assert len(names) >= 22, sorted(names)
    for _, s in _sources(os.path.join(REPO, "molkgnn_amd"), (".py",)):
        names |= set(re.findall(r"""os\.(?:environ(?:\.get\(|\[|\.setdefault\()|getenv\()\s*["'](MKGNN_[A-Z0-9_]+)["']""", s))
    doc = open(os.path.join(REPO, "INTEGRATION.md"), encoding="utf-8").read()
    table = set(re.findall(r"^\| `(MKGNN_[A-Z0-9_]+)` \|", doc, flags=re.M))
    assert not names - table, sorted(names - table)
    assert not table - names, sorted(table - names)          # (and no row for a switch nothing reads)
