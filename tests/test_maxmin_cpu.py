"""Host side of MaxMin picking (``mkgnn_maxmin_pick``, ``readout.maxmin_pick``, ``screening.maxmin_pick_reference`` /
``pick_maxmin_embeddings`` / ``select_maxmin``): the additive exports, the workspace's closed form, the numpy walk on hand-made
matrices and on an arc, the conditions under which the GPU tests may compare with float64, and everything that is refused before
a launch."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import _diverse_cases as DC
from tests import _maxmin_cases as MC

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")


def test_entry_points_are_additive_to_abi_8():
    from molkgnn_amd import _lib
    with open(os.path.join(REPO, "include", "molkgnn_hip.h")) as f:
        h = f.read()
    m = re.search(r"#define\s+MKGNN_ABI_VERSION\s+(\d+)", h)
    assert m and int(m.group(1)) == 8 and _lib.ABI_VERSION == 8
    assert re.search(r"\bsize_t mkgnn_maxmin_pick_workspace_bytes\(int64_t n_rows\);", h)
    assert re.search(r"\bint mkgnn_maxmin_pick\(const float\* emb, int64_t emb_stride, int64_t n_rows, int32_t H, "
                     r"const float\* start_sim /\* \[n_rows\] or null \*/,\s+float stop_sim, int32_t k_max, int32_t\* picks, "
                     r"float\* pick_sim, int32_t\* n_picks, int32_t\* leader,\s+float\* leader_sim, void\* workspace, "
                     r"size_t workspace_bytes, void\* stream\);", h)
    m = re.search(r"#define\s+MKGNN_MAXMIN_MAX_ROWS\s+(\d+)\b", h)
    assert m and int(m.group(1)) == _lib.MAXMIN_MAX_ROWS == 1 << 20
    m = re.search(r"#define\s+MKGNN_MAXMIN_MAX_PICKS\s+(\d+)\b", h)
    assert m and int(m.group(1)) == _lib.MAXMIN_MAX_PICKS == 4096
    raw = ctypes.CDLL(_lib.LIB_PATH)
    raw.mkgnn_abi_version.restype = ctypes.c_int
    assert raw.mkgnn_abi_version() == 8
    lib = _lib.load()
    for name, n_args, restype in (("mkgnn_maxmin_pick", 15, ctypes.c_int), ("mkgnn_maxmin_pick_workspace_bytes", 1, ctypes.c_size_t)):
        assert hasattr(raw, name) and name in _lib.EXPORTS
        assert getattr(lib, name).restype is restype and len(getattr(lib, name).argtypes) == n_args, name
    assert lib.mkgnn_maxmin_pick.argtypes[5] is ctypes.c_float
    # what was there is what it was
    assert lib.mkgnn_diverse_pick.restype is ctypes.c_int and len(lib.mkgnn_diverse_pick.argtypes) == 13
    assert lib.mkgnn_embed_max_cosine.restype is ctypes.c_int and len(lib.mkgnn_embed_max_cosine.argtypes) == 12
    # the source is part of the library's build, compiles the shared evaluation and mirrors its constants to the binding
    csrc = os.path.join(REPO, "molkgnn_amd", "csrc")
    with open(os.path.join(csrc, "Makefile")) as f:
        assert re.search(r"^SRCS :=.*\bkgnn_maxmin\.hip\b", f.read(), flags=re.M)
    with open(os.path.join(csrc, "kgnn_maxmin.hip")) as f:
        text = f.read()
    assert "#pragma clang fp contract(off)" in text and '#include "kgnn_cosine.h"' in text
    for fn in ("mc_dot<W>(", "half_wave_dot(", "half_wave_row_sumsq(", "inv_clamped_norm("):
        assert fn in text, fn
    for name, value in (("MM_MAX_H", _lib.MAXMIN_MAX_H), ("MM_TILE", _lib.MAXMIN_TILE), ("MM_ROWS", _lib.MAXMIN_ROWS)):
        m = re.search(r"constexpr int %s = (\d+);" % name, text)
        assert m and int(m.group(1)) == value, name
    assert _lib.MAXMIN_TILE == MC.TILE == 1024 and _lib.MAXMIN_MAX_H == 64
    m = re.search(r"MM_UPDATE_WIDE_BELOW = (\d+)", text)       # (test_maxmin_gpu.py places a size at this edge of the update launch)
    assert m and int(m.group(1)) == 2048
    # no float atomics, no cooperative launch, no grid barrier
    assert not re.search(r"atomic|cooperative|grid_group|__threadfence", re.sub(r"//.*", "", text))


def test_workspace_size_on_the_host():
    """The closed form the header states (host code only: nothing is launched)."""
    from molkgnn_amd import _lib
    lib = _lib.load()

    def ceil4(x):
        return (x + 3) // 4 * 4

    for n in (1, 2, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 2085, 65536, _lib.MAXMIN_MAX_ROWS - 1, _lib.MAXMIN_MAX_ROWS):
        assert lib.mkgnn_maxmin_pick_workspace_bytes(n) == 4 * (3 * ceil4(n) + 2 * ceil4(-(-n // 256)) + 72), n
    for n in (0, -1, _lib.MAXMIN_MAX_ROWS + 1, 1 << 31):
        assert lib.mkgnn_maxmin_pick_workspace_bytes(n) == 0, n


def _walk(sim, k_max, stop_sim=INF, start_sim=None):
    from molkgnn_amd.screening import maxmin_pick_reference
    sim = np.asarray(sim)
    picks, pick_sim, n_picks, leader, leader_sim = maxmin_pick_reference(sim, k_max, stop_sim, start_sim)
    assert picks.dtype == np.int32 and leader.dtype == np.int32 and picks.shape == pick_sim.shape == (k_max,)
    assert pick_sim.dtype == leader_sim.dtype == sim.dtype and leader.shape == leader_sim.shape == (sim.shape[0],)
    assert (picks[n_picks:] == -1).all() and np.isnan(pick_sim[n_picks:]).all() and (picks[:n_picks] >= 0).all()
    taken = pick_sim[:n_picks]
    assert (taken[1:] >= taken[:-1]).all()                         # non-decreasing
    return picks[:n_picks].tolist(), taken, leader.tolist(), leader_sim


def _same(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), equal_nan=True)


def test_reference_on_hand_made_matrices():
    for dtype in (np.float32, np.float64):
        # three rows on a line: 0 and 2 far apart, 1 between them and nearer to 2
        sim = np.array([[1, 0.5, 0.1], [0.5, 1, 0.7], [0.1, 0.7, 1]], dtype=dtype)
        picks, taken, leader, lsim = _walk(sim, 3)
        assert picks == [0, 2, 1] and _same(taken, [-INF, dtype(0.1), dtype(0.7)]) and leader == [0, 1, 2] and _same(lsim, [1, 1, 1])
        picks, taken, leader, lsim = _walk(sim, 2)
        assert picks == [0, 2] and leader == [0, 2, 2] and _same(lsim, [1, dtype(0.7), 1])
        # k_max = 1: the first valid row, and everything is assigned to it
        picks, taken, leader, lsim = _walk(sim, 1)
        assert picks == [0] and leader == [0, 0, 0] and _same(lsim, [1, dtype(0.5), dtype(0.1)])
        # strictness of stop_sim: a candidate AT it is not taken, the next float above it lets it through
        t = dtype(0.1)
        assert _walk(sim, 3, t)[0] == [0] and _walk(sim, 3, np.nextafter(t, dtype(1)))[0] == [0, 2]
        assert _walk(sim, 3, -INF)[0] == [] and _walk(sim, 3, -INF)[2] == [-1, -1, -1]
        assert _walk(sim, 3, INF)[0] == [0, 2, 1]
        # ties go to the lower row; -0.0 and +0.0 are equal, through start_sim too, and pick_sim keeps the start value's bits
        sim = np.array([[1, 0.0, -0.0, 0.9], [0.0, 1, 0.3, 0.0], [-0.0, 0.3, 1, -0.0], [0.9, 0.0, -0.0, 1]], dtype=dtype)
        picks, taken, leader, lsim = _walk(sim, 2)
        assert picks == [0, 1] and np.signbit(taken[1]) == False                     # rows 1 (+0.0) and 2 (-0.0) tie: row 1
        picks, taken, _, _ = _walk(sim, 1, start_sim=np.array([0.0, 0.5, -0.0, -0.0], dtype=dtype))
        assert picks == [0] and not np.signbit(taken[0])
        picks, taken, _, _ = _walk(sim, 1, start_sim=np.array([0.5, 0.5, -0.0, 0.0], dtype=dtype))
        assert picks == [2] and np.signbit(taken[0])
        # the earlier pick leads among equals
        sim = np.array([[1, 0.2, 0.6], [0.2, 1, 0.6], [0.6, 0.6, 1]], dtype=dtype)
        picks, _, leader, _ = _walk(sim, 2)
        assert picks == [0, 1] and leader == [0, 1, 0]
        # a NaN diagonal: never picked, takes no part, leads nothing -- whatever its row and column say
        sim = np.array([[1, 0.99, 0.2], [0.99, NAN, 0.99], [0.2, 0.0, 1]], dtype=dtype)
        picks, _, leader, lsim = _walk(sim, 3)
        assert picks == [0, 2] and leader == [0, -1, 2] and _same(lsim, [1, NAN, 1])
        # a NaN off the diagonal never replaces a value: the row keeps what it had, or its start
        sim = np.array([[1, 0.1, 0.1], [NAN, 1, 0.4], [0.3, NAN, 1]], dtype=dtype)
        picks, taken, leader, lsim = _walk(sim, 2)
        assert picks == [0, 1] and _same(taken, [-INF, -INF]) and leader == [0, 1, 0] and _same(lsim, [1, 1, dtype(0.3)])
        picks, _, leader, lsim = _walk(sim, 1)
        assert leader == [0, -1, 0] and _same(lsim, [1, -INF, dtype(0.3)])
        # an excluded row (a NaN start) is assigned but never picked; with every other row taken the candidates are exhausted
        sim = np.array([[1, 0.5, 0.1], [0.5, 1, 0.7], [0.1, 0.7, 1]], dtype=dtype)
        picks, taken, leader, lsim = _walk(sim, 3, start_sim=np.array([-INF, -INF, NAN], dtype=dtype))
        assert picks == [0, 1] and leader == [0, 1, 1] and _same(lsim, [1, 1, dtype(0.7)]) and _same(taken, [-INF, dtype(0.5)])
        picks, _, leader, lsim = _walk(sim, 3, start_sim=np.array([NAN, NAN, NAN], dtype=dtype))
        assert picks == [] and leader == [-1, -1, -1] and np.isnan(lsim).all()
        # a deck that is nearer than every pick: the row keeps -1 and the start value's bits; the start decides the order too
        start = np.array([0.2, 0.95, 0.3], dtype=dtype)
        picks, taken, leader, lsim = _walk(sim, 2, start_sim=start)
        assert picks == [0, 2] and _same(taken, [dtype(0.2), dtype(0.3)]) and leader == [0, -1, 2] and _same(lsim, [1, dtype(0.95), 1])
        assert _walk(sim, 3, 0.9, start)[0] == [0, 2]                              # row 1 lies within 0.9 of the deck
    from molkgnn_amd.screening import maxmin_pick_reference
    for bad in (np.zeros((2, 3)), np.zeros(4), np.zeros((2, 2), dtype=np.int32)):
        with pytest.raises(ValueError):
            maxmin_pick_reference(bad, 1)
    for k in (0, 3):
        with pytest.raises(ValueError):
            maxmin_pick_reference(np.eye(2), k)
    with pytest.raises(ValueError):
        maxmin_pick_reference(np.eye(2), 1, NAN)
    with pytest.raises(ValueError):
        maxmin_pick_reference(np.eye(2), 1, 0.5, np.zeros(3))
    got = maxmin_pick_reference(torch.eye(3), 3, start_sim=torch.zeros(3))         # tensors are taken as they are
    assert got[2] == 3 and got[1].dtype == np.float32
    assert maxmin_pick_reference(np.eye(3, dtype=np.float16), 3)[4].dtype == np.float16


def test_the_arc_is_walked_from_its_ends_to_its_middle():
    """On an arc the farthest row from the first is the other end, then comes the middle; from wherever the walk starts, the picks
    behind pick 0 are the ends first."""
    from molkgnn_amd.screening import cosine_reference
    rows = DC.arc(16, np.random.default_rng(4)).astype(np.float32)
    sim = cosine_reference(rows, rows)
    last = DC.ARC_ROWS - 1
    picks, taken, leader, _ = _walk(sim, 3)
    assert picks[:2] == [0, last] and picks[2] in (3, 4)
    assert abs(taken[1] - np.cos(last * DC.ARC_STEP)) < 1e-6
    assert all(leader[j] in picks and abs(leader[j] - j) <= 2 for j in range(DC.ARC_ROWS))
    for first in range(1, last):                                   # start anywhere inside (start values below every cosine):
        start = np.full(DC.ARC_ROWS, -2.0)                         # the end farther from the start follows (7 is odd: no tie)
        start[first] = -3.0
        got = _walk(sim, 2, start_sim=start)[0]
        assert got == [first, last if first < last - first else 0]
    # walked from the other end the same molecules come out: beyond pick 0 the walk does not depend on where it starts
    order = np.arange(DC.ARC_ROWS)[::-1]
    back = [int(order[p]) for p in _walk(cosine_reference(rows[order], rows[order]), 3)[0]]
    assert back[:2] == [last, 0] and back[2] in (3, 4)


def test_fixtures_keep_their_decisions_apart():
    """Every (H, n) the GPU test compares with the float64 walk: in every round behind the first the two smallest ``cur`` values lie
    more than 4 times the sum of their error bounds apart (the helper takes the first seed ``seed_of(n, H) + 1000 j`` for which
    they do), so float32 inside its bound picks as float64 does -- no case is left out; a row's leader is compared only where its
    best and second-best pick are that far apart, and at most 1 % of a case's rows are not."""
    from molkgnn_amd import _lib
    assert MC.SIZES == (1, 5, _lib.MAXMIN_TILE - 1, _lib.MAXMIN_TILE, _lib.MAXMIN_TILE + 1, 2 * _lib.MAXMIN_TILE + 37)
    later = 0
    for H in MC.F64_WIDTHS:
        for n in MC.SIZES:
            emb, picks, leader, margin, sure, j = MC.float64_case(n, H)
            assert emb.shape == (n, H) and emb.dtype == np.float32 and np.isfinite(emb).all()
            assert margin > MC.MARGIN, (H, n, margin)
            assert len(picks) == min(n, MC.F64_PICKS) and picks[0] == 0 and len(set(picks.tolist())) == len(picks)
            assert (~sure).sum() <= 0.01 * n, (H, n, int((~sure).sum()))
            assert (leader >= 0).all() and (leader[picks] == picks).all()
            later += j > 0
    assert later <= 5                                              # (most cases keep the diverse fixtures' own seed)


@pytest.fixture(scope="module")
def cpu_shard(tmp_path_factory):
    from molkgnn_amd import shards as S
    from molkgnn_amd.synthetic import make_batch
    path = str(tmp_path_factory.mktemp("maxmin") / "lib.mkgs")
    S.write_shard(path, make_batch(40, seed=6, assay="all9", with_receptive_fields=False))
    return S.ResidentShard(path, "cpu")


def test_rejections_before_any_launch(cpu_shard, monkeypatch):
    """A NaN ``stop_sim``, ``k`` beyond the rows or the picks of one call, too many rows, CPU tensors, a CPU model or shard, wrong shapes
    and dtypes: ``ValueError`` from every entry point, and the library is not even loaded."""
    from molkgnn_amd import _lib, readout, screening
    from molkgnn_amd.train import GNNModel

    def no_load():
        raise AssertionError("the library was loaded before the refusal")

    monkeypatch.setattr(_lib, "load", no_load)
    torch.manual_seed(0)
    nine = GNNModel(num_layers=1, task_dim=9)                      # (on the CPU)
    emb = torch.zeros(10, 32)
    with pytest.raises(ValueError, match="stop_sim"):
        readout.maxmin_pick(emb, 4, NAN)
    with pytest.raises(ValueError, match="stop_sim"):
        screening.pick_maxmin_embeddings(emb, 4, NAN)
    with pytest.raises(ValueError, match="stop_sim"):
        screening.select_maxmin(nine, [cpu_shard], 4, 32, NAN)
    for k in (0, 11, -1):
        with pytest.raises(ValueError, match="k = "):
            readout.maxmin_pick(emb, k)
        with pytest.raises(ValueError, match="k = "):
            screening.pick_maxmin_embeddings(emb, k)
    many = torch.zeros(1, 1).expand(_lib.MAXMIN_MAX_PICKS + 10, 1)  # (a view: no memory behind the rows)
    with pytest.raises(ValueError, match="MKGNN_MAXMIN_MAX_PICKS"):
        readout.maxmin_pick(many, _lib.MAXMIN_MAX_PICKS + 1)
    with pytest.raises(ValueError, match="k = "):
        screening.pick_maxmin_embeddings(many, _lib.MAXMIN_MAX_PICKS + 1)
    with pytest.raises(ValueError, match="k = "):
        screening.select_maxmin(nine, [cpu_shard], _lib.MAXMIN_MAX_PICKS + 1, 32)
    with pytest.raises(ValueError, match="k = "):
        screening.select_maxmin(nine, [cpu_shard], 0, 32)
    huge = torch.zeros(1, 1).expand(_lib.MAXMIN_MAX_ROWS + 1, 1)
    with pytest.raises(ValueError, match="rows"):
        readout.maxmin_pick(huge, 4)
    with pytest.raises(ValueError, match="rows"):
        screening.pick_maxmin_embeddings(huge, 4)
    with pytest.raises(ValueError, match="GPU"):
        readout.maxmin_pick(emb, 4)
    with pytest.raises(ValueError, match="GPU"):
        readout.maxmin_pick(emb, 4, 0.9, torch.zeros(10))
    with pytest.raises(ValueError, match="GPU"):
        screening.pick_maxmin_embeddings(emb, 4)
    with pytest.raises(ValueError, match="GPU"):
        screening.select_maxmin(nine, [cpu_shard], 4, 32)
    with pytest.raises(ValueError, match="batch_size"):
        screening.select_maxmin(nine, [cpu_shard], 4, 0)
    for args in ((emb.double(), 4), (emb[0], 4), (torch.zeros(10, 0), 4), (emb, 4, 0.9, torch.zeros(9)), (emb, 4, 0.9, torch.zeros(10).double())):
        with pytest.raises(ValueError):
            readout.maxmin_pick(*args)
    for kw in (dict(deck=torch.zeros(3, 31)), dict(deck=torch.zeros(0, 32)), dict(deck=torch.zeros(3, 32).double()), dict(deck=torch.zeros(32)),
               dict(exclude=torch.zeros(10)), dict(exclude=torch.zeros(9, dtype=torch.bool)), dict(ids=torch.zeros(10)),
               dict(ids=torch.zeros(9, dtype=torch.int32))):
        with pytest.raises(ValueError):
            screening.pick_maxmin_embeddings(emb, 4, **kw)
    with pytest.raises(ValueError):
        screening.pick_maxmin_embeddings(emb.double(), 4)
