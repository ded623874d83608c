"""Host side of the diverse picks (``mkgnn_diverse_pick``, ``readout.diverse_pick``, ``screening.diverse_pick_reference`` /
``pick_diverse_embeddings`` / ``screen_diverse``): the additive exports, the numpy walk on hand-made matrices, the condition under
which the GPU tests may compare with float64, and everything that is refused before a launch."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import _diverse_cases as DC

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")


def test_entry_points_are_additive_to_abi_8():
    from molkgnn_amd import _lib
    with open(os.path.join(REPO, "include", "molkgnn_hip.h")) as f:
        h = f.read()
    m = re.search(r"#define\s+MKGNN_ABI_VERSION\s+(\d+)", h)
    assert m and int(m.group(1)) == 8 and _lib.ABI_VERSION == 8
    assert re.search(r"\bsize_t mkgnn_diverse_pick_workspace_bytes\(int64_t n_rows\);", h)
    assert re.search(r"\bint mkgnn_diverse_pick\(const float\* emb, int64_t emb_stride, int64_t n_rows, int32_t H, float max_sim, "
                     r"int32_t k_max,\s+int32_t\* picks, int32_t\* n_picks, int32_t\* leader, float\* leader_sim, void\* workspace,\s+"
                     r"size_t workspace_bytes, void\* stream\);", h)
    m = re.search(r"#define\s+MKGNN_DIVERSE_MAX_ROWS\s+(\d+)\b", h)
    assert m and int(m.group(1)) == _lib.DIVERSE_MAX_ROWS == 1 << 20
    raw = ctypes.CDLL(_lib.LIB_PATH)
    raw.mkgnn_abi_version.restype = ctypes.c_int
    assert raw.mkgnn_abi_version() == 8
    lib = _lib.load()
    for name, n_args, restype in (("mkgnn_diverse_pick", 13, ctypes.c_int), ("mkgnn_diverse_pick_workspace_bytes", 1, ctypes.c_size_t)):
        assert hasattr(raw, name) and name in _lib.EXPORTS
        assert getattr(lib, name).restype is restype and len(getattr(lib, name).argtypes) == n_args, name
    assert lib.mkgnn_diverse_pick.argtypes[4] is ctypes.c_float
    # what was there is what it was
    assert lib.mkgnn_embed_max_cosine.restype is ctypes.c_int and len(lib.mkgnn_embed_max_cosine.argtypes) == 12
    assert lib.mkgnn_embed_cosine.restype is ctypes.c_int and len(lib.mkgnn_embed_cosine.argtypes) == 11
    # the source is part of the library's build, and the shared evaluation has one text
    with open(os.path.join(REPO, "molkgnn_amd", "csrc", "Makefile")) as f:
        assert re.search(r"^SRCS :=.*\bkgnn_diverse\.hip\b", f.read(), flags=re.M)
    texts = {}
    csrc = os.path.join(REPO, "molkgnn_amd", "csrc")
    for name in sorted(os.listdir(csrc)):
        if name.endswith((".h", ".hip")):
            with open(os.path.join(csrc, name)) as f:
                texts[name] = f.read()
    defines = {name: len(re.findall(r"float mc_dot\(const float", text)) for name, text in texts.items()}
    assert defines.pop("kgnn_cosine.h") == 1 and not any(defines.values()), defines       # once, and in no .hip file (nor elsewhere)
    assert "mc_dot<W>(" in texts["kgnn_max_cosine.hip"] and "mc_dot<W>(" in texts["kgnn_diverse.hip"]
    assert "#pragma clang fp contract(off)" in texts["kgnn_diverse.hip"] and "#pragma clang fp contract(off)" in texts["kgnn_cosine.h"]
    # its siblings: every piece of a cosine's evaluation has one definition under csrc/, and the kernel the others are defined
    # against spells none of them out by hand
    for fn in ("half_wave_sumsq", "half_wave_dot", "inv_clamped_norm"):
        defines = {name: len(re.findall(r"float %s\(" % fn, text)) for name, text in texts.items()}
        assert defines.pop("kgnn_cosine.h") == 1 and not any(defines.values()), (fn, defines)
    assert "sqrtf(" not in texts["kgnn_embed_cosine.hip"] and "ec_sumsq" not in texts["kgnn_embed_cosine.hip"]
    with open(os.path.join(csrc, "Makefile")) as f:
        hdrs = re.search(r"^HDRS :=(.*)$", f.read(), flags=re.M).group(1).split()
    assert "kgnn_cosine.h" in hdrs and "kgnn_ranked.h" in hdrs


def test_sizes_on_the_host():
    """The workspace size, the limits and the tile the binding mirrors (host code only: nothing is launched)."""
    from molkgnn_amd import _lib
    lib = _lib.load()
    for n in (1, 2, 3, 4, 5, 1023, 1024, 1025, 65536, _lib.DIVERSE_MAX_ROWS):
        assert lib.mkgnn_diverse_pick_workspace_bytes(n) == 4 * (2 * ((n + 3) // 4 * 4) + 4), n
    for n in (0, -1, _lib.DIVERSE_MAX_ROWS + 1, 1 << 31):
        assert lib.mkgnn_diverse_pick_workspace_bytes(n) == 0, n
    with open(os.path.join(REPO, "molkgnn_amd", "csrc", "kgnn_diverse.hip")) as f:
        text = f.read()
    for W in (32, 64):
        m = re.search(r"struct DvTile<%d> \{ static constexpr int value = (\d+); \};" % W, text)
        assert m and int(m.group(1)) == _lib.diverse_tile(W) == _lib.diverse_tile(W - 31) and int(m.group(1)) in (512, 1024)
    for H in (0, 65):
        with pytest.raises(ValueError):
            _lib.diverse_tile(H)


def _walk(sim, max_sim, k_max):
    from molkgnn_amd.screening import diverse_pick_reference
    picks, n_picks, leader, leader_sim = diverse_pick_reference(np.asarray(sim), max_sim, k_max)
    assert picks.dtype == np.int32 and leader.dtype == np.int32 and picks.shape == (k_max,) and leader_sim.dtype == np.asarray(sim).dtype
    assert (picks[n_picks:] == -1).all()
    return picks[:n_picks].tolist(), leader.tolist(), leader_sim


def _same(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), equal_nan=True)


def test_reference_on_hand_made_matrices():
    X = 7.0                                                       # the upper triangle is never read: any value may stand there
    for dtype in (np.float32, np.float64):
        # strictness: a similarity EQUAL to the threshold does not cover, the next float above it does
        t = dtype(0.5)
        up = np.nextafter(t, dtype(1))
        sim = np.array([[1, X, X], [t, 1, X], [up, 0.1, 1]], dtype=dtype)
        picks, leader, lsim = _walk(sim, t, 3)
        assert picks == [0, 1] and leader == [0, 1, 0] and _same(lsim, [1, 1, up])
        # the FIRST covering pick in pick order, not the most similar one
        sim = np.array([[1, X, X], [0.1, 1, X], [0.6, 0.9, 1]], dtype=dtype)
        picks, leader, lsim = _walk(sim, 0.5, 3)
        assert picks == [0, 1] and leader == [0, 1, 0] and _same(lsim, [1, 1, dtype(0.6)])
        # a NaN diagonal: never picked, never covered -- whatever its row says -- and it covers nothing
        sim = np.array([[1, X, X, X], [0.99, NAN, X, X], [0.2, 0.99, 1, X], [0.1, 0.99, 0.3, 1]], dtype=dtype)
        picks, leader, lsim = _walk(sim, 0.5, 4)
        assert picks == [0, 2, 3] and leader == [0, -1, 2, 3] and _same(lsim, [1, NAN, 1, 1])
        # a NaN off the diagonal never covers: the row goes on to the next pick, or becomes one
        sim = np.array([[1, X, X, X], [0.1, 1, X, X], [NAN, 0.8, 1, X], [NAN, NAN, 0.2, 1]], dtype=dtype)
        picks, leader, lsim = _walk(sim, 0.5, 4)
        assert picks == [0, 1, 3] and leader == [0, 1, 1, 3] and _same(lsim, [1, 1, dtype(0.8), 1])
        # a full list: later rows are still assigned to the picks that cover them, the others keep (-1, NaN)
        sim = np.array([[1, X, X, X, X], [0.0, 1, X, X, X], [0.0, 0.0, 1, X, X], [0.0, 0.7, 0.9, 1, X], [0.9, 0.0, 0.0, 0.0, 1]],
                       dtype=dtype)
        picks, leader, lsim = _walk(sim, 0.5, 2)
        assert picks == [0, 1] and leader == [0, 1, -1, 1, 0] and _same(lsim, [1, 1, NAN, dtype(0.7), dtype(0.9)])
        picks, leader, lsim = _walk(sim, 0.5, 5)
        assert picks == [0, 1, 2] and leader == [0, 1, 2, 1, 0]
        # k_max = 1: the best row, and whatever it covers
        picks, leader, lsim = _walk(sim, 0.5, 1)
        assert picks == [0] and leader == [0, -1, -1, -1, 0] and _same(lsim, [1, NAN, NAN, NAN, dtype(0.9)])
        # a -0.0 threshold: +0.0 > -0.0 is false
        sim = np.array([[1, X], [0.0, 1]], dtype=dtype)
        assert _walk(sim, -0.0, 2)[0] == [0, 1] and _walk(sim, -1e-30, 2)[0] == [0]
    from molkgnn_amd.screening import diverse_pick_reference
    for bad in (np.zeros((2, 3)), np.zeros(4), np.zeros((2, 2), dtype=np.int32)):
        with pytest.raises(ValueError):
            diverse_pick_reference(bad, 0.5, 1)
    for k in (0, 3):
        with pytest.raises(ValueError):
            diverse_pick_reference(np.eye(2), 0.5, k)
    with pytest.raises(ValueError):
        diverse_pick_reference(np.eye(2), NAN, 1)
    assert torch.is_tensor(torch.eye(3)) and diverse_pick_reference(torch.eye(3), 0.5, 3)[1] == 3          # tensors are taken as they are


def test_the_arc_depends_on_the_order_of_the_walk():
    """Neighbours on the arc are more similar than 0.9, second neighbours less: walked forwards the picks are every other row from
    the first, walked backwards every other row from the last -- different molecules."""
    from molkgnn_amd.screening import cosine_reference
    rows = DC.arc(16, np.random.default_rng(4)).astype(np.float32)
    sim = cosine_reference(rows, rows)
    assert abs(sim[1, 0] - np.cos(DC.ARC_STEP)) < 1e-6 and abs(sim[2, 0] - np.cos(2 * DC.ARC_STEP)) < 1e-6
    assert sim[1, 0] > DC.MAX_SIM > sim[2, 0]
    forward, leader, _ = _walk(sim, DC.MAX_SIM, DC.ARC_ROWS)
    assert forward == [0, 2, 4, 6] and leader == [0, 0, 2, 2, 4, 4, 6, 6]
    back = rows[::-1]
    backward, leader, _ = _walk(cosine_reference(back, back), DC.MAX_SIM, DC.ARC_ROWS)
    assert backward == [0, 2, 4, 6] and leader == [0, 0, 2, 2, 4, 4, 6, 6]
    assert [DC.ARC_ROWS - 1 - p for p in backward] == [7, 5, 3, 1]          # in terms of the same molecules: the other half


def test_fixtures_keep_their_distance_from_the_threshold():
    """Every (H, n) the GPU test compares with the float64 walk: no similarity of the lower triangle lies within 4 error bounds of
    the threshold, so a float32 evaluation inside its bound decides every comparison as float64 does -- and no case needs leaving
    out.  The larger cases give several picks, spread over more than one tile."""
    from molkgnn_amd import _lib
    for H in DC.WIDTHS:
        tile = _lib.diverse_tile(H)
        assert DC.sizes(H) == (1, 5, tile - 1, tile, tile + 1, 2 * tile + 37)
        for n in DC.sizes(H):
            emb, picks, n_picks, leader, margin = DC.float64_case(n, H)
            assert emb.shape == (n, H) and emb.dtype == np.float32 and np.isfinite(emb).all()
            assert margin > 4, (H, n, margin)
            assert 1 <= n_picks <= n and (leader >= 0).all(), (H, n)
            if n >= tile - 1 and H >= 2:
                assert n_picks >= 16, (H, n, n_picks)
            if n > 2 * tile and H >= 2:                            # (new centres keep turning up: picks in the later tiles too)
                assert (picks[:n_picks] >= tile).sum() >= 8 and (picks[:n_picks] < tile).sum() >= 8, (H, n, n_picks)
            if n > tile:                                           # (and rows of a later tile led by a pick of an earlier one)
                assert (leader[tile:] < tile).any(), (H, n)


def test_rank_order_follows_the_running_list():
    """``rank_order`` against ``topk_update_reference`` fed the whole vector: NaN last (torch's descending sort puts it first), signed
    zeros tied, ties to the lower row, a true -inf score in front of the NaNs."""
    from molkgnn_amd.screening import empty_top, rank_order, topk_update_reference
    s = np.array([0.5, NAN, -0.0, 0.0, 2.0, -np.inf, 0.5, NAN, np.inf, -3.0, 0.0], dtype=np.float32)
    want = topk_update_reference(empty_top(len(s)), s, np.arange(len(s), dtype=np.int32), len(s), 0)[2]
    got = rank_order(torch.from_numpy(s))
    assert got.dtype == torch.int64 and got.tolist() == want.tolist() == [8, 4, 0, 6, 2, 3, 10, 9, 5, 1, 7]


@pytest.fixture(scope="module")
def cpu_shard(tmp_path_factory):
    from molkgnn_amd import shards as S
    from molkgnn_amd.synthetic import make_batch
    path = str(tmp_path_factory.mktemp("diverse") / "lib.mkgs")
    S.write_shard(path, make_batch(40, seed=6, assay="all9", with_receptive_fields=False))
    return S.ResidentShard(path, "cpu")


def test_rejections_before_any_launch(cpu_shard, monkeypatch):
    """A NaN or infinite threshold, k beyond the pool or the rows, a pool beyond the running list, a multi-task model, CPU tensors, a
    CPU model or shard, wrong shapes and dtypes: ``ValueError`` from every entry point, and the library is not even loaded."""
    from molkgnn_amd import _lib, readout, screening
    from molkgnn_amd.train import GNNModel

    def no_load():
        raise AssertionError("the library was loaded before the refusal")

    monkeypatch.setattr(_lib, "load", no_load)
    torch.manual_seed(0)
    one, nine = GNNModel(num_layers=1, task_dim=1), GNNModel(num_layers=1, task_dim=9)      # (hidden_dim = 32 = G; on the CPU)
    for bad in (NAN, float("inf"), float("-inf")):
        with pytest.raises(ValueError, match="max_sim"):
            screening.screen_diverse(one, [cpu_shard], 4, 32, bad)
        with pytest.raises(ValueError, match="max_sim"):
            screening.pick_diverse_embeddings(torch.zeros(10, 32), torch.zeros(10), bad, 4)
        with pytest.raises(ValueError, match="max_sim"):
            readout.diverse_pick(torch.zeros(10, 32), bad)
    with pytest.raises(ValueError, match="pool"):
        screening.screen_diverse(one, [cpu_shard], 65, 32, 0.9, pool=64)
    with pytest.raises(ValueError, match="pool"):
        screening.screen_diverse(one, [cpu_shard], 4, 32, 0.9, pool=1025)
    with pytest.raises(ValueError, match="pool"):
        screening.screen_diverse(one, [cpu_shard], 0, 32, 0.9)
    with pytest.raises(ValueError, match="one-task"):
        screening.screen_diverse(nine, [cpu_shard], 4, 32, 0.9)
    with pytest.raises(ValueError, match="GPU"):
        screening.screen_diverse(one, [cpu_shard], 4, 32, 0.9)
    with pytest.raises(ValueError, match="batch_size"):
        screening.screen_diverse(one, [cpu_shard], 4, 0, 0.9)
    emb, scores = torch.zeros(10, 32), torch.zeros(10)
    with pytest.raises(ValueError, match="GPU"):
        screening.pick_diverse_embeddings(emb, scores, 0.9, 4)
    with pytest.raises(ValueError, match="GPU"):
        readout.diverse_pick(emb, 0.9)
    for args in ((emb.double(), scores, 0.9, 4), (emb, scores.double(), 0.9, 4), (emb, scores[:9], 0.9, 4), (emb[0], scores, 0.9, 4),
                 (emb, scores, 0.9, 0), (emb, scores, 0.9, 11), (emb, scores, 0.9, 4, torch.zeros(10)), (emb, scores, 0.9, 4, torch.zeros(9, dtype=torch.int32))):
        with pytest.raises(ValueError):
            screening.pick_diverse_embeddings(*args)
    for args in ((emb.double(), 0.9), (emb[0], 0.9), (torch.zeros(10, 0), 0.9)):
        with pytest.raises(ValueError):
            readout.diverse_pick(*args)
