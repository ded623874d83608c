"""Host side of the novelty filter (``mkgnn_embed_max_cosine``, ``mkgnn_select_rows``, ``readout.embedding_max_cosine`` /
``select_rows``, ``screening.reference_similarity_resident`` / ``screen_novel``): the additive exports, the two numpy definitions on
planted cases against brute-force loops, and everything that is refused before a launch."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_points_are_additive_to_abi_8():
    from molkgnn_amd import _lib
    with open(os.path.join(REPO, "include", "molkgnn_hip.h")) as f:
        h = f.read()
    m = re.search(r"#define\s+MKGNN_ABI_VERSION\s+(\d+)", h)
    assert m and int(m.group(1)) == 8 and _lib.ABI_VERSION == 8
    assert re.search(r"\bint mkgnn_embed_max_cosine\(const float\* emb, int64_t emb_stride, int64_t n_rows, int32_t H, const float\* refs,", h)
    assert re.search(r"\bsize_t mkgnn_embed_max_cosine_workspace_bytes\(int64_t n_rows, int32_t R\);", h)
    assert re.search(r"\bint mkgnn_select_rows\(const float\* scores, const int32_t\* ids, const float\* key, int32_t B,", h)
    m = re.search(r"#define\s+MKGNN_MAX_COSINE_MAX_REFS\s+(\d+)\b", h)
    assert m and int(m.group(1)) == _lib.MAX_COSINE_MAX_REFS >= 65536
    raw = ctypes.CDLL(_lib.LIB_PATH)
    raw.mkgnn_abi_version.restype = ctypes.c_int
    assert raw.mkgnn_abi_version() == 8
    lib = _lib.load()
    for name, n_args, restype in (("mkgnn_embed_max_cosine", 12, ctypes.c_int), ("mkgnn_select_rows", 10, ctypes.c_int),
                                  ("mkgnn_embed_max_cosine_workspace_bytes", 2, ctypes.c_size_t)):
        assert hasattr(raw, name) and name in _lib.EXPORTS
        assert getattr(lib, name).restype is restype and len(getattr(lib, name).argtypes) == n_args, name
    # what was there is what it was
    assert lib.mkgnn_embed_cosine.restype is ctypes.c_int and len(lib.mkgnn_embed_cosine.argtypes) == 11
    assert lib.mkgnn_topk_update.restype is ctypes.c_int and len(lib.mkgnn_topk_update.argtypes) == 12
    assert _lib.EMBED_COSINE_MAX_QUERIES == 32


def test_sizes_on_the_host():
    """The workspace size follows the split the binding mirrors; rejected sizes have size 0 (host code only: nothing is launched)."""
    from molkgnn_amd import _lib
    lib = _lib.load()
    rows, tile, parts = _lib.MAX_COSINE_ROWS, _lib.MAX_COSINE_TILE, _lib.MAX_COSINE_MAX_PARTS
    for n, R in ((1, 1), (rows, tile), (rows + 1, tile + 1), (1000, 3 * tile), (17, tile * parts + 1), (4096, 16384), (256, 1024),
                 (100000, 5), (3, _lib.MAX_COSINE_MAX_REFS)):
        per_part, p = _lib.max_cosine_split(n, R)
        assert per_part % tile == 0 and 1 <= p <= parts and (p - 1) * per_part < R <= p * per_part, (n, R)
        norms = (R + n + 3) // 4 * 4
        assert lib.mkgnn_embed_max_cosine_workspace_bytes(n, R) == 4 * (norms + (2 * p * n if p > 1 else 0)), (n, R)
    assert _lib.max_cosine_split(1000, 3 * tile) == (tile, 3)
    assert _lib.max_cosine_split(17, tile * parts + 1) == (2 * tile, parts // 2 + 1)
    for n, R in ((0, 5), (-1, 5), (5, 0), (5, _lib.MAX_COSINE_MAX_REFS + 1), (1 << 31, 5)):
        assert lib.mkgnn_embed_max_cosine_workspace_bytes(n, R) == 0, (n, R)


def _brute_max(sim):
    """The stated order, one comparison at a time."""
    out, arg = np.full(len(sim), np.nan), np.zeros(len(sim), dtype=np.int64)
    for i, row in enumerate(sim):
        have = False
        for r, s in enumerate(row):
            if np.isnan(s):
                continue
            if not have or s > out[i]:
                out[i], arg[i], have = s, r, True
    return out, arg


def test_max_cosine_reference_on_planted_cases():
    from molkgnn_amd.screening import cosine_reference, max_cosine_reference
    rng = np.random.default_rng(3)
    H = 7
    refs = rng.standard_normal((9, H)).astype(np.float32)
    refs[6] = refs[2]                                              # a duplicate: the lower index wins
    refs[4] = np.nan                                               # a NaN reference is skipped
    emb = rng.standard_normal((8, H)).astype(np.float32)
    emb[0] = 0.0                                                   # a zero row: every similarity 0 -> index 0
    emb[1] = refs[2]                                               # equal to the duplicated reference
    emb[2] = np.nan                                                # an all-NaN row -> (NaN, 0)
    emb[3] = -refs[0]
    got, arg = max_cosine_reference(emb, refs)
    assert got.dtype == np.float64 and arg.dtype == np.int64 and got.shape == arg.shape == (8,)
    want, warg = _brute_max(cosine_reference(emb, refs))
    assert np.array_equal(arg, warg) and np.array_equal(got, want, equal_nan=True)
    assert arg[1] == 2 and abs(got[1] - 1.0) < 1e-12
    assert got[0] == 0.0 and arg[0] == 0
    assert np.isnan(got[2]) and arg[2] == 0
    assert (arg != 4).all() and not np.isnan(np.delete(got, 2)).any()
    # the NaN reference in FRONT: index 0 is skipped as well, and stays the answer only of the all-NaN row
    refs2 = np.concatenate([np.full((1, H), np.nan, dtype=np.float32), refs])
    got2, arg2 = max_cosine_reference(emb, refs2)
    assert np.array_equal(np.delete(arg2, 2), np.delete(arg, 2) + 1) and arg2[2] == 0
    # -0.0 and +0.0 tie: a zero row against references of either sign, and orthogonal vectors whose products are signed zeros
    e = np.array([[0.0, 0.0], [1.0, 0.0]], dtype=np.float32)
    q = np.array([[-1.0, -1.0], [1.0, 1.0], [0.0, -2.0], [0.0, 2.0]], dtype=np.float32)
    got3, arg3 = max_cosine_reference(e, q)
    assert got3[0] == 0.0 and arg3[0] == 0                         # (-0.0, +0.0, -0.0, +0.0): the first
    e[1] = (0.0, 1.0)
    q = np.array([[-3.0, 0.0], [3.0, 0.0]], dtype=np.float32)      # sims (-0.0, +0.0)
    assert max_cosine_reference(e, q)[1].tolist() == [0, 0]
    # tensors are taken as they are; a width mismatch and an empty reference set are refused
    assert np.array_equal(max_cosine_reference(torch.from_numpy(emb), torch.from_numpy(refs))[1], arg)
    with pytest.raises(ValueError):
        max_cosine_reference(emb, refs[:, :H - 1])
    with pytest.raises(ValueError):
        max_cosine_reference(emb, refs[:0])


def _brute_select(scores, ids, key, n_valid, lo, hi):
    s, d = [], []
    for i in range(len(scores)):
        if i < n_valid and lo <= key[i] <= hi:
            s.append(scores[i])
            d.append(ids[i])
    return np.array(s, dtype=np.float32), np.array(d, dtype=np.int32), len(s)


def test_select_rows_reference_on_planted_cases():
    from molkgnn_amd.screening import select_rows_reference
    B = 12
    rng = np.random.default_rng(5)
    scores = rng.standard_normal(B).astype(np.float32)
    scores[3], scores[5] = np.float32(-0.0), np.float32(np.nan)    # bits are carried: a zero's sign, a NaN
    ids = (100 + np.arange(B)).astype(np.int32)
    key = np.linspace(-1, 1, B).astype(np.float32)
    key[4], key[7] = np.nan, np.nan
    lo, hi = float(key[2]), float(key[9])                          # bounds AT keys: both kept
    for n_valid in (0, -3, 1, 5, B - 1, B, B + 5):
        for a, b in ((lo, hi), (-np.inf, hi), (lo, np.inf), (-np.inf, np.inf), (hi, lo), (lo, lo)):
            s, d, n = select_rows_reference(scores, ids, key, n_valid, a, b)
            ws, wd, wn = _brute_select(scores, ids, key, n_valid, np.float32(a), np.float32(b))
            assert n == wn == len(s) == len(d) and s.dtype == np.float32 and d.dtype == np.int32
            assert np.array_equal(s.view(np.int32), ws.view(np.int32)) and np.array_equal(d, wd), (n_valid, a, b)
    s, d, n = select_rows_reference(scores, ids, key, B + 5, lo, hi)
    assert d.tolist() == [102, 103, 105, 106, 108, 109] and n == 6          # keys 2..9 without the two NaN keys; the ends are kept
    assert select_rows_reference(scores, ids, key, B, -np.inf, np.inf)[2] == B - 2      # a NaN key fails infinite bounds too
    assert select_rows_reference(scores, ids, key, 0, -np.inf, np.inf)[2] == 0
    assert select_rows_reference(scores, ids, key, -3, -np.inf, np.inf)[2] == 0
    with pytest.raises(ValueError):
        select_rows_reference(scores, ids[:-1], key, B, lo, hi)


@pytest.fixture(scope="module")
def cpu_shard(tmp_path_factory):
    from molkgnn_amd import shards as S
    from molkgnn_amd.synthetic import make_batch
    path = str(tmp_path_factory.mktemp("novel") / "lib.mkgs")
    S.write_shard(path, make_batch(40, seed=6, assay="all9", with_receptive_fields=False))
    return S.ResidentShard(path, "cpu")


def test_rejections_before_any_launch(cpu_shard, monkeypatch):
    """CPU tensors, a wrong width or dtype, R = 0, no bound or crossed bounds, a multi-task model, a CPU model or shard: ``ValueError``
    from every entry point, and the library is not even loaded."""
    from molkgnn_amd import _lib, readout, screening
    from molkgnn_amd.train import GNNModel

    def no_load():
        raise AssertionError("the library was loaded before the refusal")

    monkeypatch.setattr(_lib, "load", no_load)
    torch.manual_seed(0)
    one, nine = GNNModel(num_layers=1, task_dim=1), GNNModel(num_layers=1, task_dim=9)      # (hidden_dim = 32 = G; on the CPU)
    G = 32
    good = torch.zeros(3, G)
    bad = {"at least one": torch.zeros(0, G), "wide": torch.zeros(3, G + 1), "float32": torch.zeros(3, G, dtype=torch.float64),
           r"\[R, ": torch.zeros(G)}
    for word, refs in bad.items():
        with pytest.raises(ValueError, match=word):
            screening.reference_similarity_resident(nine, cpu_shard, refs, 32)
        with pytest.raises(ValueError, match=word):
            screening.screen_novel(one, [cpu_shard], 4, 32, refs, max_sim=0.9)
        with pytest.raises(ValueError):
            readout.embedding_max_cosine(torch.zeros(10, G), refs)
    # well-formed references, on the CPU: the device is what is refused
    with pytest.raises(ValueError, match="GPU"):
        screening.reference_similarity_resident(nine, cpu_shard, good, 32)
    with pytest.raises(ValueError, match="GPU"):
        screening.screen_novel(one, [cpu_shard], 4, 32, good, max_sim=0.9)
    with pytest.raises(ValueError, match="GPU"):
        screening.screen_novel(one, [cpu_shard], 4, 32, cpu_shard, min_sim=0.1)         # (references as a shard: embedded first)
    with pytest.raises(ValueError, match="GPU"):
        readout.embedding_max_cosine(torch.zeros(10, G), good)
    with pytest.raises(ValueError):
        readout.embedding_max_cosine(torch.zeros(10, G, dtype=torch.float64), good)
    with pytest.raises(ValueError):
        readout.embedding_max_cosine(torch.zeros(10, G), good, n_rows=11)
    # the bounds, and the model's head, before anything else
    with pytest.raises(ValueError, match="max_sim"):
        screening.screen_novel(one, [cpu_shard], 4, 32, good)
    with pytest.raises(ValueError, match="no similarity"):
        screening.screen_novel(one, [cpu_shard], 4, 32, good, max_sim=0.2, min_sim=0.3)
    with pytest.raises(ValueError, match="no similarity"):
        screening.screen_novel(one, [cpu_shard], 4, 32, good, max_sim=float("nan"))
    with pytest.raises(ValueError, match="one-task"):
        screening.screen_novel(nine, [cpu_shard], 4, 32, good, max_sim=0.9)
    # select_rows: dtypes, lengths, the device
    s, i, k, b = torch.zeros(8), torch.zeros(8, dtype=torch.int32), torch.zeros(8), torch.zeros(2)
    with pytest.raises(ValueError, match="GPU"):
        readout.select_rows(s, i, k, 8, b)
    for args in ((s.double(), i, k, 8, b), (s, i.long(), k, 8, b), (s, i, k[:7], 8, b), (s, i, k, 8, torch.zeros(3)),
                 (s[:0], i[:0], k[:0], 0, b)):
        with pytest.raises(ValueError):
            readout.select_rows(*args)
