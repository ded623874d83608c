"""Host side of the analogue search for any number of queries (``mkgnn_embed_knn_update``, ``readout.embedding_knn_update``,
``screening.NearestLists`` / ``nearest_many`` / ``nearest_embeddings``): the additive exports, the split the binding mirrors, the
workspace size, and everything that is refused before the library is loaded or anything is launched."""
import ctypes
import os
import re

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_points_are_additive_to_abi_8():
    from molkgnn_amd import _lib
    with open(os.path.join(REPO, "include", "molkgnn_hip.h")) as f:
        h = f.read()
    m = re.search(r"#define\s+MKGNN_ABI_VERSION\s+(\d+)", h)
    assert m and int(m.group(1)) == 8 and _lib.ABI_VERSION == 8
    assert re.search(r"\bint mkgnn_embed_knn_update\(const float\* emb, int64_t emb_stride, int64_t n_rows, int32_t H, const int32_t\* ids,", h)
    assert re.search(r"\bsize_t mkgnn_embed_knn_workspace_bytes\(int64_t n_rows, int32_t Q, int32_t K\);", h)
    for name, value in (("MKGNN_KNN_MAX_K", _lib.KNN_MAX_K), ("MKGNN_KNN_MAX_QUERIES", _lib.KNN_MAX_QUERIES),
                        ("MKGNN_KNN_MAX_ROWS", _lib.KNN_MAX_ROWS)):
        m = re.search(r"#define\s+" + name + r"\s+(\d+)\b", h)
        assert m and int(m.group(1)) == value, name
    assert (_lib.KNN_MAX_K, _lib.KNN_MAX_QUERIES, _lib.KNN_MAX_ROWS) == (64, 1 << 20, 1 << 20)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    raw.mkgnn_abi_version.restype = ctypes.c_int
    assert raw.mkgnn_abi_version() == 8
    lib = _lib.load()
    for name, n_args, restype in (("mkgnn_embed_knn_update", 17, ctypes.c_int), ("mkgnn_embed_knn_workspace_bytes", 3, ctypes.c_size_t)):
        assert hasattr(raw, name) and name in _lib.EXPORTS
        assert getattr(lib, name).restype is restype and len(getattr(lib, name).argtypes) == n_args, name
    # what was there is what it was
    assert lib.mkgnn_embed_cosine.restype is ctypes.c_int and len(lib.mkgnn_embed_cosine.argtypes) == 11
    assert lib.mkgnn_embed_max_cosine.restype is ctypes.c_int and len(lib.mkgnn_embed_max_cosine.argtypes) == 12
    assert lib.mkgnn_topk_update_tasks.restype is ctypes.c_int and len(lib.mkgnn_topk_update_tasks.argtypes) == 15
    assert lib.mkgnn_kernel_exemplars_update.restype is ctypes.c_int and len(lib.mkgnn_kernel_exemplars_update.argtypes) == 22
    assert _lib.EMBED_COSINE_MAX_QUERIES == 32 and _lib.TASK_HEAD_MAX_TASKS == 32


def _header_split(n, Q):
    """The split as include/molkgnn_hip.h words it: parts of whole tiles of 64 rows, at least two tiles each, at most 32 parts, and
    no more than bring the grid to 1 024 blocks of four queries."""
    tiles = (n + 63) // 64
    blocks = (Q + 3) // 4
    want = min((1024 + blocks - 1) // blocks, 32)
    per_part = max((tiles + want - 1) // want, 2)
    return per_part * 64, max((tiles + per_part - 1) // per_part, 1)


def test_split_on_planted_sizes():
    """``_lib.knn_split`` equals what the header says, parts never exceed the bound, and every row is covered exactly once."""
    from molkgnn_amd import _lib
    tile, parts_max = _lib.KNN_TILE, _lib.KNN_MAX_PARTS
    assert (_lib.KNN_WAVES, tile, _lib.KNN_MIN_PART_TILES, parts_max, _lib.KNN_TARGET_BLOCKS) == (4, 64, 2, 32, 1024)
    sizes = [(n, Q) for n in (0, 1, 63, 64, 65, 127, 128, 129, 385, 4096, 4097, 16001, 16384, 65536, (1 << 20) - 1, 1 << 20)
             for Q in (1, 2, 3, 4, 5, 33, 128, 129, 256, 2048, 4092, 4093, 4096, 1 << 20)]
    for n, Q in sizes:
        per_part, parts = _lib.knn_split(n, Q)
        assert (per_part, parts) == _header_split(n, Q), (n, Q)
        assert per_part % tile == 0 and per_part >= _lib.KNN_MIN_PART_TILES * tile and 1 <= parts <= parts_max, (n, Q)
        # part p takes the rows [p * per_part, min(n, (p + 1) * per_part)): disjoint by construction, none empty but a lone first
        # one, and together all n rows
        assert (parts - 1) * per_part < max(n, 1) <= parts * per_part, (n, Q)
        blocks = -(-Q // _lib.KNN_WAVES)
        assert parts == 1 or parts * blocks < _lib.KNN_TARGET_BLOCKS + blocks, (n, Q)      # the grid is not overfilled
        if Q > 4092:
            assert parts == 1, (n, Q)
    # more than one part, and parts of more than one tile, at Q = 1 within 16 384 rows
    assert _lib.knn_split(129, 1) == (128, 2) and _lib.knn_split(385, 1) == (128, 4)
    assert _lib.knn_split(16384, 1) == (512, 32) and _lib.knn_split(16001, 1) == (512, 32)
    assert _lib.knn_split(1 << 20, 256) == (65536, 16) and _lib.knn_split(4096, 256) == (256, 16)


def test_workspace_bytes_on_the_host():
    """The workspace follows the split: the norms, and the parts' lists only where there is more than one part; rejected sizes
    have size 0 (host code only: nothing is launched)."""
    from molkgnn_amd import _lib
    lib = _lib.load()
    for n, Q, K in ((1, 1, 1), (0, 7, 3), (129, 1, 64), (385, 33, 5), (16384, 1, 64), (4096, 256, 16), (1 << 20, 2048, 64),
                    (1 << 20, 1 << 20, 64), (1000, 4093, 8)):
        _, parts = _lib.knn_split(n, Q)
        norms = (Q + n + 3) // 4 * 4
        assert lib.mkgnn_embed_knn_workspace_bytes(n, Q, K) == 4 * (norms + (3 * parts * Q * K if parts > 1 else 0)), (n, Q, K)
        # a small multiple of the lists' own size, and bounded whatever Q
        lists = 12 * parts * Q * K if parts > 1 else 0
        assert lists <= 32 * 12 * Q * K and lists <= 2047 * 4 * K * 12
    for n, Q, K in ((-1, 5, 5), ((1 << 20) + 1, 5, 5), (5, 0, 5), (5, -2, 5), (5, (1 << 20) + 1, 5), (5, 5, 0), (5, 5, 65), (5, 5, -1)):
        assert lib.mkgnn_embed_knn_workspace_bytes(n, Q, K) == 0, (n, Q, K)


@pytest.fixture(scope="module")
def cpu_shard(tmp_path_factory):
    from molkgnn_amd import shards as S
    from molkgnn_amd.synthetic import make_batch
    path = str(tmp_path_factory.mktemp("knn") / "lib.mkgs")
    S.write_shard(path, make_batch(40, seed=6, assay="all9", with_receptive_fields=False))
    return S.ResidentShard(path, "cpu")


def test_rejections_before_any_launch(cpu_shard, monkeypatch):
    """A CPU tensor, ``K`` = 0 or 65, ``Q`` = 0, a width mismatch, a wrong dtype, a non-contiguous list, ``NearestLists`` on a CPU
    device, a CPU model or shard: ``ValueError`` from every entry point, and the library is not even loaded."""
    from molkgnn_amd import _lib, readout, screening
    from molkgnn_amd.train import GNNModel

    def no_load():
        raise AssertionError("the library was loaded before the refusal")

    monkeypatch.setattr(_lib, "load", no_load)
    G, n = 32, 10

    def lists(Q, K, wide=None):
        shape = (Q, K if wide is None else wide)
        out = (torch.zeros(shape), torch.zeros(shape, dtype=torch.int32), torch.zeros(shape, dtype=torch.int32))
        return tuple(t[:, :K] for t in out)

    emb, q = torch.zeros(n, G), torch.zeros(3, G)
    assert readout.embedding_knn_supported(1, 1) and readout.embedding_knn_supported(64, 64)
    assert not readout.embedding_knn_supported(65, 8) and not readout.embedding_knn_supported(32, 65)
    assert not readout.embedding_knn_supported(0, 8) and not readout.embedding_knn_supported(32, 0)
    with pytest.raises(ValueError, match="GPU"):                   # all is well but the device
        readout.embedding_knn_update(emb, q, *lists(3, 8))
    with pytest.raises(ValueError, match="outside"):
        readout.embedding_knn_update(emb, q, *lists(3, 0))
    with pytest.raises(ValueError, match="rank_embeddings"):
        readout.embedding_knn_update(emb, q, *lists(3, 65))
    with pytest.raises(ValueError, match="queries"):
        readout.embedding_knn_update(emb, q[:0], *lists(0, 8))
    with pytest.raises(ValueError, match="wide"):
        readout.embedding_knn_update(emb, torch.zeros(3, G + 1), *lists(3, 8))
    with pytest.raises(ValueError, match="float32"):
        readout.embedding_knn_update(emb.double(), q, *lists(3, 8))
    with pytest.raises(ValueError, match="contiguous"):
        readout.embedding_knn_update(emb, q, *lists(3, 8, wide=9))
    with pytest.raises(ValueError, match=r"\[3, 8\]"):
        readout.embedding_knn_update(emb, q, *lists(4, 8))
    s, h, m = lists(3, 8)
    with pytest.raises(ValueError, match="int32"):
        readout.embedding_knn_update(emb, q, s, h.long(), m)
    # the running lists
    with pytest.raises(ValueError, match="GPU"):
        screening.NearestLists(8, 3, "cpu")
    for k in (0, 65):
        with pytest.raises(ValueError, match="MKGNN_KNN_MAX_K"):
            screening.NearestLists(k, 3, "cuda:0")
    for Q in (0, (1 << 20) + 1):
        with pytest.raises(ValueError, match="MKGNN_KNN_MAX_QUERIES"):
            screening.NearestLists(8, Q, "cuda:0")
    # the screening entry points: the queries' value checks first, the device last
    torch.manual_seed(0)
    model = GNNModel(num_layers=1, task_dim=9)                     # (hidden_dim = 32 = G; on the CPU)
    bad = {"queries outside": torch.zeros(0, G), "wide": torch.zeros(3, G + 1), "float32": torch.zeros(3, G, dtype=torch.float64),
           r"\[Q, ": torch.zeros(G)}
    for word, queries in bad.items():
        with pytest.raises(ValueError, match=word):
            screening.nearest_many(model, queries, [cpu_shard], 8, 32)
        with pytest.raises(ValueError, match=word):
            screening.nearest_many_resident(model, cpu_shard, queries, 32, lists=None)
        with pytest.raises(ValueError, match=word):
            screening.nearest_embeddings(emb, queries, None)
    for k in (0, 65):
        with pytest.raises(ValueError, match="MKGNN_KNN_MAX_K"):
            screening.nearest_many(model, q, [cpu_shard], k, 32)
    with pytest.raises(ValueError, match="GPU"):
        screening.nearest_many(model, q, [cpu_shard], 8, 32)
    with pytest.raises(ValueError, match="GPU"):
        screening.nearest_many(model, cpu_shard, [cpu_shard], 8, 32)                       # (queries as a shard: embedded first)
    with pytest.raises(ValueError, match="GPU"):
        screening.nearest_many_resident(model, cpu_shard, q, 32, lists=None)
    with pytest.raises(ValueError, match="GPU"):
        screening.nearest_embeddings(emb, q, None)
    with pytest.raises(ValueError, match="float32"):
        screening.nearest_embeddings(emb.double(), q, None)
