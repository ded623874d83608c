"""Host side of analogue search (``mkgnn_embed_cosine``, ``readout.embedding_cosine``, ``screening.nearest*`` / ``embed_resident`` /
``rank_embeddings``): the additive export, the numpy definition against torch's ``cosine_similarity`` in float64, a sequential
float32 emulation of the definition against the stated error bound over a sweep of widths and scales, and everything that is
refused before a launch."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS32 = float(np.float32(1e-8))
WIDTHS = (1, 2, 31, 32, 33, 63, 64)
SCALES = (1e-30, 1e-25, 1e-20, 1e-15, 1e-10, 1e-5, 1.0, 1e5, 1e10, 1e15)


def test_entry_point_is_additive_to_abi_8():
    from molkgnn_amd import _lib
    with open(os.path.join(REPO, "include", "molkgnn_hip.h")) as f:
        h = f.read()
    m = re.search(r"#define\s+MKGNN_ABI_VERSION\s+(\d+)", h)
    assert m and int(m.group(1)) == 8 and _lib.ABI_VERSION == 8
    assert re.search(r"\bint mkgnn_embed_cosine\(const float\* emb, int64_t emb_stride, int64_t n_rows, int32_t H,", h)
    assert re.search(r"#define\s+MKGNN_EMBED_COSINE_MAX_QUERIES\s+32\b", h)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    raw.mkgnn_abi_version.restype = ctypes.c_int
    assert raw.mkgnn_abi_version() == 8
    assert hasattr(raw, "mkgnn_embed_cosine") and "mkgnn_embed_cosine" in _lib.EXPORTS
    lib = _lib.load()
    assert lib.mkgnn_embed_cosine.restype is ctypes.c_int and len(lib.mkgnn_embed_cosine.argtypes) == 11
    assert _lib.EMBED_COSINE_MAX_QUERIES == 32 <= _lib.TASK_HEAD_MAX_TASKS
    # what was there is what it was
    assert lib.mkgnn_task_scores.restype is ctypes.c_int and len(lib.mkgnn_task_scores.argtypes) == 11


def _vectors(n, H, scale, seed):
    """float32 ``[n, H]`` rows at ``scale`` whose first rows are the hazards: zeros, a row below the clamp, denormals."""
    rng = np.random.default_rng(seed)
    a = (rng.standard_normal((n, H)) * scale).astype(np.float32)
    a[0] = 0.0
    a[1] = np.float32(3e-9) / np.sqrt(np.float32(H))                        # norm 3e-9 < eps
    a[2] = (np.float32(1e-41) * np.arange(1, H + 1)).astype(np.float32)     # denormals
    return a


@pytest.mark.parametrize("H", WIDTHS)
def test_reference_is_torchs_cosine_similarity_in_float64(H):
    """1e-12 relative plus 1e-14 absolute, on rows at every scale, zero rows and rows with a norm below eps included; torch is given
    the definition's eps, float32(1e-8), as a double."""
    from molkgnn_amd.screening import COSINE_EPS, cosine_reference
    assert float(COSINE_EPS) == EPS32
    for scale in SCALES:
        e, q = _vectors(12, H, scale, 7 * H), _vectors(5, H, 1.0, 7 * H + 1)
        got = cosine_reference(e, q)
        assert got.shape == (12, 5) and got.dtype == np.float64
        e64, q64 = torch.from_numpy(e).double(), torch.from_numpy(q).double()
        want = torch.nn.functional.cosine_similarity(e64[:, None, :], q64[None, :, :], dim=-1, eps=EPS32).numpy()
        assert (np.abs(got - want) <= 1e-12 * np.abs(want) + 1e-14).all(), (H, scale, np.abs(got - want).max())
        assert (got[0] == 0).all() and (got[:, 0] == 0).all()               # a zero row, a zero query
    # tensors are taken as they are; a NaN stays in its row and its column
    e, q = torch.randn(6, H), torch.randn(4, H)
    assert np.array_equal(cosine_reference(e, q), cosine_reference(e.numpy(), q.numpy()))
    e[2, 0], q[1, H - 1] = float("nan"), float("nan")
    nan = np.isnan(cosine_reference(e, q))
    want = np.zeros((6, 4), dtype=bool)
    want[2, :], want[:, 1] = True, True
    assert np.array_equal(nan, want)
    with pytest.raises(ValueError):
        cosine_reference(np.zeros((3, H)), np.zeros((2, H + 1)))


def _float32_cosine(e, q):
    """The definition evaluated in float32, sequentially, one rounding per operation: products and sums left to right, the square
    root, the clamp, the division, ``(dot * ie) * iq``."""
    f = np.float32

    def inv(v):
        s = f(0)
        for x in v:
            s = f(s + f(x * x))
        return f(f(1) / max(np.sqrt(s), f(1e-8)))

    out = np.empty((len(e), len(q)), dtype=np.float32)
    ie, iq = [inv(r) for r in e], [inv(r) for r in q]
    for i, r in enumerate(e):
        for j, c in enumerate(q):
            d = f(0)
            for x, y in zip(r, c):
                d = f(d + f(x * y))
            out[i, j] = f(f(d * ie[i]) * iq[j])
    return out


@pytest.mark.parametrize("H", WIDTHS)
def test_float32_emulation_stays_inside_the_bound(H):
    """Every element, at every scale from 1e-30 to 1e15, with zero, clamped, denormal, equal and opposite rows.  The half spacing of
    the denormals is reached exactly at H = 1, scale 1e-20: with the bound's factor two the ratio stays at or below one half
    there."""
    from molkgnn_amd.screening import cosine_bound, cosine_reference
    worst = 0.0
    with np.errstate(under="ignore", over="ignore"):
        for scale in SCALES:
            for qscale in (1.0, scale):
                q = (np.random.default_rng(H).standard_normal((4, H)) * qscale).astype(np.float32)
                e = _vectors(10, H, scale, 100 + H)
                e[3], e[4] = q[1] * np.float32(scale / qscale), -q[2]       # a multiple of a query, the negative of one
                e[5] = q[3]
                got = _float32_cosine(e, q).astype(np.float64)
                err = np.abs(got - cosine_reference(e, q))
                bound = cosine_bound(e, q)
                assert bound.shape == (10, 4) and (bound >= 2.0 ** -149).all()
                assert (err <= bound).all(), (H, scale, qscale, float((err / bound).max()))
                worst = max(worst, float((err / bound).max()))
    print(f"H={H}: worst error / bound = {worst:.3f}")
    assert worst <= 1.0


@pytest.fixture(scope="module")
def cpu_shard(tmp_path_factory):
    from molkgnn_amd import shards as S
    from molkgnn_amd.synthetic import make_batch
    path = str(tmp_path_factory.mktemp("nearest") / "lib.mkgs")
    S.write_shard(path, make_batch(40, seed=6, assay="all9", with_receptive_fields=False))
    return S.ResidentShard(path, "cpu")


def test_rejections_before_any_launch(cpu_shard, monkeypatch):
    """A CPU tensor, Q = 0 or Q = 33, a wrong G, a wrong dtype, a CPU model or shard: ``ValueError`` from every entry point, and the
    library is not even loaded."""
    from molkgnn_amd import _lib, readout, screening
    from molkgnn_amd.train import GNNModel

    def no_load():
        raise AssertionError("the library was loaded before the refusal")

    monkeypatch.setattr(_lib, "load", no_load)
    torch.manual_seed(0)
    model = GNNModel(num_layers=1, task_dim=9)                  # (hidden_dim = 32 = G; on the CPU)
    G = 32
    good = torch.zeros(3, G)
    bad = {"queries outside": torch.zeros(0, G), "33 queries": torch.zeros(33, G), "wide": torch.zeros(3, G + 1),
           "float32": torch.zeros(3, G, dtype=torch.float64), r"\[Q, ": torch.zeros(G)}
    for word, q in bad.items():
        with pytest.raises(ValueError, match=word):
            screening.nearest_resident(model, cpu_shard, q, 32)
        with pytest.raises(ValueError, match=word):
            screening.nearest(model, q, [cpu_shard], 4, 32)
        with pytest.raises(ValueError, match=word):
            screening.rank_embeddings(torch.zeros(10, G), q, None)
        with pytest.raises(ValueError):
            readout.embedding_cosine(torch.zeros(10, G), q)
    # well-formed queries, on the CPU: the device is what is refused
    with pytest.raises(ValueError, match="GPU"):
        screening.nearest_resident(model, cpu_shard, good, 32)
    with pytest.raises(ValueError, match="GPU"):
        screening.nearest(model, good, [cpu_shard], 4, 32)
    with pytest.raises(ValueError, match="query shard"):
        screening.nearest(model, cpu_shard, [cpu_shard], 4, 32)                 # (a query shard of 40 molecules)
    with pytest.raises(ValueError, match="GPU"):
        screening.embed_resident(model, cpu_shard, 32)
    with pytest.raises(ValueError, match="GPU"):
        screening.rank_embeddings(torch.zeros(10, G), good, None)
    with pytest.raises(ValueError, match="GPU"):
        readout.embedding_cosine(torch.zeros(10, G), good)
    with pytest.raises(ValueError):
        screening.rank_embeddings(torch.zeros(10, G, dtype=torch.float64), good, None)
    with pytest.raises(ValueError):
        readout.embedding_cosine(torch.zeros(10, G, dtype=torch.float64), good)
    # embedding a shard takes any task_dim; the single-score entry points refuse a multi-task model as before
    with pytest.raises(ValueError, match="one-task"):
        screening.score_resident(model, cpu_shard, 32)
