"""Host side of the neighbour counts (``mkgnn_embed_count_within``, ``readout.embedding_count_within``,
``screening.count_within_reference`` / ``neighbour_counts``): the additive exports, the workspace size along the mirrored split, the
numpy definition on planted cases against a brute-force loop, everything that is refused before a launch, and the distance of the
fixtures from the threshold that lets the GPU test compare with float64."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import _count_cases as CC

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")


def test_entry_points_are_additive_to_abi_8():
    from molkgnn_amd import _lib
    with open(os.path.join(REPO, "include", "molkgnn_hip.h")) as f:
        h = f.read()
    m = re.search(r"#define\s+MKGNN_ABI_VERSION\s+(\d+)", h)
    assert m and int(m.group(1)) == 8 and _lib.ABI_VERSION == 8
    assert re.search(r"\bsize_t mkgnn_embed_count_within_workspace_bytes\(int64_t n_rows, int32_t R\);", h)
    assert re.search(r"\bint mkgnn_embed_count_within\(const float\* emb, int64_t emb_stride, int64_t n_rows, int32_t H, const float\* refs,"
                     r"\s*int64_t ref_stride,\s*int32_t R, float min_sim, int32_t\* counts, void\* workspace, size_t workspace_bytes,"
                     r"\s*void\* stream\);", h)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    raw.mkgnn_abi_version.restype = ctypes.c_int
    assert raw.mkgnn_abi_version() == 8
    lib = _lib.load()
    for name, n_args, restype in (("mkgnn_embed_count_within", 12, ctypes.c_int),
                                  ("mkgnn_embed_count_within_workspace_bytes", 2, ctypes.c_size_t)):
        assert hasattr(raw, name) and name in _lib.EXPORTS
        assert getattr(lib, name).restype is restype and len(getattr(lib, name).argtypes) == n_args, name
    assert lib.mkgnn_embed_count_within.argtypes[7] is ctypes.c_float          # min_sim, by value
    # what was there is what it was
    assert lib.mkgnn_embed_max_cosine.restype is ctypes.c_int and len(lib.mkgnn_embed_max_cosine.argtypes) == 12
    assert lib.mkgnn_embed_max_cosine_workspace_bytes.restype is ctypes.c_size_t
    assert lib.mkgnn_diverse_pick.restype is ctypes.c_int and len(lib.mkgnn_diverse_pick.argtypes) == 13
    assert lib.mkgnn_embed_cosine.restype is ctypes.c_int and len(lib.mkgnn_embed_cosine.argtypes) == 11
    assert lib.mkgnn_embed_knn_update.restype is ctypes.c_int and len(lib.mkgnn_embed_knn_update.argtypes) == 17
    # the walk over the tiles has one text: the count is a policy of max_cosine_kernel, in the file that is already built
    with open(os.path.join(REPO, "molkgnn_amd", "csrc", "kgnn_max_cosine.hip")) as f:
        text = f.read()
    assert len(re.findall(r"stage_padded_tile<", text)) == 1 and len(re.findall(r"__global__[^;{]*\bmax_cosine_kernel\(", text)) == 1
    assert len(re.findall(r"__global__[^;{]*\bnorms_kernel\(", text)) == 1 and len(re.findall(r"\bMcSplit mc_split\(", text)) == 1
    assert "max_cosine_kernel<32, McCountAbove>" in text and "max_cosine_kernel<32, McFirstMax>" in text
    assert "#pragma clang fp contract(off)" in text
    for name, mirror in (("MC_ROWS", _lib.MAX_COSINE_ROWS), ("MC_TILE", _lib.MAX_COSINE_TILE), ("MC_MAX_PARTS", _lib.MAX_COSINE_MAX_PARTS),
                         ("MC_TARGET_BLOCKS", _lib.MAX_COSINE_TARGET_BLOCKS)):
        m = re.search(r"constexpr int %s = (\d+);" % name, text)
        assert m and int(m.group(1)) == mirror, name


def test_sizes_on_the_host():
    """The workspace size follows the split the binding mirrors -- the norms, and one int32 partial count per part and row when
    the references are split; rejected sizes have size 0 (host code only: nothing is launched)."""
    from molkgnn_amd import _lib
    lib = _lib.load()
    rows, tile, parts = CC.tiling()
    for n, R in CC.shapes() + ((1000, 3 * tile), (4096, 16384), (256, 1024), (100000, 5), (3, _lib.MAX_COSINE_MAX_REFS), (65536, 65536),
                               (1 << 20, 1 << 20)):
        per_part, p = _lib.count_within_split(n, R)
        assert (per_part, p) == _lib.max_cosine_split(n, R)
        assert per_part % tile == 0 and 1 <= p <= parts and (p - 1) * per_part < R <= p * per_part, (n, R)
        norms = (R + n + 3) // 4 * 4
        assert lib.mkgnn_embed_count_within_workspace_bytes(n, R) == 4 * (norms + (p * n if p > 1 else 0)), (n, R)
    assert all(_lib.count_within_split(n, 3 * tile) == (tile, 3) for n in (1, 5, rows - 1, rows, rows + 1, 2 * rows + 37))
    assert _lib.count_within_split(17, tile * parts + 1) == (2 * tile, parts // 2 + 1)
    assert _lib.count_within_split(5, tile + 1) == (tile, 2) and _lib.count_within_split(5, tile) == (tile, 1)
    for n, R in ((0, 5), (-1, 5), (5, 0), (5, _lib.MAX_COSINE_MAX_REFS + 1), (1 << 31, 5)):
        assert lib.mkgnn_embed_count_within_workspace_bytes(n, R) == 0, (n, R)
    # its sibling's sizes are what they were
    assert lib.mkgnn_embed_max_cosine_workspace_bytes(1000, 3 * tile) == 4 * ((3 * tile + 1000 + 3) // 4 * 4 + 2 * 3 * 1000)


def _brute_count(sim, bound):
    """One comparison at a time, in the matrix's own dtype."""
    out = np.zeros(len(sim), dtype=np.int64)
    for i, row in enumerate(sim):
        for s in row:
            if not np.isnan(s) and s > bound:
                out[i] += 1
    return out


def test_count_within_reference_on_planted_cases():
    from molkgnn_amd.screening import count_within_reference
    for dtype in (np.float32, np.float64):
        t = dtype(0.5)
        up, down = np.nextafter(t, dtype(1)), np.nextafter(t, dtype(-1))
        sim = np.array([[t, up, down, t, NAN, 1.0],               # a threshold EQUAL to two elements: strict, they do not count
                        [NAN, NAN, NAN, NAN, NAN, NAN],            # a NaN row counts nothing
                        [-0.0, 0.0, -0.0, 0.0, -1.0, NAN],
                        [up, up, up, up, up, up]], dtype=dtype)
        got = count_within_reference(sim, t)
        assert got.dtype == np.int64 and got.tolist() == [2, 0, 0, 6] and np.array_equal(got, _brute_count(sim, t))
        assert count_within_reference(sim, down).tolist() == [4, 0, 0, 6]          # the two elements at the threshold count again
        assert count_within_reference(sim, up).tolist() == [1, 0, 0, 0]
        # -0.0 against +0.0: neither lies above the other, whichever is the threshold
        assert count_within_reference(sim, 0.0)[2] == 0 and count_within_reference(sim, -0.0)[2] == 0
        assert count_within_reference(sim, -1e-30)[2] == 4 and np.array_equal(count_within_reference(sim, -1e-30), _brute_count(sim, dtype(-1e-30)))
        # every non-NaN element, and none
        assert count_within_reference(sim, -1.5).tolist() == [5, 0, 5, 6] and count_within_reference(sim, 1.5).tolist() == [0, 0, 0, 0]
        rng = np.random.default_rng(11)
        big = rng.uniform(-1, 1, (13, 37)).astype(dtype)
        big[rng.integers(0, 13, 20), rng.integers(0, 37, 20)] = np.nan
        for bound in (0.0, 0.3, float(big[2, 2]) if not np.isnan(big[2, 2]) else 0.1, -0.99):
            assert np.array_equal(count_within_reference(big, bound), _brute_count(big, dtype(bound)))
    # the threshold is rounded to the matrix's dtype first: 0.1 in float32 lies above 0.1 in float64
    assert float(np.float32(0.1)) > 0.1
    s32 = np.array([[np.float32(0.1)]], dtype=np.float32)
    assert count_within_reference(s32, 0.1).tolist() == [0] and count_within_reference(s32.astype(np.float64), 0.1).tolist() == [1]
    assert count_within_reference(torch.from_numpy(s32), 0.1).tolist() == [0]            # tensors are taken as they are
    assert count_within_reference(np.zeros((3, 0)), 0.5).tolist() == [0, 0, 0]
    for bad in (np.zeros(4), np.zeros((2, 2), dtype=np.int32)):
        with pytest.raises(ValueError):
            count_within_reference(bad, 0.5)
    for bad in (NAN, np.inf, -np.inf):
        with pytest.raises(ValueError):
            count_within_reference(np.eye(2), bad)


def test_rejections_before_any_launch(monkeypatch):
    """CPU tensors, a wrong width, shape or dtype, no reference, a NaN or infinite threshold, ``n_rows`` beyond the tensor, a
    recorded gradient: ``ValueError`` / ``RuntimeError`` from both entry points, and the library is not even loaded."""
    from molkgnn_amd import _lib, readout, screening

    def no_load():
        raise AssertionError("the library was loaded before the refusal")

    monkeypatch.setattr(_lib, "load", no_load)
    G = 32
    emb, refs = torch.zeros(10, G), torch.zeros(3, G)
    for bad in (NAN, float("inf"), float("-inf")):
        with pytest.raises(ValueError, match="finite"):
            readout.embedding_count_within(emb, refs, bad)
        with pytest.raises(ValueError, match="finite"):
            screening.neighbour_counts(emb, refs, bad)
    for e, r in ((emb, torch.zeros(0, G)), (emb, torch.zeros(3, G + 1)), (emb, refs.double()), (emb.double(), refs), (emb, torch.zeros(G)),
                 (emb[0], refs), (torch.zeros(10, 0), torch.zeros(3, 0)), (emb.numpy(), refs)):
        with pytest.raises(ValueError):
            readout.embedding_count_within(e, r, 0.9)
        with pytest.raises(ValueError):
            screening.neighbour_counts(e, r, 0.9)
    with pytest.raises(ValueError, match="GPU"):
        readout.embedding_count_within(emb, refs, 0.9)
    with pytest.raises(ValueError, match="GPU"):
        screening.neighbour_counts(emb, refs, 0.9)
    with pytest.raises(ValueError, match="GPU"):
        readout.embedding_count_within(emb, emb, 0.9)
    grad = emb.clone().requires_grad_()
    with torch.enable_grad():
        with pytest.raises((ValueError, RuntimeError)):            # (on the CPU the device is refused first)
            readout.embedding_count_within(grad, refs, 0.9)
    assert readout.embedding_count_within_supported(1, 1) and readout.embedding_count_within_supported(_lib.MAX_COSINE_MAX_REFS, 64)
    assert not readout.embedding_count_within_supported(_lib.MAX_COSINE_MAX_REFS + 1, 64)
    assert not readout.embedding_count_within_supported(5, 65) and not readout.embedding_count_within_supported(0, 5)


def test_fixtures_keep_their_distance_from_the_threshold():
    """Every (H, n, R) the GPU test compares with the float64 count, and every self-join: no element of the WHOLE float64
    similarity matrix lies within 4 error bounds of the threshold, so a float32 evaluation inside its bound decides every
    comparison as float64 does -- and no case needs leaving out.  The larger cases count something, and not everything."""
    rows, tile, parts = CC.tiling()
    assert CC.shapes()[-1] == (17, tile * parts + 1) and len(CC.shapes()) == 31
    for H in CC.WIDTHS:
        for n, R in CC.shapes():
            emb, refs, counts, margin = CC.float64_case(n, R, H)
            assert emb.shape == (n, H) and refs.shape == (R, H) and emb.dtype == refs.dtype == np.float32
            assert np.isfinite(emb).all() and np.isfinite(refs).all()
            assert margin > 4, (H, n, R, margin)
            assert counts.shape == (n,) and (counts >= 0).all() and (counts <= R).all()
            if H >= 2 and n >= rows - 1 and R >= tile - 1:
                assert counts.max() >= 2 and (counts == 0).any() and counts.max() < R, (H, n, R)
        for n in CC.self_sizes():
            emb, counts, margin = CC.float64_self_case(n, H)
            assert margin > 4, (H, n, margin)
            assert (counts >= 1).all() and (H < 2 or n < rows - 1 or (2 <= counts.max() < n and len(set(counts.tolist())) >= 4)), (H, n)
