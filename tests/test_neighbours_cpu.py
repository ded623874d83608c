"""The neighbour lists without a GPU: ``neighbours_reference`` against a brute-force loop, its strictness, NaN rule and order; that
the header, the binding and the library agree on the two new operators (declared, exported, typed, the ABI version still 8, the
workspace formulas); and what every Python entry point refuses before a launch."""
import os
import re

import numpy as np
import pytest
import torch

from tests import _components_cases as CC

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _brute(sim, t):
    ptr, nbr, val = [0], [], []
    for i in range(sim.shape[0]):
        for r in range(sim.shape[1]):
            if sim[i, r] > sim.dtype.type(t):
                nbr.append(r)
                val.append(sim[i, r])
        ptr.append(len(nbr))
    return np.array(ptr, dtype=np.int64), np.array(nbr, dtype=np.int32), np.array(val, dtype=sim.dtype)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_reference_is_the_brute_force_loop(dtype):
    from molkgnn_amd.screening import count_within_reference, neighbours_reference
    rng = np.random.default_rng(3)
    sim = rng.uniform(-1, 1, size=(23, 41)).astype(dtype)
    sim[9] = -1.0                                                  # an empty list in the middle
    sim[4] = np.nan                                                # a NaN row has no neighbours
    sim[:, 7] = np.nan                                             # a NaN reference is nobody's neighbour
    for t in (0.3, -0.2, -1.5, 1.5, float(sim[2, 5])):
        ptr, nbr, val = neighbours_reference(sim, t)
        want = _brute(sim, t)
        assert ptr.dtype == np.int64 and nbr.dtype == np.int32 and val.dtype == dtype
        assert np.array_equal(ptr, want[0]) and np.array_equal(nbr, want[1]) and np.array_equal(val, want[2])
        assert np.array_equal(np.diff(ptr), count_within_reference(sim, t))
        assert ptr[5] == ptr[4] and 7 not in nbr.tolist()
        for i in range(sim.shape[0]):
            assert (np.diff(nbr[ptr[i]:ptr[i + 1]]) > 0).all()     # ascending references inside every row
    ptr, nbr, val = neighbours_reference(sim, 1.5)
    assert ptr.tolist() == [0] * 24 and nbr.shape == val.shape == (0,)
    ptr, _, _ = neighbours_reference(sim, -1.5)
    assert ptr[-1] == (~np.isnan(sim)).sum()
    assert np.array_equal(neighbours_reference(torch.from_numpy(sim), 0.3)[1], neighbours_reference(sim, 0.3)[1])


def test_reference_is_strict_at_a_value_and_compares_in_the_matrix_dtype():
    from molkgnn_amd.screening import neighbours_reference
    sim = np.array([[0.5, 0.9, np.float32(0.9), 0.95]], dtype=np.float32)
    at = float(sim[0, 1])
    assert neighbours_reference(sim, at)[1].tolist() == [3]
    assert neighbours_reference(sim, float(np.nextafter(np.float32(at), np.float32(-2))))[1].tolist() == [1, 2, 3]
    assert neighbours_reference(sim, 0.9)[1].tolist() == [3]       # 0.9 is rounded to float32 first: equal, so not above
    just_below = 0.89999997                                        # float32(0.9) = 0.899999976...: this rounds to it in float32
    assert np.float32(just_below) == sim[0, 1] and float(sim[0, 1]) > just_below
    assert neighbours_reference(sim, just_below)[1].tolist() == [3]
    assert neighbours_reference(sim.astype(np.float64), just_below)[1].tolist() == [1, 2, 3]
    for bad in (float("nan"), float("inf"), float("-inf")):
        with pytest.raises(ValueError):
            neighbours_reference(sim, bad)
    for bad in (sim[0], sim.astype(np.float16), sim.astype(np.int32)):
        with pytest.raises(ValueError):
            neighbours_reference(bad, 0.5)


def _header():
    return open(os.path.join(REPO, "include", "molkgnn_hip.h")).read()


def test_header_binding_and_library_agree():
    import ctypes as C
    from molkgnn_amd import _lib
    text = _header()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = ("mkgnn_embed_neighbours_within", "mkgnn_embed_neighbours_within_workspace_bytes", "mkgnn_graph_components",
             "mkgnn_graph_components_workspace_bytes")
    lib = _lib.load()
    for name in names:
        assert re.search(r"\b" + name + r"\s*\(", code), name
        assert name in _lib.EXPORTS and hasattr(lib, name)
    assert re.search(r"#define\s+MKGNN_ABI_VERSION\s+8\b", text) and _lib.ABI_VERSION == 8 and lib.mkgnn_abi_version() == 8
    P, I64, I32 = C.c_void_p, C.c_int64, C.c_int32
    assert lib.mkgnn_embed_neighbours_within.argtypes == [P, I64, I64, I32, P, I64, I32, C.c_float, P, I64, P, P, P, P, C.c_size_t, P]
    assert lib.mkgnn_graph_components.argtypes == [P, P, I32, P, P, I32, P, C.c_size_t, P]
    assert lib.mkgnn_embed_neighbours_within_workspace_bytes.restype == lib.mkgnn_graph_components_workspace_bytes.restype == C.c_size_t
    # the parameter lists of the header, token by token
    fill = re.search(r"int\s+mkgnn_embed_neighbours_within\s*\((.*?)\);", code, flags=re.S).group(1)
    assert [p.split()[-1].lstrip("*") for p in fill.split(",")] == [
        "emb", "emb_stride", "n_rows", "H", "refs", "ref_stride", "R", "min_sim", "row_ptr", "capacity", "nbr_ref", "nbr_sim", "found",
        "workspace", "workspace_bytes", "stream"]
    comp = re.search(r"int\s+mkgnn_graph_components\s*\((.*?)\);", code, flags=re.S).group(1)
    assert [p.split()[-1].lstrip("*") for p in comp.split(",")] == ["row_ptr", "col", "n", "labels", "state", "resume", "workspace",
                                                                     "workspace_bytes", "stream"]
    assert int(re.search(r"#define\s+MKGNN_COMPONENTS_MAX_VERTICES\s+(\d+)", text).group(1)) == _lib.COMPONENTS_MAX_VERTICES


def test_workspace_formulas():
    """The header's statement: the norms block of the count, plus ``parts * n_rows`` int32 when the references are split -- and the
    count's own formula is what it was."""
    from molkgnn_amd import _lib
    lib = _lib.load()
    text = " ".join(_header().split())
    assert "[inverse norms: R + n_rows floats, padded to a multiple of 4][parts x n_rows int32, when parts > 1]" in text.replace("* ", "")
    rows, tile, parts = CC.tiling()
    split_seen = set()
    for n, R in CC.shapes() + ((4096, 16384), (256, 1024), (1, 1), (70000, 3)):
        per_part, n_parts = _lib.count_within_split(n, R)
        want = 4 * ((R + n + 3) // 4 * 4 + (n_parts * n if n_parts > 1 else 0))
        assert lib.mkgnn_embed_neighbours_within_workspace_bytes(n, R) == want, (n, R)
        assert lib.mkgnn_embed_count_within_workspace_bytes(n, R) == want, (n, R)
        split_seen.add(n_parts > 1)
    assert split_seen == {True, False}
    assert lib.mkgnn_embed_count_within_workspace_bytes(rows + 1, 3 * tile) == 4 * ((3 * tile + rows + 1 + 3) // 4 * 4 + 3 * (rows + 1))
    for n, R in ((0, 5), (-1, 5), (5, 0), (5, _lib.MAX_COSINE_MAX_REFS + 1), (1 << 31, 5)):
        assert lib.mkgnn_embed_neighbours_within_workspace_bytes(n, R) == 0
    for n in (0, 1, 17, 4097):
        assert lib.mkgnn_graph_components_workspace_bytes(n) == 4 * (2 * n + 72)
    assert lib.mkgnn_graph_components_workspace_bytes(-1) == lib.mkgnn_graph_components_workspace_bytes(_lib.COMPONENTS_MAX_VERTICES + 1) == 0
    assert "4 (2 n + 72)" in text.replace("* ", "")
    for n in (1, 2, 3, 4, 5, 17, 257, 1025, 4096, 4097):
        assert _lib.components_rounds(n) == CC.round_bound(n) + 1


def test_supported_shapes():
    from molkgnn_amd import _lib, readout
    assert readout.embedding_neighbours_within_supported(1, 1) and readout.embedding_neighbours_within_supported(_lib.MAX_COSINE_MAX_REFS, 64)
    assert not readout.embedding_neighbours_within_supported(5, 65)
    assert not readout.embedding_neighbours_within_supported(_lib.MAX_COSINE_MAX_REFS + 1, 32)
    assert not readout.embedding_neighbours_within_supported(0, 32)


def test_python_entry_points_refuse_before_a_launch():
    from molkgnn_amd import readout, screening
    e, r = torch.zeros(6, 8), torch.zeros(4, 8)
    lists = (readout.embedding_neighbours_within, screening.neighbour_lists)
    for fn in lists:
        for bad_e, bad_r in ((e[0], r), (e, r[0]), (e.double(), r), (e, r.half()), (e, torch.zeros(4, 9)), (e, torch.zeros(0, 8)),
                             (e.numpy(), r), (torch.zeros(6, 0), torch.zeros(4, 0))):
            with pytest.raises(ValueError):
                fn(bad_e, bad_r, 0.5)
        for bad in (float("nan"), float("inf"), float("-inf")):
            with pytest.raises(ValueError, match="finite"):
                fn(e, r, bad)
        with pytest.raises(ValueError, match="max_pairs"):
            fn(e, r, 0.5, max_pairs=-1)
        with pytest.raises(ValueError, match="GPU"):               # there is no CPU path
            fn(e, r, 0.5)
    with pytest.raises(ValueError, match="max_pairs"):
        screening.neighbour_lists(e, r, 0.5, max_pairs=1.5)
    with torch.enable_grad():
        with pytest.raises(RuntimeError, match="forward only"):
            readout.embedding_neighbours_within(e.clone().requires_grad_(), r, 0.5)
        with pytest.raises(RuntimeError, match="forward only"):
            readout.embedding_neighbours_within(e, r.clone().requires_grad_(), 0.5)
    with pytest.raises(ValueError):
        readout.embedding_neighbours_within(e, r, 0.5, n_rows=7)
    with pytest.raises(ValueError, match="raw form"):
        readout.embedding_neighbours_within(e, r, 0.5, found=torch.zeros(6, dtype=torch.int32))
    cluster = screening.cluster_components_embeddings
    for bad in (e[0], e.double(), torch.zeros(0, 8), torch.zeros(6, 0), e.numpy()):
        with pytest.raises(ValueError):
            cluster(bad, 0.5)
    for kw in (dict(scores=torch.zeros(5)), dict(scores=torch.zeros(6).double()), dict(ids=torch.zeros(6)), dict(ids=torch.zeros(5).long()),
               dict(max_pairs=-3)):
        with pytest.raises(ValueError):
            cluster(e, 0.5, **kw)
    with pytest.raises(ValueError, match="finite"):
        cluster(e, float("nan"))
    with pytest.raises(ValueError, match="GPU"):
        cluster(e, 0.5)
    ptr, col = torch.zeros(4, dtype=torch.int64), torch.zeros(0, dtype=torch.int32)
    for bad_ptr, bad_col, n in ((ptr.int(), col, 3), (ptr, col.long(), 3), (ptr, col, 4), (ptr, col, -1), (ptr[::2], col, 1),
                                (ptr, col.reshape(0, 1), 3), (ptr.numpy(), col, 3)):
        with pytest.raises(ValueError):
            readout.graph_components(bad_ptr, bad_col, n)
    with pytest.raises(ValueError, match="GPU"):
        readout.graph_components(ptr, col, 3)
