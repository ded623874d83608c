"""Host side of library screening (molkgnn_amd.screening): the two additive exports, the numpy definition of the ranking's order
against a brute-force sort by the written key, and ``ResidentLoader(drop_last=False)``.  Every comparison is exact."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import _screen_cases as SC

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header() -> str:
    with open(os.path.join(REPO, "include", "molkgnn_hip.h")) as f:
        return f.read()


def test_topk_entry_points_are_additive_to_abi_8():
    from molkgnn_amd import _lib
    h = _header()
    m = re.search(r"#define\s+MKGNN_ABI_VERSION\s+(\d+)", h)
    assert m and int(m.group(1)) == 8 and _lib.ABI_VERSION == 8
    assert re.search(r"\bint mkgnn_topk_update\(const float\* scores, const int32_t\* ids, int32_t B, const int32_t\* n_valid,", h)
    assert re.search(r"\bsize_t mkgnn_topk_workspace_bytes\(int32_t B, int32_t K\);", h)
    m = re.search(r"#define\s+MKGNN_TOPK_MAX_K\s+(\d+)", h)
    assert m and int(m.group(1)) == _lib.TOPK_MAX_K >= 1024
    raw = ctypes.CDLL(_lib.LIB_PATH)
    raw.mkgnn_abi_version.restype = ctypes.c_int
    assert raw.mkgnn_abi_version() == 8
    for name in ("mkgnn_topk_update", "mkgnn_topk_workspace_bytes"):
        assert hasattr(raw, name), name
        assert name in _lib.EXPORTS, name
    lib = _lib.load()
    assert lib.mkgnn_topk_workspace_bytes.restype is ctypes.c_size_t
    assert lib.mkgnn_topk_update.restype is ctypes.c_int and len(lib.mkgnn_topk_update.argtypes) == 12
    prev = 0
    for B in (1, 63, 64, 1024, 1025, 4096, 100000, 2 ** 31 - 1):
        row = [lib.mkgnn_topk_workspace_bytes(B, K) for K in (1, 2, 64, 100, 1024)]
        assert all(v > 0 for v in row), (B, row)
        assert row == sorted(row), (B, row)                   # does not decrease as K grows ...
        assert row[0] >= prev, (B, row)                       # ... nor as B grows
        prev = row[0]
        assert lib.mkgnn_topk_workspace_bytes(B, 1024) >= lib.mkgnn_topk_workspace_bytes(max(B // 2, 1), 1024)
    # sizes the update rejects have no workspace
    assert lib.mkgnn_topk_workspace_bytes(0, 4) == 0 and lib.mkgnn_topk_workspace_bytes(4, _lib.TOPK_MAX_K + 1) == 0


@pytest.mark.parametrize("kind", SC.CASES)
@pytest.mark.parametrize("K,n", [(1, 1), (16, 500), (100, 500), (700, 500)])
def test_reference_matches_brute_force(kind, K, n):
    """(K = 700 is more than everything seen: empty slots stay at the end.)"""
    from molkgnn_amd.screening import empty_top, topk_update_reference
    top_r = top_b = empty_top(K)
    for u in range(3):
        scores, ids = SC.case_inputs(kind, n, seed=10 * K + u)
        n_valid = (n, n - 1, n + 5)[u]
        top_r = topk_update_reference(top_r, scores, ids, n_valid, u)
        top_b = SC.brute_force_update(top_b, scores, ids, n_valid, u)
        assert SC.same_list(top_r, top_b), (kind, K, u)
    occupied = min(K, n + (n - 1) + n)
    assert (top_r[1][:occupied] >= 0).all() and (top_r[1][occupied:] == -1).all() and (top_r[2][occupied:] == -1).all()
    assert (SC.bits(top_r[0][occupied:]) == SC.bits([-np.inf])[0]).all()


def test_reference_order_of_the_special_values():
    from molkgnn_amd.screening import empty_top, topk_update_reference
    scores = np.array([SC.NAN_A, -np.inf, SC.NEG_ZERO, 0.0, np.inf, SC.NAN_B, 2.0, 0.0], dtype=np.float32)
    ids = np.array([7, 6, 5, 4, 3, 2, 1, 0], dtype=np.int32)
    s, h, m = topk_update_reference(empty_top(10), scores, ids, 8, 3)
    # +inf, 2.0, the three zeros by id (their own bits kept), the real -inf, the NaNs by id (payloads kept), then empty slots
    assert m.tolist() == [3, 1, 0, 4, 5, 6, 2, 7, -1, -1] and h.tolist() == [3] * 8 + [-1, -1]
    want = np.array([np.inf, 2.0, 0.0, 0.0, SC.NEG_ZERO, -np.inf, SC.NAN_B, SC.NAN_A, -np.inf, -np.inf], dtype=np.float32)
    assert np.array_equal(SC.bits(s), SC.bits(want))
    # a list that is full of real entries takes a better one and drops its last
    s2, h2, m2 = topk_update_reference((s[:3], h[:3], m[:3]), np.array([1.0, 5.0], dtype=np.float32), np.array([9, 9], dtype=np.int32), 2, 0)
    assert s2.tolist() == [np.inf, 5.0, 2.0] and h2.tolist() == [3, 0, 3] and m2.tolist() == [3, 9, 1]
    # n_valid = 0 and a negative n_valid change nothing
    for nv in (0, -3):
        assert SC.same_list(topk_update_reference((s, h, m), scores, ids, nv, 0), (s, h, m))


@pytest.mark.parametrize("kind", SC.CASES)
def test_successive_updates_equal_one_update_with_the_concatenation(kind):
    from molkgnn_amd.screening import empty_top, topk_update_reference
    for K in (5, 64, 2000):
        parts = [SC.case_inputs(kind, n, seed=K + n) for n in (130, 1, 257)]
        top = empty_top(K)
        for scores, ids in parts:
            top = topk_update_reference(top, scores, ids, len(scores), 4)
        both = topk_update_reference(empty_top(K), np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]), 388, 4)
        assert SC.same_list(top, both), (kind, K)


@pytest.fixture(scope="module")
def cpu_shard(tmp_path_factory):
    from molkgnn_amd import shards as S
    from molkgnn_amd.synthetic import make_batch
    path = str(tmp_path_factory.mktemp("screen") / "lib.mkgs")
    S.write_shard(path, make_batch(70, seed=5, assay="all9", with_receptive_fields=False))
    return S.ResidentShard(path, "cpu")


def test_resident_loader_keeps_the_tail(cpu_shard):
    from molkgnn_amd import shards as S
    r = cpu_shard
    ids = np.arange(70)
    keep = S.ResidentLoader(r, 32, ids, drop_last=False)
    assert len(keep) == 3 and keep.n_live.tolist() == [32, 32, 6] and keep.n_live.dtype == np.int32
    plan = keep.plan()
    assert plan.shape == (3, 32)
    assert plan[:2].reshape(-1).tolist() == list(range(64))
    assert plan[2].tolist() == list(range(64, 70)) + [69] * 26           # the filler is the last real id
    # the plan covers the filled batch: its degree histogram fits the shape, its largest molecule is inside the bounds
    target = np.array([keep.shape[f"n{k}"] for k in range(1, 5)])
    for row in plan:
        assert (r.mol_deg[row].sum(axis=0) <= target).all()
    heavy = S.ResidentLoader(r, 32, ids[:64].tolist() + [int(np.argmax(r.mol_atoms))] * 6, drop_last=False)
    assert heavy.max_mol_atoms >= int(r.mol_atoms.max())
    assert (r.mol_deg[heavy.plan()[2]].sum(axis=0) <= np.array([heavy.shape[f"n{k}"] for k in range(1, 5)])).all()
    batches = list(keep)                                                 # (the CPU path gathers the filled batches)
    assert len(batches) == 3 and all(b.n_valid_molecules == 32 for b in batches)
    # the default is what it was: full batches only, the same ids
    drop = S.ResidentLoader(r, 32, ids)
    assert len(drop) == 2 and drop.n_live.tolist() == [32, 32]
    assert np.array_equal(drop.plan(), plan[:2])
    assert np.array_equal(S.ResidentLoader(r, 32, ids, drop_last=True).plan(), drop.plan())
    # a stream that divides evenly has no filler either way
    even = S.ResidentLoader(r, 35, ids, drop_last=False)
    assert len(even) == 2 and even.n_live.tolist() == [35, 35]
    # fewer molecules than one batch: one filled batch (the default has none and raises)
    one = S.ResidentLoader(r, 32, ids[:5], drop_last=False)
    assert len(one) == 1 and one.n_live.tolist() == [5] and one.plan()[0].tolist() == [0, 1, 2, 3, 4] + [4] * 27
    with pytest.raises(ValueError):
        S.ResidentLoader(r, 32, ids[:5])
    with pytest.raises(ValueError):
        S.ResidentLoader(r, 32, ids, world=2, drop_last=False)
    with pytest.raises(ValueError):
        S.ResidentLoader(r, 32, ids, rank=1, world=2, drop_last=False)


def test_screening_rejects_what_it_cannot_run(cpu_shard):
    """Before any launch: a model that is not on a GPU, more than one task, a list that is too long."""
    from molkgnn_amd import _lib, screening
    from molkgnn_amd.train import GNNModel, evaluate_resident
    torch.manual_seed(0)
    with pytest.raises(ValueError):
        screening.score_resident(GNNModel(num_layers=1), cpu_shard, 32)
    with pytest.raises(ValueError):
        screening.screen(GNNModel(num_layers=1, task_dim=2), [cpu_shard], 4, 32)
    with pytest.raises(ValueError):
        screening.screen(GNNModel(num_layers=1), [], 4, 32)
    with pytest.raises(ValueError):
        screening.TopK(_lib.TOPK_MAX_K + 1, "cuda:0")
    with pytest.raises(ValueError):
        screening.TopK(4, "cpu")
    with pytest.raises(ValueError):
        evaluate_resident(GNNModel(num_layers=1), cpu_shard, 32, metrics=("no such metric",))
