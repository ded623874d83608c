"""Host side of per-task library screening (``screening.*_tasks``, ``mkgnn_task_scores``, ``mkgnn_topk_update_tasks``): the three
additive exports, the workspace size, the numpy definition list by list against a brute-force sort, and everything that is
refused before a launch.  Every comparison is exact."""
import ctypes
import os
import re

import pytest
import torch

from tests import _screen_cases as SC

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("mkgnn_task_scores", "mkgnn_topk_tasks_workspace_bytes", "mkgnn_topk_update_tasks")


def test_entry_points_are_additive_to_abi_8():
    from molkgnn_amd import _lib
    with open(os.path.join(REPO, "include", "molkgnn_hip.h")) as f:
        h = f.read()
    m = re.search(r"#define\s+MKGNN_ABI_VERSION\s+(\d+)", h)
    assert m and int(m.group(1)) == 8 and _lib.ABI_VERSION == 8
    assert re.search(r"\bint mkgnn_task_scores\(const float\* emb, int64_t emb_stride, int64_t n_rows, int32_t H, int32_t T,", h)
    assert re.search(r"\bsize_t mkgnn_topk_tasks_workspace_bytes\(int32_t B, int32_t K, int32_t T\);", h)
    assert re.search(r"\bint mkgnn_topk_update_tasks\(const float\* scores, int64_t score_row_stride, int64_t score_task_stride,", h)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    raw.mkgnn_abi_version.restype = ctypes.c_int
    assert raw.mkgnn_abi_version() == 8
    for name in ENTRIES:
        assert hasattr(raw, name), name
        assert name in _lib.EXPORTS, name
    lib = _lib.load()
    assert lib.mkgnn_task_scores.restype is ctypes.c_int and len(lib.mkgnn_task_scores.argtypes) == 11
    assert lib.mkgnn_topk_tasks_workspace_bytes.restype is ctypes.c_size_t and len(lib.mkgnn_topk_tasks_workspace_bytes.argtypes) == 3
    assert lib.mkgnn_topk_update_tasks.restype is ctypes.c_int and len(lib.mkgnn_topk_update_tasks.argtypes) == 15
    assert _lib.TASK_HEAD_MAX_TASKS == 32
    # the single-list entry points are what they were
    assert lib.mkgnn_topk_update.restype is ctypes.c_int and len(lib.mkgnn_topk_update.argtypes) == 12


def test_workspace_bytes_of_the_task_lists():
    from molkgnn_amd import _lib
    lib = _lib.load()
    size = lib.mkgnn_topk_tasks_workspace_bytes
    Bs, Ks, Ts = (1, 63, 1024, 1025, 4096, 100000, 2 ** 31 - 1), (1, 2, 100, 1024), (1, 2, 9, 32)
    for B in Bs:
        for K in Ks:
            row = [size(B, K, T) for T in Ts]
            assert all(v > 0 for v in row) and row == sorted(row), (B, K, row)                     # monotone in T
            assert row[0] >= lib.mkgnn_topk_workspace_bytes(B, K) > 0, (B, K)                      # T = 1 covers the single list
        for T in Ts:
            row = [size(B, K, T) for K in Ks]
            assert row == sorted(row), (B, T, row)                                                 # monotone in K
    for K in Ks:
        for T in Ts:
            row = [size(B, K, T) for B in Bs]
            assert row == sorted(row), (K, T, row)                                                 # monotone in B
    # the runs of every task have room beside each other: T times the single list's runs
    one, nine = size(4096, 1024, 1), size(4096, 1024, 9)
    assert nine - 256 == 9 * (one - 256) and one - 256 == 4 * 1024 * 16
    # sizes the update rejects have no workspace
    for B, K, T in ((4, 4, 0), (4, 4, 33), (4, 1025, 2), (0, 4, 2), (4, 0, 2), (-1, 4, 2), (4, 4, -1)):
        assert size(B, K, T) == 0, (B, K, T)


@pytest.mark.parametrize("kind", SC.CASES)
@pytest.mark.parametrize("K,n", [(1, 1), (16, 500), (700, 500)])
def test_tasks_reference_is_the_single_reference_list_by_list(kind, K, n):
    """T = 3, a different seed per task (the ids are the batch's: one vector), against the brute-force sort."""
    import numpy as np
    from molkgnn_amd.screening import empty_top, topk_update_tasks_reference
    T = 3
    top = tuple(np.stack([a] * T) for a in empty_top(K))
    brute = [empty_top(K) for _ in range(T)]
    for u in range(3):
        per_task = [SC.case_inputs(kind, n, seed=10 * K + u + 100 * t) for t in range(T)]
        ids = per_task[0][1]
        scores = np.stack([p[0] for p in per_task])
        n_valid = (n, n - 1, n + 5)[u]
        top = topk_update_tasks_reference(top, scores, ids, n_valid, u)
        assert all(a.shape == (T, K) for a in top) and top[0].dtype == np.float32 and top[1].dtype == top[2].dtype == np.int32
        for t in range(T):
            brute[t] = SC.brute_force_update(brute[t], scores[t], ids, n_valid, u)
            assert SC.same_list(tuple(a[t] for a in top), brute[t]), (kind, K, u, t)


@pytest.mark.parametrize("kind", SC.CASES)
def test_two_successive_updates_equal_one_update_with_the_concatenation(kind):
    import numpy as np
    from molkgnn_amd.screening import empty_top, topk_update_tasks_reference
    T = 3
    for K in (5, 64, 700):
        parts = []
        for n in (130, 257):
            per_task = [SC.case_inputs(kind, n, seed=K + n + 31 * t) for t in range(T)]
            parts.append((np.stack([p[0] for p in per_task]), per_task[0][1]))
        empty = tuple(np.stack([a] * T) for a in empty_top(K))
        top = empty
        for scores, ids in parts:
            top = topk_update_tasks_reference(top, scores, ids, scores.shape[1], 4)
        both = topk_update_tasks_reference(empty, np.concatenate([p[0] for p in parts], axis=1), np.concatenate([p[1] for p in parts]), 387, 4)
        for t in range(T):
            assert SC.same_list(tuple(a[t] for a in top), tuple(a[t] for a in both)), (kind, K, t)


@pytest.fixture(scope="module")
def cpu_shard(tmp_path_factory):
    from molkgnn_amd import shards as S
    from molkgnn_amd.synthetic import make_batch
    path = str(tmp_path_factory.mktemp("screen_tasks") / "lib.mkgs")
    S.write_shard(path, make_batch(70, seed=5, assay="all9", with_receptive_fields=False))
    return path


def test_rejections_before_any_launch(cpu_shard):
    """A model that is not on a GPU, more outputs than the kernels take, lists off the GPU or outside their limits, no shard, an
    unknown metric, a shard that does not know its molecules' tasks."""
    from molkgnn_amd import _lib, screening
    from molkgnn_amd import shards as S
    from molkgnn_amd.synthetic import NINE_ASSAYS
    from molkgnn_amd.train import GNNModel, evaluate_resident_tasks
    torch.manual_seed(0)
    plain = S.ResidentShard(cpu_shard, "cpu")
    nine = S.ResidentShard(cpu_shard, "cpu", assays=[int(a) for a in NINE_ASSAYS])
    with pytest.raises(ValueError):
        screening.score_resident_tasks(GNNModel(num_layers=1, task_dim=9), plain, 32)              # a CPU model
    with pytest.raises(ValueError):
        screening.screen_tasks(GNNModel(num_layers=1, task_dim=9), [plain], 4, 32)
    with pytest.raises(ValueError, match="outputs"):
        screening.score_resident_tasks(GNNModel(num_layers=1, task_dim=33), plain, 32)
    with pytest.raises(ValueError, match="outputs"):
        screening.screen_tasks(GNNModel(num_layers=1, task_dim=33), [plain], 4, 32)
    with pytest.raises(ValueError):
        screening.TopKTasks(4, 9, "cpu")
    with pytest.raises(ValueError):
        screening.TopKTasks(_lib.TOPK_MAX_K + 1, 9, "cuda:0")
    with pytest.raises(ValueError):
        screening.TopKTasks(4, 0, "cuda:0")
    with pytest.raises(ValueError):
        screening.TopKTasks(4, 33, "cuda:0")
    with pytest.raises(ValueError):
        screening.screen_tasks(GNNModel(num_layers=1, task_dim=9), [], 4, 32)                      # an empty shard sequence
    with pytest.raises(ValueError, match="metric"):
        evaluate_resident_tasks(GNNModel(num_layers=1, task_dim=9), nine, 32, metrics=("no such metric",))
    with pytest.raises(ValueError, match="assays"):
        evaluate_resident_tasks(GNNModel(num_layers=1, task_dim=9), plain, 32)
    with pytest.raises(ValueError):
        evaluate_resident_tasks(GNNModel(num_layers=1, task_dim=9), nine, 32)                      # (with assays: the CPU model)
    # the single-score entry points refuse a multi-task model as before
    with pytest.raises(ValueError):
        screening.score_resident(GNNModel(num_layers=1, task_dim=9), plain, 32)
