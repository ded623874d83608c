"""Host side of the kernel exemplars (``mkgnn_kernel_exemplars_update``, ``screening.KernelExemplars`` /
``kernel_exemplars_reference`` / ``kernel_exemplars``, ``GNNModel.kernel_scores``): the additive exports, the workspace size, what the
C call refuses before any launch, the numpy definition against a brute-force sort on hand-made cases, and the Python refusals."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import _exemplar_cases as EC

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = np.float32(np.nan), np.float32(np.inf)


def test_entry_points_are_additive_to_abi_8():
    from molkgnn_amd import _lib
    with open(os.path.join(REPO, "include", "molkgnn_hip.h")) as f:
        h = f.read()
    m = re.search(r"#define\s+MKGNN_ABI_VERSION\s+(\d+)", h)
    assert m and int(m.group(1)) == 8 and _lib.ABI_VERSION == 8
    assert re.search(r"\bsize_t mkgnn_kernel_exemplars_workspace_bytes\(const int64_t count\[MKGNN_MAX_DEGREE\], "
                     r"const int32_t num_kernels\[MKGNN_MAX_DEGREE\],\s+int32_t K, int32_t C\);", h)
    assert re.search(r"\bint mkgnn_kernel_exemplars_update\(const float\* sim, int64_t sim_stride, int64_t n_atoms,", h)
    for name, mirror, value in (("MKGNN_EXEMPLARS_MAX_K", _lib.EXEMPLARS_MAX_K, 64),
                                ("MKGNN_EXEMPLARS_MAX_COLUMNS", _lib.EXEMPLARS_MAX_COLUMNS, 256)):
        m = re.search(r"#define\s+%s\s+(\d+)\b" % name, h)
        assert m and int(m.group(1)) == mirror == value, name
    raw = ctypes.CDLL(_lib.LIB_PATH)
    raw.mkgnn_abi_version.restype = ctypes.c_int
    assert raw.mkgnn_abi_version() == 8
    lib = _lib.load()
    for name, n_args, restype in (("mkgnn_kernel_exemplars_update", 22, ctypes.c_int),
                                  ("mkgnn_kernel_exemplars_workspace_bytes", 4, ctypes.c_size_t)):
        assert hasattr(raw, name) and name in _lib.EXPORTS
        assert getattr(lib, name).restype is restype and len(getattr(lib, name).argtypes) == n_args, name
    # what was there is what it was
    assert lib.mkgnn_topk_update.restype is ctypes.c_int and len(lib.mkgnn_topk_update.argtypes) == 12
    assert lib.mkgnn_topk_update_tasks.restype is ctypes.c_int and len(lib.mkgnn_topk_update_tasks.argtypes) == 15
    # the source is part of the library's build, and the binding mirrors its tiling
    with open(os.path.join(REPO, "molkgnn_amd", "csrc", "Makefile")) as f:
        assert re.search(r"^SRCS :=.*\bkgnn_exemplars\.hip\b", f.read(), flags=re.M)
    with open(os.path.join(REPO, "molkgnn_amd", "csrc", "kgnn_exemplars.hip")) as f:
        text = f.read()
    for name, mirror in (("EX_TILE", _lib.EXEMPLARS_TILE), ("EX_CHUNK", _lib.EXEMPLARS_CHUNK)):
        m = re.search(r"constexpr int %s = (\d+);" % name, text)
        assert m and int(m.group(1)) == mirror, name
    from molkgnn_amd import screening
    assert (screening.EXEMPLARS_MAX_K, screening.EXEMPLARS_MAX_COLUMNS) == (_lib.EXEMPLARS_MAX_K, _lib.EXEMPLARS_MAX_COLUMNS)


def test_the_order_of_the_lists_and_the_span_check_have_one_text():
    """The list kernels promise each other's bits, so the order they share is compiled from ``kgnn_ranked.h`` alone: one rank
    function, one spelling of the empty slot's bits and one ``pow2_at_least`` under ``csrc/``, none of them in a ``.hip`` file; the
    host's overlap check of a call's spans likewise has one definition, outside the ``.hip`` files."""
    csrc = os.path.join(REPO, "molkgnn_amd", "csrc")
    texts = {}
    for name in sorted(os.listdir(csrc)):
        if name.endswith((".h", ".hip", ".cpp")):
            with open(os.path.join(csrc, name)) as f:
                texts[name] = f.read()
    hips = [name for name in texts if name.endswith(".hip")]
    assert {"kgnn_topk.hip", "kgnn_exemplars.hip", "kgnn_knn.hip"} <= set(hips)
    for pattern in (r"uint32_t score_rank\(", r"0xFF800000", r"int32_t pow2_at_least\("):
        count = {name: len(re.findall(pattern, text, flags=re.I)) for name, text in texts.items()}
        assert count.pop("kgnn_ranked.h") == 1 and not any(count.values()), (pattern, count)
    for name in ("kgnn_topk.hip", "kgnn_exemplars.hip", "kgnn_knn.hip"):
        assert '#include "kgnn_ranked.h"' in texts[name] and "score_rank(" in texts[name], name
        assert not re.search(r"\brank_key\b", texts[name]), name
    count = {name: len(re.findall(r"\bstruct Span\b", text)) for name, text in texts.items()}
    assert sum(count.values()) == 1 and not any(count[name] for name in hips), count
    assert sum(len(re.findall(r"^int spans_disjoint\(", text, flags=re.M)) for text in texts.values()) == 2    # declared, defined
    for name in ("kgnn_knn.hip", "kgnn_exemplars.hip", "kgnn_max_cosine.hip", "kgnn_diverse.hip"):
        assert "spans_disjoint(who, " in texts[name] and "auto overlap" not in texts[name], name
    with open(os.path.join(csrc, "Makefile")) as f:
        hdrs = re.search(r"^HDRS :=(.*)$", f.read(), flags=re.M).group(1).split()
    assert "kgnn_ranked.h" in hdrs and "kgnn_cosine.h" in hdrs


def _size(counts, Ls, K, C):
    from molkgnn_amd import _lib
    return _lib.load().mkgnn_kernel_exemplars_workspace_bytes(_lib.Int64x4(*counts), _lib.Int32x4(*Ls), K, C)


def test_workspace_size():
    """0 for every refused size, positive otherwise, and enough for a flag and a run of Kp entries per (tile, column)."""
    from molkgnn_amd import _lib
    T = _lib.EXEMPLARS_TILE
    for counts, Ls, K, C in (((1, 0, 0, 0), (1, 0, 0, 0), 1, 1), ((T + 1, T, 0, 5), (10, 20, 30, 50), 5, 110),
                             ((1000, 2000, 3000, 4000), (64, 64, 64, 64), 64, 256), ((0, 0, 0, 0), (10, 20, 30, 50), 8, 110),
                             ((5, 5, 5, 5), (0, 0, 0, 0), 8, 3), ((7, 0, 0, 0), (256, 0, 0, 0), 33, 256)):
        pairs = sum(-(-c // T) * L for c, L in zip(counts, Ls))
        Kp = 1 << (K - 1).bit_length()
        assert _size(counts, Ls, K, C) >= 4 * pairs + 20 * pairs * Kp and _size(counts, Ls, K, C) > 0, (counts, Ls, K, C)
    ok = ((5, 5, 5, 5), (1, 2, 3, 4))
    for K, C in ((0, 10), (65, 10), (-1, 10), (8, 0), (8, 257), (8, -3)):
        assert _size(*ok, K, C) == 0, (K, C)
    assert _size((5, -1, 5, 5), (1, 2, 3, 4), 8, 10) == 0
    assert _size((5, 5, 5, 5), (1, -2, 3, 4), 8, 10) == 0
    assert _size((5, 5, 5, 5), (1, 2, 3, 11), 8, 10) == 0                  # a block wider than C
    assert _size((5, 5, 5, (1 << 30) + 1), (1, 2, 3, 4), 8, 10) == 0
    lib = _lib.load()
    assert lib.mkgnn_kernel_exemplars_workspace_bytes(None, _lib.Int32x4(1, 2, 3, 4), 8, 10) == 0
    assert lib.mkgnn_kernel_exemplars_workspace_bytes(_lib.Int64x4(5, 5, 5, 5), None, 8, 10) == 0


# made-up addresses, far apart: every refusal comes before a launch, so nothing is ever read through them
_ADDRESS = {name: 0x10000000 * (i + 1) for i, name in enumerate(
    ("sim", "atom_mol", "mol_ptr", "mol_ids", "n_live", "n_valid_atoms", "shard_tag", "top_score", "top_shard", "top_mol", "top_atom",
     "workspace", "sel0", "sel1", "sel2", "sel3"))}


def _call(**change):
    """The C call on a valid set of arguments with ``change`` applied; returns ``(rc, message)``.  Never called unchanged."""
    from molkgnn_amd import _lib
    assert change, "a valid call would launch"
    lib = _lib.load()
    a = dict(_ADDRESS, sim_stride=12, n_atoms=40, counts=(10, 10, 10, 10), col_begin=(0, 1, 3, 6), L=(1, 2, 3, 4), B=6, K=8, C=10,
             workspace_bytes=None, buckets=True, begin_ptr=True, L_ptr=True)
    a.update(change)
    bk = _lib.Buckets4()
    for d in range(4):
        bk[d].count = a["counts"][d]
        bk[d].selected_index = a[f"sel{d}"]
    size = _size([max(c, 0) for c in a["counts"]], a["L"], a["K"], a["C"]) if a["workspace_bytes"] is None else a["workspace_bytes"]
    rc = lib.mkgnn_kernel_exemplars_update(
        a["sim"], a["sim_stride"], a["n_atoms"], bk if a["buckets"] else None, _lib.Int32x4(*a["col_begin"]) if a["begin_ptr"] else None,
        _lib.Int32x4(*a["L"]) if a["L_ptr"] else None, a["atom_mol"], a["mol_ptr"], a["mol_ids"], a["B"], a["n_live"], a["n_valid_atoms"],
        a["shard_tag"], a["K"], a["C"], a["top_score"], a["top_shard"], a["top_mol"], a["top_atom"], a["workspace"], size, None)
    return rc, lib.mkgnn_last_error().decode()


def test_the_c_call_refuses_before_any_launch():
    for K in (0, 65):
        rc, msg = _call(K=K)
        assert rc != 0 and "K = " in msg, msg
    for C in (0, 257):
        rc, msg = _call(C=C, sim_stride=300)
        assert rc != 0 and "C = " in msg, msg
    # column blocks: overlapping, past the end, in front of the beginning, wider than what is left
    for begin, L in (((0, 1, 2, 6), (1, 2, 3, 4)), ((0, 1, 3, 7), (1, 2, 3, 4)), ((-1, 1, 3, 6), (1, 2, 3, 4)), ((0, 1, 3, 6), (1, 2, 3, 5)),
                     ((0, 0, 3, 6), (1, 2, 3, 4)), ((0, 1, 3, 11), (1, 2, 3, 0)), ((0, 1, 3, 6), (1, -2, 3, 4))):
        rc, msg = _call(col_begin=begin, L=L)
        assert rc != 0 and "column blocks" in msg, (begin, L, msg)
    rc, msg = _call(sim_stride=9)
    assert rc != 0 and "sim_stride" in msg, msg
    rc, msg = _call(counts=(10, -1, 10, 10))
    assert rc != 0 and "negative count" in msg, msg
    rc, msg = _call(counts=(10, 41, 10, 10))
    assert rc != 0 and "slots of degree 2" in msg, msg
    rc, msg = _call(B=0)
    assert rc != 0 and "B = 0" in msg, msg
    rc, msg = _call(n_atoms=0)
    assert rc != 0 and "atoms" in msg, msg
    for name in ("sim", "atom_mol", "mol_ptr", "mol_ids", "n_live", "shard_tag", "top_score", "top_shard", "top_mol", "top_atom",
                 "workspace"):
        rc, msg = _call(**{name: None})
        assert rc != 0 and "null pointer" in msg, (name, msg)
    for name in ("buckets", "begin_ptr", "L_ptr"):
        rc, msg = _call(**{name: False})
        assert rc != 0 and "null pointer" in msg, (name, msg)
    rc, msg = _call(sel2=None)
    assert rc != 0 and "null selected_index of degree 3" in msg, msg
    # an output aliasing an input, or another output (the spans are what the call reads and writes: 10 x 8 entries per list)
    for out, other in (("top_score", "sim"), ("top_atom", "atom_mol"), ("top_mol", "mol_ids"), ("top_shard", "shard_tag"),
                       ("workspace", "sel1"), ("top_score", "n_valid_atoms"), ("top_mol", "n_live"), ("top_atom", "mol_ptr")):
        rc, msg = _call(**{out: _ADDRESS[other]})
        assert rc != 0 and "aliases an input" in msg, (out, other, msg)
    rc, msg = _call(top_mol=_ADDRESS["sim"] + 4 * (39 * 12 + 9))          # the last float sim holds
    assert rc != 0 and "aliases an input" in msg, msg
    for out, other, slot in (("top_score", "top_shard", 79), ("top_mol", "top_atom", 79), ("workspace", "top_score", 76)):
        rc, msg = _call(**{out: _ADDRESS[other] + 4 * slot})               # the last slot of the other (the workspace: aligned)
        assert rc != 0 and "alias each other" in msg, (out, other, msg)
    need = _size((10, 10, 10, 10), (1, 2, 3, 4), 8, 10)
    rc, msg = _call(workspace_bytes=need - 1)
    assert rc != 0 and "workspace" in msg, msg
    rc, msg = _call(workspace=_ADDRESS["workspace"] + 4)
    assert rc != 0 and "16-byte aligned" in msg, msg


def _lists(rows, K=None):
    """``rows``: per column a list of ``(score, shard, mol, atom)``; the rest of each list of ``K`` is empty slots."""
    from molkgnn_amd.screening import empty_exemplars
    K = max(max(len(r) for r in rows), 1) if K is None else K
    out = empty_exemplars(len(rows), K)
    for c, r in enumerate(rows):
        for t, e in enumerate(r):
            for a, v in zip(out, e):
                a[c, t] = v
    return out


def _one_degree_case(scores, atom_mol, mol_ptr, ids, n_live, n_valid_atoms=None, extra_columns=0):
    """Every atom in the bucket of degree 1, one column per entry of ``scores[n]``; ``extra_columns`` columns of degree 2 without
    atoms follow."""
    sim = np.asarray(scores, dtype=np.float32)
    N, L = sim.shape
    sim = np.concatenate([sim, np.full((N, extra_columns), 99.0, dtype=np.float32)], axis=1)
    return {"sim": sim, "buckets": [np.arange(N, dtype=np.int64)] + [np.zeros(0, dtype=np.int64)] * 3, "col_begin": [0, L, L + extra_columns, L + extra_columns],
            "L": [L, extra_columns, 0, 0], "atom_mol": np.asarray(atom_mol, dtype=np.int32), "mol_ptr": np.asarray(mol_ptr, dtype=np.int32),
            "ids": np.asarray(ids, dtype=np.int32), "n_live": n_live, "n_valid_atoms": n_valid_atoms, "C": L + extra_columns, "B": len(ids)}


def _rows(lists, c):
    return [(float(lists[0][c, t]), int(lists[1][c, t]), int(lists[2][c, t]), int(lists[3][c, t])) for t in range(lists[0].shape[1])]


def _check(lists, case, tag):
    got, want = EC.reference(lists, case, tag), EC.brute_force(lists, case, tag)
    assert EC.same_lists(got, want)
    return got


def test_reference_on_hand_made_cases():
    E = (-np.inf, -1, -1, -1)
    # ties in score broken by shard, then molecule, then atom: two molecules of two atoms each, ids 7 and 3, all scores 1.0
    case = _one_degree_case([[1.0]] * 4, [0, 0, 1, 1], [0, 2, 4], [7, 3], 2)
    out = _check(_lists([[(1.0, 0, 9, 0), (1.0, 2, 1, 0)]], K=6), case, 1)
    assert _rows(out, 0) == [(1.0, 0, 9, 0), (1.0, 1, 3, 0), (1.0, 1, 3, 1), (1.0, 1, 7, 0), (1.0, 1, 7, 1), (1.0, 2, 1, 0)]
    # -0.0 and +0.0 tie (the molecule decides) and keep their signs; NaNs come behind every number, alike whatever the payload
    case = _one_degree_case([[-0.0], [0.0], [NAN], [-1.0], [EC.NAN_PAYLOAD]], [0, 1, 2, 3, 4], [0, 1, 2, 3, 4, 5], [5, 4, 3, 2, 1], 5)
    out = _check(_lists([[E] * 6]), case, 0)
    assert [r[2] for r in _rows(out, 0)] == [4, 5, 2, 1, 3, -1]
    assert EC.bits(out[0][0, :2]).tolist() == EC.bits(np.array([0.0, -0.0], dtype=np.float32)).tolist()
    assert EC.bits(out[0][0, 3:5]).tolist() == EC.bits(case["sim"][[4, 2], 0]).tolist()
    assert EC.bits(case["sim"][4, 0]).item() != EC.bits(case["sim"][2, 0]).item()
    # a real -inf score ranks before the empty slots and before a NaN: a NaN is behind every number
    case = _one_degree_case([[-np.inf], [NAN]], [0, 0], [0, 2], [8], 1)
    out = _check(_lists([[E] * 4]), case, 3)
    assert _rows(out, 0)[0] == (float("-inf"), 3, 8, 0) and np.isnan(out[0][0, 1]) and _rows(out, 0)[2:] == [E, E]
    # fewer candidates than K: the rest stays empty; a column of a degree without atoms keeps its list
    case = _one_degree_case([[2.0, 5.0]], [0], [0, 1], [6], 1, extra_columns=1)
    old = _lists([[E] * 3, [E] * 3, [(4.0, 0, 1, 1), E, E]])
    out = _check(old, case, 0)
    assert _rows(out, 0) == [(2.0, 0, 6, 0), E, E] and _rows(out, 1) == [(5.0, 0, 6, 0), E, E] and _rows(out, 2) == [(4.0, 0, 1, 1), E, E]
    # a candidate equal in score to the last entry: a lower (shard, molecule, atom) displaces it, a higher one does not, and one
    # alike in all of it arrives later and stays out
    full = [(3.0, 1, 5, 2), (2.0, 1, 5, 2)]
    for mol_id, tag, atoms_before, enters in ((4, 1, 2, True), (6, 1, 2, False), (5, 1, 1, True), (5, 1, 3, False), (5, 1, 2, False),
                                              (9, 0, 2, True), (0, 2, 2, False)):
        case = _one_degree_case([[0.0]] * atoms_before + [[2.0]], [0] * (atoms_before + 1), [0, atoms_before + 1], [mol_id], 1)
        out = _check(_lists([full]), case, tag)
        assert _rows(out, 0) == [full[0], (2.0, tag, mol_id, atoms_before) if enters else full[1]], (mol_id, tag, atoms_before)
    # atoms at or past n_valid_atoms and molecules at or past n_live carry the largest scores and never enter; n_live is clamped
    scores = [[1.0], [2.0], [50.0], [60.0], [70.0]]
    case = _one_degree_case(scores, [0, 0, 1, 1, 2], [0, 2, 4, 5], [10, 11, 12], 2, n_valid_atoms=3)
    out = _check(_lists([[E] * 4]), case, 0)
    assert _rows(out, 0) == [(50.0, 0, 11, 0), (2.0, 0, 10, 1), (1.0, 0, 10, 0), E]
    for n_live, n in ((1, 2), (0, 0), (-5, 0), (3, 3), (99, 3)):
        case = _one_degree_case(scores, [0, 0, 1, 1, 2], [0, 2, 4, 5], [10, 11, 12], n_live, n_valid_atoms=3)
        out = _check(_lists([[E] * 4]), case, 0)
        assert sum(r != E for r in _rows(out, 0)) == n, n_live


@pytest.mark.parametrize("kind", ["normal", "quantised", "special"])
def test_reference_against_brute_force_on_random_batches(kind):
    """Three updates of a running list on the reference's layout and on one with an empty degree and an empty block."""
    from molkgnn_amd.screening import empty_exemplars
    for counts, Ls, K in (((9, 14, 11, 6), (2, 3, 1, 2), 5), ((12, 0, 7, 5), (3, 2, 0, 1), 3)):
        lists = empty_exemplars(sum(Ls), K)
        for u, tag in enumerate((2, 0, 2)):
            case = EC.make_case(counts, Ls, 6, seed=10 * u + len(kind), kind=kind, outside=np.nan, poison=u == 1, id_range=4,
                                n_valid_atoms=None if u == 2 else "inside")
            got = EC.reference(lists, case, tag)
            assert EC.same_lists(got, EC.brute_force(lists, case, tag)), (kind, counts, u)
            assert kind == "special" or not np.isposinf(got[0]).any()      # (only atoms that are no candidates score +inf)
            lists = got


@pytest.fixture(scope="module")
def cpu_shard(tmp_path_factory):
    from molkgnn_amd import shards as S
    from molkgnn_amd.synthetic import make_batch
    path = str(tmp_path_factory.mktemp("exemplars") / "lib.mkgs")
    S.write_shard(path, make_batch(40, seed=6, assay="all9", with_receptive_fields=False))
    return S.ResidentShard(path, "cpu")


def test_python_refusals_before_any_launch(cpu_shard, monkeypatch):
    from molkgnn_amd import _lib, screening
    from molkgnn_amd.train import GNNModel

    def no_load():
        raise AssertionError("the library was loaded before the refusal")

    monkeypatch.setattr(_lib, "load", no_load)
    torch.manual_seed(0)
    model = GNNModel(num_layers=3, task_dim=9)
    with pytest.raises(ValueError, match="evaluation mode"):
        model.kernel_scores(None, 0)
    with pytest.raises(ValueError, match="evaluation mode"):
        model.gnn_model.kernel_scores(None, 0)
    model.eval()
    for layer in (-1, 3):
        with pytest.raises(ValueError, match="layer"):
            model.kernel_scores(None, layer)
        with pytest.raises(ValueError, match="layer"):
            screening.kernel_exemplars(model, [cpu_shard], layer, 8, 32)
    for k in (0, 65):
        with pytest.raises(ValueError, match="k = "):
            screening.kernel_exemplars(model, [cpu_shard], 0, k, 32)
    wide = GNNModel(num_layers=2, kernels_1hop=(65, 65, 65, 65)).eval()
    with pytest.raises(ValueError, match="260 kernels"):
        screening.kernel_exemplars(wide, [cpu_shard], 0, 8, 32)
    with pytest.raises(ValueError, match="batch_size"):
        screening.kernel_exemplars(model, [cpu_shard], 0, 8, 0)
    with pytest.raises(ValueError, match="GPU"):
        screening.kernel_exemplars(model, [cpu_shard], 0, 8, 32)          # neither the model nor the shard is on the GPU
    with pytest.raises(ValueError, match="at least one shard"):
        screening.kernel_exemplars(model, [], 0, 8, 32)
    with pytest.raises(ValueError, match="at least one shard"):
        screening.kernel_exemplars(model, (r for r in ()), 2, 64, 32)
    assert model.training is False
    for n_columns, k in ((0, 8), (257, 8), (10, 0), (10, 65)):
        with pytest.raises(ValueError):
            screening.KernelExemplars(n_columns, k, "cuda:0")
    with pytest.raises(ValueError, match="GPU"):
        screening.KernelExemplars(10, 8, "cpu")
    # the column layout needs no device
    degree, kernel = model.gnn_model.kernel_column_layout(1)
    assert degree.dtype == kernel.dtype == torch.int32
    assert degree.tolist() == [1] * 10 + [2] * 20 + [3] * 30 + [4] * 50
    assert kernel.tolist() == list(range(10)) + list(range(20)) + list(range(30)) + list(range(50))
