"""Host side of the per-atom contributions (``mkgnn_atom_contributions``, ``readout.atom_contributions*``,
``GNNModel.atom_contributions``, ``screening.explain_resident``): the additive export, the float64 definition against the modules
and its completeness, a sequential float32 emulation of the kernel's stated evaluation order against the error criterion, and
everything that is refused before a launch."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LS = (10, 20, 30, 50)


def test_entry_point_is_additive_to_abi_8():
    from molkgnn_amd import _lib
    with open(os.path.join(REPO, "include", "molkgnn_hip.h")) as f:
        h = f.read()
    m = re.search(r"#define\s+MKGNN_ABI_VERSION\s+(\d+)", h)
    assert m and int(m.group(1)) == 8 and _lib.ABI_VERSION == 8
    assert re.search(r"\bint mkgnn_atom_contributions\(const mkgnn_atom_contrib_args\* args, void\* workspace, size_t workspace_bytes,", h)
    assert re.search(r"\bsize_t mkgnn_atom_contributions_workspace_bytes\(int32_t K, int32_t H, int32_t G, int64_t n_atoms\);", h)
    assert re.search(r"#define\s+MKGNN_ATOM_CONTRIB_MAX_TASKS\s+32\b", h)
    assert re.search(r"\}\s*mkgnn_atom_contrib_args;", h)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    raw.mkgnn_abi_version.restype = ctypes.c_int
    assert raw.mkgnn_abi_version() == 8
    for name in ("mkgnn_atom_contributions", "mkgnn_atom_contributions_workspace_bytes"):
        assert hasattr(raw, name) and name in _lib.EXPORTS, name
    lib = _lib.load()
    assert lib.mkgnn_atom_contributions.restype is ctypes.c_int and len(lib.mkgnn_atom_contributions.argtypes) == 4
    assert lib.mkgnn_atom_contributions_workspace_bytes.restype is ctypes.c_size_t
    assert len(lib.mkgnn_atom_contributions_workspace_bytes.argtypes) == 4
    assert _lib.ATOM_CONTRIB_MAX_TASKS == 32
    names = [f[0] for f in _lib.AtomContribArgs._fields_]
    assert names == ["sim", "sim_stride", "num_kernels", "buckets", "in_rowptr", "in_col", "n_atoms", "readout", "head_weight",
                     "head_stride", "T", "contrib", "contrib_stride"]
    # the z rows of the batch, and nothing for a shape outside the kernel or an empty batch (host only: no GPU is touched)
    assert lib.mkgnn_atom_contributions_workspace_bytes(110, 32, 32, 1000) == lib.mkgnn_tail_score_workspace_bytes(110, 32, 32, 1000, 7)
    assert lib.mkgnn_atom_contributions_workspace_bytes(110, 32, 32, 1000) >= 1000 * 32 * 4
    assert lib.mkgnn_atom_contributions_workspace_bytes(110, 32, 32, 0) == 0
    # what was there is what it was
    assert lib.mkgnn_tail_score.restype is ctypes.c_int
    assert lib.mkgnn_tail_score.argtypes == [ctypes.POINTER(_lib.TailArgs), ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    assert len(_lib.TailArgs._fields_) == 34


def _modules(K, H, G, T, seed, bias1=True, bias2=True):
    torch.manual_seed(seed)
    return (torch.nn.Linear(K, H, bias=bias1).double(), torch.nn.Linear(H, G, bias=bias2).double(),
            torch.nn.Linear(G, T).double())


def _detached(m):
    return None if m is None else m.detach()


@pytest.mark.parametrize("bias1,bias2", [(True, True), (False, True), (True, False)])
@pytest.mark.parametrize("K,H,G,T", [(110, 32, 32, 1), (110, 30, 7, 9), (5, 1, 1, 32)])
def test_reference_is_the_modules_in_float64(K, H, G, T, bias1, bias2):
    """Atom by atom to 1e-12 relative; and completeness -- segment sums plus the head's bias are ``ffn(pool(lin2(swish(lin1(h)))))``
    -- on a batch with an empty molecule and a one-atom molecule."""
    from molkgnn_amd.readout import atom_contributions_reference
    lin1, lin2, ffn = _modules(K, H, G, T, 100 * K + T, bias1, bias2)
    g = torch.Generator().manual_seed(K + H + G + T)
    h = torch.randn(23, K, generator=g, dtype=torch.float64) * 2.0
    got = atom_contributions_reference(h, lin1.weight, lin1.bias, lin2.weight, lin2.bias, ffn.weight)
    assert isinstance(got, np.ndarray) and got.dtype == np.float64 and got.shape == (23, T)
    with torch.no_grad():
        pre = lin1(h)
        per_atom = lin2(pre * torch.sigmoid(pre))
        want = (per_atom @ ffn.weight.t()).numpy()
    assert (np.abs(got - want) <= 1e-12 * np.abs(want).max()).all(), np.abs(got - want).max()
    # arrays and float32 inputs are taken as they are
    again = atom_contributions_reference(h.numpy(), lin1.weight.detach().numpy(), _detached(lin1.bias), lin2.weight.detach().numpy(),
                                         _detached(lin2.bias), ffn.weight.detach().numpy())
    assert np.array_equal(again, got)
    # completeness: molecules of 9, 0, 1 and 13 atoms
    batch = torch.tensor([0] * 9 + [2] + [3] * 13)
    with torch.no_grad():
        pooled = torch.zeros(4, G, dtype=torch.float64).index_add_(0, batch, per_atom)
        pred = ffn(pooled).numpy()
    sums = np.zeros((4, T))
    np.add.at(sums, batch.numpy(), got)
    total = sums + ffn.bias.detach().numpy()
    assert (np.abs(total - pred) <= 1e-12 * max(np.abs(pred).max(), 1.0)).all()
    assert (sums[1] == 0).all() and np.array_equal(sums[2], got[9])
    with pytest.raises(ValueError):
        atom_contributions_reference(h[:, :-1], lin1.weight, lin1.bias, lin2.weight, lin2.bias, ffn.weight)


# ------------------------------------------------------------------ the stated evaluation order, emulated in float32 --
def _f32(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32)


def _fma32(a, b, c):
    """fmaf on float32 arrays: the product of two float32 values is exact in float64."""
    return _f32(a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64))


def _emulate(sim, block_of, rowptr, col, w1, b1, w2, b2, wh, rng):
    """kgnn_atom_contrib.hip's order with one rounding per operation: the projection and the edge-by-edge propagate in float32, V
    and c0 formed first by fmaf over g, the sigmoid off by its stated 2^-22 + |v| 2^-23 either way, lane l's four fmaf, the xor
    tree over the 8 lanes (offsets 4, 2, 1), + c0."""
    n, H, G, T = sim.shape[0], w1.shape[0], w2.shape[0], wh.shape[0]
    z = np.zeros((n, 32), dtype=np.float32)
    for off, L, atoms in block_of:
        for k in range(L):
            z[atoms, :H] = _fma32(sim[atoms, off + k][:, None], w1[None, :, off + k], z[atoms, :H])
    V = np.zeros((T, 32), dtype=np.float32)
    c0 = np.zeros(T, dtype=np.float32)
    for g in range(G):
        V[:, :H] = _fma32(wh[:, g][:, None], w2[g][None, :], V[:, :H])
        c0 = _fma32(wh[:, g], np.broadcast_to(b2[g], (T,)), c0)
    s = np.zeros((n, 32), dtype=np.float32)
    deg = np.diff(rowptr)
    for k in range(int(deg.max()) if n else 0):
        has = np.nonzero(deg > k)[0]
        s[has] = s[has] + z[col[rowptr[has] + k]]
    pre = s.copy()
    pre[:, :H] = s[:, :H] + b1[None, :]
    p64 = pre.astype(np.float64)
    with np.errstate(over="ignore"):
        sig = 1.0 / (1.0 + np.exp(-p64))
    sig = _f32(sig * (1.0 + rng.choice([-1.0, 1.0], size=sig.shape) * (2.0 ** -22 + np.abs(p64) * 2.0 ** -23)))
    act = pre * sig                                          # (float32 * float32 -> float32)
    out = np.empty((n, T), dtype=np.float32)
    for t in range(T):
        lanes = act[:, 0::4] * V[t, 0::4][None, :]
        for c in (1, 2, 3):
            lanes = _fma32(np.broadcast_to(V[t, c::4][None, :], lanes.shape), act[:, c::4], lanes)
        for o in (4, 2, 1):
            lanes = lanes + lanes[:, np.arange(8) ^ o]
        out[:, t] = lanes[:, 0] + c0[t]
    return out


@pytest.mark.parametrize("T", [1, 9, 32])
@pytest.mark.parametrize("n_mols", [1, 2, 300])
def test_float32_emulation_of_the_evaluation_order_meets_the_criterion(n_mols, T):
    """Against the float64 definition on the same ``sim``: ``max |got - want| <= 2e-5 max(max |want|, 1e-6)`` over ``[N, T]``, and for
    the molecule sums ``<= 2e-5 max(A_g, 1) scale``.  (Measured here: at most 6e-7 of the scale per atom, 7e-8 of ``A_g * scale`` for
    the sums.)"""
    from molkgnn_amd.readout import atom_contributions_reference
    from molkgnn_amd.synthetic import make_batch
    b = make_batch(n_mols, seed=500 + n_mols, with_receptive_fields=False)
    n = b.x.shape[0]
    src, dst = b.edge_index[0].numpy(), b.edge_index[1].numpy()
    degree = np.bincount(src, minlength=n)
    order = np.argsort(dst, kind="stable")
    col = src[order]
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(dst, minlength=n))])
    rng = np.random.default_rng(7 * n_mols + T)
    K = sum(LS)
    sim = np.zeros((n, K), dtype=np.float32)
    block_of, off = [], 0
    for d, L in enumerate(LS, start=1):
        atoms = np.nonzero(degree == d)[0]
        sim[atoms, off:off + L] = rng.standard_normal((atoms.size, L)).astype(np.float32)
        block_of.append((off, L, atoms))
        off += L
    torch.manual_seed(31 + T)
    lin1, lin2, ffn = torch.nn.Linear(K, 32), torch.nn.Linear(32, 32), torch.nn.Linear(32, T)
    w1, b1, w2, b2, wh = (p.detach().numpy() for p in (lin1.weight, lin1.bias, lin2.weight, lin2.bias, ffn.weight))
    got = _emulate(sim, block_of, rowptr, col, w1, b1, w2, b2, wh, rng).astype(np.float64)
    h = np.zeros((n, K))
    np.add.at(h, dst, sim[src].astype(np.float64))
    want = atom_contributions_reference(h, w1, b1, w2, b2, wh)
    scale = max(float(np.abs(want).max()), 1e-6)
    err = float(np.abs(got - want).max())
    print(f"per atom: max error {err:.3e} at scale {scale:.3e} ({err / scale:.2e} of it; bound 2e-5)")
    assert err <= 2e-5 * scale
    mol = b.batch.numpy()
    atoms_of = np.bincount(mol, minlength=n_mols)
    sums, want_sums = np.zeros((n_mols, T)), np.zeros((n_mols, T))
    np.add.at(sums, mol, got)
    np.add.at(want_sums, mol, want)
    ratio = float((np.abs(sums - want_sums) / (np.maximum(atoms_of, 1)[:, None] * scale)).max())
    print(f"molecule sums: max error {ratio:.2e} of A_g * scale (bound 2e-5)")
    assert ratio <= 2e-5


# --------------------------------------------------------------------------------- refused before any launch --
def test_training_mode_is_refused_before_the_batch_is_looked_at():
    from molkgnn_amd.train import GNNModel
    torch.manual_seed(0)
    model = GNNModel(task_dim=3).train()
    with pytest.raises(ValueError, match="atom_contributions needs evaluation mode"):
        model.atom_contributions(object())                   # (not a batch: nothing of it may be read)
    assert model.training


def test_explain_resident_refusals(tmp_path):
    from molkgnn_amd import shards as S
    from molkgnn_amd.screening import explain_resident
    from molkgnn_amd.synthetic import make_batch
    from molkgnn_amd.train import GNNModel
    b = make_batch(12, seed=77, assay="all9", with_receptive_fields=False)
    path = str(tmp_path / "lib.mkgs")
    S.write_shard(path, b)
    resident = S.ResidentShard(path, "cpu")
    torch.manual_seed(1)
    model = GNNModel(task_dim=2).train()
    for ids in ([], np.zeros(0, dtype=np.int64), torch.zeros(0, dtype=torch.long)):
        with pytest.raises(ValueError, match="at least one molecule id"):
            explain_resident(model, resident, ids)
    for ids in ([0, 12], [-1], torch.tensor([3, 99])):
        with pytest.raises(ValueError, match=r"outside \[0, 12\)"):
            explain_resident(model, resident, ids)
    with pytest.raises(ValueError, match="batch_size"):
        explain_resident(model, resident, [1, 2], batch_size=0)
    with pytest.raises(ValueError, match="screening runs on the GPU"):
        explain_resident(model, resident, [3, 1, 3])
    assert model.training


def test_the_switch_is_read_once_at_import_and_documented():
    from molkgnn_amd import readout as R
    assert R._ATOM_CONTRIB is (os.environ.get("MKGNN_ATOM_CONTRIB", "1") != "0")
    doc = open(os.path.join(REPO, "INTEGRATION.md"), encoding="utf-8").read()
    assert re.search(r"^\| `MKGNN_ATOM_CONTRIB` \|", doc, flags=re.M)
    assert "mkgnn_atom_contributions" in doc
