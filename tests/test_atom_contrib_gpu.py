"""Every atom's exact share of every logit (csrc/kgnn_atom_contrib.hip, ``mkgnn_atom_contributions``, ``readout.atom_contributions``,
``GNNModel.atom_contributions``, ``screening.explain_resident``).  ``pytest -m gpu``.

The kernel is called through the C ABI with buffers of the test's own and held to the float64 formula of the reference
(KernelLayer.py:119-123, MolKGNNNet.py:144-146, model.py:147-150) on the same ``sim``, NaN outside every atom's block:
``max |got - want| <= 2e-5 max(max |want|, 1e-6)`` over the whole ``[N, T]`` result -- the criterion of tests/test_tail.py and
tests/test_score_tail.py, taken as it stands because the output is a linear functional of the ``swish(pre)`` values those tests hold
to it -- and, for the molecule sums, ``|sum_n c[n, t] + bh[t] - pred64[g, t]| <= 2e-5 max(A_g, 1) scale_c`` (the per-atom bound,
``A_g`` times).  Every atom of every case is compared; the output always sits at a stride of ``T + 3`` between patterned guard
rows.
"""
import ctypes

import numpy as np
import pytest
import torch

from tests import _topologies as T_
from tests._resident_library import bits, build_library, eval_model
from tests.test_tail import _block_rows

pytestmark = pytest.mark.gpu

LS = (10, 20, 30, 50)
PATTERN = 0x5A5A5A5A
GUARD = 2                                                # patterned rows in front of and behind the output
REL = 2e-5


def _dev():
    assert torch.cuda.is_available(), "pytest -m gpu needs the MI355X"
    return torch.device("cuda:0")


def _bits(t):
    return t.contiguous().view(torch.int32)


def _modules(dev, T, H=32, G=32, seed=5, bias1=True, bias2=True, K=110):
    torch.manual_seed(seed)
    return (torch.nn.Linear(K, H, bias=bias1).to(dev), torch.nn.Linear(H, G, bias=bias2).to(dev), torch.nn.Linear(G, T).to(dev))


class _Call:
    """One filled ``mkgnn_atom_contrib_args`` with every buffer owned here: ``contrib`` is the ``[n, T]`` view of a patterned
    ``[GUARD + n + GUARD, T + 3]`` buffer.  ``wh`` / ``head_stride``: the head rows to pass instead of ``ffn.weight``."""

    def __init__(self, sim, plan, mods, dev, wh=None, head_stride=None, n_atoms=None):
        from molkgnn_amd import _lib
        from molkgnn_amd import readout as R
        lin1, lin2, ffn = mods
        n, K = sim.shape
        self.w = [lin1.weight.detach().contiguous(), lin2.weight.detach().contiguous(),
                  ffn.weight.detach().contiguous() if wh is None else wh]
        self.b = [None if m.bias is None else m.bias.detach() for m in (lin1, lin2)]
        H, G = self.w[0].shape[0], self.w[1].shape[0]
        T = self.w[2].shape[0]
        self.T, self.n, self.stride = T, n, T + 3
        self.buf = torch.full((n + 2 * GUARD, self.stride), PATTERN, dtype=torch.int32, device=dev)
        self.contrib = self.buf.view(torch.float32)[GUARD:GUARD + n, :T]
        self.keep = [sim, plan, mods]
        self.before = [t.clone() for t in [sim] + self.w + [x for x in self.b if x is not None]]
        a = _lib.AtomContribArgs()
        a.sim, a.sim_stride = sim.data_ptr(), R._stride0(sim)
        for i, L in enumerate(LS):
            a.num_kernels[i] = L
        self.bk = R._sel_buckets(plan)
        a.buckets = ctypes.cast(self.bk, ctypes.c_void_p)
        rin, cin = plan.csr_in
        a.in_rowptr, a.in_col = rin.data_ptr(), cin.data_ptr()
        a.n_atoms = n if n_atoms is None else n_atoms
        a.readout = R._params(self.w[0], self.b[0], self.w[1], self.b[1])
        a.head_weight, a.head_stride, a.T = self.w[2].data_ptr(), (G if head_stride is None else head_stride), T
        a.contrib, a.contrib_stride = self.contrib.data_ptr(), self.stride
        self.a, self.dims, self.dev = a, (K, H, G, n), dev

    def need(self):
        from molkgnn_amd import _lib
        return int(_lib.load().mkgnn_atom_contributions_workspace_bytes(*self.dims))

    def raw(self, ws_bytes=None, guard=4096):
        """The call itself: ``(return code, the guard bytes behind the workspace)``."""
        from molkgnn_amd import _lib
        lib = _lib.load()
        need = self.need()
        ws = torch.full((max(need, 1) + guard,), 0x5A, dtype=torch.uint8, device=self.dev)
        with torch.cuda.device(self.dev):
            rc = lib.mkgnn_atom_contributions(ctypes.byref(self.a), ws.data_ptr(), need if ws_bytes is None else ws_bytes,
                                              _lib.stream_ptr(self.dev))
        torch.cuda.synchronize()
        return rc, ws[need:]

    def run(self):
        from molkgnn_amd import _lib
        assert self.need() >= self.n * 32 * 4
        rc, guard = self.raw()
        _lib.check(rc, "mkgnn_atom_contributions")
        assert bool((guard == 0x5A).all()), "bytes behind mkgnn_atom_contributions_workspace_bytes were written"
        return self

    def nothing_else_written(self):
        """The guard rows and the gap columns keep their pattern; sim and the parameters are what they were."""
        assert bool((self.buf[:GUARD] == PATTERN).all()) and bool((self.buf[GUARD + self.n:] == PATTERN).all())
        assert bool((self.buf[:, self.T:] == PATTERN).all())
        now = [self.keep[0]] + self.w + [x for x in self.b if x is not None]
        for was, t in zip(self.before, now):
            assert torch.equal(_bits(was), _bits(t))

    def untouched(self):
        assert bool((self.buf == PATTERN).all())


def _h64(b, inblock, sim0, dev):
    """h = propagate(sim) in float64, the blocks' values alone."""
    dense = torch.where(inblock, sim0, torch.zeros((), device=dev)).double()
    return torch.zeros_like(dense).index_add_(0, b.edge_index[1], dense[b.edge_index[0]]).cpu()


def _want(h64, mods):
    from molkgnn_amd.readout import atom_contributions_reference
    lin1, lin2, ffn = mods
    return atom_contributions_reference(h64, lin1.weight, lin1.bias, lin2.weight, lin2.bias, ffn.weight)


def _close(got, want, rel=REL, what=""):
    got = got.detach().double().cpu().numpy() if torch.is_tensor(got) else got
    assert got.shape == want.shape and np.isfinite(got).all()
    err, scale = float(np.abs(got - want).max()), max(float(np.abs(want).max()), 1e-6)
    print(f"{what}max error {err:.3e} at scale {scale:.3e} ({err / scale:.2e} of it; bound {rel:.0e})")
    assert err <= rel * scale, (what, err, scale)
    return scale


def _complete(got, want, batch, n_mols, what=""):
    """Molecule sums of the float32 contributions, in float64, against those of the float64 ones (the head's bias cancels)."""
    mol = batch.cpu().numpy()
    atoms = np.bincount(mol, minlength=n_mols)
    sums, want_sums = np.zeros((n_mols, want.shape[1])), np.zeros((n_mols, want.shape[1]))
    np.add.at(sums, mol, got.detach().double().cpu().numpy())
    np.add.at(want_sums, mol, want)
    scale = max(float(np.abs(want).max()), 1e-6)
    ratio = float((np.abs(sums - want_sums) / (np.maximum(atoms, 1)[:, None] * scale)).max())
    print(f"{what}molecule sums: {ratio:.2e} of A_g * scale (bound {REL:.0e})")
    assert ratio <= REL


def _case(b, plan, sim0, inblock, mods, dev, h64=None, what=""):
    """Definition, completeness, nothing else written, two calls bit-equal.  Returns the contributions."""
    c = _Call(sim0, plan, mods, dev).run()
    c.nothing_else_written()
    want = _want(_h64(b, inblock, sim0, dev) if h64 is None else h64, mods)
    _close(c.contrib, want, what=what)
    _complete(c.contrib, want, b.batch, int(b.num_graphs), what=what)
    again = _Call(sim0, plan, mods, dev).run()
    assert torch.equal(_bits(again.contrib), _bits(c.contrib))
    return c.contrib


# (H, G, T, lin1 bias, lin2 bias): every T of {1, 2, 9, 32} and every (H, G) of {(32, 32), (30, 7), (1, 1)} together
SHAPES = [(H, G, T, not (H == 30 and T == 2), not (H == 1 and T == 9))
          for H, G in ((32, 32), (30, 7), (1, 1)) for T in (1, 2, 9, 32)]


@pytest.mark.parametrize("n_mols", [1, 2, 300, 1400])
def test_definition(n_mols):
    """One molecule is fewer atoms than one pass of a workgroup's 32 atom slots; 300 give many workgroups and a ragged last one; 1 400
    lie beyond the grid's cap (1 024 workgroups of 32 atoms), so workgroups take a second pass -- there two shapes are enough."""
    from molkgnn_amd.plan import plan_from_data
    from molkgnn_amd.synthetic import make_batch
    dev = _dev()
    b = make_batch(n_mols, seed=900 + n_mols).to(dev)
    plan = plan_from_data(b)
    n = b.x.shape[0]
    if n_mols == 1:
        assert n < 32
    if n_mols == 1400:
        assert n > 32 * 1024
    sim0, inblock = _block_rows(b, plan, LS, dev, n_mols)
    h64 = _h64(b, inblock, sim0, dev)
    shapes = SHAPES if n_mols != 1400 else [s for s in SHAPES if (s[0], s[2]) in ((32, 9), (30, 32))]
    assert any(not s[3] for s in SHAPES) and any(not s[4] for s in SHAPES)
    for H, G, T, bias1, bias2 in shapes:
        mods = _modules(dev, T, H, G, seed=7 * T + H, bias1=bias1, bias2=bias2)
        _case(b, plan, sim0, inblock, mods, dev, h64, what=f"H={H} G={G} T={T}: ")


SPECS = [T_.single(), T_.pair(), T_.star(6), T_.circulant(130), T_.tree(30), T_.empty()]


def test_topologies():
    """An atom with no in-edge and no bucket, a hub with six in-edges in no bucket, a molecule beyond the fused tail's chunk."""
    from molkgnn_amd import readout as R
    from molkgnn_amd.plan import plan_from_data
    dev = _dev()
    b = T_.batch_of(SPECS, seed=21).to(dev)
    plan = plan_from_data(b)
    seg = R.molecule_segments(b.batch, b.num_graphs)
    assert not R._tail_limits_ok(seg, plan)
    deg = T_.degrees(b)
    assert int(deg[0]) == 0 and int(deg.max()) == 6
    sim0, inblock = _block_rows(b, plan, LS, dev, 21)
    assert not bool(inblock[0].any()) and not bool(inblock[int(deg.argmax())].any())
    for T in (1, 9):
        mods = _modules(dev, T, seed=40 + T)
        got = _case(b, plan, sim0, inblock, mods, dev, what=f"T={T}: ")
        # the isolated atom: V swish(b1) + c0
        lin1, lin2, ffn = mods
        with torch.no_grad():
            pre = lin1.bias.double()
            lone = (lin2.weight.double() @ (pre * torch.sigmoid(pre)) + lin2.bias.double()) @ ffn.weight.double().t()
        assert float((got[0].double() - lone).abs().max()) <= REL * max(float(got.abs().max()), 1e-6)


def test_locality_of_the_bits_other_molecules():
    """(a) The same molecules behind another one: the contributions of their atoms are bit for bit the same."""
    from molkgnn_amd.plan import plan_from_data
    dev = _dev()
    b0 = T_.batch_of(SPECS, seed=22).to(dev)
    b1 = T_.batch_of([T_.tree(17)] + SPECS, seed=23).to(dev)
    plan0, plan1 = plan_from_data(b0), plan_from_data(b1)
    sim0, inblock0 = _block_rows(b0, plan0, LS, dev, 22)
    sim1, inblock1 = _block_rows(b1, plan1, LS, dev, 23)
    assert torch.equal(inblock1[17:], inblock0)
    sim1[17:] = sim0
    mods = _modules(dev, 9, seed=3)
    c0 = _Call(sim0, plan0, mods, dev).run().contrib
    c1 = _Call(sim1, plan1, mods, dev).run().contrib
    assert torch.equal(_bits(c1[17:]), _bits(c0))


def test_locality_of_the_bits_tasks_and_strides():
    """(b) T = 9 against nine T = 1 calls on head row t: column t is bit-equal; and a head with padded rows changes nothing."""
    from molkgnn_amd.plan import plan_from_data
    from molkgnn_amd.synthetic import make_batch
    dev = _dev()
    b = make_batch(20, seed=31).to(dev)
    plan = plan_from_data(b)
    sim0, _ = _block_rows(b, plan, LS, dev, 31)
    for H, G in ((32, 32), (30, 7)):
        mods = _modules(dev, 9, H, G, seed=H)
        all9 = _Call(sim0, plan, mods, dev).run().contrib
        wh = mods[2].weight.detach().contiguous()
        for t in range(9):
            one = _Call(sim0, plan, mods, dev, wh=wh[t:t + 1]).run()
            assert one.T == 1 and torch.equal(_bits(one.contrib[:, 0]), _bits(all9[:, t])), t
        wide = torch.full((9, G + 5), float("nan"), device=dev)
        wide[:, :G] = wh
        padded = _Call(sim0, plan, mods, dev, wh=wide[:, :G], head_stride=G + 5)
        assert padded.T == 9
        assert torch.equal(_bits(padded.run().contrib), _bits(all9))


def test_locality_of_the_bits_padded_batch():
    """(c) padding.pad_batch: the real atoms of the padded batch are bit for bit those of the unpadded one (the construction of
    test_score_tail_on_padded_batches_equals_the_unpadded_batch)."""
    from molkgnn_amd import padding as P
    from molkgnn_amd.plan import plan_from_data
    from molkgnn_amd.receptive_field import attach_receptive_fields
    from molkgnn_amd.synthetic import make_batch
    dev = _dev()
    B = 120
    raw = make_batch(B, seed=4100, with_receptive_fields=False)
    shape = P.fixed_shape([P.degree_histogram(raw)])
    for d in range(1, 5):
        shape[f"n{d}"] += 20
    shape["atoms"] = sum(shape[f"n{d}"] for d in range(1, 5))
    shape["edges"] = sum(d * shape[f"n{d}"] for d in range(1, 5))
    plain = attach_receptive_fields(raw.to(dev))
    padded = attach_receptive_fields(P.pad_batch(raw, shape, B).to(dev), sizes=[shape[f"n{d}"] for d in range(1, 5)])
    plan0, plan1 = plan_from_data(plain), plan_from_data(padded)
    sim0, inblock0 = _block_rows(plain, plan0, LS, dev, 77)
    sim1, inblock1 = _block_rows(padded, plan1, LS, dev, 78)
    n_real = plain.x.shape[0]
    assert padded.x.shape[0] >= n_real + 64 and torch.equal(inblock1[:n_real], inblock0)
    sim1[:n_real] = sim0
    mods = _modules(dev, 9, seed=8)
    c0 = _Call(sim0, plan0, mods, dev).run().contrib
    c1 = _Call(sim1, plan1, mods, dev).run()
    c1.nothing_else_written()
    assert torch.equal(_bits(c1.contrib[:n_real]), _bits(c0))
    assert bool(torch.isfinite(c1.contrib).all())


def test_c_level_refusals_launch_nothing():
    from molkgnn_amd import _lib
    from molkgnn_amd.plan import plan_from_data
    from molkgnn_amd.synthetic import make_batch
    dev = _dev()
    lib = _lib.load()
    b = make_batch(5, seed=12).to(dev)
    plan = plan_from_data(b)
    sim0, _ = _block_rows(b, plan, LS, dev, 12)
    mods = _modules(dev, 9, seed=2)

    def refused(call, ws_bytes=None, word=None):
        rc, guard = call.raw(ws_bytes)
        msg = lib.mkgnn_last_error().decode()
        assert rc != 0 and "mkgnn_atom_contributions" in msg and (word is None or word in msg), (rc, msg)
        call.untouched()
        assert bool((guard == 0x5A).all())

    c = _Call(sim0, plan, mods, dev)
    c.a.T = 0
    refused(c, word="tasks")
    c = _Call(sim0, plan, mods, dev)
    c.a.T = 33
    refused(c, word="tasks")
    refused(_Call(sim0, plan, _modules(dev, 9, H=33), dev))
    c = _Call(sim0, plan, mods, dev)
    c.a.contrib = None
    refused(c, word="null")
    c = _Call(sim0, plan, mods, dev)
    c.a.contrib_stride = c.T - 1
    refused(c, word="contrib stride")
    c = _Call(sim0, plan, mods, dev)
    c.a.head_stride = 31
    refused(c, word="head stride")
    c = _Call(sim0, plan, mods, dev)
    refused(c, ws_bytes=c.need() - 1, word="workspace")
    c = _Call(sim0, plan, mods, dev)
    c.a.sim = sim0.data_ptr() + 4                            # misaligned rows
    refused(c, word="aligned")
    # an empty batch is a no-op
    c = _Call(sim0, plan, mods, dev, n_atoms=0)
    rc, _ = c.raw()
    assert rc == 0
    c.untouched()
    # ... and the call still works
    _Call(sim0, plan, mods, dev).run()


# ------------------------------------------------------------------------------------------------------ model level --
def _spy(monkeypatch, mod, name):
    calls = []
    real = getattr(mod, name)
    monkeypatch.setattr(mod, name, lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    return calls


def _sums_against_pred(contrib, pred, mol_ptr, bias, what=""):
    """Molecule sums plus the head's bias against the model's own predictions: 2e-5 A_g scale_c + 2e-5 scale_pred."""
    ptr = mol_ptr.cpu().numpy().astype(np.int64)
    c = contrib.detach().double().cpu().numpy()
    p = pred.detach().double().cpu().numpy()
    scale_c, scale_p = max(float(np.abs(c).max()), 1e-6), max(float(np.abs(p).max()), 1e-6)
    worst = 0.0
    for g in range(p.shape[0]):
        lo, hi = int(ptr[g]), int(ptr[g + 1])
        err = np.abs(c[lo:hi].sum(axis=0) + bias - p[g]).max()
        bound = REL * (hi - lo) * scale_c + REL * scale_p
        worst = max(worst, float(err / bound))
        assert err <= bound, (what, g, err, bound)
    print(f"{what}molecule sums against predict_tasks: worst error / bound = {worst:.3f}")


@pytest.fixture(scope="module")
def library(tmp_path_factory):
    return build_library(tmp_path_factory.mktemp("library_explain"), _dev(), counts=(70,), shard_seed=40,
                         labels=lambda n: (torch.arange(n) % 3 == 0).float(), model_seed=9, num_layers=3, task_dim=9)


@pytest.mark.parametrize("task_dim", [1, 9])
def test_model_atom_contributions(task_dim, library, monkeypatch):
    from molkgnn_amd import molecule as M
    from molkgnn_amd import readout as R
    from molkgnn_amd.synthetic import make_batch
    dev = _dev()
    nine, residents, gathered = library
    model = nine if task_dim == 9 else eval_model(dev, 1, num_layers=3, task_dim=1)
    bias = model.ffn.bias.detach().double().cpu().numpy()
    def check(data, ptr, what):
        pred0 = model.predict_tasks(data)[0].clone()
        one0 = model.predict(data)[0].clone()
        state0 = {n: v.clone() for n, v in model.state_dict().items()}
        hip = _spy(monkeypatch, R, "atom_contributions")
        resident_step = _spy(monkeypatch, M, "net_forward")
        got = model.atom_contributions(data)
        torch.cuda.synchronize()
        assert len(hip) == 1 and not resident_step, "the HIP route, without the molecule-resident step"
        monkeypatch.undo()
        assert got.shape == (data.x.shape[0], task_dim) and got.dtype == torch.float32 and not got.requires_grad
        _sums_against_pred(got, pred0, ptr, bias, what)
        # the operator route of MKGNN_ATOM_CONTRIB=0 (the module flag the variable sets at import)
        hip = _spy(monkeypatch, R, "atom_contributions")
        monkeypatch.setattr(R, "_ATOM_CONTRIB", False)
        slow = model.atom_contributions(data)
        assert not hip
        monkeypatch.undo()
        n_real = int(ptr[pred0.shape[0]])                   # (behind them: padding atoms)
        _close(got[:n_real], slow[:n_real].double().cpu().numpy(), rel=2 * REL, what=what + "against the operator route: ")
        # nothing of the model moved, and its predictions are what they were
        assert not model.training
        for n, v in model.state_dict().items():
            assert torch.equal(v, state0[n]), n
        assert torch.equal(_bits(model.predict_tasks(data)[0]), _bits(pred0))
        assert torch.equal(_bits(model.predict(data)[0]), _bits(one0))

    plain = make_batch(40, seed=61).to(dev)
    check(plain, R.molecule_segments(plain.batch, 40).mol_ptr, "plain: ")
    for k, (data, live) in enumerate(gathered(residents[0])):
        check(data, data.mol_ptr, f"gathered {k}: ")
        if k == 1:
            break


def test_explain_resident(library):
    """``ids = arange(70)`` at batch 32: bit for bit ``model.atom_contributions`` on the gathered batches, cut at the real atoms.  A
    shuffled subset with a repeat, from a model that comes in training mode: completeness against ``score_resident_tasks`` on the
    same shard at the same batch size, with the bound of ``test_model_atom_contributions`` -- every molecule is explained in the
    batch the shard pass scores it in.  (In ANOTHER layout the network itself gives a few molecules another logit: gathered in
    batches of 8, ``predict_tasks`` of molecules 12, 20, 24, 46, 53, 56 and 62 of this shard differs from their batch-32 scores by up
    to 1.41e-2 at a scale of 5.8, with every input row bit-equal -- last-bit differences in the first layer's output decide
    between tied permutations in the second.  A first version that explained the subset in batches of its own missed this bound
    by 1.31e-2 against 2.5e-4 for that reason.)"""
    from molkgnn_amd.screening import explain_resident, score_resident_tasks
    dev = _dev()
    model, residents, gathered = library
    resident = residents[0]
    ids = np.arange(70)
    out = explain_resident(model, resident, ids, batch_size=32)
    assert set(out) == {"atom_ptr", "contrib", "bias"}
    atom_ptr = out["atom_ptr"]
    assert atom_ptr.dtype == np.int64 and np.array_equal(atom_ptr, np.concatenate([[0], np.cumsum(resident.mol_atoms[ids])]))
    assert out["contrib"].shape == (int(atom_ptr[-1]), 9) and out["contrib"].dtype == torch.float32 and out["contrib"].device == dev
    assert torch.equal(out["bias"], model.ffn.bias.detach())
    eager = []
    for data, live in gathered(resident):
        n_real = int(data.mol_ptr[live])
        eager.append(model.atom_contributions(data)[:n_real].clone())
    assert np.array_equal(bits(out["contrib"]), bits(torch.cat(eager)))
    # a shuffled subset with a repeat, from a model that comes in training mode: completeness against the shard's scores
    scores = score_resident_tasks(model, resident, 32)
    rng = np.random.default_rng(5)
    sub = rng.permutation(70)[:23]
    sub[7] = sub[2]
    model.train()
    try:
        some = explain_resident(model, resident, torch.from_numpy(sub), batch_size=32)
        assert model.training
    finally:
        model.eval()
    ptr = some["atom_ptr"]
    assert np.array_equal(np.diff(ptr), resident.mol_atoms[sub])
    _sums_against_pred(some["contrib"], scores[torch.from_numpy(sub).to(dev)], torch.from_numpy(ptr), some["bias"].double().cpu().numpy())
