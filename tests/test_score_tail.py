"""The forward-only tail of evaluation mode (csrc/kgnn_tail.hip ``tail_middle_kernel<.., FWD>``, ``mkgnn_tail_score``,
``readout.tail_score``, ``GNNModel.predict``, ``train.evaluate``).  ``pytest -m gpu``.

The kernel is pinned to the training tail -- ``pred`` and ``emb`` BIT FOR BIT those ``mkgnn_tail_fused`` writes at dropout 0, padded
batches included; both entry points are called through the C ABI with buffers of the test's own -- and, like it, held to the float64
PyTorch formula of the reference (KernelLayer.py:119-123, MolKGNNNet.py:144-146, model.py:147-150) within 2e-5 of the result's scale
(the criterion of tests/test_tail.py and tests/test_readout_dropout_tail.py).  Every molecule of every case is compared.
"""
import ctypes

import pytest
import torch

from tests import _topologies as T
from tests.test_tail import _block_rows

pytestmark = pytest.mark.gpu

LS = (10, 20, 30, 50)
PATTERN = 0x5A5A5A5A                                      # what "not to be written" buffers are filled with (as int32)


def _dev():
    assert torch.cuda.is_available(), "pytest -m gpu needs the MI355X"
    return torch.device("cuda:0")


def _close(got, want, rel=2e-5):
    err, scale = float((got.double() - want.double()).abs().max()), max(float(want.abs().max()), 1e-6)
    print(f"max error {err:.3e} at scale {scale:.3e} (bound {rel * scale:.3e})")
    assert err <= rel * scale, (err, scale)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _modules(dev, seed=5, bias=True, K=110, H=32, G=32):
    torch.manual_seed(seed)
    return torch.nn.Linear(K, H).to(dev), torch.nn.Linear(H, G).to(dev), torch.nn.Linear(G, 1, bias=bias).to(dev)


def _patterned(shape, dev):
    return torch.full(shape, PATTERN, dtype=torch.int32, device=dev)


class _Call:
    """One filled ``mkgnn_tail_args`` with every buffer owned here (``tests`` reach the C ABI through ``_lib``): ``pred`` and ``emb``
    are the call's outputs; the training tail's other outputs start out as a pattern."""

    def __init__(self, sim, plan, seg, mods, n_rows, y, loss_kind, dev):
        from molkgnn_amd import _lib
        from molkgnn_amd import readout as R
        lin1, lin2, ffn = mods
        n, K = sim.shape
        G = lin2.weight.shape[0]
        self.keep = [sim, plan, seg, mods, y]
        self.pred = _patterned((n_rows,), dev).view(torch.float32)
        self.emb = _patterned((seg.size, G), dev).view(torch.float32)
        self.loss = _patterned((1,), dev).view(torch.float32)
        K4 = K + (-K) % 4
        self.gsim = _patterned((n, K4), dev).view(torch.float32)
        self.grads = [_patterned(tuple(p.shape), dev).view(torch.float32) if p is not None else None
                      for p in (lin1.weight, lin1.bias, lin2.weight, lin2.bias, ffn.weight, ffn.bias)]
        self.rng = torch.tensor([PATTERN, 7], dtype=torch.int64, device=dev)
        self.rng_used = torch.tensor([PATTERN, PATTERN], dtype=torch.int64, device=dev)
        a = _lib.TailArgs()
        a.sim, a.sim_stride = sim.data_ptr(), R._stride0(sim)
        for i, L in enumerate(LS):
            a.num_kernels[i] = L
        self.bk = R._sel_buckets(plan)
        a.buckets = ctypes.cast(self.bk, ctypes.c_void_p)
        (rin, cin), (rout, cout) = plan.csr_in, plan.csr_out
        a.in_rowptr, a.in_col, a.out_rowptr, a.out_col = rin.data_ptr(), cin.data_ptr(), rout.data_ptr(), cout.data_ptr()
        a.mol_ptr, a.atom_mol = seg.mol_ptr.data_ptr(), seg.atom_mol.data_ptr()
        a.n_atoms, a.n_mols, a.n_loss_mols = n, seg.size, n_rows
        self.w = [lin1.weight.detach().contiguous(), lin2.weight.detach().contiguous(), ffn.weight.detach().reshape(-1).contiguous()]
        a.readout = R._params(self.w[0], lin1.bias.detach(), self.w[1], lin2.bias.detach())
        a.head_weight, a.head_bias = self.w[2].data_ptr(), _lib.ptr(None if ffn.bias is None else ffn.bias.detach())
        a.target = y.data_ptr()
        a.dropout_p, a.rng_state, a.rng_used = 0.0, self.rng.data_ptr(), self.rng_used.data_ptr()
        a.emb, a.emb_stride = self.emb.data_ptr(), G
        a.pred, a.loss = self.pred.data_ptr(), self.loss.data_ptr()
        a.grad_sim, a.grad_sim_stride = self.gsim.data_ptr(), K4
        (a.grad_lin1_weight, a.grad_lin1_bias, a.grad_lin2_weight, a.grad_lin2_bias, a.grad_head_weight,
         a.grad_head_bias) = [_lib.ptr(g) for g in self.grads]
        a.defer_reduce, a.loss_kind = 0, int(loss_kind)
        self.a, self.dims, self.dev = a, (K, lin1.weight.shape[0], G, n, seg.size), dev

    def fused(self):
        from molkgnn_amd import _lib
        lib = _lib.load()
        ws = torch.empty(int(lib.mkgnn_tail_workspace_bytes(*self.dims)), dtype=torch.uint8, device=self.dev)
        with torch.cuda.device(self.dev):
            _lib.check(lib.mkgnn_tail_fused(ctypes.byref(self.a), ws.data_ptr(), ws.numel(), _lib.stream_ptr(self.dev)), "mkgnn_tail_fused")
        torch.cuda.synchronize()
        return self

    def score(self, guard=4096):
        """``mkgnn_tail_score`` on a workspace with ``guard`` patterned bytes behind what it asks for; returns those bytes."""
        from molkgnn_amd import _lib
        lib = _lib.load()
        need = int(lib.mkgnn_tail_score_workspace_bytes(*self.dims))
        assert 0 < need <= int(lib.mkgnn_tail_workspace_bytes(*self.dims))
        ws = torch.full((need + guard,), 0x5A, dtype=torch.uint8, device=self.dev)
        with torch.cuda.device(self.dev):
            _lib.check(lib.mkgnn_tail_score(ctypes.byref(self.a), ws.data_ptr(), need, _lib.stream_ptr(self.dev)), "mkgnn_tail_score")
        torch.cuda.synchronize()
        return ws[need:]

    def untouched(self):
        """Everything but ``pred`` and ``emb`` still holds its pattern."""
        for t in [self.loss, self.gsim] + [g for g in self.grads if g is not None]:
            assert bool((_bits(t) == PATTERN).all())
        assert self.rng.tolist() == [PATTERN, 7] and self.rng_used.tolist() == [PATTERN, PATTERN]


def _reference_f64(b, inblock, sim0, mods, n_mols, dev):
    """propagate, lin1, swish, lin2, add-pool, ffn -- the reference's formula in float64."""
    lin1, lin2, ffn = mods
    dense = torch.where(inblock, sim0, torch.zeros((), device=dev)).double()
    src, dst = b.edge_index[0], b.edge_index[1]
    h = torch.zeros_like(dense).index_add_(0, dst, dense[src])
    z = h @ lin1.weight.double().t() + lin1.bias.double()
    z = z * torch.sigmoid(z)
    z = z @ lin2.weight.double().t() + lin2.bias.double()
    emb = torch.zeros(n_mols, z.shape[1], dtype=torch.float64, device=dev).index_add_(0, b.batch, z)
    pred = emb @ ffn.weight.double().t()
    if ffn.bias is not None:
        pred = pred + ffn.bias.double()
    return pred.view(-1).detach(), emb.detach()


def _targets(target, n, dev, seed):
    """(y, loss kind of the training call): binary activity labels with BCE, docking scores with the summed squared error."""
    from molkgnn_amd import _lib
    g = torch.Generator(device=dev).manual_seed(seed)
    if target == "activity":
        return (torch.rand(n, generator=g, device=dev) < 0.3).float(), _lib.LOSS_BCE_MEAN
    return torch.randn(n, generator=g, device=dev) * 1.5 - 8.0, _lib.LOSS_SQERR_SUM


def _score_case(b, plan, seg, sim0, inblock, n_rows, target, dev, bias=True, seed=5):
    """Training tail at dropout 0 and score tail on the same inputs: bit-equal ``pred`` / ``emb``, nothing else written, two calls
    identical, float64 formula met.  Returns (pred, emb) of the score call."""
    mods = _modules(dev, seed, bias)
    y, kind = _targets(target, n_rows, dev, seed)
    train = _Call(sim0, plan, seg, mods, n_rows, y, kind, dev).fused()
    assert bool(torch.isfinite(train.loss).all())
    sc = _Call(sim0, plan, seg, mods, n_rows, y, kind, dev)
    guard = sc.score()
    assert bool((guard == 0x5A).all()), "bytes behind mkgnn_tail_score_workspace_bytes were written"
    sc.untouched()
    assert torch.equal(_bits(sc.pred), _bits(train.pred)), float((sc.pred - train.pred).abs().max())
    assert torch.equal(_bits(sc.emb), _bits(train.emb)), float((sc.emb - train.emb).abs().max())
    again = _Call(sim0, plan, seg, mods, n_rows, y, kind, dev)
    again.score()
    assert torch.equal(_bits(again.pred), _bits(sc.pred)) and torch.equal(_bits(again.emb), _bits(sc.emb))
    return sc.pred, sc.emb, mods


@pytest.mark.parametrize("target", ["activity", "docking_score"])
@pytest.mark.parametrize("n_mols", [1, 2, 300, 4096])
def test_score_tail_is_the_training_tail_forward_bit_for_bit(n_mols, target):
    from molkgnn_amd import readout as R
    from molkgnn_amd.plan import plan_from_data
    from molkgnn_amd.synthetic import make_batch
    dev = _dev()
    b = make_batch(n_mols, seed=900 + n_mols, target=target).to(dev)
    plan = plan_from_data(b)
    seg = R.molecule_segments(b.batch, n_mols)
    assert R.tail_supported(110, 32, 32, LS) and R._tail_limits_ok(seg, plan)
    sim0, inblock = _block_rows(b, plan, LS, dev, n_mols)
    pred, emb, mods = _score_case(b, plan, seg, sim0, inblock, n_mols, target, dev, bias=(n_mols != 2))
    want_pred, want_emb = _reference_f64(b, inblock, sim0, mods, n_mols, dev)
    _close(pred, want_pred)
    _close(emb, want_emb)


@pytest.mark.parametrize("extra", [0, 20], ids=["fewer_than_64_padding_atoms", "at_least_64_padding_atoms"])
def test_score_tail_on_padded_batches_equals_the_unpadded_batch(extra):
    """padding.pad_batch: 64 padding molecules behind the real ones.  ``extra = 0``: one padding atom per degree (or two) -- most
    padding molecules are empty; ``extra = 20``: 80+ padding atoms."""
    from molkgnn_amd import padding as P
    from molkgnn_amd import readout as R
    from molkgnn_amd.plan import plan_from_data
    from molkgnn_amd.receptive_field import attach_receptive_fields
    from molkgnn_amd.synthetic import make_batch
    dev = _dev()
    B = 700
    raw = make_batch(B, seed=4100, with_receptive_fields=False)
    shape = P.fixed_shape([P.degree_histogram(raw)])
    for d in range(1, 5):                                # (+20 of every degree: 200 more bond stubs, still even)
        shape[f"n{d}"] += extra
    shape["atoms"] = sum(shape[f"n{d}"] for d in range(1, 5))
    shape["edges"] = sum(d * shape[f"n{d}"] for d in range(1, 5))
    n_pad = shape["atoms"] - raw.x.shape[0]
    assert (n_pad >= 64) if extra else (0 < n_pad < 64), n_pad
    plain = attach_receptive_fields(raw.to(dev))
    padded = attach_receptive_fields(P.pad_batch(raw, shape, B).to(dev), sizes=[shape[f"n{d}"] for d in range(1, 5)])
    plan0, plan1 = plan_from_data(plain), plan_from_data(padded)
    seg0 = R.molecule_segments(plain.batch, B)
    seg1 = R.MoleculeSegments.from_tensors(padded.mol_ptr, padded.atom_mol, padded.max_mol_atoms, padded.max_mol_edges)
    assert seg1.size == B + P.PAD_MOLECULES and R._tail_limits_ok(seg1, plan1)
    sim0, inblock0 = _block_rows(plain, plan0, LS, dev, 77)
    sim1, inblock1 = _block_rows(padded, plan1, LS, dev, 78)
    n_real = plain.x.shape[0]
    assert torch.equal(inblock1[:n_real], inblock0)
    sim1[:n_real] = sim0                                  # the real atoms' rows; the padding atoms keep random ones
    pred0, emb0, mods = _score_case(plain, plan0, seg0, sim0, inblock0, B, "activity", dev)
    pred1, emb1, _ = _score_case(padded, plan1, seg1, sim1, inblock1, B, "activity", dev)
    assert pred1.shape == (B,) and torch.equal(_bits(pred1), _bits(pred0))
    assert torch.equal(_bits(emb1[:B]), _bits(emb0))
    want_pred, want_emb = _reference_f64(padded, inblock1, sim1, mods, B + P.PAD_MOLECULES, dev)
    _close(pred1, want_pred[:B])
    # (the padding molecules' rows are cut off by every consumer: pad_batch bonds padding atoms across padding molecules, which
    # the chunked kernels -- training and score tail alike, compared bit for bit above -- do not follow)
    _close(emb1[:B], want_emb[:B])


def test_score_tail_with_a_molecule_at_the_atom_limit():
    """128 atoms and 512 edges each way in one molecule (MKGNN_TAIL_MAX_ATOMS, MKGNN_TAIL_MAX_EDGES) next to small ones."""
    from molkgnn_amd import _lib
    from molkgnn_amd import readout as R
    from molkgnn_amd.plan import plan_from_data
    dev = _dev()
    specs = [T.tree(12), T.circulant(_lib.TAIL_MAX_ATOMS), T.single(), T.tree(30)]
    b = T.batch_of(specs, seed=13).to(dev)
    plan = plan_from_data(b)
    seg = R.molecule_segments(b.batch, b.num_graphs)
    assert R._tail_limits_ok(seg, plan) and max(T.molecule_sizes(b)) == _lib.TAIL_MAX_ATOMS
    sim0, inblock = _block_rows(b, plan, LS, dev, 13)
    pred, emb, mods = _score_case(b, plan, seg, sim0, inblock, b.num_graphs, "activity", dev)
    want_pred, want_emb = _reference_f64(b, inblock, sim0, mods, b.num_graphs, dev)
    _close(pred, want_pred)
    _close(emb, want_emb)


def test_oversize_molecule_is_loud_in_the_score_kernel():
    """One molecule beyond a chunk: NaN in its prediction and its embedding row, the others as the float64 formula has them."""
    from molkgnn_amd import readout as R
    from molkgnn_amd.plan import plan_from_data
    dev = _dev()
    b = T.batch_of([T.tree(12), T.circulant(130), T.tree(30)], seed=14).to(dev)
    plan = plan_from_data(b)
    seg = R.molecule_segments(b.batch, 3)
    assert not R._tail_limits_ok(seg, plan)
    sim0, inblock = _block_rows(b, plan, LS, dev, 14)
    mods = _modules(dev)
    c = _Call(sim0, plan, seg, mods, 3, torch.zeros(3, device=dev), 0, dev)
    c.score()
    want_pred, want_emb = _reference_f64(b, inblock, sim0, mods, 3, dev)
    assert bool(torch.isnan(c.pred[1])) and bool(torch.isnan(c.emb[1]).all())
    _close(c.pred[[0, 2]], want_pred[[0, 2]])
    _close(c.emb[[0, 2]], want_emb[[0, 2]])


def test_tail_score_refuses_to_drop_a_gradient():
    from molkgnn_amd import readout as R
    from molkgnn_amd.plan import plan_from_data
    from molkgnn_amd.synthetic import make_batch
    dev = _dev()
    b = make_batch(20, seed=3).to(dev)
    plan = plan_from_data(b)
    seg = R.molecule_segments(b.batch, 20)
    lin1, lin2, ffn = _modules(dev)
    sim0, inblock = _block_rows(b, plan, LS, dev, 3)
    with pytest.raises(RuntimeError, match="forward only"):
        R.tail_score(sim0, plan, LS, lin1, lin2, ffn, seg)            # (the parameters require a gradient, grad mode is on)
    with torch.no_grad():
        pred, emb = R.tail_score(sim0, plan, LS, lin1, lin2, ffn, seg, n_rows=17)
    assert pred.shape == (17,) and emb.shape == (20, 32) and not pred.requires_grad and not emb.requires_grad
    want_pred, want_emb = _reference_f64(b, inblock, sim0, (lin1, lin2, ffn), 20, dev)
    _close(pred, want_pred[:17])
    _close(emb, want_emb)


# ------------------------------------------------------------------------------------------------ GNNModel.predict, evaluate --
def _model(dev, seed, bias=True, loss_func=None, ffn_dropout=0.25):
    """The default shape (3 layers, 10/20/30/50 kernels, H = G = 32) with non-trivial running statistics."""
    from molkgnn_amd.train import GNNModel
    torch.manual_seed(seed)
    model = GNNModel(ffn_dropout_rate=ffn_dropout, loss_func=loss_func)
    if not bias:
        model.ffn = torch.nn.Linear(32, 1, bias=False)
    for bn in (model.gnn_model.node_batch_norm, model.gnn_model.edge_batch_norm):
        with torch.no_grad():
            bn.running_mean.normal_(0.0, 0.3)
            bn.running_var.uniform_(0.5, 1.5)
            bn.weight.uniform_(0.5, 1.5)
            bn.bias.normal_(0.0, 0.2)
            bn.num_batches_tracked.fill_(11)
    return model.to(dev)


def _spy(monkeypatch, R, name):
    calls = []
    real = getattr(R, name)
    monkeypatch.setattr(R, name, lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    return calls


def _fallback(model, batch, monkeypatch, R):
    """``model.eval(); model(data)`` on the MKGNN_SCORE_TAIL=0 route (the module flag the variable sets at import)."""
    monkeypatch.setattr(R, "_SCORE_TAIL", False)
    try:
        model.eval()
        with torch.no_grad():
            pred, emb = model(batch)
        torch.cuda.synchronize()
        return pred.clone(), emb.clone()
    finally:
        monkeypatch.setattr(R, "_SCORE_TAIL", True)


@pytest.mark.parametrize("bias", [True, False])
def test_predict_equals_the_separate_operators_and_changes_no_state(bias, monkeypatch):
    from molkgnn_amd import functional as Fn
    from molkgnn_amd import readout as R
    from molkgnn_amd.synthetic import make_batch
    dev = _dev()
    model = _model(dev, 1798, bias).eval()
    b = make_batch(300, seed=61).to(dev)
    want_pred, want_emb = _fallback(model, b, monkeypatch, R)
    R.reset_head_rng(dev, seed=4321)
    rng0 = R.head_rng_state(dev).clone()
    state0 = {k: v.clone() for k, v in model.state_dict().items()}
    scores = _spy(monkeypatch, R, "tail_score")
    separate = _spy(monkeypatch, R, "readout_blocks")
    saved = []
    real_impl = Fn._forward_impl
    monkeypatch.setattr(Fn, "_forward_impl", lambda *a, **k: (saved.append(a[7]), real_impl(*a, **k))[1])
    pred, emb = model.predict(b)
    torch.cuda.synchronize()
    assert len(scores) == 1 and not separate, "predict takes the forward-only tail"
    assert saved == [False] * 3, "no convolution writes pair records under no_grad"
    assert pred.shape == (300, 1) and emb.shape == (300, 32) and not pred.requires_grad
    _close(pred, want_pred)
    _close(emb, want_emb)
    state1 = model.state_dict()
    assert state0.keys() == state1.keys()
    for k, v in state0.items():
        assert torch.equal(v, state1[k]), k
    assert torch.equal(R.head_rng_state(dev), rng0)
    assert not model.training
    # MKGNN_FUSED_TAIL=0 forces the separate operators too
    monkeypatch.setattr(R, "_FUSED_TAIL", False)
    pred2, emb2 = model.predict(b)
    assert len(scores) == 1
    assert torch.equal(pred2, want_pred) and torch.equal(emb2, want_emb)


def test_predict_on_a_padded_batch_returns_the_real_molecules(monkeypatch):
    from molkgnn_amd import padding as P
    from molkgnn_amd import readout as R
    from molkgnn_amd.receptive_field import attach_receptive_fields
    from molkgnn_amd.synthetic import make_batch
    dev = _dev()
    model = _model(dev, 7).eval()
    B = 200
    raw = make_batch(B, seed=4200, with_receptive_fields=False)
    shape = P.fixed_shape([P.degree_histogram(raw), P.degree_histogram(make_batch(B, seed=4201, with_receptive_fields=False))])
    plain = attach_receptive_fields(raw.to(dev))
    padded = attach_receptive_fields(P.pad_batch(raw, shape, B).to(dev), sizes=[shape[f"n{d}"] for d in range(1, 5)])
    scores = _spy(monkeypatch, R, "tail_score")
    pred0, emb0 = model.predict(plain)
    pred1, emb1 = model.predict(padded)
    assert len(scores) == 2
    assert pred1.shape == (B, 1) and emb1.shape == (B, 32)
    want_pred, want_emb = _fallback(model, plain, monkeypatch, R)
    _close(pred0, want_pred)
    _close(pred1, want_pred)
    _close(emb1, want_emb)


def test_predict_falls_back_for_a_molecule_over_the_tail_limit(monkeypatch):
    from molkgnn_amd import readout as R
    dev = _dev()
    model = _model(dev, 9).eval()
    b = T.batch_of([T.tree(12), T.circulant(130), T.tree(30)] + [T.tree(20)] * 8, seed=15).to(dev)
    want_pred, want_emb = _fallback(model, b, monkeypatch, R)
    scores = _spy(monkeypatch, R, "tail_score")
    pred, emb = model.predict(b)
    assert not scores, "a molecule beyond a chunk keeps the separate operators"
    assert bool(torch.isfinite(pred).all())
    _close(pred, want_pred)
    _close(emb, want_emb)


def test_predict_inside_a_deferred_region_leaves_the_training_step_alone():
    """Between ``model.loss`` and ``backward`` of a ``deferred_tail_reduce`` region a reduction is pending on the workspace the
    score tail shares: ``predict`` launches it first, and the step's loss and gradients are bit for bit what they are without."""
    from molkgnn_amd import readout as R
    from molkgnn_amd.synthetic import make_batch
    from molkgnn_amd.train import backward as train_backward
    dev = _dev()
    b = make_batch(600, seed=47).to(dev)
    other = make_batch(1500, seed=48).to(dev)               # (more atoms: its z rows reach beyond the training call's z and d z rows)

    def step(with_predict):
        model = _model(dev, 1798).train()
        R.reset_head_rng(dev, seed=99)
        model.zero_grad(set_to_none=True)
        out = None
        with R.deferred_tail_reduce(dev):
            loss = model.loss(b)
            if with_predict:
                model.eval()
                out = model.predict(other)
                model.train()
            train_backward(loss)
        torch.cuda.synchronize()
        return loss.detach().clone(), {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}, out, model

    l0, g0, _, _ = step(False)
    l1, g1, out, model = step(True)
    assert torch.equal(_bits(l1), _bits(l0))
    assert g0.keys() == g1.keys() and len(g0) > 70
    for n in g0:
        assert torch.equal(_bits(g1[n]), _bits(g0[n])), n
    # ... and the predictions made in the middle are those made outside
    model.eval()
    pred, emb = model.predict(other)
    assert torch.equal(_bits(out[0]), _bits(pred)) and torch.equal(_bits(out[1]), _bits(emb))


@pytest.mark.parametrize("task", ["activity", "docking_score"])
def test_evaluate_over_three_batches_equals_the_fallback_route(task, monkeypatch):
    from molkgnn_amd import evaluation as E
    from molkgnn_amd import readout as R
    from molkgnn_amd.synthetic import make_batch
    from molkgnn_amd.train import evaluate
    dev = _dev()
    regression = task == "docking_score"
    loss_func = torch.nn.MSELoss(reduction="sum") if regression else None
    metrics = ("RMSE",) if regression else ("accuracy", "logAUC_0.001_0.1", "logAUC_0.001_1", "ppv", "f1_score", "AUC")
    model = _model(dev, 21, loss_func=loss_func).train()
    batches = [make_batch(n, seed=70 + n, target=task).to(dev) for n in (300, 150, 40)]
    scores = _spy(monkeypatch, R, "tail_score")
    got = evaluate(model, batches, metrics)
    assert len(scores) == 3 and model.training            # the score tail took every batch; the mode came back
    want_pred = torch.cat([_fallback(model, b, monkeypatch, R)[0].view(-1) for b in batches])
    true_y = torch.cat([b.y.view(-1) for b in batches])
    assert torch.equal(got["true_y"], true_y) and got["pred_y"].shape == (490,)
    _close(got["pred_y"], want_pred)
    _close(got["loss"], model.loss_func(want_pred, true_y.float()))
    table = {"accuracy": E.calculate_accuracy, "RMSE": E.calculate_rmse, "logAUC_0.001_0.1": E.calculate_logAUC,
             "logAUC_0.001_1": lambda y, s: E.calculate_logAUC(y, s, FPR_range=(0.001, 1)), "ppv": E.calculate_ppv,
             "f1_score": E.calculate_f1_score, "AUC": E.calculate_auc}
    same_order = torch.equal(torch.argsort(got["pred_y"], stable=True), torch.argsort(want_pred, stable=True))
    same_calls = torch.equal(got["pred_y"] > 0, want_pred > 0)
    for m in metrics:
        assert got[m] == table[m](got["true_y"], got["pred_y"]), m          # a function of the two vectors alone
        want = table[m](true_y, want_pred)
        print(m, got[m], want)
        if m == "RMSE":
            assert abs(got[m] - want) <= 2e-5 * max(abs(want), float(want_pred.abs().max())), (got[m], want)
        elif (m in ("accuracy", "ppv", "f1_score") and same_calls) or (m in ("AUC", "logAUC_0.001_0.1", "logAUC_0.001_1") and same_order):
            assert got[m] == want, (m, got[m], want)     # functions of the predictions' order / sign only: exactly
