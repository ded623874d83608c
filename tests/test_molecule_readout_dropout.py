"""The readout's dropout (MolKGNNNet's ``drop_ratio``, reference MolKGNNNet.py:144-146; the authors train with 0.2) inside the
molecule-resident step (``MKGNN_MOLECULE_READOUT_DROPOUT``): the one-launch step and the forward-only + GRAD_EMB pair against
the per-operator kernels fed the same mask (``readout.readout_dropout_mask``), the same mask as the fused tail, CapturedSteps,
eval mode and the dispatch of ``GNNModel.loss``.  (The file name carries ``test_molecule``: tests/conftest.py leaves the
molecule-resident path on for it.)  ``pytest -m gpu``."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu


def _dev():
    assert torch.cuda.is_available(), "pytest -m gpu needs the MI355X"
    return torch.device("cuda:0")


def _batch(mols, seed, dev):
    from molkgnn_amd.synthetic import make_batch
    b = make_batch(mols, seed=seed)
    b.num_graphs = mols
    b.y = (torch.rand(mols, generator=torch.Generator().manual_seed(seed)) < 0.3).float()
    return b.to(dev)


def _spy_run(monkeypatch, M):
    calls = []
    orig = M._run
    monkeypatch.setattr(M, "_run", lambda *a, **k: (calls.append(a[6]), orig(*a, **k))[1])
    return calls


def _per_operator_with_mask(monkeypatch, M, R, mask_of):
    """The per-operator kernels (no molecule step, no fused tail) whose readout takes ``mask_of(n_atoms)`` as its keep."""
    monkeypatch.setattr(M, "_MODE", "0")
    monkeypatch.setattr(R, "_FUSED_TAIL", False)
    ro, rb = R._ReadoutFn.apply, R._ReadoutBlocksFn.apply
    monkeypatch.setattr(R._ReadoutFn, "apply", lambda h, w1, b1, w2, b2, keep, seg: ro(h, w1, b1, w2, b2, mask_of(h.shape[0]), seg))
    monkeypatch.setattr(R._ReadoutBlocksFn, "apply", lambda sim, w1, b1, w2, b2, keep, seg, plan, blocks:
                        rb(sim, w1, b1, w2, b2, mask_of(sim.shape[0]), seg, plan, blocks))


def _readout_f64(sim, bd, params, keep, head=None, cot=None):
    """float64 autograd of the readout with the dropout mask ``keep`` (MolKGNNNet.py:144-146) on the step's OWN last-layer
    ``sim`` (captured by ``molecule.debug_capture``) -> emb, and with ``head`` = (keep of the head, targets): pred, BCE loss
    (model.py:147-150, 169, 190-198); the gradients of lin1, lin2 (and ffn) for that loss, or for ``(emb * cot).sum()``."""
    p64 = [p.detach().double().requires_grad_(True) for p in params]
    w1, b1, w2, b2 = p64[:4]
    s = sim.double()
    h = torch.zeros_like(s).index_add_(0, bd.edge_index[1], s[bd.edge_index[0]])     # KernelLayer.py:119-123
    z = h @ w1.t() + b1
    z = keep.double() * (z * torch.sigmoid(z))
    z = z @ w2.t() + b2
    emb = torch.zeros(int(bd.batch.max()) + 1, w2.shape[0], dtype=torch.float64, device=s.device).index_add_(0, bd.batch, z)
    if head is None:
        out, pred = (emb * cot.double()).sum(), None
    else:
        hk, y = head
        wh, bh = p64[4:]
        pred = ((emb * hk.double()) @ wh.t() + bh).view(-1)
        out = torch.nn.functional.binary_cross_entropy_with_logits(pred, y.double())
    grads = torch.autograd.grad(out, p64)
    return emb.detach(), None if pred is None else pred.detach(), out.detach(), grads


def _close(got, want, rel=2e-5, what=""):
    err, scale = float((got.double() - want.double()).abs().max()), max(float(want.abs().max()), 1e-6)
    assert err <= rel * scale, (what, err, scale)


def _grads(model):
    return {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}


# (batch seeds: 1017 and 1035 have no molecule above 32 atoms -- the half-size kernel; 819 and 835 have -- the full-size one)
@pytest.mark.parametrize("mols,layers,chunk,seed", [(16, 3, 32, 1017), (16, 3, 64, 819), (32, 3, 64, 835), (16, 4, 32, 1035)])
def test_one_launch_step_against_float64_and_the_per_operator_kernels_with_the_same_mask(mols, layers, chunk, seed, monkeypatch):
    """HEAD | BACKWARD | READOUT_DROPOUT in one launch: emb, pred, loss and the readout's and head's gradients against float64
    of the masked formula on the step's own last-layer rows; the whole network against the per-operator kernels fed the same
    mask (other kernels, other summation orders and possibly other tie choices in the convolutions: the loose bound of
    tests/test_molecule_regression.py)."""
    from molkgnn_amd import _lib
    from molkgnn_amd import molecule as M
    from molkgnn_amd import readout as R
    from molkgnn_amd.train import GNNModel
    from molkgnn_amd.train import backward as train_backward
    from tests import _philox as P
    dev = _dev()
    torch.manual_seed(60 + mols + layers)
    model = GNNModel(num_layers=layers, dropout_ratio=0.2, ffn_dropout_rate=0.25).to(dev).train()
    ref = copy.deepcopy(model)
    bd = _batch(mols, seed, dev)
    monkeypatch.setattr(M, "_MODE", "1")
    plans = []
    build = M.build_molecule_plan                       # chunks of at most 32 atoms (the half-size kernel) or 64
    monkeypatch.setattr(M, "build_molecule_plan", lambda plan, bv, n, cap=None: plans.append(build(plan, bv, n, chunk)) or plans[-1])
    cap = {}
    monkeypatch.setattr(M, "debug_capture", cap)
    calls = _spy_run(monkeypatch, M)
    R.reset_head_rng(dev, seed=55)
    loss = model.loss(bd)
    assert len(plans) == 1 and (plans[0].max_chunk_atoms <= 32) == (chunk == 32), plans[0].max_chunk_atoms
    train_backward(loss)
    torch.cuda.synchronize()
    assert calls == [_lib.MOLECULE_HEAD | _lib.MOLECULE_BACKWARD | _lib.MOLECULE_READOUT_DROPOUT], calls
    assert R.head_rng_state(dev).tolist() == [55, 1]                  # one advance for both masks
    pair = torch.tensor([55, 0], dtype=torch.int64, device=dev)
    n = bd.x.shape[0]
    keep = R.readout_dropout_mask(pair, n, 32, 0.2)
    hk = torch.from_numpy(P.head_mask(55, 0, mols, 32, 0.25)).to(dev)
    g = model.gnn_model
    params = [g.graph_embedding_lin1.weight, g.graph_embedding_lin1.bias, g.graph_embedding_lin2.weight,
              g.graph_embedding_lin2.bias, model.ffn.weight, model.ffn.bias]
    emb64, pred64, loss64, grads64 = _readout_f64(cap["sims"][-1], bd, params, keep, head=(hk, bd.y))
    _close(cap["emb"], emb64, what="emb")
    _close(cap["pred"], pred64, what="pred")
    assert abs(float(loss) - float(loss64)) <= 2e-6 * max(1.0, abs(float(loss64))), (float(loss), float(loss64))
    for p, w in zip(params, grads64):
        _close(p.grad, w, what=tuple(p.shape))
    # (without the readout's mask the float64 embedding is another one: the check above sees the mask)
    emb_nomask = _readout_f64(cap["sims"][-1], bd, params, torch.ones_like(keep), head=(hk, bd.y))[0]
    assert float((emb_nomask - emb64).abs().max()) > 1e-2 * float(emb64.abs().max())
    monkeypatch.setattr(M, "debug_capture", None)
    _per_operator_with_mask(monkeypatch, M, R, lambda k: R.readout_dropout_mask(pair, k, 32, 0.2))
    R.reset_head_rng(dev, seed=55)
    loss_ref = ref.loss(bd)
    loss_ref.backward()
    torch.cuda.synchronize()
    assert len(calls) == 1
    # (the bound of tests/test_molecule_regression.py for three layers; a fourth layer carries the convolutions' differences
    # further: 1.9e-3 measured at 16 molecules)
    assert abs(float(loss) - float(loss_ref)) <= (1e-3 if layers == 3 else 4e-3) * abs(float(loss_ref)), (float(loss), float(loss_ref))
    got, want = _grads(model), _grads(ref)
    assert got.keys() == want.keys() and all(torch.isfinite(v).all() for v in got.values())


@pytest.mark.parametrize("mols", [16, 32])
def test_forward_only_and_grad_emb_backward_redraw_one_mask(mols, monkeypatch):
    """The forward-only call draws the mask and records its pair; the GRAD_EMB backward redraws it from that pair without
    advancing: the embedding and the readout's gradients against float64 of the masked formula."""
    from molkgnn_amd import _lib
    from molkgnn_amd import molecule as M
    from molkgnn_amd import readout as R
    from molkgnn_amd.MolKGNNNet import MolKGNNNet
    dev = _dev()
    names = [f"num_kernel{d}_{h}" for h in ("1hop", "Nhop") for d in range(1, 5)]
    torch.manual_seed(70 + mols)
    net = MolKGNNNet(num_layers=3, x_dim=28, p_dim=3, edge_attr_dim=7, drop_ratio=0.2, graph_embedding_dim=32,
                     **dict(zip(names, (10, 20, 30, 50) * 2))).to(dev).train()
    bd = _batch(mols, 900 + mols, dev)
    cot = torch.randn(mols, 32, generator=torch.Generator().manual_seed(2)).to(dev)
    monkeypatch.setattr(M, "_MODE", "1")
    cap = {}
    monkeypatch.setattr(M, "debug_capture", cap)
    calls = _spy_run(monkeypatch, M)
    R.reset_head_rng(dev, seed=66)
    emb = net(bd)
    assert calls == [_lib.MOLECULE_READOUT_DROPOUT], calls
    sim_fwd = cap["sims"][-1].clone()
    (emb * cot).sum().backward()
    torch.cuda.synchronize()
    assert calls == [_lib.MOLECULE_READOUT_DROPOUT, _lib.MOLECULE_BACKWARD | _lib.MOLECULE_GRAD_EMB | _lib.MOLECULE_READOUT_DROPOUT]
    assert R.head_rng_state(dev).tolist() == [66, 1]                  # the forward advanced, the backward did not
    assert torch.equal(cap["emb"], emb.detach())                      # the backward's recomputed forward: the same bits
    keep = R.readout_dropout_mask(torch.tensor([66, 0], dtype=torch.int64, device=dev), bd.x.shape[0], 32, 0.2)
    params = [net.graph_embedding_lin1.weight, net.graph_embedding_lin1.bias, net.graph_embedding_lin2.weight,
              net.graph_embedding_lin2.bias]
    emb64, _, _, grads64 = _readout_f64(sim_fwd, bd, params, keep, cot=cot)
    _close(emb, emb64, what="emb")
    for p, w in zip(params, grads64):
        _close(p.grad, w, what=tuple(p.shape))
    assert all(p.grad is None or torch.isfinite(p.grad).all() for p in net.parameters())


@pytest.mark.parametrize("p_head", [0.0, 0.25])
def test_molecule_step_and_fused_tail_draw_the_same_mask(p_head, monkeypatch):
    """One batch, one generator state: the fused tail fed the molecule step's own last-layer rows gives the molecule step's loss
    and readout gradients to rounding -- both draw the same readout (and head) mask."""
    from molkgnn_amd import molecule as M
    from molkgnn_amd import readout as R
    from molkgnn_amd.plan import plan_from_data
    from molkgnn_amd.train import GNNModel
    dev = _dev()
    torch.manual_seed(5)
    model = GNNModel(dropout_ratio=0.5, ffn_dropout_rate=p_head).to(dev).train()
    bd = _batch(16, 1616, dev)
    monkeypatch.setattr(M, "_MODE", "1")
    cap = {}
    monkeypatch.setattr(M, "debug_capture", cap)
    R.reset_head_rng(dev, seed=8)
    l_mol = model.loss(bd)
    l_mol.backward()
    torch.cuda.synchronize()
    g = model.gnn_model
    mods = (g.graph_embedding_lin1, g.graph_embedding_lin2, model.ffn)
    params = [p for m in mods for p in m.parameters()]
    g_mol = [p.grad.clone() for p in params]
    for p in params:
        p.grad = None
    Ls = tuple(g.gnn.layers[-1].L)
    K = sum(Ls)
    store = torch.zeros(bd.x.shape[0], K + (-K) % 4, device=dev)
    store[:, :K] = cap["sims"][-1]
    sim = store[:, :K].requires_grad_(True)
    plan = plan_from_data(bd)
    seg = R.molecule_segments(bd.batch, 16)
    assert R._tail_limits_ok(seg, plan)
    R.reset_head_rng(dev, seed=8)
    l_tail = R.tail_loss(sim, plan, Ls, *mods, bd.y, seg, p_head, 16, readout_dropout_p=0.5)
    l_tail.backward()
    torch.cuda.synchronize()
    assert abs(float(l_mol) - float(l_tail)) <= 2e-6 * max(1.0, abs(float(l_tail))), (float(l_mol), float(l_tail))
    for p, w in zip(params, g_mol):
        _close(p.grad, w, what=tuple(p.shape))
    assert R.head_rng_state(dev).tolist() == [8, 1]
    R.reset_head_rng(dev, seed=9)                                      # another pair: another mask, another loss
    for p in params:
        p.grad = None
    l_other = R.tail_loss(sim, plan, Ls, *mods, bd.y, seg, p_head, 16, readout_dropout_p=0.5)
    assert abs(float(l_other) - float(l_tail)) > 1e-4 * max(1.0, abs(float(l_tail)))


def test_captured_steps_replay_the_eager_steps_bit_for_bit():
    from molkgnn_amd import readout as R
    from molkgnn_amd.train import CapturedSteps, GNNModel, backward as train_backward, configure_optimizer
    dev = _dev()
    torch.manual_seed(22)
    model = GNNModel(num_layers=4, dropout_ratio=0.2, ffn_dropout_rate=0.25).to(dev).train()
    twin = copy.deepcopy(model)
    batches = [_batch(16, 310 + i, dev) for i in range(2)]
    opt, opt_t = configure_optimizer(model, lr=1e-3, fused=True), configure_optimizer(twin, lr=1e-3, fused=True)
    R.reset_head_rng(dev, seed=4)
    eager = []
    for _ in range(4):
        for b in batches:
            twin.zero_grad(set_to_none=True)
            lt = twin.loss(b)
            train_backward(lt)
            opt_t.step()
            eager.append(lt.detach().clone())
    torch.cuda.synchronize()
    st_eager = R.head_rng_state(dev).clone()
    R.reset_head_rng(dev, seed=4)
    steps = CapturedSteps(model, opt)
    replayed = [steps(b).detach().clone() for _ in range(4) for b in batches]
    torch.cuda.synchronize()
    assert len(steps._graphs) == 2
    assert st_eager.tolist() == [4, 8] and torch.equal(R.head_rng_state(dev), st_eager)
    assert all(torch.equal(a, c) for a, c in zip(eager, replayed)), [(float(a), float(c)) for a, c in zip(eager, replayed)]
    for (nm, p), (_, q) in zip(model.named_parameters(), twin.named_parameters()):
        assert torch.equal(p, q), nm


def test_eval_mode_ignores_the_drop_ratio(monkeypatch):
    from molkgnn_amd import molecule as M
    from molkgnn_amd.train import GNNModel
    dev = _dev()
    monkeypatch.setattr(M, "_MODE", "1")
    bd = _batch(16, 77, dev)
    out = []
    for p in (0.0, 0.2):
        torch.manual_seed(9)
        model = GNNModel(dropout_ratio=p).to(dev).eval()
        calls = _spy_run(monkeypatch, M)
        with torch.no_grad():
            emb = model.gnn_model(bd)
            loss = model.loss(bd)
        assert calls and all(c & 32 == 0 for c in calls), calls
        out.append((emb.clone(), loss.clone()))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])


@pytest.mark.parametrize("drop_ratio", [0.2, 1.0])
def test_model_loss_takes_the_molecule_step_with_readout_dropout(drop_ratio, monkeypatch):
    """GNNModel(dropout_ratio=0.2).loss in training mode at 16 molecules: the one-launch step (_MoleculeLossFn); p = 1 keeps
    the per-operator route."""
    from molkgnn_amd import molecule as M
    from molkgnn_amd.train import GNNModel
    dev = _dev()
    torch.manual_seed(13)
    model = GNNModel(dropout_ratio=drop_ratio).to(dev).train()
    bd = _batch(16, 1313, dev)
    taken = []
    real = M._MoleculeLossFn.apply
    monkeypatch.setattr(M._MoleculeLossFn, "apply", lambda *a: (taken.append(a[8]), real(*a))[1])
    loss = model.loss(bd)
    loss.backward()
    torch.cuda.synchronize()
    assert torch.isfinite(loss)
    assert taken == ([drop_ratio] if drop_ratio < 1.0 else []), taken
