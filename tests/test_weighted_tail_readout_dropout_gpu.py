"""The weighted fused tail together with the readout's dropout (``readout.tail_loss(..., readout_dropout_p=..., sample_weight= /
pos_weight= / weight_table=)`` -> ``mkgnn_tail_fused_weighted`` with ``readout_dropout_p > 0``: the instantiations
``tail_middle_kernel<LK, RD = true, FWD = false, WT = true>``, csrc/kgnn_tail.hip): against the separate operators fed the same
mask (``readout.readout_dropout_mask``) + the weighted head, against float64, inside a deferred region, the generator state, and
the bit links to ``mkgnn_tail_fused_readout_dropout``.  ``pytest -m gpu``.  Bounds: ``tests/test_readout_dropout_tail.py``'s."""
import pytest
import torch
import torch.nn.functional as F

from tests.test_readout_dropout_tail import LS, _close, _params, _setup

pytestmark = pytest.mark.gpu

P_RO = 0.25
VARIANTS = {"bce": ("weights_pos", "table_pos", "pos", "weights"), "mse": ("weights", "table"), "mse_sum": ("weights", "table")}
CASES = [(k, v) for k, vs in VARIANTS.items() for v in vs]


def _weights(variant, n_rows, mols, dev, seed):
    """(weight keywords of tail_loss / head_loss, the weight of every loss molecule [n_rows], pos_weight or None)"""
    g = torch.Generator().manual_seed(seed)
    s = 0.1 + 2.9 * torch.rand(n_rows, generator=g)
    s[torch.arange(n_rows) % 5 == 2] = 0.0
    pw = torch.tensor([37.5], device=dev) if "pos" in variant else None
    kw = {} if pw is None else dict(pos_weight=pw)
    if variant == "pos":
        return kw, torch.ones(n_rows, device=dev), pw
    if variant.startswith("table"):
        M = 2 * mols
        ids = torch.randperm(M, generator=g)[torch.arange(mols) // 2 * 2].to(torch.int32)       # repeated ids
        table = torch.full((M,), float("nan"))
        for r in range(n_rows - 1, -1, -1):
            table[ids[r]] = s[r]
        ids[3:n_rows:11] = M + 5                                                                 # outside the table: weight 0
        inside = (ids[:n_rows] >= 0) & (ids[:n_rows] < M)
        s_eff = torch.where(inside, table[ids[:n_rows].long().clamp(0, M - 1)], torch.zeros(()))
        return dict(kw, weight_table=table.to(dev), row_ids=ids.to(dev)), s_eff.to(dev), pw
    full = torch.cat([s, torch.full((mols - n_rows,), float("nan"))]).to(dev)                    # (NaN behind the loss molecules)
    return dict(kw, sample_weight=full), s.to(dev), pw


def _run(how, kind, kw, mods, plan, seg, sim0, inblock, y, n_rows, p_head, p_ro, dev, seed=1234):
    """(loss, block-row grad_sim, the six parameter gradients, generator state after) of one forward + backward."""
    from molkgnn_amd import readout as R
    from molkgnn_amd.train import backward
    lin1, lin2, ffn = mods
    params = _params(mods)
    R.reset_head_rng(dev, seed=seed)
    for p in params:
        p.grad = None
    sim = sim0.detach().requires_grad_(True)
    if how == "separate":
        keep = R.readout_dropout_mask(R.head_rng_state(dev).clone(), sim.shape[0], 32, p_ro)
        emb = R._ReadoutBlocksFn.apply(sim, lin1.weight, lin1.bias, lin2.weight, lin2.bias, keep, seg, plan, LS)
        out = R.head_loss(emb, ffn, y, kind, dropout_p=p_head, n_rows=n_rows, **kw)
        out.backward()
        if p_head == 0.0:                                       # (the fused paths advance once for either dropout)
            R.head_rng_state(dev)[1] += 1
    elif how == "deferred":
        with R.deferred_tail_reduce(dev):
            out = R.tail_loss(sim, plan, LS, lin1, lin2, ffn, y, seg, p_head, n_rows, loss=kind, readout_dropout_p=p_ro, **kw)
            backward(out)
    else:
        out = R.tail_loss(sim, plan, LS, lin1, lin2, ffn, y, seg, p_head, n_rows, loss=kind, readout_dropout_p=p_ro, **kw)
        assert type(out.grad_fn).__name__ == ("_WeightedTailFnBackward" if kw else "_TailFnBackward")
        out.backward()
    torch.cuda.synchronize()
    gsim = torch.where(inblock, sim.grad, torch.zeros((), device=dev))
    return out.detach().clone(), gsim, [p.grad.clone() for p in params], R.head_rng_state(dev).clone()


@pytest.mark.parametrize("kind,variant", CASES)
@pytest.mark.parametrize("p_head", [0.0, 0.25])
@pytest.mark.parametrize("mols,n_pad", [(300, 7), (4096, 0)])
def test_weighted_tail_with_readout_dropout_matches_the_separate_operators(kind, variant, p_head, mols, n_pad):
    dev, b, plan, seg, mods, sim0, inblock, y, n_rows = _setup(mols, n_pad, 600 + n_pad, kind)
    kw, _, _ = _weights(variant, n_rows, mols, dev, 11 + mols)
    l0, gs0, gp0, st0 = _run("separate", kind, kw, mods, plan, seg, sim0, inblock, y, n_rows, p_head, P_RO, dev)
    l1, gs1, gp1, st1 = _run("fused", kind, kw, mods, plan, seg, sim0, inblock, y, n_rows, p_head, P_RO, dev)
    print(f"weighted tail + readout dropout {kind} {variant} {mols}/{n_pad}/{p_head}: separate {float(l0)!r} fused {float(l1)!r}")
    assert torch.isfinite(l1) and abs(float(l0) - float(l1)) <= 2e-6 * max(1.0, abs(float(l0))), (float(l0), float(l1))
    _close(gs1, gs0)
    for a, c in zip(gp1, gp0):
        _close(a, c)
    assert st1.tolist() == [1234, 1] and torch.equal(st0, st1)          # advanced by exactly one, as the unweighted call
    for how in ("fused", "deferred"):                                   # the same bits again, and inside a deferred region
        l2, gs2, gp2, st2 = _run(how, kind, kw, mods, plan, seg, sim0, inblock, y, n_rows, p_head, P_RO, dev)
        assert torch.equal(l1, l2) and torch.equal(gs1, gs2) and all(torch.equal(u, v) for u, v in zip(gp1, gp2)), how
        assert torch.equal(st1, st2)


@pytest.mark.parametrize("kind,variant", [("bce", "weights_pos"), ("bce", "table_pos"), ("mse", "weights"), ("mse_sum", "table")])
def test_weighted_tail_with_readout_dropout_against_float64(kind, variant):
    from molkgnn_amd import readout as R
    mols = 1000
    dev, b, plan, seg, mods, sim0, inblock, y, n_rows = _setup(mols, 9, 93, kind)
    kw, s_eff, pw = _weights(variant, n_rows, mols, dev, 5)
    l1, gs1, gp1, _ = _run("fused", kind, kw, mods, plan, seg, sim0, inblock, y, n_rows, 0.0, P_RO, dev, seed=31)
    keep = R.readout_dropout_mask(torch.tensor([31, 0], dtype=torch.int64, device=dev), sim0.shape[0], 32, P_RO).double()
    dense = torch.where(inblock, sim0, torch.zeros((), device=dev)).double().requires_grad_(True)
    p64 = [p.detach().double().requires_grad_(True) for p in _params(mods)]
    w1, b1, w2, b2, wh, bh = p64
    src, dst = b.edge_index[0], b.edge_index[1]
    h = torch.zeros_like(dense).index_add_(0, dst, dense[src])                       # KernelLayer.py:119-123
    z = h @ w1.t() + b1
    z = keep * (z * torch.sigmoid(z))                                                # MolKGNNNet.py:144-146 with the dropout
    z = z @ w2.t() + b2
    emb = torch.zeros(mols, 32, dtype=torch.float64, device=dev).index_add_(0, b.batch, z)
    pred = (emb[:n_rows] @ wh.t() + bh).view(-1)
    if kind == "bce":
        ref = F.binary_cross_entropy_with_logits(pred, y.double(), weight=s_eff.double(), pos_weight=None if pw is None else pw.double())
    else:
        ref = (s_eff.double() * (pred - y.double()) ** 2).sum()
        if kind == "mse":
            ref = ref / n_rows
    grads = torch.autograd.grad(ref, [dense] + p64)
    print(f"weighted tail + readout dropout {kind} {variant}: loss {float(l1)!r} float64 {float(ref.detach())!r}")
    assert abs(float(l1) - float(ref.detach())) <= 2e-5 * max(1.0, abs(float(ref.detach()))), (float(l1), float(ref.detach()))
    _close(gs1, torch.where(inblock, grads[0], torch.zeros((), device=dev, dtype=torch.float64)))
    for g, w in zip(gp1, grads[1:]):
        _close(g, w)


@pytest.mark.parametrize("kind", ["bce", "mse", "mse_sum"])
@pytest.mark.parametrize("p_head", [0.0, 0.25])
def test_null_and_all_ones_weights_are_the_readout_dropout_tail_bit_for_bit(kind, p_head):
    """At ``readout_dropout_p = 0.25``: a ``mkgnn_loss_weights`` whose pointers are all NULL (``mkgnn_tail_fused_readout_dropout``'s
    own kernels), and sample weights of exactly 1.0 per molecule and through a table (the weighted kernels): loss, block-row
    gradient, the six parameter gradients and the generator state of ``tail_loss(..., readout_dropout_p=0.25)`` without keywords."""
    from molkgnn_amd import readout as R
    mols, n_pad = 300, 7
    dev, b, plan, seg, mods, sim0, inblock, y, n_rows = _setup(mols, n_pad, 611, kind)
    want = _run("fused", kind, {}, mods, plan, seg, sim0, inblock, y, n_rows, p_head, P_RO, dev)
    assert want[3].tolist() == [1234, 1]
    forms = [dict(sample_weight=torch.ones(mols, device=dev)),
             dict(weight_table=torch.ones(3, device=dev), row_ids=(torch.arange(mols, device=dev) % 3).to(torch.int32))]
    for kw in forms:
        for how in ("fused", "deferred"):
            got = _run(how, kind, kw, mods, plan, seg, sim0, inblock, y, n_rows, p_head, P_RO, dev)
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and torch.equal(got[3], want[3]), (list(kw), how)
            assert all(torch.equal(u, v) for u, v in zip(got[2], want[2])), (list(kw), how)
    lin1, lin2, ffn = mods
    params = _params(mods)
    R.reset_head_rng(dev, seed=1234)
    for p in params:
        p.grad = None
    sim = sim0.detach().requires_grad_(True)
    out = R._WeightedTailFn.apply(sim, lin1.weight, lin1.bias, lin2.weight, lin2.bias, ffn.weight, ffn.bias, y, seg, plan, tuple(LS),
                                  float(p_head), n_rows, R.loss_kind(kind), P_RO, None, None, None)
    out.backward()
    torch.cuda.synchronize()
    assert torch.equal(out.detach(), want[0]) and torch.equal(torch.where(inblock, sim.grad, torch.zeros((), device=dev)), want[1])
    assert all(torch.equal(p.grad, v) for p, v in zip(params, want[2])) and torch.equal(R.head_rng_state(dev), want[3])


def test_model_with_readout_dropout_and_weights_takes_the_weighted_tail():
    """``GNNModel(dropout_ratio=0.2, loss_func=BCEWithLogitsLoss(pos_weight=...))`` on a batch with weights, in training mode: the
    weighted tail with the readout's dropout inside it; one generator advance; the same bits from the same seed."""
    from molkgnn_amd import readout as R
    from molkgnn_amd.synthetic import make_batch
    from molkgnn_amd.train import GNNModel, backward
    dev = torch.device("cuda:0")
    b = make_batch(64, seed=23).to(dev)
    b.weight = (torch.arange(64, device=dev) % 5).float() * 0.5
    torch.manual_seed(2)
    model = GNNModel(dropout_ratio=0.2, loss_func=torch.nn.BCEWithLogitsLoss(pos_weight=torch.tensor([7.0]))).to(dev).train()
    seen = []
    for _ in range(2):
        R.reset_head_rng(dev, seed=55)
        model.zero_grad(set_to_none=True)
        loss = model.loss(b)
        assert type(loss.grad_fn).__name__ == "_WeightedTailFnBackward"
        backward(loss)
        torch.cuda.synchronize()
        assert R.head_rng_state(dev).tolist() == [55, 1]
        seen.append([loss.detach().clone()] + [p.grad.clone() for p in model.parameters() if p.grad is not None])
    assert bool(torch.isfinite(seen[0][0])) and len(seen[0]) > 70
    assert all(torch.equal(u, v) for u, v in zip(*seen))
