"""The fused tail with a weighted loss (``readout.tail_loss(..., sample_weight= / weight_table= / pos_weight=)`` ->
``_WeightedTailFn``; ``mkgnn_tail_fused_weighted``, csrc/kgnn_tail.hip, template parameter WT): against the separate operators +
the weighted head, against the float64 formula, inside a deferred region, and its bit links to the unweighted tail.
``pytest -m gpu``.  The bounds are ``tests/test_regression_tail.py``'s: ``_close`` (rel 2e-5) and its loss bounds."""
import pytest
import torch
import torch.nn.functional as F

from tests.test_regression_tail import LS, _close, _setup

pytestmark = pytest.mark.gpu

VARIANTS = ("pos", "weights", "table_pos", "mse_weights", "mse_sum_weights")
SHAPES = [(5, 0, 0.0), (300, 7, 0.25), (4096, 0, 0.0), (4096, 0, 0.25)]       # (molecules, padding molecules, head dropout)


def _variant(variant, n_rows, mols, b_y, dev, seed):
    """(loss kind, targets [n_rows], weight keywords of tail_loss / head_loss, the weight of every row [n_rows], pos_weight or None)"""
    g = torch.Generator().manual_seed(seed)
    loss = {"mse_weights": "mse", "mse_sum_weights": "mse_sum"}.get(variant, "bce")
    y = (torch.rand(n_rows, generator=g) < 0.3).float().to(dev) if loss == "bce" else b_y
    s = (0.1 + 2.9 * torch.rand(n_rows, generator=g))
    s[torch.arange(n_rows) % 5 == 2] = 0.0
    pw = torch.tensor([37.5], device=dev) if variant in ("pos", "table_pos") else None
    if variant == "pos":
        return loss, y, dict(pos_weight=pw), torch.ones(n_rows, device=dev), pw
    if variant == "table_pos":
        M = 2 * mols
        ids = torch.randperm(M, generator=g)[torch.arange(mols) // 2 * 2].to(torch.int32)       # repeated ids
        table = torch.full((M,), float("nan"))
        for r in range(n_rows - 1, -1, -1):
            table[ids[r]] = s[r]
        if n_rows >= 8:
            ids[3:n_rows:11] = M + 5                                                             # outside the table: weight 0
        inside = (ids[:n_rows] >= 0) & (ids[:n_rows] < M)
        s_eff = torch.where(inside, table[ids[:n_rows].long().clamp(0, M - 1)], torch.zeros(()))
        return loss, y, dict(weight_table=table.to(dev), row_ids=ids.to(dev), pos_weight=pw), s_eff.to(dev), pw
    # (per molecule, one per slot of the batch: NaN behind the loss molecules, where nothing may read)
    full = torch.cat([s, torch.full((mols - n_rows,), float("nan"))]).to(dev)
    return loss, y, dict(sample_weight=full), s.to(dev), pw


def _params(mods):
    lin1, lin2, ffn = mods
    return list(lin1.parameters()) + list(lin2.parameters()) + list(ffn.parameters())


def _run(how, loss, kw, mods, plan, seg, sim0, inblock, y, n_rows, p_drop, dev):
    """(loss, block-row grad_sim, the six parameter gradients, generator state) of one forward + backward."""
    from molkgnn_amd import readout as R
    from molkgnn_amd.train import backward
    lin1, lin2, ffn = mods
    params = _params(mods)
    R.reset_head_rng(dev, seed=1234)
    for p in params:
        p.grad = None
    sim = sim0.detach().requires_grad_(True)
    if how == "separate":
        emb = R.readout_blocks(sim, plan, LS, lin1, lin2, None, seg)
        out = R.head_loss(emb, ffn, y, loss, dropout_p=p_drop, n_rows=n_rows, **kw)
        out.backward()
    elif how == "deferred":
        with R.deferred_tail_reduce(dev):
            out = R.tail_loss(sim, plan, LS, lin1, lin2, ffn, y, seg, p_drop, n_rows, loss=loss, **kw)
            backward(out)
    else:
        out = R.tail_loss(sim, plan, LS, lin1, lin2, ffn, y, seg, p_drop, n_rows, loss=loss, **kw)
        if kw:
            assert type(out.grad_fn).__name__ == "_WeightedTailFnBackward"
        out.backward()
    torch.cuda.synchronize()
    gsim = torch.where(inblock, sim.grad, torch.zeros((), device=dev))
    return out.detach().clone(), gsim, [p.grad.clone() for p in params], R.head_rng_state(dev).clone()


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("mols,n_pad,p_drop", SHAPES)
def test_weighted_tail_matches_the_separate_operators(variant, mols, n_pad, p_drop):
    dev, b, plan, seg, mods, sim0, inblock, by, n_rows = _setup(mols, n_pad, 161 + mols)
    loss, y, kw, _, _ = _variant(variant, n_rows, mols, by, dev, 7 + mols)
    l0, gs0, gp0, st0 = _run("separate", loss, kw, mods, plan, seg, sim0, inblock, y, n_rows, p_drop, dev)
    l1, gs1, gp1, st1 = _run("fused", loss, kw, mods, plan, seg, sim0, inblock, y, n_rows, p_drop, dev)
    print(f"weighted tail {variant} {mols}/{n_pad}/{p_drop}: loss separate {float(l0)!r} fused {float(l1)!r}")
    assert torch.isfinite(l1) and abs(float(l0) - float(l1)) <= 2e-6 * max(1.0, abs(float(l0))), (float(l0), float(l1))
    _close(gs1, gs0)
    for a, c in zip(gp1, gp0):
        _close(a, c)
    assert torch.equal(st0, st1)
    # bit-reproducible, and the same bits inside a deferred region (the reduction launched later, same order)
    for how in ("fused", "deferred"):
        l2, gs2, gp2, st2 = _run(how, loss, kw, mods, plan, seg, sim0, inblock, y, n_rows, p_drop, dev)
        assert torch.equal(l1, l2) and torch.equal(gs1, gs2) and all(torch.equal(u, v) for u, v in zip(gp1, gp2)), how
        assert torch.equal(st1, st2)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("mols,n_pad", [(5, 0), (300, 7), (4096, 0)])
def test_weighted_tail_against_the_float64_formula(variant, mols, n_pad):
    dev, b, plan, seg, mods, sim0, inblock, by, n_rows = _setup(mols, n_pad, 171 + mols)
    loss, y, kw, s_eff, pw = _variant(variant, n_rows, mols, by, dev, 9 + mols)
    params = _params(mods)
    l1, gs1, gp1, _ = _run("fused", loss, kw, mods, plan, seg, sim0, inblock, y, n_rows, 0.0, dev)
    dense = torch.where(inblock, sim0, torch.zeros((), device=dev)).double().requires_grad_(True)
    p64 = [p.detach().double().requires_grad_(True) for p in params]
    w1, b1, w2, b2, wh, bh = p64
    src, dst = b.edge_index[0], b.edge_index[1]
    h = torch.zeros_like(dense).index_add_(0, dst, dense[src])                       # KernelLayer.py:119-123
    z = h @ w1.t() + b1
    z = z * torch.sigmoid(z)
    z = z @ w2.t() + b2
    emb = torch.zeros(mols, 32, dtype=torch.float64, device=dev).index_add_(0, b.batch, z)     # MolKGNNNet.py:144-146
    pred = (emb[:n_rows] @ wh.t() + bh).view(-1)
    if loss == "bce":
        ref = F.binary_cross_entropy_with_logits(pred, y.double(), weight=s_eff.double(), pos_weight=None if pw is None else pw.double())
    else:
        ref = (s_eff.double() * (pred - y.double()) ** 2).sum()
        if loss == "mse":
            ref = ref / n_rows
    grads = torch.autograd.grad(ref, [dense] + p64)
    print(f"weighted tail {variant} {mols}/{n_pad}: loss {float(l1)!r} float64 {float(ref)!r}")
    assert abs(float(l1) - float(ref)) <= 2e-5 * max(1.0, abs(float(ref))), (float(l1), float(ref))
    _close(gs1, torch.where(inblock, grads[0], torch.zeros((), device=dev, dtype=torch.float64)))
    for g, w in zip(gp1, grads[1:]):
        _close(g, w)


@pytest.mark.parametrize("loss", ["bce", "mse", "mse_sum"])
@pytest.mark.parametrize("p_drop", [0.0, 0.25])
def test_null_and_all_ones_weights_are_the_unweighted_tail_bit_for_bit(loss, p_drop):
    """A ``mkgnn_loss_weights`` whose pointers are all NULL (the unweighted kernels are launched), and sample weights of exactly
    1.0 -- per molecule, and through a table -- on the weighted kernels: ``torch.equal`` to ``tail_loss`` without keywords."""
    from molkgnn_amd import readout as R
    mols, n_pad = 300, 7
    dev, b, plan, seg, mods, sim0, inblock, by, n_rows = _setup(mols, n_pad, 183)
    y = (torch.rand(n_rows, device=dev) < 0.3).float() if loss == "bce" else by
    want = _run("fused", loss, {}, mods, plan, seg, sim0, inblock, y, n_rows, p_drop, dev)
    forms = [dict(sample_weight=torch.ones(mols, device=dev)),
             dict(weight_table=torch.ones(3, device=dev), row_ids=(torch.arange(mols, device=dev) % 3).to(torch.int32))]
    for kw in forms:
        for how in ("fused", "deferred"):
            got = _run(how, loss, kw, mods, plan, seg, sim0, inblock, y, n_rows, p_drop, dev)
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and torch.equal(got[3], want[3]), (kw.keys(), how)
            assert all(torch.equal(u, v) for u, v in zip(got[2], want[2])), (kw.keys(), how)
    # the NULL struct, straight through the operator
    lin1, lin2, ffn = mods
    params = _params(mods)
    R.reset_head_rng(dev, seed=1234)
    for p in params:
        p.grad = None
    sim = sim0.detach().requires_grad_(True)
    out = R._WeightedTailFn.apply(sim, lin1.weight, lin1.bias, lin2.weight, lin2.bias, ffn.weight, ffn.bias, y, seg, plan, tuple(LS),
                                  float(p_drop), n_rows, R.loss_kind(loss), 0.0, None, None, None)
    out.backward()
    torch.cuda.synchronize()
    assert torch.equal(out.detach(), want[0]) and torch.equal(torch.where(inblock, sim.grad, torch.zeros((), device=dev)), want[1])
    assert all(torch.equal(p.grad, v) for p, v in zip(params, want[2])) and torch.equal(R.head_rng_state(dev), want[3])


def test_zero_weights_and_refusals():
    """Molecules of weight 0 hand back an all-zero block-row gradient; ``pos_weight`` with a squared-error kind, a weight that
    requires a gradient and a short weight vector are refused."""
    from molkgnn_amd import readout as R
    mols, n_pad = 300, 7
    dev, b, plan, seg, mods, sim0, inblock, by, n_rows = _setup(mols, n_pad, 191)
    loss, y, kw, s_eff, _ = _variant("weights", n_rows, mols, by, dev, 3)
    _, gsim, _, _ = _run("fused", loss, kw, mods, plan, seg, sim0, inblock, y, n_rows, 0.0, dev)
    dead = torch.cat([s_eff == 0, torch.ones(n_pad, dtype=torch.bool, device=dev)])[b.batch]
    assert bool(dead.any()) and float(gsim[dead].abs().max()) == 0.0 and float(gsim[~dead].abs().max()) > 0.0
    lin1, lin2, ffn = mods
    sim = sim0.detach().requires_grad_(True)
    one = torch.ones(1, device=dev)
    for bad in (dict(loss="mse", pos_weight=one), dict(loss="bce", pos_weight=torch.ones(2, device=dev)),
                dict(loss="bce", sample_weight=torch.ones(mols, device=dev, requires_grad=True)),
                dict(loss="bce", sample_weight=torch.ones(n_rows - 1, device=dev)), dict(loss="bce", weight_table=one)):
        with pytest.raises(ValueError):
            R.tail_loss(sim, plan, LS, lin1, lin2, ffn, y, seg, 0.0, n_rows, **bad)
    # the raw entry point: pos_weight with a squared-error kind, before any launch
    from molkgnn_amd import _lib
    lw = _lib.LossWeights()
    lw.pos_weight = one.data_ptr()
    a = _lib.TailArgs()
    a.loss_kind = _lib.LOSS_SQERR_MEAN
    assert _lib.load().mkgnn_tail_fused_weighted(a, 0.0, lw, None, 0, None) != 0 and _lib.load().mkgnn_last_error()


def test_predict_after_a_deferred_weighted_call_sees_flushed_results():
    """Between ``model.loss`` (the weighted tail, its reduction pending) and ``backward`` of a ``deferred_tail_reduce`` region,
    ``predict`` launches the pending work first: the step's loss and gradients are bit for bit what they are without it, and the
    predictions are those made outside."""
    from molkgnn_amd import readout as R
    from molkgnn_amd.synthetic import make_batch
    from molkgnn_amd.train import GNNModel, backward
    dev = torch.device("cuda:0")
    b = make_batch(600, seed=47).to(dev)
    b.weight = (torch.arange(600, device=dev) % 4).float()
    other = make_batch(1500, seed=48).to(dev)

    def step(with_predict):
        torch.manual_seed(3)
        model = GNNModel(loss_func=torch.nn.BCEWithLogitsLoss(pos_weight=torch.tensor([7.0]))).to(dev).train()
        R.reset_head_rng(dev, seed=99)
        model.zero_grad(set_to_none=True)
        out = None
        with R.deferred_tail_reduce(dev):
            loss = model.loss(b)
            assert type(loss.grad_fn).__name__ == "_WeightedTailFnBackward"
            if with_predict:
                model.eval()
                out = model.predict(other)
                model.train()
            backward(loss)
        torch.cuda.synchronize()
        return loss.detach().clone(), {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}, out, model

    l0, g0, _, _ = step(False)
    l1, g1, out, model = step(True)
    assert torch.equal(l1, l0) and bool(torch.isfinite(l1))
    assert g0.keys() == g1.keys() and len(g0) > 70
    for n in g0:
        assert torch.equal(g1[n], g0[n]), n
    model.eval()
    pred, emb = model.predict(other)
    assert torch.equal(out[0], pred) and torch.equal(out[1], emb)
