"""State that outlives one call: the fused tail's deferred reduction (``readout.deferred_tail_reduce``), the padding
``padding.pad_batch`` deals to the tail kernel, the ``KernelSetConv._bank_params`` cache and ``train.CapturedSteps``' visit
counts.  ``pytest -m gpu``.

Each stateful path is compared with the plain one -- the same model and batch through ``model.loss`` + ``train.backward``
outside any region, the same kernels, so bit for bit unless a case says otherwise -- or with the float64 oracle.  The
conftest's NaN-filled free memory makes a read of a gradient nobody has written yet visible.
"""
import gc

import pytest
import torch

pytestmark = pytest.mark.gpu

HOOKED = ("gnn_model.graph_embedding_lin1.weight", "gnn_model.graph_embedding_lin2.bias", "ffn.weight")


def _dev():
    assert torch.cuda.is_available(), "pytest -m gpu needs the MI355X"
    return torch.device("cuda:0")


def _fresh(dev, seed=1798, rng=99):
    from molkgnn_amd import readout as R
    from molkgnn_amd.train import GNNModel
    torch.manual_seed(seed)
    model = GNNModel(ffn_dropout_rate=0.25).to(dev).train()
    R.reset_head_rng(dev, seed=rng)
    return model


def _grads(model):
    return {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}


def _plain(model, batch):
    """The plain path: loss -> backward outside any deferred region."""
    from molkgnn_amd.train import backward
    model.zero_grad(set_to_none=True)
    loss = model.loss(batch)
    backward(loss)
    torch.cuda.synchronize()
    return loss.detach().clone(), _grads(model)


def _spy_tail(monkeypatch):
    from molkgnn_amd import readout as R
    calls = []
    real = R.tail_loss

    def spy(*a, **k):
        calls.append(1)
        return real(*a, **k)
    monkeypatch.setattr(R, "tail_loss", spy)
    return calls


def _noncontiguous_lin1(model):
    lin1 = model.gnn_model.graph_embedding_lin1
    w = lin1.weight.detach()
    lin1.weight = torch.nn.Parameter(w.t().contiguous().t())
    assert not lin1.weight.is_contiguous() and torch.equal(lin1.weight, w)


# ------------------------------------------------------------------------------------------------------------- 1 --
@pytest.mark.parametrize("case", ["post_accumulate_hook", "tensor_hook", "noncontiguous_parameter"])
def test_deferred_tail_with_hooks_or_a_cloning_accumulate_grad(case, monkeypatch):
    """``train.training_step`` defers the tail's last reduction only where autograd adopts its six gradients untouched: a
    post-accumulate hook or a tensor hook on a tail parameter reads them in the backward, and a non-contiguous parameter makes
    AccumulateGrad copy them into its strides -- all before the deferred reduction would have written them.  Every hook
    snapshot and every ``.grad`` is bit for bit the plain path's."""
    from molkgnn_amd.synthetic import make_batch
    from molkgnn_amd.train import training_step
    dev = _dev()
    b = make_batch(600, seed=47).to(dev)
    calls = _spy_tail(monkeypatch)

    model = _fresh(dev)
    if case == "noncontiguous_parameter":
        _noncontiguous_lin1(model)
    l_ref, g_ref = _plain(model, b)
    assert calls == [1]                                   # (the fused tail takes this batch)
    p_ref = None
    if case == "noncontiguous_parameter":
        opt = torch.optim.AdamW(model.parameters(), lr=1e-3)
        opt.step()
        torch.cuda.synchronize()
        p_ref = {n: p.detach().clone() for n, p in model.named_parameters()}

    model = _fresh(dev)
    params = dict(model.named_parameters())
    snaps = {}
    if case == "post_accumulate_hook":
        for n in HOOKED:
            params[n].register_post_accumulate_grad_hook(lambda p, n=n: snaps.__setitem__(n, p.grad.clone()))
    elif case == "tensor_hook":
        for n in HOOKED:
            params[n].register_hook(lambda g, n=n: snaps.setdefault(n, g.clone()))
    else:
        _noncontiguous_lin1(model)
        opt = torch.optim.AdamW(model.parameters(), lr=1e-3)
    loss = training_step(model, b)
    torch.cuda.synchronize()
    assert len(calls) == 2
    assert torch.equal(loss, l_ref), (float(loss), float(l_ref))
    g = _grads(model)
    assert g.keys() == g_ref.keys()
    for n in g_ref:
        assert torch.equal(g[n], g_ref[n]), n
    if case != "noncontiguous_parameter":
        assert snaps.keys() == set(HOOKED)
        for n, s in snaps.items():
            assert torch.equal(s, g_ref[n]), n
    else:
        assert not model.gnn_model.graph_embedding_lin1.weight.grad.is_contiguous()    # (AccumulateGrad copied: its strides)
        opt.step()
        torch.cuda.synchronize()
        for n, p in model.named_parameters():
            assert torch.equal(p.detach(), p_ref[n]), n
        # the fused AdamW takes contiguous parameters only, and says so (it does not update a wrong element order)
        from molkgnn_amd._lib import MolKGNNLibraryError
        from molkgnn_amd.train import configure_optimizer
        with pytest.raises(MolKGNNLibraryError, match="contiguous"):
            configure_optimizer(model, lr=1e-3).step()


# ------------------------------------------------------------------------------------------------------------- 2 --
def test_two_tail_calls_in_one_deferred_region(monkeypatch):
    """Two ``model.loss`` calls in one region before any backward: the first call's reduction, still pending, is launched in front
    of the second call's kernels -- which overwrite the tail's workspace slabs and read the dropout generator it advances.  The
    losses are bit for bit the plain path's (same order), and so is the generator state afterwards; the gradients agree to
    rounding (one backward of the sum seeds the tail with a non-unit gradient and scales)."""
    from molkgnn_amd import readout as R
    from molkgnn_amd.synthetic import make_batch
    dev = _dev()
    b1, b2 = make_batch(600, seed=47).to(dev), make_batch(640, seed=48).to(dev)
    calls = _spy_tail(monkeypatch)

    model = _fresh(dev)
    model.zero_grad(set_to_none=True)
    l1, l2 = model.loss(b1), model.loss(b2)
    (l1 + l2).backward()
    torch.cuda.synchronize()
    ref = (l1.detach().clone(), l2.detach().clone(), R.head_rng_state(dev).clone(), _grads(model))
    assert len(calls) == 2

    model = _fresh(dev)
    model.zero_grad(set_to_none=True)
    with R.deferred_tail_reduce(dev):
        l1, l2 = model.loss(b1), model.loss(b2)
        (l1 + l2).backward()
    torch.cuda.synchronize()
    assert len(calls) == 4
    assert torch.equal(l1, ref[0]) and torch.equal(l2, ref[1]), (float(l1), float(ref[0]), float(l2), float(ref[1]))
    assert torch.equal(R.head_rng_state(dev), ref[2])
    g = _grads(model)
    assert g.keys() == ref[3].keys()
    for n, want in ref[3].items():
        assert float((g[n] - want).abs().max()) <= 2e-5 * max(float(want.abs().max()), 1e-3) + 1e-7, n


def test_two_loss_backward_pairs_in_one_deferred_region(monkeypatch):
    """Two loss -> backward pairs in one region, kernel banks frozen, batch norm trainable, the registered unit seed: the first
    pair's reduction stays pending through its backward (unit seed, no ``.grad`` yet) and is launched either by a convolution
    backward's helper stream or in front of the second tail call.  Both losses and both sets of gradients are bit for bit the
    plain path's."""
    from molkgnn_amd import readout as R
    from molkgnn_amd.synthetic import make_batch
    dev = _dev()
    b1, b2 = make_batch(600, seed=47).to(dev), make_batch(600, seed=48).to(dev)
    calls = _spy_tail(monkeypatch)
    one = torch.ones((), device=dev)
    R.register_unit_gradient(one)

    def backward(loss):
        loss.backward(one)

    def frozen():
        model = _fresh(dev)
        for n, p in model.named_parameters():
            if "kernelconv_set" in n:
                p.requires_grad_(False)
        assert any(p.requires_grad for n, p in model.named_parameters() if "batch_norm" in n)
        return model

    def plain(model, b):
        model.zero_grad(set_to_none=True)
        loss = model.loss(b)
        backward(loss)
        torch.cuda.synchronize()
        return loss.detach().clone(), _grads(model)

    model = frozen()
    ref = [plain(model, b1), plain(model, b2)]
    assert len(calls) == 2
    assert not any("kernelconv_set" in n for n in ref[0][1])

    model = frozen()
    got = []
    model.zero_grad(set_to_none=True)
    with R.deferred_tail_reduce(dev):
        for b in (b1, b2):
            loss = model.loss(b)
            backward(loss)
            got.append((loss, {n: p.grad for n, p in model.named_parameters() if p.grad is not None}))   # (read after the region)
            model.zero_grad(set_to_none=True)
    torch.cuda.synchronize()
    assert len(calls) == 4
    for (loss, g), (l_ref, g_ref) in zip(got, ref):
        assert torch.equal(loss, l_ref), (float(loss), float(l_ref))
        assert g.keys() == g_ref.keys()
        for n in g_ref:
            assert torch.equal(g[n], g_ref[n]), n


# ------------------------------------------------------------------------------------------------------------- 3 --
# padding per degree (n1, n2, n3, n4) for a total of n_pad atoms; the padding's bond stubs pair up (an even stub count)
PADS = {0: (0, 0, 0, 0), 1: (0, 1, 0, 0), 2: (2, 0, 0, 0), 7: (6, 1, 0, 0), 63: (62, 1, 0, 0), 64: (64, 0, 0, 0),
        65: (64, 1, 0, 0)}


def _tail_group_size(n_loss):
    """kgnn_tail.hip ``tail_group_size``: molecules per group, from the number of real molecules (TAIL_MAX_BLOCKS = 768)."""
    return min(max((n_loss + 768 - 1) // 768, 1), 8)


def test_fused_tail_with_fewer_padding_atoms_than_padding_molecules(monkeypatch):
    """``pad_batch`` deals ``n_pad`` padding atoms to 64 padding molecules: with ``n_pad < 64`` some of them are empty, and a group
    of the tail kernel can hold no atom at all (the empty molecules trail the batch: its first atom is one past the last).  For
    every ``n_pad`` the loss is bit for bit the unpadded batch's and every gradient agrees to rounding."""
    from molkgnn_amd import padding as P
    from molkgnn_amd import readout as R
    from molkgnn_amd.receptive_field import attach_receptive_fields
    from molkgnn_amd.synthetic import make_batch
    dev = _dev()
    B = 700
    raw = make_batch(B, seed=4100, with_receptive_fields=False)
    raw.y = (torch.arange(B) % 5 == 0).long()
    h = P.degree_histogram(raw)
    assert h[5] == 0
    calls = _spy_tail(monkeypatch)
    mg = _tail_group_size(B)

    def run(batch):
        model = _fresh(dev, seed=3, rng=11)
        model.zero_grad(set_to_none=True)
        loss = model.loss(batch)
        loss.backward()
        torch.cuda.synchronize()
        return loss.detach().clone(), _grads(model)

    l_ref, g_ref = run(attach_receptive_fields(raw.to(dev)))
    for n_pad, pad in PADS.items():
        assert sum(pad) == n_pad
        t = [h[d] + pad[d - 1] for d in range(1, 5)]
        shape = {"n1": t[0], "n2": t[1], "n3": t[2], "n4": t[3], "atoms": sum(t),
                 "edges": sum(d * t[d - 1] for d in range(1, 5))}
        padded = P.pad_batch(raw, shape, B)
        ptr = padded.mol_ptr.long()
        n_mols = ptr.numel() - 1
        empty_groups = [g for g in range((n_mols + mg - 1) // mg) if ptr[min((g + 1) * mg, n_mols)] == ptr[g * mg]]
        if n_pad < P.PAD_MOLECULES:
            assert empty_groups, n_pad                    # the A == 0 chunk really occurs
            assert int(ptr[empty_groups[-1] * mg]) == shape["atoms"]    # ... at the very end of the atoms
        else:
            assert not empty_groups, n_pad
        n_calls = len(calls)
        loss, g = run(attach_receptive_fields(padded.to(dev), sizes=t))
        assert len(calls) == n_calls + 1, n_pad           # through the fused tail
        assert torch.equal(loss, l_ref), (n_pad, float(loss), float(l_ref))
        assert g.keys() == g_ref.keys()
        for n, want in g_ref.items():
            assert float((g[n] - want).abs().max()) <= 2e-5 * max(float(want.abs().max()), 1e-3) + 1e-7, (n_pad, n)


# ------------------------------------------------------------------------------------------------------------- 4 --
OP_PARAM_NAMES = ("x_center", "x_support", "edge_attr_support", "p_support", "support_attr_sc_weight", "center_attr_sc_weight",
                  "edge_attr_support_sc_weight")


@pytest.mark.parametrize("name", OP_PARAM_NAMES)
def test_reassigned_bank_parameter_reaches_the_kernels(name):
    """A layer at the benchmark banks (10, 20, 30, 50; the last layer, whose degree-4 scores also read ``p_support``) whose
    degree-4 ``name`` is re-assigned after a first forward: the forward and all 25 gradients follow the NEW values (the oracle's
    float64 replay, at tests/test_scale_parity.py's tolerances), the new Parameter receives the gradient, the old one none."""
    from oracle import kgnn_oracle as O
    from molkgnn_amd.kernels import KernelSetConv
    from molkgnn_amd.plan import plan_from_data
    from molkgnn_amd.synthetic import make_batch
    from tests.test_scale_parity import FWD_TOL, _check_gradients, _run_build
    dev = _dev()
    width, last = 110, True
    cpu = make_batch(160, seed=2024)
    bd = cpu.to(dev)
    plan = plan_from_data(bd)
    torch.manual_seed(31)
    layer = KernelSetConv(10, 20, 30, 50, D=3, node_attr_dim=width, edge_attr_dim=7).to(dev)
    n = cpu.x.shape[0]
    g = torch.Generator().manual_seed(7)
    x_cpu = torch.randn(n, width, generator=g)
    cot_cpu = torch.randn(n, 110, generator=g)
    store = torch.zeros(n, width + (-width) % 4, device=dev)
    store[:, :width] = x_cpu.to(dev)
    _run_build(layer, store, width, plan, last, "mfma", "fast", cot_cpu.to(dev))        # the cache holds the old objects now
    conv = layer.trainable_kernelconv_set[3]
    old = getattr(conv, name)
    new_value = torch.randn_like(old) if old.dim() else old.detach() + 0.3
    new = torch.nn.Parameter(new_value, requires_grad=old.requires_grad)
    setattr(conv, name, new)
    old.grad = None
    state = {k: v.detach().cpu().clone() for k, v in layer.state_dict().items()}
    assert torch.equal(state[f"trainable_kernelconv_set.3.{name}"], new_value.cpu())
    out, idx, gx, grads = _run_build(layer, store, width, plan, last, "mfma", "fast", cot_cpu.to(dev))
    per_degree = O.kernelset_params(state)
    assert O.kernelset_tie_aware_mismatch(per_degree, x_cpu, cpu, last, out, idx, tol=FWD_TOL) == 0
    bad, differ = O.kernelset_forced_mismatch(per_degree, x_cpu, cpu, last, out, idx, form="cosmat", tol=FWD_TOL)
    assert bad == 0, bad
    _, gx_o, grads_o = O.kernelset_gradients(state, x_cpu, cpu, last, cot_cpu, forced_idx=idx, form="faithful")
    _check_gradients(gx, grads, gx_o, grads_o, n, ("reassigned", name))
    assert old.grad is None
    if name == "p_support":
        assert new.grad is None                           # (no gradient reaches p_support: SURVEY 8 a-9)
    else:
        assert new.grad is not None and torch.equal(new.grad.cpu(), grads[f"trainable_kernelconv_set.3.{name}"])


# ------------------------------------------------------------------------------------------------------------- 5 --
def _set_head_rng(dev, seed):
    """The dropout generator state, written IN PLACE (a captured step keeps reading the same tensor)."""
    from molkgnn_amd import readout as R
    R.head_rng_state(dev).copy_(torch.tensor([seed, 0], dtype=torch.int64))


def _steps_model(dev, opt="fused"):
    from molkgnn_amd.train import configure_optimizer
    model = _fresh(dev, seed=5, rng=3)
    if opt == "fused":
        return model, configure_optimizer(model, lr=1e-3)
    return model, torch.optim.AdamW(model.parameters(), lr=1e-3)


def test_captured_steps_with_streamed_batches(monkeypatch):
    """A streaming loader: every batch is new, and made after the previous one is freed -- its object id and ``x`` address are
    likely to be the freed one's.  None is captured (each is seen once), and every loss is the eager ``training_step``'s."""
    from molkgnn_amd.synthetic import make_batch
    from molkgnn_amd.train import CapturedSteps, training_step
    dev = _dev()
    captured = []
    real = torch.cuda.CUDAGraph

    def spy(*a, **k):
        captured.append(1)
        return real(*a, **k)
    monkeypatch.setattr(torch.cuda, "CUDAGraph", spy)
    model, opt = _steps_model(dev)
    twin, twin_opt = _steps_model(dev)
    steps = CapturedSteps(model, opt)
    for i in range(12):
        b = make_batch(96, seed=600 + i).to(dev)
        _set_head_rng(dev, 40 + i)
        loss = steps(b)
        torch.cuda.synchronize()
        got = float(loss)
        _set_head_rng(dev, 40 + i)
        want = float(training_step(twin, b, twin_opt).detach())
        assert abs(got - want) <= 1e-6 * abs(want), (i, got, want)
        del b, loss
    assert not captured, f"{len(captured)} of 12 batches seen once were captured"


def test_captured_steps_forget_freed_batches():
    """A freed batch leaves no visit count behind, and the counts are bounded: at most ``4 * max_graphs`` batches."""
    from molkgnn_amd.synthetic import make_batch
    from molkgnn_amd.train import CapturedSteps
    dev = _dev()
    model, opt = _steps_model(dev)
    steps = CapturedSteps(model, opt, max_graphs=2)
    b = make_batch(96, seed=700).to(dev)
    key = steps._key(b)
    steps(b)
    assert key in steps._seen
    del b
    gc.collect()
    assert key not in steps._seen
    alive = []
    for i in range(20):
        alive.append(make_batch(96, seed=710 + i).to(dev))
        steps(alive[-1])
        assert len(steps._seen) <= 4 * steps.max_graphs, (i, len(steps._seen))
    torch.cuda.synchronize()


def test_captured_steps_with_an_optimizer_that_cannot_be_captured():
    """``torch.optim.AdamW`` without ``capturable=True``: three visits of one batch stay eager -- the optimiser is checked before a
    capture starts -- and equal the eager loop, loss by loss and parameter by parameter."""
    from molkgnn_amd.synthetic import make_batch
    from molkgnn_amd.train import CapturedSteps, training_step
    dev = _dev()
    b = make_batch(96, seed=800).to(dev)
    model, opt = _steps_model(dev, opt="torch")
    twin, twin_opt = _steps_model(dev, opt="torch")
    steps = CapturedSteps(model, opt, warmup=1)
    for i in range(3):
        _set_head_rng(dev, 50 + i)
        got = steps(b).clone()
        _set_head_rng(dev, 50 + i)
        want = training_step(twin, b, twin_opt)
        torch.cuda.synchronize()
        assert torch.equal(got, want), (i, float(got), float(want))
    assert not steps._graphs
    for (n, p), q in zip(model.named_parameters(), twin.parameters()):
        assert torch.equal(p, q), n
