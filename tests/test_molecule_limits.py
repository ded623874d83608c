"""The molecule-resident step (csrc/kgnn_molecule.hip) and the fused tail (csrc/kgnn_tail.hip, readout.tail_loss) at their shape
and chunk limits, against the oracle network in float64 (tests/_f64.py).  ``pytest -m gpu``.

Shapes: every width of ``mkgnn_molecule_supported`` at its maximum (x_dim 32, E 8, K 112, 256 pass rows, H = G = 64), one
layer with H = 1, L_d = 64, 5 * L4 = 255, absent degrees with 4 layers; one shape past a limit goes to the per-operator path.
Batches (tests/_topologies.py): chunks of exactly 16 molecules and of 32 atoms, one-atom molecules (no focal atom, no bond),
molecules of 32, 33 and 64 atoms, a batch of one atom, and the fused tail's 128 atoms / 512 edges in one molecule.
"""
import pytest
import torch

from oracle import kgnn_oracle as O
from tests import _f64 as F64
from tests import _topologies as T
from tests._molecule_oracle import MOLECULE_LIMIT_SHAPES, _check_against_oracle, _forced_from_capture

pytestmark = pytest.mark.gpu

REF_SHAPE = (28, 7, (10, 20, 30, 50), 3, 32)


def _dev():
    assert torch.cuda.is_available(), "pytest -m gpu needs the MI355X"
    return torch.device("cuda:0")


def _gnn_model(shape, seed, dev, train):
    """train.GNNModel of (x_dim, E, counts, layers, H = G), batch-norm statistics and affine parameters randomised."""
    from molkgnn_amd.train import GNNModel
    x_dim, E, counts, layers, H = shape
    torch.manual_seed(seed)
    model = GNNModel(num_layers=layers, kernels_1hop=counts, kernels_Nhop=counts, node_feature_dim=x_dim, edge_feature_dim=E,
                     hidden_dim=H, ffn_dropout_rate=0.0)
    bn = model.gnn_model.node_batch_norm
    with torch.no_grad():
        bn.running_mean.normal_(0.0, 0.3)
        bn.running_var.uniform_(0.5, 1.5)
        bn.weight.uniform_(0.5, 1.5)
        bn.bias.normal_(0.0, 0.2)
    state = {k: v.detach().clone() for k, v in model.state_dict().items()}
    return model.to(dev).train(train), state


def _sub(state, prefix="gnn_model."):
    return {k[len(prefix):]: v for k, v in state.items() if k.startswith(prefix)}


def _spy_run(monkeypatch):
    from molkgnn_amd import molecule as M
    calls = []
    orig = M._run
    monkeypatch.setattr(M, "_run", lambda *a, **k: (calls.append(a[6]), orig(*a, **k))[1])
    return calls


def _spy_tail(monkeypatch):
    from molkgnn_amd import readout as R
    calls = []
    real = R.tail_loss
    monkeypatch.setattr(R, "tail_loss", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    return calls


def _layers_tie_aware(state, b, layers, train_bn, sims, forced):
    """Every layer's scores (build) against the oracle: tie-aware criterion, then equal to the oracle replayed with the build's
    choices."""
    h_o = O.batch_norm(b.x, state["node_batch_norm.weight"], state["node_batch_norm.bias"],
                       state["node_batch_norm.running_mean"].clone(), state["node_batch_norm.running_var"].clone(), train_bn)
    for i in range(layers):
        per_degree = O.kernelset_params(state, f"gnn.layers.{i}.")
        sim = sims[i].cpu()
        assert O.kernelset_tie_aware_mismatch(per_degree, h_o, b, i == layers - 1, sim, forced[i]) == 0, f"layer {i}"
        sim_o = O.kernelsetconv(per_degree, h_o, b, i == layers - 1, form="faithful", forced_idx=forced[i])
        assert torch.allclose(sim, sim_o, atol=1e-5, rtol=0), (i, float((sim - sim_o).abs().max()))
        h_o = O.propagate_add(b.edge_index, sim_o)


def _forced_from_graph(root, layers):
    """The permutation choices the per-operator forward really made: the pair records its kernel-convolution nodes keep for
    their backward (functional._KernelSetConvFn, ``ctx.saved_t``), read from the autograd graph before the backward runs.
    Nodes are met from the output backwards, so the last layer comes first."""
    nodes, seen, todo = [], set(), [root]
    while todo:
        nxt = []
        for fn in todo:
            if fn is None or fn in seen:
                continue
            seen.add(fn)
            if type(fn).__name__ == "_KernelSetConvFnBackward":
                nodes.append(fn)
            nxt += [f for f, _ in fn.next_functions]
        todo = nxt
    assert len(nodes) == layers, len(nodes)
    return [[None if pr is None else pr[..., 3].contiguous().view(torch.int32).t().cpu().long() for pr, _ in fn.saved_t]
            for fn in reversed(nodes)]


def _per_operator_choices(net, state, bd, b, train_bn, forced):
    """Checks the per-operator path's choices ``forced`` (from ``_forced_from_graph``): the layers replayed by
    functional.kernelsetconv_details (as tests/test_hip_parity.py ``test_three_layer_network_tie_aware`` does) pass the
    tie-aware criterion, and every choice of the real forward scores within 1e-6 of the oracle's maximum."""
    from molkgnn_amd import functional as Fn
    from molkgnn_amd.plan import plan_from_data
    layers = len(net.gnn.layers)
    if all(getattr(b, f"selected_index_deg{d}").numel() == 0 for d in range(1, 5)):
        assert all(i is None for layer in forced for i in layer)
        return
    plan = plan_from_data(bd)
    replayed, sims = [], []
    dev = bd.x.device
    with torch.no_grad():
        h = torch.nn.functional.batch_norm(bd.x, state["node_batch_norm.running_mean"].clone().to(dev),
                                           state["node_batch_norm.running_var"].clone().to(dev), net.node_batch_norm.weight,
                                           net.node_batch_norm.bias, train_bn, 0.1, 1e-5)
        for i, layer in enumerate(net.gnn.layers):
            params, E = layer._bank_params("train", h)
            sim, saved = Fn.kernelsetconv_details(h, plan, i == layers - 1, params, E)
            replayed.append([None if s[0] is None else s[0].cpu().long() for s in saved])
            sims.append(sim)
            h = Fn.propagate_add(sim, plan, out_pad=(-sim.shape[1]) % 4)
    _layers_tie_aware(state, b, layers, train_bn, sims, replayed)
    h_o = O.batch_norm(b.x, state["node_batch_norm.weight"], state["node_batch_norm.bias"],
                       state["node_batch_norm.running_mean"].clone(), state["node_batch_norm.running_var"].clone(), train_bn)
    for i in range(layers):
        per_degree = O.kernelset_params(state, f"gnn.layers.{i}.")
        for d in range(1, 5):
            sel, idx = getattr(b, f"selected_index_deg{d}"), forced[i][d - 1]
            assert (idx is None) == (sel.numel() == 0 or per_degree[d - 1]["x_center"].shape[0] == 0), (i, d)
            if idx is None:
                continue
            nei = getattr(b, f"nei_index_deg{d}")
            _, table, _, _ = O.kernelconv_cosmat(per_degree[d - 1], h_o[sel], getattr(b, f"p_focal_deg{d}"),
                                                 h_o[nei].reshape(-1, d, h_o.shape[-1]), getattr(b, f"nei_p_deg{d}"),
                                                 getattr(b, f"nei_edge_attr_deg{d}"), i == layers - 1, forced_idx=idx)
            chosen = torch.gather(table, 1, idx.unsqueeze(1)).squeeze(1)
            assert float((table.max(dim=1).values - chosen).max()) <= 1e-6, (i, d)
        h_o = O.propagate_add(b.edge_index, O.kernelsetconv(per_degree, h_o, b, i == layers - 1, form="faithful",
                                                            forced_idx=forced[i]))


def _head_step(model, bd, monkeypatch, molecule):
    """``GNNModel.loss`` + ``train.backward`` on one path -> (loss, {gnn parameter: grad} + ffn grads, capture)."""
    from molkgnn_amd import molecule as M
    from molkgnn_amd.train import backward as train_backward
    cap = {}
    monkeypatch.setattr(M, "debug_capture", cap if molecule else None)
    model.zero_grad(set_to_none=True)
    loss = model.loss(bd)
    if not molecule and loss.grad_fn is not None:
        cap["graph_forced"] = _forced_from_graph(loss.grad_fn, len(model.gnn_model.gnn.layers))
    train_backward(loss)
    torch.cuda.synchronize()
    grads = {nm[len("gnn_model."):]: p.grad for nm, p in model.named_parameters() if nm.startswith("gnn_model.")}
    grads["ffn.weight"], grads["ffn.bias"] = model.ffn.weight.grad, model.ffn.bias.grad
    return loss.detach(), grads, cap


def _check_head(state, b, layers, train_bn, forced, loss, grads, pred, tag):
    gstate = _sub(state)
    head = (state["ffn.weight"], state["ffn.bias"], b.y)
    f32 = F64.network(gstate, b, layers, train_bn, forced, torch.float32, head=head)
    f64 = F64.network(gstate, b, layers, train_bn, forced, torch.float64, head=head)
    got = {"loss": loss, **grads}
    if pred is not None:
        got["pred"] = pred
    for nm, g in grads.items():                          # no gradient from the build <=> none (or zero) in the oracle
        if g is None:
            assert nm not in f64 or float(f64[nm].abs().max()) == 0.0, (tag, nm)
    return F64.check(got, f32, f64, tag)


# ------------------------------------------------------------------------------------------ shapes at the limits ----
def _shape_batch(shape, seed):
    x_dim, E = shape[0], shape[1]
    specs = [T.tree(12), T.star(4), T.pair(), T.tree(20), T.single(), T.tree(9), T.tree(7, ring=False), T.tree(16)]
    return T.batch_of(specs, F=x_dim, E=E, seed=seed)


_SHAPE_RUNS = [(name, mode, train) for name in MOLECULE_LIMIT_SHAPES for mode, train in (("emb", True), ("head", False))] + \
              [("widest", "emb", False), ("widest", "head", True), ("tiny", "head", True), ("gaps", "emb", False)]


@pytest.mark.parametrize("name,mode,train_bn", _SHAPE_RUNS)
def test_molecule_step_at_its_shape_limits(name, mode, train_bn, monkeypatch):
    """GRAD_EMB (forward + a random cotangent) and HEAD (GNNModel.loss, then train.backward) with training- and eval-mode batch
    norm, each shape at a limit of mkgnn_molecule_supported: the molecule-resident kernels run, and every score, the
    embedding / loss / pred and every gradient agree with the oracle (fp32 criteria and the float64 bound)."""
    dev = _dev()
    from molkgnn_amd import molecule as M
    monkeypatch.setattr(M, "_MODE", "1")
    shape = MOLECULE_LIMIT_SHAPES[name]
    layers, H = shape[3], shape[4]
    seed = sum(map(ord, name)) + (mode == "head") + 2 * train_bn
    model, state = _gnn_model(shape, seed, dev, train_bn)
    b = _shape_batch(shape, seed)
    bd = b.to(dev)
    calls = _spy_run(monkeypatch)
    tag = f"shape/{name}/{mode}/{train_bn}"
    if mode == "emb":
        net = model.gnn_model
        cap = {}
        monkeypatch.setattr(M, "debug_capture", cap)
        emb = net(bd)
        assert calls == [0], calls
        fwd_cap = dict(cap)
        cot = torch.randn(b.num_graphs, H, generator=torch.Generator().manual_seed(seed))
        (emb * cot.to(dev)).sum().backward()
        assert calls == [0, 6], calls
        grads = {nm: p.grad for nm, p in net.named_parameters()}
        assert _check_against_oracle(net, _sub(state), b, layers, train_bn, emb, fwd_cap, cot, grads, tag=tag) >= 6
    else:
        loss, grads, cap = _head_step(model, bd, monkeypatch, True)
        assert calls == [3], calls
        forced = _forced_from_capture(cap, layers)
        _layers_tie_aware(_sub(state), b, layers, train_bn, cap["sims"], forced)
        assert _check_head(state, b, layers, train_bn, forced, loss, grads, cap["pred"], tag) >= 8


def test_shape_past_a_limit_takes_the_per_operator_path(monkeypatch):
    """x_dim 33 (one past the first layer's 32): with MKGNN_MOLECULE=1 the host refuses the model (model_qualifies), the
    molecule-resident kernels are never called, and the per-operator path's embedding and gradients meet the float64 bound."""
    dev = _dev()
    from molkgnn_amd import molecule as M
    monkeypatch.setattr(M, "_MODE", "1")
    shape = (33, 7, (10, 20, 30, 50), 3, 32)
    model, state = _gnn_model(shape, 33, dev, True)
    net = model.gnn_model
    b = _shape_batch(shape, 33)
    bd = b.to(dev)
    assert not M.model_qualifies(net, bd)
    calls = _spy_run(monkeypatch)
    emb = net(bd)
    forced = _forced_from_graph(emb.grad_fn, 3)
    cot = torch.randn(b.num_graphs, 32, generator=torch.Generator().manual_seed(3))
    (emb * cot.to(dev)).sum().backward()
    assert calls == []
    gstate = _sub(state)
    _per_operator_choices(net, gstate, bd, b, True, forced)
    f32 = F64.network(gstate, b, 3, True, forced, torch.float32, cot=cot)
    f64 = F64.network(gstate, b, 3, True, forced, torch.float64, cot=cot)
    got = {"emb": emb, **{nm: p.grad for nm, p in net.named_parameters()}}
    assert F64.check(got, f32, f64, "past_limit/x_dim33") >= 20


# ------------------------------------------------------------------------------------------ chunks at the limits ----
def _b1():
    """40 one-atom molecules in runs of 16, 17 and 7, eight ordinary molecules between and around them; the ordinary ones
    fill 32-atom chunks, so the runs start chunks of their own: 16 molecules exactly."""
    s = T.single()
    return [T.tree(20), T.tree(12)] + [s] * 16 + [T.tree(18), T.tree(14)] + [s] * 17 + [T.tree(9), T.tree(22)] + [s] * 7 + \
        [T.tree(10), T.tree(15)]


def _b2():
    return [T.pair()] * 48 + [T.single()] * 17


def _b3():
    return [T.pair(), T.tree(32), T.star(4), T.tree(33), T.single(), T.tree(64), T.tree(7), T.tree(11, ring=False)]


def _b4():
    return [T.single()]


_CHUNK_BATCHES = {"B1": (_b1, True), "B2": (_b2, True), "B3": (_b3, True), "B4": (_b4, False)}


def _chunk_table(bd):
    from molkgnn_amd import molecule as M
    mp = M.build_molecule_plan(M._plan_of(bd), bd.batch, bd.num_graphs)
    assert mp is not None
    ptr = mp.chunk_ptr.cpu().tolist()
    sizes = torch.bincount(bd.batch.cpu(), minlength=bd.num_graphs).tolist()
    return [(c - a, sum(sizes[a:c])) for a, c in zip(ptr, ptr[1:])]


@pytest.mark.parametrize("which", list(_CHUNK_BATCHES))
@pytest.mark.parametrize("path", ["molecule", "per_operator"])
def test_chunk_limits_both_paths(which, path, monkeypatch):
    """B1 .. B4 through GNNModel.loss + train.backward on the molecule-resident step (MKGNN_MOLECULE=1) and on the per-operator
    kernels + fused tail (=0): loss (and pred) and every gradient within the float64 bound; B1 .. B3 three times bit for bit."""
    dev = _dev()
    from molkgnn_amd import molecule as M
    from molkgnn_amd import readout as R
    make, train_bn = _CHUNK_BATCHES[which]
    monkeypatch.setattr(M, "_MODE", "1" if path == "molecule" else "0")
    b = T.batch_of(make(), seed=len(which) + ord(which[1]))
    bd = b.to(dev)
    chunks = _chunk_table(bd)
    if which == "B1":
        assert chunks == [(2, 32), (16, 16), (2, 32), (16, 16), (3, 32), (9, 32)], chunks   # 16 one-atom molecules: chunks of their own
    if which == "B2":
        assert chunks.count((16, 32)) == 3 and chunks[-2:] == [(16, 16), (1, 1)], chunks
    if which == "B3":
        assert chunks == [(1, 2), (1, 32), (1, 5), (1, 33), (1, 1), (1, 64), (2, 18)], chunks
    model, state = _gnn_model(REF_SHAPE, 70 + ord(which[1]), dev, train_bn)
    calls, tails = _spy_run(monkeypatch), _spy_tail(monkeypatch)
    if path == "per_operator":
        seg = R.molecule_segments(bd.batch, bd.num_graphs)
        from molkgnn_amd.plan import plan_from_data
        tail_ok = R.tail_supported(110, 32, 32, (10, 20, 30, 50)) and R._tail_limits_ok(seg, plan_from_data(bd))
        if which != "B4":
            assert tail_ok
    runs = []
    state_now = {k: v.clone() for k, v in model.state_dict().items()}
    for _ in range(3 if which != "B4" else 1):
        model.load_state_dict(state_now)                                # (batch-norm statistics as before the first run)
        runs.append(_head_step(model, bd, monkeypatch, path == "molecule"))
    if path == "molecule":
        assert calls == [3] * len(runs), calls
    else:
        assert calls == [] and (which == "B4" or len(tails) == len(runs)), (calls, tails)
    loss, grads, cap = runs[0]
    for l2, g2, _ in runs[1:]:
        assert torch.equal(loss, l2)
        assert all((g2[nm] is None and g is None) or torch.equal(g, g2[nm]) for nm, g in grads.items())
    if path == "molecule":
        forced = _forced_from_capture(cap, 3)
        _layers_tie_aware(_sub(state), b, 3, train_bn, cap["sims"], forced)
        pred = cap["pred"]
    else:
        forced = cap["graph_forced"]
        _per_operator_choices(model.gnn_model, _sub(state), bd, b, train_bn, forced)
        pred = None
    present = sum(1 for d in range(1, 5) if getattr(b, f"selected_index_deg{d}").numel() > 0)
    assert _check_head(state, b, 3, train_bn, forced, loss, grads, pred, f"chunks/{which}/{path}") >= 6 * present * 3 + 7


@pytest.mark.parametrize("which", ["hub5", "atoms65"])
def test_batches_the_molecule_step_refuses(which, monkeypatch):
    """A 65-atom molecule (beyond MKGNN_MOLECULE_MAX_ATOMS) and a degree-5 hub (beyond every degree bucket): build_molecule_plan
    returns None, the step is not called, and the per-operator path meets the float64 bound (the hub's own score row is zero,
    its neighbours still receive it through propagate)."""
    dev = _dev()
    from molkgnn_amd import molecule as M
    monkeypatch.setattr(M, "_MODE", "1")
    specs = [T.tree(10), T.star(5), T.pair()] if which == "hub5" else [T.tree(10), T.tree(65), T.pair()]
    b = T.batch_of(specs, seed=5 if which == "hub5" else 65)
    bd = b.to(dev)
    assert M.build_molecule_plan(M._plan_of(bd), bd.batch, bd.num_graphs) is None
    model, state = _gnn_model(REF_SHAPE, 91, dev, True)
    calls = _spy_run(monkeypatch)
    loss, grads, cap = _head_step(model, bd, monkeypatch, False)
    assert calls == []
    forced = cap["graph_forced"]
    _per_operator_choices(model.gnn_model, _sub(state), bd, b, True, forced)
    assert _check_head(state, b, 3, True, forced, loss, grads, None, f"refused/{which}") >= 60


# -------------------------------------------------------------------------------------- the fused tail, directly ----
def _tail_reference(b, inblock, sim0, lin1, lin2, ffn, y, dtype, dev):
    """Loss and every gradient of the reference's formula on the dense h = propagate(sim), by autograd in ``dtype``."""
    params = [p.detach().to(dtype).requires_grad_(True) for p in (lin1.weight, lin1.bias, lin2.weight, lin2.bias, ffn.weight, ffn.bias)]
    w1, b1, w2, b2, wh, bh = params
    dense = torch.where(inblock, sim0, torch.zeros((), device=dev)).to(dtype).requires_grad_(True)
    src, dst = b.edge_index[0], b.edge_index[1]
    h = torch.zeros_like(dense).index_add_(0, dst, dense[src])                       # KernelLayer.py:119-123
    z = h @ w1.t() + b1
    z = z * torch.sigmoid(z)
    z = z @ w2.t() + b2
    emb = torch.zeros(b.num_graphs, z.shape[1], dtype=dtype, device=dev).index_add_(0, b.batch, z)   # MolKGNNNet.py:144-146
    pred = emb @ wh.t() + bh
    loss = torch.nn.functional.binary_cross_entropy_with_logits(pred.view(-1), y.to(dtype))
    grads = torch.autograd.grad(loss, [dense] + params)
    names = ("gsim", "w1", "b1", "w2", "b2", "wh", "bh")
    out = {"loss": loss.detach()}
    out.update({nm: (torch.where(inblock, g, torch.zeros((), device=dev, dtype=dtype)) if nm == "gsim" else g)
                for nm, g in zip(names, grads)})
    return out


def _tail_case(specs, Ls, H, G, seed, tag, monkeypatch):
    from molkgnn_amd import readout as R
    from molkgnn_amd.plan import plan_from_data
    from tests.test_tail import _block_rows
    dev = _dev()
    K = sum(Ls)
    b = T.batch_of(specs, seed=seed).to(dev)
    plan = plan_from_data(b)
    seg = R.molecule_segments(b.batch, b.num_graphs)
    assert R.tail_supported(K, H, G, Ls) and R._tail_limits_ok(seg, plan), tag
    torch.manual_seed(seed)
    lin1, lin2, ffn = torch.nn.Linear(K, H).to(dev), torch.nn.Linear(H, G).to(dev), torch.nn.Linear(G, 1).to(dev)
    sim0, inblock = _block_rows(b, plan, Ls, dev, seed)
    y = (torch.rand(b.num_graphs, device=dev) < 0.4).float()
    tails = _spy_tail(monkeypatch)
    sim = sim0.detach().requires_grad_(True)
    loss = R.tail_loss(sim, plan, Ls, lin1, lin2, ffn, y, seg, 0.0, None)
    loss.backward()
    assert len(tails) == 1
    got = {"loss": loss.detach(), "gsim": torch.where(inblock, sim.grad, torch.zeros((), device=dev))}
    got.update({nm: p.grad for nm, p in zip(("w1", "b1", "w2", "b2", "wh", "bh"),
                                            list(lin1.parameters()) + list(lin2.parameters()) + list(ffn.parameters()))})
    f32 = _tail_reference(b, inblock, sim0, lin1, lin2, ffn, y, torch.float32, dev)
    f64 = _tail_reference(b, inblock, sim0, lin1, lin2, ffn, y, torch.float64, dev)
    assert F64.check(got, f32, f64, tag) == 8
    for nm in got:                                       # ... and the existing criterion of test_fused_tail_against_the_pytorch_formula
        err = float((got[nm].double() - f64[nm]).abs().max())
        assert err <= 2e-5 * max(float(f64[nm].abs().max()), 1e-6), (tag, nm, err)


_TAIL_MIX = [T.tree(20), T.single(), T.tree(9), T.pair(), T.star(4), T.tree(33), T.tree(14, ring=False)] * 3


@pytest.mark.parametrize("H,G,Ls", [(1, 1, (10, 20, 30, 50)), (5, 7, (5, 10, 15, 25)), (17, 32, (1, 1, 1, 1)),
                                    (32, 1, (3, 0, 5, 0)), (32, 32, (3, 0, 5, 0)), (5, 7, (1, 1, 1, 1)), (17, 32, (10, 20, 30, 50))])
def test_fused_tail_shapes(H, G, Ls, monkeypatch):
    """readout.tail_loss at H, G from 1 to 32 and block widths down to one kernel and absent degrees (pairwise subset)."""
    _tail_case(_TAIL_MIX, Ls, H, G, 7 * H + G, f"tail/{H}/{G}/{Ls}", monkeypatch)


@pytest.mark.parametrize("which", ["B1", "B2", "circulant128"])
def test_fused_tail_chunk_limits(which, monkeypatch):
    """readout.tail_loss on one-atom molecules in long runs, 16-molecule 32-atom runs, and a molecule of exactly 128 atoms and
    512 edges each way (MKGNN_TAIL_MAX_ATOMS, MKGNN_TAIL_MAX_EDGES) next to small ones."""
    specs = {"B1": _b1(), "B2": _b2(), "circulant128": [T.tree(12), T.circulant(128), T.single(), T.tree(30)]}[which]
    _tail_case(specs, (10, 20, 30, 50), 32, 32, 11, f"tail/{which}", monkeypatch)


def test_fused_tail_with_dropout_on_chunk_limits():
    """p_drop > 0 on B1 + the 128-atom molecule: the fused tail against the separate operators, same generator state."""
    from molkgnn_amd import readout as R
    from molkgnn_amd.plan import plan_from_data
    from tests.test_tail import _block_rows
    dev = _dev()
    Ls = (10, 20, 30, 50)
    b = T.batch_of(_b1() + [T.circulant(128)], seed=13).to(dev)
    plan = plan_from_data(b)
    seg = R.molecule_segments(b.batch, b.num_graphs)
    assert R.tail_supported(110, 32, 32, Ls) and R._tail_limits_ok(seg, plan)
    torch.manual_seed(13)
    lin1, lin2, ffn = torch.nn.Linear(110, 32).to(dev), torch.nn.Linear(32, 32).to(dev), torch.nn.Linear(32, 1).to(dev)
    sim0, inblock = _block_rows(b, plan, Ls, dev, 13)
    y = (torch.rand(b.num_graphs, device=dev) < 0.3).float()
    params = list(lin1.parameters()) + list(lin2.parameters()) + list(ffn.parameters())

    def run(fused):
        R.reset_head_rng(dev, seed=4321)
        for p in params:
            p.grad = None
        sim = sim0.detach().requires_grad_(True)
        if fused:
            loss = R.tail_loss(sim, plan, Ls, lin1, lin2, ffn, y, seg, 0.3, None)
        else:
            emb = R.readout_blocks(sim, plan, Ls, lin1, lin2, None, seg)
            loss = R.bce_head_loss(emb, ffn, y, dropout_p=0.3)
        loss.backward()
        torch.cuda.synchronize()
        return loss.detach().clone(), torch.where(inblock, sim.grad, torch.zeros((), device=dev)), [p.grad.clone() for p in params], \
            R.head_rng_state(dev).clone()

    l0, gs0, gp0, st0 = run(False)
    l1, gs1, gp1, st1 = run(True)
    assert torch.isfinite(l1) and abs(float(l0) - float(l1)) <= 2e-6 * max(1.0, abs(float(l0))), (float(l0), float(l1))
    assert float((gs0 - gs1).abs().max()) <= 2e-5 * max(float(gs0.abs().max()), 1e-8)
    for a, c, nm in zip(gp0, gp1, ("w1", "b1", "w2", "b2", "wh", "bh")):
        assert float((a - c).abs().max()) <= 2e-5 * max(float(a.abs().max()), 1e-6), nm
    assert torch.equal(st0, st1)
