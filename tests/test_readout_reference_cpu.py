"""The references and the case table of ``tests/_readout_f64.py`` pinned without a GPU: every reference in float64 against an
independent restatement (``torch.nn.functional`` operators through autograd, the readout pooled BEFORE ``lin2`` as the kernels
associate it), every row's predicate, every listed edge value, and that the float32 yardstick is alive."""
import pytest
import torch
import torch.nn.functional as Fnn

from tests import _readout_f64 as RF

REL = 1e-12


def _agree(a, b, what):
    a, b = a.double(), b.double()
    assert a.shape == b.shape, what
    scale = max(float(b.abs().max()) if b.numel() else 0.0, 1e-300)
    assert float((a - b).abs().max() if b.numel() else 0.0) <= REL * scale, (what, float((a - b).abs().max()), scale)


def _restated_readout(h, w1, b1, w2, b2, keep, batch, size, cot):
    """The kernels' association: pooled_g = sum_n keep_n silu(lin1 h_n), out_g = W2 pooled_g + |g| b2."""
    leaves = [t.detach().clone().requires_grad_(True) if t is not None else None for t in (h, w1, b1, w2, b2)]
    h, w1, b1, w2, b2 = leaves
    act = Fnn.silu(Fnn.linear(h, w1, b1))
    if keep is not None:
        act = keep * act
    pooled = torch.zeros(size, w1.shape[0], dtype=h.dtype).index_add(0, batch, act)
    out = Fnn.linear(pooled, w2)
    if b2 is not None:
        out = out + torch.bincount(batch, minlength=size).to(h.dtype)[:, None] * b2
    grads = torch.autograd.grad((out * cot).sum(), [t for t in leaves if t is not None])
    names = [nm for nm, t in zip(("h", "w1", "b1", "w2", "b2"), leaves) if t is not None]
    return dict(zip(names, grads), out=out.detach())


@pytest.mark.parametrize("name,bias,keep", [("w27x31x32", True, True), ("w65x64x1", False, True), ("w1x1x1", True, False),
                                            ("edges_h20", True, True), ("n17_h40", False, False), ("slabs9_h20", True, True)])
def test_dense_reference_agrees_with_the_pooled_first_restatement(name, bias, keep):
    i = RF.dense_inputs(name, bias, keep)
    _, f64 = RF.dense_reference(name, bias, keep)
    args = [RF.cast(i[k], torch.float64) for k in ("h", "w1", "b1", "w2", "b2", "keep", "batch", "size", "cot")]
    want = _restated_readout(*args)
    assert set(want) == set(f64)
    for nm in want:
        _agree(f64[nm], want[nm], (name, nm))


@pytest.mark.parametrize("name,H,full", [("c3251", 5, True), ("c4_0_9_0", 33, False), ("hubs", 32, True), ("pairs_only", 64, True),
                                         ("all_bucketed", 5, False)])
def test_block_row_reference_agrees_with_restatement_and_with_the_dense_reference(name, H, full):
    i = RF.block_inputs(name, H, full)
    _, f64 = RF.block_reference(name, H, full)
    d = lambda k: RF.cast(i[k], torch.float64)
    # an independent propagate: the dense adjacency matrix A[dst, src] = number of edges src -> dst
    n = i["sim"].shape[0]
    A = torch.zeros(n, n, dtype=torch.float64).index_put_((i["edge_index"][1], i["edge_index"][0]), torch.ones((), dtype=torch.float64),
                                                           accumulate=True)
    sim = d("sim").clone().requires_grad_(True)
    h = A @ sim
    _agree(f64["h_value"], h.detach(), (name, "h = propagate(sim)"))
    want = _restated_readout(h.detach(), d("w1"), d("b1"), d("w2"), d("b2"), d("keep"), i["batch"], i["size"], d("cot"))
    # the dense reference on h = propagate(sim) is the same function
    dense = RF.dense(f64["h_value"], d("w1"), d("b1"), d("w2"), d("b2"), d("keep"), i["batch"], i["size"], d("cot"))
    for nm in ("out", "w1", "b1", "w2", "b2"):
        if nm in f64:
            _agree(f64[nm], want[nm], (name, nm))
            _agree(f64[nm], dense[nm], (name, nm, "dense"))
    _agree(f64["sim"], A.t() @ want["h"], (name, "grad sim = propagate^T(grad h)"))
    _agree(f64["sim"], f64["dz"] @ d("w1"), (name, "grad sim = d z W1"))          # (d z: what the kernels' association carries)
    assert not bool(i["sim"][~i["mask"]].any())                   # zero outside every atom's own block


@pytest.mark.parametrize("name,kind", [(nm, k) for nm in ("B17xH33", "B15xH31", "B1xH1", "B528xH64") for k in RF.HEAD_KINDS]
                         + [(RF.SATURATED.name, "bce")])
def test_head_reference_agrees_with_torch_losses(name, kind):
    c =RF.SATURATED if name == RF.SATURATED.name else RF.HEAD_CASES[name]
    i = RF.head_inputs(name, kind)
    _, f64 = RF.head_reference(name, kind, RF.HEAD_SCALE)
    emb = i["emb"][:c.B].double().requires_grad_(True)
    w = i["w"].double().requires_grad_(True)
    b = None if i["b"] is None else i["b"].double().requires_grad_(True)
    e = emb if i["keep"] is None else emb * i["keep"].double()
    pred = Fnn.linear(e, w[None, :], b).view(-1)
    y = i["y"].double()
    loss = (Fnn.binary_cross_entropy_with_logits(pred, y) if kind == "bce" else
            Fnn.mse_loss(pred, y, reduction="sum" if kind == "mse_sum" else "mean"))
    leaves = [t for t in (emb, w, b) if t is not None]
    grads = dict(zip(("emb", "w", "b"), torch.autograd.grad(loss * RF.HEAD_SCALE, leaves)))
    _agree(f64["pred"], pred.detach(), (name, kind, "pred"))
    _agree(f64["loss"], loss.detach(), (name, kind, "loss"))
    for nm, g in grads.items():
        _agree(f64[nm], g, (name, kind, nm))
    if name == RF.SATURATED.name:
        assert f64["pred"][:6].tolist() == list(RF.SATURATED_LOGITS)
        assert bool(torch.isfinite(f64["loss"]))


def test_every_predicate_holds():
    for c in RF.DENSE_WIDTHS + RF.DENSE_SIZES:
        assert c.reaches(c.launch()), (c.name, c.edge, c.launch())
    for c in RF.BLOCK_CASES_LIST:
        for H in c.hidden:
            assert c.reaches(c.launch(H)), (c.name, H, c.edge, {k: v for k, v in c.launch(H).items() if k != "sizes"})
    for c in RF.HEAD_CASES_LIST + [RF.SATURATED]:
        assert c.reaches(c.launch()), (c.name, c.edge, c.launch())


def test_every_listed_value_occurs():
    from collections import Counter
    for values, got in ((RF.DENSE_F, Counter(c.F for c in RF.DENSE_WIDTHS)), (RF.DENSE_H, Counter(c.H for c in RF.DENSE_WIDTHS)),
                        (RF.DENSE_G, Counter(c.G for c in RF.DENSE_WIDTHS))):
        assert all(got[v] >= 2 for v in values), (values, got)
    sizes = {c.launch()["n"] for c in RF.DENSE_SIZES}
    assert {1, 15, 16, 17, 63, 65} <= sizes
    for hw in ("h20", "h40"):
        assert {RF.DENSE_CASES[f"slabs{k}_{hw}"].launch()["nblk_atoms"] for k in (7, 8, 9)} == {7, 8, 9}
        assert RF.DENSE_CASES[f"n1_{hw}"].launch()["nblk_atoms"] == 1
        assert RF.DENSE_CASES[f"many_small_{hw}"].launch()["nblk_atoms"] == 256
        assert RF.DENSE_CASES[f"edges_{hw}"].launch()["sizes"] == (0, 1, 7, 8, 9, 0, 15, 16, 17, 300, 1, 0)
    assert RF.DENSE_CASES["many_small_h20"].H <= 32 < RF.DENSE_CASES["many_small_h40"].H
    counts = {c.counts for c in RF.BLOCK_CASES_LIST}
    assert {(1, 1, 1, 1), (3, 2, 5, 1), (16, 17, 48, 49), (64, 64, 64, 63), (10, 20, 30, 50), (4, 0, 9, 0)} <= counts
    for c in RF.BLOCK_CASES_LIST:
        assert c.name in ("many_small", "half_small_wide") or (set(c.hidden) & {5, 32} and set(c.hidden) & {33, 64}), c.name
    assert RF.BLOCK_CASES["many_small"].hidden[0] <= 32 < RF.BLOCK_CASES["half_small_wide"].hidden[0]
    # load4_at: every alignment 1, 2, 3 is met by a block of at least four columns or by a partial chunk somewhere
    assert {a for c in RF.BLOCK_CASES_LIST for a in c.launch()["align"]} == {0, 1, 2, 3}
    assert RF.BLOCK_CASES["c3251"].launch()["align"] == (0, 3, 1, 2)
    hb, hh = Counter(c.B for c in RF.HEAD_CASES_LIST), Counter(c.H for c in RF.HEAD_CASES_LIST)
    assert all(hb[v] >= 1 for v in RF.HEAD_B) and all(hh[v] >= 2 for v in RF.HEAD_H), (hb, hh)
    assert {c.launch()["nb"] for c in RF.HEAD_CASES_LIST} >= {1, 2, 31, 32, 33, 36, 37, 257}
    for flag in ("bias", "emb_grad"):
        assert {getattr(c, flag) for c in RF.HEAD_CASES_LIST} == {True, False}
    assert {c.p for c in RF.HEAD_CASES_LIST} == {0.0, 0.25}
    assert any(c.n_pad > 0 for c in RF.HEAD_CASES_LIST)
    names = [c.name for c in RF.DENSE_WIDTHS + RF.DENSE_SIZES] + [c.name for c in RF.BLOCK_CASES_LIST] + [c.name for c in RF.HEAD_CASES_LIST]
    assert len(RF.DENSE_CASES) == len(RF.DENSE_WIDTHS + RF.DENSE_SIZES) and len(RF.HEAD_CASES) == len(RF.HEAD_CASES_LIST)
    assert all(nm and " " not in nm for nm in names)


def test_many_small_float32_leg_is_a_live_yardstick():
    """On the largest rows the float32 leg's distance from the float64 leg is finite and not zero for every tensor."""
    legs = [RF.dense_reference("many_small_h20", True, True), RF.block_reference("many_small", 20, True)]
    for f32, f64 in legs:
        assert set(f32) == set(f64)
        for nm in f64:
            assert f32[nm].dtype == torch.float32 and f64[nm].dtype == torch.float64, nm
            d = float((f32[nm].double() - f64[nm]).abs().max())
            assert 0.0 < d < float("inf"), (nm, d)
            assert d <= 1e-3 * float(f64[nm].abs().max()), (nm, d)
    f32, f64 = RF.head_reference("B4097xH64", "bce", 1.0)
    for nm in f64:
        d = float((f32[nm].double() - f64[nm]).abs().max())
        assert 0.0 < d < float("inf"), (nm, d)
