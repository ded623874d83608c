"""The backward of the three head Functions (``readout._BceHeadFn``, ``_TaskHeadFn``, ``_WeightedTaskHeadFn``: one body,
``_HeadFnBase``) behind a FUSED forward: the hand-out of the gradients the forward already wrote (as they are for the registered
unit seed, scaled for any other incoming gradient) and, once they are handed out, the separate backward entry from the saved
``pred`` and ``rng_used`` (a second backward over a retained graph).  ``pytest -m gpu``.

Shapes: 17 real rows inside an embedding of 19 (a ragged last 16-row block, two padding rows), H = 5 and H = 33 (the column pass
beyond 32 lanes), T = 3 with one unlabelled row and task 1 absent, dropout 0 and 0.25 from a fixed generator state.

Bound of (a): what each family's own test asserts of the fused form against the split one under a unit seed -- the same bits
(``torch.equal``; tests/test_head_f64.py, test_task_head_gpu.py, test_weighted_head_gpu.py).  The first backward here is seeded
by autograd's own 1.0, which is not the registered tensor: a multiplication by 1.0f, exact.  (c) is one float32 multiplication by
3.0f on either side.
"""
import pytest
import torch

from tests import _task_head_cases as TC
from tests import _weighted_head_cases as WC

pytestmark = pytest.mark.gpu

B, ROWS, T = 17, 19, 3
UNLABELLED_ROW, ABSENT_TASK = 5, 1
ROUTES = ("bce", "mse_sum", "task_table", "weighted")
FN_NAME = {"bce": "_BceHeadFnBackward", "mse_sum": "_BceHeadFnBackward", "task_table": "_TaskHeadFnBackward",
           "weighted": "_WeightedTaskHeadFnBackward"}


def _dev():
    assert torch.cuda.is_available(), "pytest -m gpu needs the MI355X"
    return torch.device("cuda:0")


def _case(route: str, H: int, dev):
    """``(ffn, emb0 [19, H], call)``: ``call(emb, p)`` is the route's loss of the leading 17 rows."""
    from molkgnn_amd import readout as R
    g = torch.Generator().manual_seed(1000 * ROUTES.index(route) + H)
    single = route in ("bce", "mse_sum")
    ffn = torch.nn.Linear(H, 1 if single else T)
    with torch.no_grad():
        ffn.weight.copy_(torch.randn(ffn.weight.shape, generator=g) * 0.5)
        ffn.bias.copy_(torch.randn(ffn.bias.shape, generator=g))
    ffn = ffn.to(dev)
    emb0 = (torch.randn(ROWS, H, generator=g) * 2).to(dev)
    if route == "bce":
        y = (torch.rand(B, generator=g) < 0.4).float().to(dev)
        return ffn, emb0, lambda emb, p: R.bce_head_loss(emb, ffn, y, dropout_p=p, n_rows=B)
    if route == "mse_sum":
        y = (torch.randn(B, generator=g) * 1.5 - 8.0).to(dev)
        return ffn, emb0, lambda emb, p: R.head_loss(emb, ffn, y, "mse_sum", dropout_p=p, n_rows=B)
    y = (torch.rand(ROWS, generator=g) < 0.4).float().to(dev)
    task = torch.tensor([0, 2] * 9 + [0], dtype=torch.int32)[:ROWS]
    task[UNLABELLED_ROW] = -1
    task[B:] = TC.SENTINEL                                           # (the padding rows' entries are never read)
    assert not bool((task[:B] == ABSENT_TASK).any()) and int((task[:B] < 0).sum()) == 1
    if route == "task_table":
        perm = torch.randperm(B, generator=g)
        table = task[:B][perm].contiguous().to(dev)                  # row i has table[ids[i]] = task[i]
        ids = torch.full((ROWS,), TC.SENTINEL, dtype=torch.int32)
        ids[:B] = torch.argsort(perm).to(torch.int32)
        ids = ids.to(dev)
        return ffn, emb0, lambda emb, p: R.task_head_loss(emb, ffn, y, None, "bce", dropout_p=p, n_rows=B, task_table=table, row_ids=ids)
    task = task.to(dev)
    lo, hi = WC.POS_RANGE
    s = (torch.rand(ROWS, generator=g) + 0.5).to(dev)
    pw = (lo + (hi - lo) * torch.rand(T, generator=g)).to(dev)
    return ffn, emb0, lambda emb, p: R.task_head_loss(emb, ffn, y, task, "bce", dropout_p=p, n_rows=B, sample_weight=s, pos_weight=pw)


def _grads(emb, ffn):
    """The three gradients (clones), then cleared."""
    torch.cuda.synchronize()
    out = {"emb": emb.grad.clone(), "w": ffn.weight.grad.clone(), "b": ffn.bias.grad.clone()}
    emb.grad = None
    ffn.zero_grad(set_to_none=True)
    return out


@pytest.mark.parametrize("p", [0.0, 0.25])
@pytest.mark.parametrize("H", [5, 33])
@pytest.mark.parametrize("route", ROUTES)
def test_backward_after_the_fused_forward(route, H, p, monkeypatch):
    from molkgnn_amd import readout as R
    from molkgnn_amd.train import backward
    dev = _dev()
    monkeypatch.setattr(R, "_SPLIT_HEAD", False)
    ffn, emb0, call = _case(route, H, dev)

    def forward():
        R.reset_head_rng(dev, seed=TC.SEED)
        emb = emb0.clone().requires_grad_(True)
        ffn.zero_grad(set_to_none=True)
        loss = call(emb, p)
        assert type(loss.grad_fn).__name__ == FN_NAME[route]
        if p > 0.0:
            assert R.head_rng_state(dev).tolist() == [TC.SEED, 1], "(d) one draw in the forward"
        return emb, loss

    def check_padding(g, tag):
        pad = g["emb"][B:]
        assert pad.shape == (ROWS - B, H) and float(pad.abs().max()) == 0.0 and not bool(torch.signbit(pad).any()), (tag, "(b) padding rows")

    # (a), (b), (d): the hand-out, then the separate backward entry over the retained graph
    emb, loss = forward()
    loss.backward(retain_graph=True)
    first = _grads(emb, ffn)
    loss.backward()
    second = _grads(emb, ffn)
    if p > 0.0:
        assert R.head_rng_state(dev).tolist() == [TC.SEED, 1], "(d) no draw in either backward"
        assert 0 < int((first["emb"][:B] == 0).sum()), "the mask is applied"
    for nm in ("emb", "w", "b"):
        assert first[nm].shape == second[nm].shape and bool(torch.isfinite(first[nm]).all())
        assert torch.equal(second[nm], first[nm]), (route, H, p, nm, "(a) the second backward differs from the first",
                                                    float((second[nm] - first[nm]).abs().max()), float(first[nm].abs().max()))
    check_padding(first, "first")
    check_padding(second, "second")
    assert float(first["emb"][:B].abs().max()) > 0.0 and float(first["w"].abs().max()) > 0.0
    if route in ("task_table", "weighted"):
        for g in (first, second):
            assert float(g["emb"][UNLABELLED_ROW].abs().max()) == 0.0
            assert float(g["w"][ABSENT_TASK].abs().max()) == 0.0 and float(g["b"][ABSENT_TASK]) == 0.0

    # (c): the registered unit seed hands the gradients out as they are; any other incoming gradient scales them
    emb, loss = forward()
    backward(loss)
    unit = _grads(emb, ffn)
    for nm in ("emb", "w", "b"):
        assert torch.equal(unit[nm], first[nm]), (route, H, p, nm, "the unit seed's gradients are the forward's")
    emb, loss = forward()
    (loss * 3).backward()
    scaled = _grads(emb, ffn)
    for nm in ("emb", "w", "b"):
        assert torch.equal(scaled[nm], unit[nm] * 3), (route, H, p, nm, "(c) not 3 * the unit-seed gradients")
    check_padding(scaled, "scaled")
