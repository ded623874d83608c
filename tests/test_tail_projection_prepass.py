"""The fused tail's d sim projection inside the last convolution's coefficient pre-pass (``mkgnn_tail_defer_projection``;
``coef_prepare_proj_kernel``, csrc/kgnn_bwd_stream.hip): inside a ``deferred_tail_reduce`` region the tail leaves out its
``block_project_bwd_mfma_kernel`` launch, the convolution's pre-pass forms every d sim value from d z and W1 in the matrix
instructions' term order, and the dW1 half runs on the helper stream.  The reference of every check is the same step with
``MKGNN_TAIL_PROJECT_IN_PREPASS=0`` -- the projection as a launch of its own -- computed ONCE, for all cases, by a child process
(the switch is read once per process).  Equality is bit for bit.  ``pytest -m gpu``."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

from tests import _tail_projection as TP

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dev():
    assert torch.cuda.is_available(), "pytest -m gpu needs the MI355X"
    return torch.device("cuda:0")


def _launches():
    """[pre-passes with a projected source, projection launches that write d sim, projection launches for dW1 alone]"""
    from molkgnn_amd import _lib
    c = (ctypes.c_int64 * 3)()
    _lib.check(_lib.load().mkgnn_debug_tail_projection_launches(ctypes.byref(c)), "mkgnn_debug_tail_projection_launches")
    return list(c)


@pytest.fixture(scope="module")
def switched_off(tmp_path_factory):
    """Every case's (loss, gradients, grad x) from a process with ``MKGNN_TAIL_PROJECT_IN_PREPASS=0``; left unchanged."""
    assert os.environ.get("MKGNN_TAIL_PROJECT_IN_PREPASS", "1") != "0", "the test process itself runs with the switch on"
    out = str(tmp_path_factory.mktemp("tail_projection") / "off.pt")
    env = dict(os.environ, MKGNN_TAIL_PROJECT_IN_PREPASS="0", MKGNN_MOLECULE="0")
    subprocess.run([sys.executable, "-m", "tests._tail_projection", out], cwd=REPO, env=env, check=True, timeout=300)
    res = torch.load(out)
    n_full = sum(1 for _ in TP.CASES)
    assert res["__launches__"] == [0, n_full, 0], res["__launches__"]      # one projection launch per step, on the chain
    return res


def _same(got, want, what):
    loss, grads, gx = got
    loss0, grads0, gx0 = want
    assert torch.isfinite(loss) and torch.equal(loss, loss0), (what, float(loss), float(loss0))
    assert grads.keys() == grads0.keys(), what
    for n in grads0:
        assert torch.isfinite(grads[n]).all(), (what, n)
        assert torch.equal(grads[n], grads0[n]), (what, n, float((grads[n] - grads0[n]).abs().max()))
    assert (gx is None) == (gx0 is None), what
    if gx0 is not None:
        assert torch.isfinite(gx).all() and torch.equal(gx, gx0), (what, float((gx - gx0).abs().max()))


@pytest.mark.parametrize("name", [n for n, c in TP.CASES.items() if c[3] == "step"])
def test_records_bit_for_bit(name, switched_off):
    """Loss, every parameter gradient (the dW1 gradient among them: same kernel, same slabs, same reduction) and the gradient of
    the last layer's input are those of the materialised projection -- and the step really took the new path: one pre-pass with
    a projected source, one dW1-only launch, no launch that writes d sim."""
    dev = _dev()
    before = _launches()
    got = TP.run_case(name, dev)
    after = _launches()
    assert [a - b for a, b in zip(after, before)] == [1, 0, 1], (name, before, after)
    assert got[2] is not None
    _same(got, switched_off[name], name)


def test_captured_and_replayed(switched_off):
    """The step captured by ``train.CapturedSteps`` and replayed three times: bit for bit the eager one every time."""
    from molkgnn_amd.train import CapturedSteps
    dev = _dev()
    batch = TP.make("b40", dev)
    model = TP.model_for(TP.REF, 32, dev, p_head=0.0)        # (no dropout: every replay draws the same -- no -- mask)
    want = TP.step(model, batch, dev)
    assert all(torch.isfinite(g).all() for g in want[1].values())
    before = _launches()
    steps = CapturedSteps(model, None, warmup=1)
    for visit in range(5):                                   # eager, capture + replay, three more replays
        loss = steps(batch)
        torch.cuda.synchronize()
        assert torch.equal(loss.cpu(), want[0]), visit
        grads = {n: p.grad for n, p in model.named_parameters() if p.grad is not None}
        assert grads.keys() == want[1].keys()
        for n, g in grads.items():
            assert torch.equal(g.cpu(), want[1][n]), (visit, n)
    after = _launches()
    assert [a - b for a, b in zip(after, before)] == [2, 0, 2], (before, after)     # the eager visit and the capture
    # ... and with the head's dropout the eager step is the switched-off process's (the generator advances once either way)
    _same(TP.run_case("b40-ref-h32", dev), switched_off["b40-ref-h32"], "after the captured steps")


@pytest.mark.parametrize("variation", TP.VARIATIONS)
def test_the_slot_is_never_left_dangling(variation, switched_off):
    """Whatever comes between the tail and the last convolution's backward -- a seed that is not the unit one, existing ``.grad``s,
    a last layer on the generic kernels, a ``tail_score`` call, no backward at all -- the projection is materialised first (one
    launch that writes d sim, no projected pre-pass), the result is the switched-off one, and nothing is left pending."""
    from molkgnn_amd import _lib
    dev = _dev()
    name = f"b40-ref-h32-{variation}"
    before = _launches()
    got = TP.run_case(name, dev)
    after = _launches()
    assert [a - b for a, b in zip(after, before)] == [0, 1, 0], (variation, before, after)
    _same(got, switched_off[name], name)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().mkgnn_tail_flush(_lib.stream_ptr(dev)), "mkgnn_tail_flush")
    assert _launches() == after, "mkgnn_tail_flush found something left"


def test_one_step_launches_the_projected_pre_pass_once():
    """Launch counting at the benchmark's model shape (three layers): the pre-pass's projected instantiation once -- for the last
    layer only, the other layers' gradients come through the neighbours -- and the full projection kernel not at all."""
    from molkgnn_amd.train import GNNModel, training_step
    dev = _dev()
    torch.manual_seed(5)
    model = GNNModel(ffn_dropout_rate=0.25).to(dev).train()
    batch = TP.make("b40", dev)
    before = _launches()
    loss = training_step(model, batch, None)
    torch.cuda.synchronize()
    assert torch.isfinite(loss)
    assert [a - b for a, b in zip(_launches(), before)] == [1, 0, 1]
