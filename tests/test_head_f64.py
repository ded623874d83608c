"""The single-task head and its three losses (``readout.head_loss`` / ``bce_head_loss`` -> ``_BceHeadFn``; ``mkgnn_head_loss_*`` and
``mkgnn_bce_head_*``, csrc/kgnn_head.hip) against float64 at the edges of its kernels: B around ``HEAD_ROWS``, block counts around
the final kernels' ``bk += 32`` / ``4 * u`` pattern and past 256, partial-row widths ``H + 1`` / ``H + 2`` crossing 64, the wide
path at H = 33, H = 1, no bias, no input gradient, dropout, padded rows, BCE at saturated logits.  The fused entry point
(forward and gradients for d loss = 1 in one pass) and, with ``readout._SPLIT_HEAD`` set, the split forward + backward entry
points with a ``grad_loss`` that is not 1.  Rows and references: ``tests/_readout_f64.py``.  ``pytest -m gpu``.

Bound: ``tests/_f64.check``, constants as they stand, the yardstick the reference's own float32 leg; ``pred``, ``loss``, each
gradient, and the rows of the first and of the last (partial) 16-row block on their own.
"""
import pytest
import torch

from tests import _f64 as F64
from tests import _readout_f64 as RF

pytestmark = pytest.mark.gpu


def _dev():
    assert torch.cuda.is_available(), "pytest -m gpu needs the MI355X"
    return torch.device("cuda:0")


def _run_head(c, kind, monkeypatch):
    from molkgnn_amd import readout as R
    from molkgnn_amd.train import backward
    dev = _dev()
    i = RF.head_inputs(c.name, kind)
    B, H = c.B, c.H
    ffn = torch.nn.Linear(H, 1, bias=c.bias)
    with torch.no_grad():
        ffn.weight.copy_(i["w"][None, :])
        if c.bias:
            ffn.bias.copy_(i["b"])
    ffn = ffn.to(dev)
    emb0, y = i["emb"].to(dev), i["y"].to(dev)

    def run(split, scale, emb_grad=True, entry=None):
        """(loss, pred, grad emb, grad w, grad b, generator state); ``scale`` None: seeded by train.backward's registered 1."""
        monkeypatch.setattr(R, "_SPLIT_HEAD", split)
        R.reset_head_rng(dev, seed=RF.HEAD_SEED)
        emb = emb0.clone().requires_grad_(emb_grad)
        ffn.zero_grad(set_to_none=True)
        if entry == "bce_head_loss":
            loss = R.bce_head_loss(emb, ffn, y, dropout_p=c.p, n_rows=B)
        else:
            loss = R.head_loss(emb, ffn, y, kind, dropout_p=c.p, n_rows=B)
        pred = loss.grad_fn.saved_tensors[3].clone()
        if scale is None:
            backward(loss)
        else:
            (loss * scale).backward()
        torch.cuda.synchronize()
        rng = R.head_rng_state(dev).clone() if c.p > 0.0 else None
        return dict(loss=loss.detach().clone(), pred=pred, emb=None if emb.grad is None else emb.grad.clone(),
                    w=ffn.weight.grad.clone().reshape(-1), b=None if not c.bias else ffn.bias.grad.clone(), rng=rng)

    runs = {"fused": run(False, None), "split": run(True, None), "split*scale": run(True, RF.HEAD_SCALE),
            "fused*scale": run(False, RF.HEAD_SCALE)}
    for how, r in runs.items():
        tag = f"head:{c.name}:{kind}:{how}"
        for nm in ("loss", "pred", "emb", "w", "b"):
            if r[nm] is not None:
                assert bool(torch.isfinite(r[nm]).all()), (tag, nm)
        assert r["emb"].shape == (B + c.n_pad, H)
        if c.n_pad:
            assert float(r["emb"][B:].abs().max()) == 0.0, (tag, "padding rows")
        if c.p > 0.0:
            assert r["rng"].tolist() == [RF.HEAD_SEED, 1], (tag, "one draw per forward")
        # against float64
        f32, f64 = RF.head_reference(c.name, kind, RF.HEAD_SCALE if how.endswith("scale") else 1.0)
        last = slice(RF.HEAD_ROWS * ((B - 1) // RF.HEAD_ROWS), B)
        got = {"pred": r["pred"], "loss": r["loss"], "emb": r["emb"][:B], "w": r["w"], "b": r["b"]}
        legs = [got, dict(f32), dict(f64)]
        for d in legs:
            d["emb[last block]"], d["emb[first block]"] = d["emb"][last], d["emb"][:RF.HEAD_ROWS]
            d["pred[last block]"] = d["pred"][last]
        assert F64.check(*legs, tag) >= 7 - (0 if c.bias else 1)
    # the fused form against the split one where they must agree to the bit: gradients seeded by the registered unit gradient
    a, s = runs["fused"], runs["split"]
    assert abs(float(a["loss"]) - float(s["loss"])) <= 1e-6 * abs(float(s["loss"])), (c.name, kind)   # (two fixed orders of the partials)
    for nm in ("emb", "w", "b"):
        if a[nm] is not None:
            assert torch.equal(a[nm], s[nm]), (c.name, kind, nm, "fused and split differ")
    # grad_emb == nullptr: the parameter gradients, pred and loss to the bit
    if not c.emb_grad:
        for split in (False, True):
            full, none = runs["split" if split else "fused"], run(split, None, emb_grad=False)
            assert none["emb"] is None
            for nm in ("loss", "pred", "w", "b"):
                if full[nm] is not None:
                    assert torch.equal(none[nm], full[nm]), (c.name, kind, split, nm, "changes when emb needs no gradient")
    if kind == "bce":                           # the v7 entry points (bce_head_loss): the same bits as kind 0 of the v8 ones
        for split in (False, True):
            old, new = run(split, None, entry="bce_head_loss"), runs["split" if split else "fused"]
            for nm in ("loss", "pred", "emb", "w", "b"):
                if new[nm] is not None:
                    assert torch.equal(old[nm], new[nm]), (c.name, split, nm)
    return runs


@pytest.mark.parametrize("kind", RF.HEAD_KINDS)
@pytest.mark.parametrize("name", [c.name for c in RF.HEAD_CASES_LIST])
def test_head_edges(name, kind, monkeypatch):
    _run_head(RF.HEAD_CASES[name], kind, monkeypatch)


def test_bce_head_at_saturated_logits(monkeypatch):
    """Logits of exactly +90, -90 and 0 for both targets: the loss is finite, d loss / d emb of those rows is (1 - y) w / B,
    (0 - y) w / B and (1/2 - y) w / B within the bound, and nothing anywhere is NaN or infinite."""
    c = RF.SATURATED
    runs = _run_head(c, "bce", monkeypatch)
    i = RF.head_inputs(c.name, "bce")
    w64 = i["w"].double()
    sig = {90.0: 1.0, -90.0: 0.0, 0.0: 0.5}
    want = torch.stack([(sig[x] - t) * w64 / c.B for x, t in zip(RF.SATURATED_LOGITS, RF.SATURATED_TARGETS)])
    _, f64 = RF.head_reference(c.name, "bce", 1.0)
    assert float((f64["emb"][:6] - want).abs().max()) <= 1e-15 * float(want.abs().max())      # (the reference itself)
    for how in ("fused", "split"):
        r = runs[how]
        assert r["pred"][:6].tolist() == list(RF.SATURATED_LOGITS), how
        got = {f"emb[row {k}]": r["emb"][k] for k in range(6)}
        F64.check(got, {k: want[n].float() for n, k in enumerate(got)}, {k: want[n] for n, k in enumerate(got)}, f"head:{c.name}:bce:{how}:rows")
        # rows whose sigmoid saturates and meets the target get an exactly zero gradient: 1 / (1 + inf) came out 0
        assert float(r["emb"][1].abs().max()) == 0.0 and float(r["emb"][2].abs().max()) == 0.0, how
