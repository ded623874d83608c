"""The float64 leg of the network-level checks: the oracle network (``oracle.kgnn_oracle.molkgnnnet``, optionally followed by
the reference's ffn + BCE head) evaluated in float64 with the build's permutation choices, and the bound every build tensor
is held to against it.

Per tensor: ``max|build - f64| <= C * max|fp32 oracle - f64| + R * max(max|f64|, FLOOR)``.  The fp32 oracle's own rounding error is the
yardstick: a float32 implementation that sums in another order may be a few times further from the exact value than the
oracle, but not orders of magnitude further -- a dropped term worth 0.1 % of a tensor's largest entry is.  ``C`` and ``R`` were
calibrated on the MI355X over every test that calls ``check`` (at least twice the worst measured need; DESIGN.md lists the
measurements).  With ``MKGNN_F64_RECORD=<file>`` every comparison is appended to that file as one JSON line before it is
asserted (re-calibration).
"""
from __future__ import annotations

import json
import os

import torch

from oracle import kgnn_oracle as O

C = 10.0
R = 2.0 ** -16
FLOOR = 1e-3        # R * FLOOR: the absolute part, for tensors that are zero in exact arithmetic (their f64 value is rounding)


def batch_as(b, dtype):
    """A shallow copy of a CPU ``GraphBatch`` with every floating tensor cast to ``dtype``."""
    from molkgnn_amd.receptive_field import GraphBatch
    out = GraphBatch()
    for k, v in b.__dict__.items():
        if torch.is_tensor(v) and v.is_floating_point():
            v = v.to(dtype)
        setattr(out, k, v)
    return out


def network(state, b, layers, train_bn, forced, dtype, cot=None, head=None):
    """The oracle network in ``dtype`` with the permutation choices ``forced`` -> {"emb", ["pred", "loss"], parameter name:
    gradient}.  ``state``: MolKGNNNet's state dict (CPU, float32); ``cot``: a cotangent of the embedding; ``head``: (ffn
    weight, ffn bias, targets) -- BCE with logits of ``emb @ w.T + bias`` (reference model.py:147-150, 169, 190-198)."""
    st = {}
    for k, v in state.items():
        v = v.detach().clone()
        if v.is_floating_point():
            v = v.to(dtype)
            if "running" not in k:
                v.requires_grad_(True)
        st[k] = v
    bb = batch_as(b, dtype)
    emb = O.molkgnnnet(st, bb, layers, training_bn=train_bn, form="faithful", forced_idx=forced)
    out = {"emb": emb.detach()}
    if head is not None:
        w = head[0].detach().cpu().to(dtype).requires_grad_(True)
        bias = head[1].detach().cpu().to(dtype).requires_grad_(True)
        pred = emb @ w.T + bias
        loss = torch.nn.functional.binary_cross_entropy_with_logits(pred.view(-1), head[2].cpu().to(dtype).view(-1))
        loss.backward()
        out.update(pred=pred.detach().view(-1), loss=loss.detach().reshape(()))
        out["ffn.weight"], out["ffn.bias"] = w.grad, bias.grad
    elif cot is not None:
        (emb * cot.to(dtype)).sum().backward()
    if head is not None or cot is not None:
        for k, v in st.items():
            if v.requires_grad and v.grad is not None:
                out[k] = v.grad
    return out


def check(got, f32, f64, tag, names=None):
    """Every tensor of ``got`` (name -> build tensor, None skipped) against the bound above; returns the number checked."""
    rows = []
    for nm in (names if names is not None else list(got)):
        g = got.get(nm)
        if g is None:
            continue
        if f64.get(nm) is None:                          # the reference has no gradient here (it never reaches the output)
            assert float(g.detach().abs().max()) == 0.0, (tag, nm)
            continue
        ref = f64[nm].detach().cpu().double()
        if ref.numel() == 0:                             # (the bank of a degree with no kernels)
            continue
        e_b = float((g.detach().cpu().double().reshape(ref.shape) - ref).abs().max())
        e_32 = float((f32[nm].detach().cpu().double().reshape(ref.shape) - ref).abs().max())
        m = float(ref.abs().max())
        rows.append((nm, e_b, e_32, m))
    path = os.environ.get("MKGNN_F64_RECORD")
    if path:
        with open(path, "a") as f:
            for nm, e_b, e_32, m in rows:
                f.write(json.dumps({"tag": tag, "name": nm, "build": e_b, "fp32": e_32, "max": m}) + "\n")
    bad = [(nm, e_b, e_32, m) for nm, e_b, e_32, m in rows if not e_b <= C * e_32 + R * max(m, FLOOR)]
    assert not bad, (tag, bad[:6])
    return len(rows)
