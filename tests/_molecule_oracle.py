"""Checks shared by the molecule-resident tests (tests/test_molecule.py, tests/test_molecule_limits.py) and the model shapes at
the limits of ``mkgnn_molecule_supported`` (also asked of the shape query in tests/test_host_cpu.py)."""
import torch

from oracle import kgnn_oracle as O
from tests import _f64 as F64

FWD_TOL = 1e-5

# (x_dim, E, counts, layers, H = G): the molecule-resident kernels' shapes AT every limit
MOLECULE_LIMIT_SHAPES = {
    "widest": (32, 8, (20, 24, 36, 32), 3, 64),        # pass rows 2*20 + 3*24 + 4*36 = 256, K = 112, x_dim, E, H, G at max
    "tiny": (1, 1, (1, 0, 0, 1), 1, 1),                # one layer (first = last), H = 1
    "one_degree": (5, 3, (64, 0, 0, 0), 2, 5),         # L_d = 64
    "degree4_only": (28, 7, (0, 0, 0, 51), 2, 33),     # 5 * L4 = 255 -> 256 rows; no rows in the pass of degrees 1..3
    "gaps": (17, 7, (3, 0, 5, 0), 4, 16),              # 4 layers, absent degrees
}


def _forced_from_capture(cap, layers):
    forced = []
    for li in range(layers):
        idx = []
        for d in range(4):
            sv = cap["saved"][li][d]
            idx.append(None if sv is None else sv[0][..., 3].contiguous().view(torch.int32).t().cpu().long())
        forced.append(idx)
    return forced


def _check_against_oracle(model, state, b, layers, train_bn, emb, cap, cot, grads_of, tag=None):
    """Layer by layer (tie-aware) and end to end (embedding, every parameter gradient) against the oracle replayed with the
    build's permutation choices."""
    forced = _forced_from_capture(cap, layers)
    ostate = {k: v.clone() for k, v in state.items()}
    h_o = O.batch_norm(b.x, ostate["node_batch_norm.weight"], ostate["node_batch_norm.bias"],
                       ostate["node_batch_norm.running_mean"].clone(), ostate["node_batch_norm.running_var"].clone(), train_bn)
    for i in range(layers):
        per_degree = O.kernelset_params(ostate, f"gnn.layers.{i}.")
        sim = cap["sims"][i].cpu()
        assert O.kernelset_tie_aware_mismatch(per_degree, h_o, b, i == layers - 1, sim, forced[i]) == 0, f"layer {i}"
        sim_o = O.kernelsetconv(per_degree, h_o, b, i == layers - 1, form="faithful", forced_idx=forced[i])
        assert torch.allclose(sim, sim_o, atol=FWD_TOL, rtol=0), (i, float((sim - sim_o).abs().max()))
        h_o = O.propagate_add(b.edge_index, sim_o)
    ostate = {k: (v.requires_grad_(True) if v.dtype.is_floating_point and "running" not in k else v) for k, v in ostate.items()}
    if "node_batch_norm.running_mean" in ostate:
        ostate["node_batch_norm.running_mean"] = ostate["node_batch_norm.running_mean"].clone()
        ostate["node_batch_norm.running_var"] = ostate["node_batch_norm.running_var"].clone()
    emb_o = O.molkgnnnet(ostate, b, layers, training_bn=train_bn, form="faithful", forced_idx=forced)
    scale = max(1.0, float(emb_o.detach().abs().max()))
    assert float((emb.detach().cpu() - emb_o.detach()).abs().max()) <= 5e-5 * scale
    if cot is None:
        return ostate, emb_o
    (emb_o * cot).sum().backward()
    checked = 0
    for nm, got in grads_of.items():
        ref = ostate[nm].grad
        if got is None:
            assert ref is None or float(ref.abs().max()) == 0.0, nm
            continue
        assert ref is not None, nm
        err = float((got.cpu() - ref).abs().max())
        assert err <= 5e-5 * max(1.0, float(ref.abs().max())) + 1e-3 * float(ref.abs().max()), (nm, err, float(ref.abs().max()))
        checked += 1
    # the float64 leg: every tensor within a small multiple of the fp32 oracle's own distance from the float64 network
    f64 = F64.network(state, b, layers, train_bn, forced, torch.float64, cot=cot)
    f32 = {"emb": emb_o.detach(), **{nm: ostate[nm].grad for nm in grads_of if ostate[nm].grad is not None}}
    got = {"emb": emb, **grads_of}
    assert F64.check(got, f32, f64, tag or "molecule") == checked + 1
    return checked
