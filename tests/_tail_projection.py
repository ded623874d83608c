"""Cases and the one step of tests/test_tail_projection_prepass.py, shared by the test process (the fused tail's d sim projection
taken into the last convolution's coefficient pre-pass) and its child (``python -m tests._tail_projection OUT``, started with
``MKGNN_TAIL_PROJECT_IN_PREPASS=0``: the projection as a launch of its own), which writes every case's result to ``OUT``.

A case is (batch, kernel counts per degree, hidden width H, what happens between loss and backward); its result holds the loss,
every parameter gradient and the gradient with respect to the last layer's input rows, on the CPU."""
from __future__ import annotations

import os
import sys

import torch

REF, HALF = (10, 20, 30, 50), (5, 10, 15, 25)
BATCHES = ("b3", "b40", "absent", "padded")
# name -> (batch, kernel counts, H, variation)
CASES = {f"{bn}-{'ref' if ls is REF else 'half'}-h{H}": (bn, ls, H, "step")
         for bn in ("b3", "b40") for ls in (REF, HALF) for H in (32, 20)}
CASES.update({"absent-ref-h32": ("absent", REF, 32, "step"), "padded-half-h20": ("padded", HALF, 20, "step"),
              "padded-ref-h32": ("padded", REF, 32, "step")})
# what may come between the tail and the last convolution's backward: each must leave the switch-off result
VARIATIONS = ("seed2", "grad_exists", "generic", "score_between", "no_backward")
CASES.update({f"b40-ref-h32-{v}": ("b40", REF, 32, v) for v in VARIATIONS})


def no_molecule_step():
    """These batches are small enough for the molecule-resident step, which has no tail: keep them on the layer kernels."""
    from molkgnn_amd import molecule
    molecule._MODE = "0"


def make(batch_name: str, dev):
    from molkgnn_amd import padding as P
    from molkgnn_amd.receptive_field import attach_receptive_fields
    from molkgnn_amd.synthetic import make_batch
    if batch_name == "b3":              # every degree's last (only) tile is partial
        return make_batch(3, seed=8103).to(dev)
    if batch_name == "b40":             # several records per pre-pass block, a degree's tiles over many blocks
        return make_batch(40, seed=8140).to(dev)
    if batch_name == "absent":          # chains and four-armed stars: no atom of degree 3
        from tests._topologies import batch_of, chain, repeat, star
        b = batch_of(repeat([chain(9), star(4), chain(2)], 5), seed=8199)
        assert sorted(set(torch.bincount(b.edge_index[0]).tolist())) == [1, 2, 4]
        return b.to(dev)
    raw = make_batch(40, seed=8141, with_receptive_fields=False)
    other = make_batch(40, seed=8142, with_receptive_fields=False)
    shape = P.fixed_shape([P.degree_histogram(raw), P.degree_histogram(other)])
    return attach_receptive_fields(P.pad_batch(raw, shape, 40).to(dev), sizes=[shape[f"n{d}"] for d in range(1, 5)])


def model_for(ls, H, dev, p_head=0.25):
    from molkgnn_amd.train import GNNModel
    torch.manual_seed(1808)
    return GNNModel(num_layers=2, kernels_1hop=ls, kernels_Nhop=ls, hidden_dim=H, ffn_dropout_rate=p_head).to(dev).train()


def step(model, batch, dev, variation="step"):
    """One ``loss -> backward`` inside a ``deferred_tail_reduce`` region; (loss, {parameter: gradient}, grad of the last layer's input)."""
    from molkgnn_amd import readout as R
    from molkgnn_amd.train import backward as train_backward
    R.reset_head_rng(dev, seed=77)
    model.zero_grad(set_to_none=True)
    if variation == "grad_exists":
        for p in model.parameters():
            p.grad = torch.ones_like(p)
    layers = model.gnn_model.gnn.layers
    layers[-1].backward_variant = "generic" if variation == "generic" else "auto"
    seen = []

    last, run_block_rows = layers[-1], layers[-1]._run_block_rows

    def grab(h, *args, **kwargs):                        # (the layers are not called as modules: no forward hook would fire)
        if torch.is_tensor(h) and h.requires_grad:
            h.register_hook(lambda g: seen.append(g.detach().clone()))
        return run_block_rows(h, *args, **kwargs)
    last._run_block_rows = grab
    try:
        with R.deferred_tail_reduce(dev):
            loss = model.loss(batch)
            if variation == "score_between":
                model.eval()
                model.predict(batch)
                model.train()
            if variation == "seed2":
                (2.0 * loss).backward()
            elif variation == "grad_exists":
                loss.backward()
            elif variation != "no_backward":
                train_backward(loss)
    finally:
        del last._run_block_rows
        layers[-1].backward_variant = "auto"
    torch.cuda.synchronize()
    grads = {n: p.grad.detach().cpu().clone() for n, p in model.named_parameters() if p.grad is not None}
    return loss.detach().cpu().clone(), grads, (seen[0].cpu() if seen else None)


def run_case(name: str, dev):
    batch_name, ls, H, variation = CASES[name]
    return step(model_for(ls, H, dev), make(batch_name, dev), dev, variation)


def main(out_path: str) -> None:
    assert os.environ.get("MKGNN_TAIL_PROJECT_IN_PREPASS") == "0"
    dev = torch.device("cuda:0")
    no_molecule_step()
    res = {name: run_case(name, dev) for name in CASES}
    # (what it launched: nothing projected, nothing for dW1 alone)
    import ctypes
    from molkgnn_amd import _lib
    c = (ctypes.c_int64 * 3)()
    _lib.check(_lib.load().mkgnn_debug_tail_projection_launches(ctypes.byref(c)), "mkgnn_debug_tail_projection_launches")
    res["__launches__"] = list(c)
    torch.save(res, out_path)


if __name__ == "__main__":
    main(sys.argv[1])
