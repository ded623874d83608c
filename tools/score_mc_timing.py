"""Time of scoring with uncertainty (``GNNModel.predict_mc``, ``mkgnn_tail_score_mc``) against the point score and against the only
other way to the same quantity.

    python tools/score_mc_timing.py [--batches 256 4096] [--samples 8 32 64] [--replays 32] [--windows 10] [--warmup 3]

Everything is captured once and replayed; the routes of one (batch, probabilities, samples) take turns inside ONE process, window
by window, and a route's figure is the median of its ``--windows`` windows of ``--replays`` replays (device events; every window is
in the line, so the spread is too).  One JSON line per (batch, probabilities, samples):

``predict``     the captured ``GNNModel.predict`` step on the same batch: what the uncertainty costs over a point score
``mc``          the captured ``predict_mc`` step on its kernel route (``readout.tail_score_mc``)
``mc_torch``    the captured ``predict_mc`` step on its PyTorch route (``MKGNN_SCORE_MC=0``, set here through the module flag): the
                network once more for ``h``, then S rounds of ``F.dropout``, ``lin2``, add-pool, ``F.dropout``, ``ffn`` -- this route
                also runs ``predict`` for its ``pred``, so ``mc_torch - predict`` is its network pass plus the S rounds
``tail_score``  the two launches of ``mkgnn_tail_score`` alone on random block rows of the batch, back to back in one graph
``tail_mc``     the two launches of ``mkgnn_tail_score_mc`` alone on the same rows (mean, std, acq; no samples, no pred)

Probabilities ``(head, readout)``: ``(0.25, 0.2)`` -- the per-sample barrier pair -- and ``(0.25, 0)`` -- the loop without barriers.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LS = (10, 20, 30, 50)
PROBS = ((0.25, 0.2), (0.25, 0.0))


def _capture(fn, dev, warm=True):
    import torch
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        if warm:
            fn()                                         # (eager once: lazily made buffers exist before the capture)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            out = fn()
    torch.cuda.current_stream(dev).wait_stream(side)
    return graph, out


def _take_turns(graphs, replays, windows, warmup):
    """``{name: [ms per replay of every window]}``: window by window, every route in turn."""
    import torch
    for g in graphs.values():
        for _ in range(warmup):
            g.replay()
    torch.cuda.synchronize()
    out = {name: [] for name in graphs}
    for _ in range(windows):
        for name, g in graphs.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(replays):
                g.replay()
            t1.record()
            torch.cuda.synchronize()
            out[name].append(t0.elapsed_time(t1) / replays)
    return out


def _block_rows(n, plan, dev, seed):
    import torch
    g = torch.Generator(device=dev).manual_seed(seed)
    K = sum(LS)
    store = torch.zeros((n, K + (-K) % 4), device=dev)
    off = 0
    for d, L in enumerate(LS):
        sel = plan.buckets[d].sel
        if sel.numel():
            store[sel, off:off + L] = torch.randn(sel.numel(), L, generator=g, device=dev)
        off += L
    return store[:, :K]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[256, 4096])
    ap.add_argument("--samples", type=int, nargs="+", default=[8, 32, 64])
    ap.add_argument("--replays", type=int, default=32)
    ap.add_argument("--windows", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    import torch
    sys.path.insert(0, REPO)
    from molkgnn_amd import readout as R
    from molkgnn_amd.plan import plan_from_data
    from molkgnn_amd.synthetic import make_batch
    from molkgnn_amd.train import GNNModel, tune_torch_backends
    assert torch.cuda.is_available(), "a timing needs the GPU"
    assert R._SCORE_MC and R._SCORE_TAIL and R._FUSED_TAIL, "the default routes are measured"
    dev = torch.device("cuda:0")
    tune_torch_backends()
    taken = []
    real = R.tail_score_mc
    R.tail_score_mc = lambda *a, **k: (taken.append(1), real(*a, **k))[1]
    for B in args.batches:
        batch = make_batch(B, seed=B, target="docking_score").to(dev)
        batch.num_graphs = B
        plan = plan_from_data(batch)
        seg = R.molecule_segments(batch.batch, B)
        assert R._tail_limits_ok(seg, plan)
        sim = _block_rows(batch.x.shape[0], plan, dev, B)
        for p_head, p_ro in PROBS:
            torch.manual_seed(0)
            model = GNNModel(dropout_ratio=p_ro, ffn_dropout_rate=p_head).to(dev).eval()
            net = model.gnn_model
            mods = (net.graph_embedding_lin1, net.graph_embedding_lin2, model.ffn)
            pair = torch.tensor([1234, 7], dtype=torch.int64, device=dev)
            for S in args.samples:
                graphs, keep = {}, []
                with torch.no_grad():
                    graphs["predict"], out = _capture(lambda: model.predict(batch), dev)
                    keep.append(out)
                    del taken[:]
                    graphs["mc"], out = _capture(lambda: model.predict_mc(batch, S, alpha=-1.0, beta=1.0), dev)
                    assert len(taken) == 2, "predict_mc did not take the kernel route"
                    keep.append(out)
                    R._SCORE_MC = False
                    try:
                        del taken[:]
                        graphs["mc_torch"], out = _capture(lambda: model.predict_mc(batch, S, alpha=-1.0, beta=1.0), dev)
                        assert not taken, "predict_mc did not take the PyTorch route"
                    finally:
                        R._SCORE_MC = True
                    keep.append(out)
                    graphs["tail_score"], out = _capture(lambda: R.tail_score(sim, plan, LS, *mods, seg), dev)
                    keep.append(out)
                    graphs["tail_mc"], out = _capture(
                        lambda: real(sim, plan, LS, *mods, seg, S, p_head, p_ro, alpha=-1.0, beta=1.0, rng_pair=pair), dev)
                    keep.append(out)
                ms = _take_turns(graphs, args.replays, args.windows, args.warmup)
                line = {"batch": B, "atoms": int(batch.x.shape[0]), "p_head": p_head, "p_readout": p_ro, "samples": S,
                        "replays": args.replays, "windows": args.windows}
                for name, w in ms.items():
                    line[name + "_ms"] = round(statistics.median(w), 5)
                    line[name + "_spread_ms"] = round(max(w) - min(w), 5)
                line["mc_over_predict"] = round(line["mc_ms"] / line["predict_ms"], 3)
                line["mc_torch_over_mc"] = round(line["mc_torch_ms"] / line["mc_ms"], 3)
                line["tail_mc_minus_tail_score_us"] = round(1e3 * (line["tail_mc_ms"] - line["tail_score_ms"]), 2)
                line["windows_ms"] = {name: [round(m, 5) for m in w] for name, w in ms.items()}
                line["mean_sum"] = float(keep[1]["mean"].double().sum())
                print(json.dumps(line), flush=True)
                del graphs, keep
            del model


if __name__ == "__main__":
    main()
