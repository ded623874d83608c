"""What MaxMin picking costs: ``mkgnn_maxmin_pick`` against the same rounds written in torch operators, on the same tensors, in one
process, the two taking turns window by window.

    python tools/maxmin_timing.py [--cases 1024:100 65536:1024] [--once 1048576:1024] [--widths 32 64] [--windows 10] [--steps 4]

Per case ``n:k`` and width ``H`` (clustered embeddings: ``n // 6`` random centres, rows = centre + 0.08 noise at a random scale; the
walk starts at row 0 on both routes: its start value is the only one below every cosine):

``kernel``  ONE call of ``readout.maxmin_pick`` (``n <= 1024``: the init and one one-workgroup launch; beyond: the init and ``2 k``
            launches) captured into a graph and replayed: the median of ``--windows`` windows of ``--steps`` replays (device events)
``torch``   the same ``k`` rounds in torch operators -- the only route there was: the rows normalised once, then per round a masked
            ``argmin`` over ``cur``, ONE ``mv`` of the normalised rows with the pick's, compare-and-select into ``cur`` and the leader.
            Captured and replayed like the kernel where the capture succeeds, launched eagerly (host clock around a synchronise)
            where it does not; the line says which
``floor``   what the update launches cannot go below: ``k`` passes over ``n H 4`` bytes at the HBM bandwidth of the data sheet (8
            TB/s), and the share of it the kernel reaches.  (A matrix that fits the 256 MiB last-level cache is not read from HBM
            every round: there the share can exceed 1.)

``--once`` cases run each route once to warm up and ONCE timed (a single window of one replay): the largest size, where the
spread between windows is not what is asked.  The picks of the two routes are compared at every timed size (the torch
similarities are not the kernel's bits; on clustered rows the decisions do not hang on the last bit, and a difference is reported,
not hidden).  One JSON line per measurement with every window, then a summary line."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_BYTES_PER_S = 8.0e12


def clustered(n, H, seed, dev):
    import torch
    g = torch.Generator().manual_seed(seed)
    centres = torch.randn(max(2, n // 6), H, generator=g)
    rows = centres[torch.randint(0, len(centres), (n,), generator=g)] + 0.08 * torch.randn(n, H, generator=g)
    rows *= torch.exp(torch.empty(n).uniform_(-3.0, 3.0, generator=g))[:, None]
    return rows.to(dev)


def torch_maxmin(unit, start, k, picks):
    """``k`` rounds in torch operators over normalised rows ``unit [n, H]``: fills ``picks`` (int64 ``[k]``), returns ``(leader, cur)``.
    Everything stays on the device; no stop rule (the timed cases have none)."""
    import torch
    n, dev = unit.shape[0], unit.device
    cur = start.clone()
    candidate = torch.ones(n, dtype=torch.bool, device=dev)
    leader = torch.full((n,), -1, dtype=torch.int64, device=dev)
    far = torch.full((n,), float("inf"), dtype=torch.float32, device=dev)
    for t in range(k):
        i = torch.argmin(torch.where(candidate, cur, far)).reshape(1)          # masked arg-min
        s = unit.mv(unit.index_select(0, i)[0])                                 # one matrix-vector pass
        nearer = s > cur                                                        # compare-and-select
        cur = torch.where(nearer, s, cur)
        leader = torch.where(nearer, i, leader)
        candidate.index_fill_(0, i, False)
        picks[t:t + 1] = i
    return leader, cur


def capture(fn, dev):
    """``fn`` run once on a side stream, then captured there: the graph, or None with the reason when the capture fails."""
    import torch
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    try:
        with torch.cuda.stream(side):
            fn()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=side):
                fn()
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize()
        return graph, None
    except Exception as exc:                                       # (reported in the line: the route is then timed eagerly)
        torch.cuda.synchronize()
        return None, f"{type(exc).__name__}: {exc}"[:200]


def window_ms(graph, fn, steps):
    import torch
    if graph is None:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / steps
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(steps):
        graph.replay()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / steps


def time_case(n, k, H, windows, steps, dev):
    import torch
    from molkgnn_amd import _lib
    from molkgnn_amd.readout import maxmin_pick
    emb = clustered(n, H, 2000 + n + H, dev)
    start = torch.full((n,), -1.5, dtype=torch.float32, device=dev)
    start[0] = -2.0
    out = (torch.empty(k, dtype=torch.int32, device=dev), torch.empty(k, dtype=torch.float32, device=dev),
           torch.empty(1, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev),
           torch.empty(n, dtype=torch.float32, device=dev))
    unit = torch.nn.functional.normalize(emb, dim=1, eps=1e-8)
    torch_picks = torch.empty(k, dtype=torch.int64, device=dev)
    state = {}

    def kernel():
        maxmin_pick(emb, k, None, start, out=out)

    def by_torch():
        state["leader"], state["cur"] = torch_maxmin(unit, start, k, torch_picks)

    kernel_graph, kernel_why = capture(kernel, dev)
    torch_graph, torch_why = capture(by_torch, dev)
    ms = {"kernel": [], "torch": []}
    for _ in range(windows):                                       # (the routes take turns: drift hits them alike)
        ms["kernel"].append(window_ms(kernel_graph, kernel, steps))
        ms["torch"].append(window_ms(torch_graph, by_torch, steps))
    same = int((out[0].long() == torch_picks).sum())
    first_difference = -1 if same == k else int(torch.nonzero(out[0].long() != torch_picks)[0])
    kernel_ms, torch_ms = statistics.median(ms["kernel"]), statistics.median(ms["torch"])
    floor_ms = k * n * H * 4 / HBM_BYTES_PER_S * 1e3
    one_workgroup = n <= _lib.MAXMIN_TILE
    return {"rows": n, "picks": k, "width": H, "form": "one workgroup" if one_workgroup else "two launches per round",
            "n_picks": int(out[2]), "kernel_ms": round(kernel_ms, 4), "kernel_windows_ms": [round(v, 4) for v in ms["kernel"]],
            "kernel_captured": kernel_graph is not None, "kernel_capture_error": kernel_why,
            "torch_ms": round(torch_ms, 4), "torch_windows_ms": [round(v, 4) for v in ms["torch"]],
            "torch_captured": torch_graph is not None, "torch_capture_error": torch_why,
            "torch_over_kernel": round(torch_ms / kernel_ms, 2), "kernel_us_per_round": round(kernel_ms * 1e3 / k, 3),
            "floor_ms": None if one_workgroup else round(floor_ms, 4),
            "share_of_floor": None if one_workgroup else round(floor_ms / kernel_ms, 3),
            "emb_megabytes": round(n * H * 4 / 2 ** 20, 1), "windows": windows, "steps": steps,
            "same_picks": same == k, "first_different_pick": first_difference}


def parse_case(text):
    n, k = text.split(":")
    return int(n), int(k)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="*", default=["1024:100", "65536:1024"], help="rows:picks, timed over --windows windows")
    ap.add_argument("--once", nargs="*", default=["1048576:1024"], help="rows:picks, each route run once")
    ap.add_argument("--widths", type=int, nargs="*", default=[32, 64])
    ap.add_argument("--windows", type=int, default=10)
    ap.add_argument("--steps", type=int, default=4)
    a = ap.parse_args()
    sys.path.insert(0, REPO)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("maxmin_timing.py measures on the GPU: none is available (nothing is measured on the CPU)")
    dev = torch.device("cuda:0")
    lines = []
    for text, windows, steps in [(c, a.windows, a.steps) for c in a.cases] + [(c, 1, 1) for c in a.once]:
        n, k = parse_case(text)
        for H in a.widths:
            line = time_case(n, k, H, windows, steps, dev)
            print(json.dumps(line), flush=True)
            lines.append(line)
    keys = ("rows", "picks", "width", "form", "kernel_ms", "torch_ms", "torch_over_kernel", "torch_captured", "share_of_floor",
            "same_picks", "windows")
    print(json.dumps({"summary": [{key: r[key] for key in keys} for r in lines]}), flush=True)


if __name__ == "__main__":
    main()
