"""``mkgnn_bootstrap_early`` on the GPU against ``evaluation.early_reference``: ``auc``, ``logauc``, ``two_u`` and ``n_pos`` EQUAL to
``mkgnn_bootstrap_roc``'s bit for bit on the same inputs, ``hits`` equal to the definition bit for bit, ``ap`` and ``rie`` within a
relative 1e-10 (``tests/_bootstrap_cases.LOGAUC_TOL``: the derivation gives (m + 16) 2^-53 < 1e-11 for the m positive terms of these
shapes, a factor 10 over it for the device's exp and expm1) -- at both sides of every tile size and of the LDS form's boundary;
cuts around a tie group that straddles a tile edge; the independence of a replicate from everything but its own arguments; inputs
outside their ranges behind guard words; the captured call; the Python layers."""
import numpy as np
import pytest
import torch

from tests import _bootstrap_cases as BC
from tests import _early_cases as EC
from tests.test_bootstrap_gpu import _dev, _edges, _host, _lib, _same_bits

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED, OFFSET = 11, 3
WINDOW = (0.001, 0.1)


def _run(inputs, split, B, cuts, alphas=EC.ALPHAS, seed=SEED, offset=OFFSET, window=WINDOW, workspace=None):
    from molkgnn_amd.readout import bootstrap_early
    return _host(bootstrap_early(*inputs, split, B, seed, offset, window[0], window[1], cuts, alphas, workspace=workspace))


def _roc(inputs, split, B, seed=SEED, offset=OFFSET, window=WINDOW):
    from molkgnn_amd.readout import bootstrap_roc
    return _host(bootstrap_roc(*inputs, split, B, seed, offset, window[0], window[1]))


def _check(got, roc, ref, what):
    """The seven outputs of one call against ``bootstrap_roc``'s four and the definition's three; returns the two errors."""
    assert _same_bits(got[:4], roc), what
    ap, hits, rie = got[4:]
    assert ap.dtype == hits.dtype == rie.dtype == np.float64 and hits.shape == ref["hits"].shape and rie.shape == ref["rie"].shape
    assert np.array_equal(got[3], ref["n_pos"]), what
    assert np.array_equal(hits.view(np.int64), ref["hits"].view(np.int64)), what
    e_ap, e_rie = EC.relative_error(ap, ref["ap"]), EC.relative_error(rie, ref["rie"])
    print(f"{what}: relative |d ap| = {e_ap:.3g}, |d rie| = {e_rie:.3g}")
    assert e_ap <= BC.LOGAUC_TOL and e_rie <= BC.LOGAUC_TOL, (what, e_ap, e_rie)
    return e_ap, e_rie


@pytest.mark.parametrize("n", _edges())
def test_kernel_matches_the_definition_at_every_edge(n):
    cuts = EC.cuts_for(n, _lib().BOOTSTRAP_TILE)
    worst = (0.0, 0.0)
    for kind in (["distinct", "grid8", "grid1", "equal", "actives_last"] if n >= 2 else ["equal"]):
        y, s = BC.case(kind, n)
        for stratified, window in ((False, (0.001, 0.1)), (True, (0.001, 1.0))):
            rank, ys, gl, split = BC.sorted_inputs(y, s, stratified)
            inputs = _dev((rank, ys, gl))
            got = _run(inputs, split, 7, cuts, window=window)
            errs = _check(got, _roc(inputs, split, 7, window=window), EC.reference(kind, n, 7, cuts, EC.ALPHAS, SEED, OFFSET, stratified),
                          (kind, n, stratified))
            worst = tuple(max(a, b) for a, b in zip(worst, errs))
    print(f"n = {n}: worst relative errors ap {worst[0]:.3g} rie {worst[1]:.3g}")


def test_cuts_around_a_tie_group_that_straddles_a_tile_edge():
    """Per replicate (one call each: the cuts are the call's) a cut strictly inside the drawn rows of the tie group that crosses the tile
    edge, one exactly at its end, and one on the first drawn row behind it."""
    from molkgnn_amd import evaluation as E
    L = _lib()
    t = L.BOOTSTRAP_TILE
    seen_inside = 0
    for n in (t + 40, L.BOOTSTRAP_LDS_MAX_N + 40):
        y, s = BC.case("straddle", n)
        rank, ys, gl, split = BC.sorted_inputs(y, s)
        inputs = _dev((rank, ys, gl))
        for b in range(6):
            c = np.bincount(rank[BC.draws(n, split, SEED, OFFSET + b)], minlength=n)
            before, rows = int(c[:t - 3].sum()), int(c[t - 3:t + 3].sum())
            cuts = tuple(k for k in (before + max(1, rows // 2), before + rows, before + rows + 1) if 1 <= k <= n)
            seen_inside += rows >= 2
            ref = E.early_reference_sorted(rank, ys, gl, split, 1, SEED, OFFSET + b, cuts, EC.ALPHAS)
            _check(_run(inputs, split, 1, cuts, offset=OFFSET + b), _roc(inputs, split, 1, offset=OFFSET + b), ref, ("straddle", n, b))
    assert seen_inside >= 6                                     # (most replicates draw two or more of the group's six rows)


def test_one_class_only():
    from molkgnn_amd import evaluation as E
    for n in (1, 300, _lib().BOOTSTRAP_LDS_MAX_N + 1):
        y, s = BC.case("one_class", n)
        rank, ys, gl, split = BC.sorted_inputs(y, s)
        inputs = _dev((rank, ys, gl))
        cuts = EC.cuts_for(n)
        got = _run(inputs, split, 9, cuts)
        ref = EC.reference("one_class", n, 9, cuts)
        _check(got, _roc(inputs, split, 9), ref, ("one_class", n))
        assert (got[3] == 0).all() and (got[4] == 0).all() and (got[5] == 0).all() and (got[6] == 0).all() and ref["n_undefined"] == 9
        d = E.early_derived(*(torch.from_numpy(a) for a in (got[4], got[5], got[6], got[3])), n, cuts, EC.ALPHAS)
        assert all(bool(torch.isnan(d[k]).all()) for k in ("AP", "EF", "BEDROC"))


def test_no_cuts_and_no_alphas():
    n = 1025
    y, s = BC.case("grid8", n)
    rank, ys, gl, split = BC.sorted_inputs(y, s)
    inputs = _dev((rank, ys, gl))
    roc = _roc(inputs, split, 5)
    full = _run(inputs, split, 5, (3, 700), (20.0, 0.5))
    for cuts, alphas in (((), ()), ((), (20.0, 0.5)), ((3, 700), ())):
        got = _run(inputs, split, 5, cuts, alphas)
        assert got[5].shape == (5, len(cuts)) and got[6].shape == (5, len(alphas))
        assert _same_bits(got[:4], roc) and _same_bits(got[4:5], full[4:5])
        assert (not cuts or _same_bits(got[5:6], full[5:6])) and (not alphas or _same_bits(got[6:7], full[6:7]))


def test_a_replicate_depends_on_its_own_arguments_alone():
    edge = _lib().BOOTSTRAP_LDS_MAX_N
    for n in (1025, edge + 1025):
        y, s = BC.case("grid8", n)
        rank, ys, gl, split = BC.sorted_inputs(y, s)
        inputs = _dev((rank, ys, gl))
        cuts = EC.cuts_for(n)
        whole = _run(inputs, split, 65, cuts)
        # replicate b of a call at `offset` is replicate 0 of a call at `offset + b`
        for b in (1, 37, 64):
            assert _same_bits(tuple(a[b:b + 1] for a in whole), _run(inputs, split, 1, cuts, offset=OFFSET + b)), (n, b)
        # 65 = 64 + 1
        head, tail = _run(inputs, split, 64, cuts), _run(inputs, split, 1, cuts, offset=OFFSET + 64)
        assert _same_bits(whole, tuple(np.concatenate(p) for p in zip(head, tail))), n
        # the same call twice
        assert _same_bits(whole, _run(inputs, split, 65, cuts)), n
    # a scratch that holds ONE replicate against the wrapper's own: 65 passes against one
    one = int(_lib().load().mkgnn_bootstrap_roc_workspace_bytes(n, 1))
    assert _same_bits(whole, _run(inputs, split, 65, cuts, workspace=torch.empty(one, dtype=torch.uint8, device=DEV)))
    with pytest.raises(ValueError, match="workspace"):
        _run(inputs, split, 65, cuts, workspace=torch.empty(one - 64, dtype=torch.uint8, device=DEV))


def _guarded_call(inputs, n, split, B, cuts, alphas):
    """The C entry with its six float64 / int64 outputs inside ONE buffer and ``n_pos`` inside another, 32 guard words around each
    output; returns the outputs (host) after checking that every guard word still holds its pattern."""
    lib = _lib().load()
    J, A, G = len(cuts), len(alphas), 32
    sizes = [B, B, B, B, B * J, B * A]                          # auc, logauc, two_u, ap, hits, rie in 8-byte words
    starts = [G + sum(sizes[:i]) + G * i for i in range(6)]
    total = starts[-1] + sizes[-1] + G
    pattern = 0x7ff8dead0badf00d                                # (as a double: a NaN with a payload)
    buf = torch.full((total,), pattern, dtype=torch.int64, device=DEV)
    nbuf = torch.full((B + 2 * G,), 0x0badf00d, dtype=torch.int32, device=DEV)
    cuts_t = torch.tensor(cuts, dtype=torch.int32, device=DEV)
    alphas_t = torch.tensor(alphas, dtype=torch.float64, device=DEV)
    ptr = [buf.data_ptr() + 8 * st for st in starts]
    ws = torch.empty(int(lib.mkgnn_bootstrap_roc_workspace_bytes(n, B)), dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    rc = lib.mkgnn_bootstrap_early(inputs[0].data_ptr(), inputs[1].data_ptr(), inputs[2].data_ptr(), n, split, B, SEED, OFFSET, WINDOW[0],
                                   WINDOW[1], cuts_t.data_ptr(), J, alphas_t.data_ptr(), A, ptr[0], ptr[1], ptr[2],
                                   nbuf.data_ptr() + 4 * G, ptr[3], ptr[4], ptr[5], ws.data_ptr(), ws.numel(), _lib().stream_ptr(buf.device))
    assert rc == 0, lib.mkgnn_last_error().decode()
    torch.cuda.synchronize()
    host, nhost = buf.cpu().numpy(), nbuf.cpu().numpy()
    guard = np.ones(total, dtype=bool)
    for st, w in zip(starts, sizes):
        guard[st:st + w] = False
    assert int(guard.sum()) == 7 * G and (host[guard] == pattern).all()
    assert (nhost[:G] == 0x0badf00d).all() and (nhost[G + B:] == 0x0badf00d).all()
    auc, logauc, two_u, ap, hits, rie = (host[st:st + w].copy() for st, w in zip(starts, sizes))
    return (auc.view(np.float64), logauc.view(np.float64), two_u, nhost[G:G + B].copy(), ap.view(np.float64),
            hits.view(np.float64).reshape(B, J), rie.view(np.float64).reshape(B, A))


def test_inputs_outside_their_ranges_change_nothing_else():
    """Cuts outside [1, n] and alphas outside (0, 500] (or NaN) give NaN columns; ranks outside [0, n) are skipped; every output sits
    between guard words that must survive."""
    for n in (300, _lib().BOOTSTRAP_LDS_MAX_N + 300):
        y, s = BC.case("grid8", n)
        rank, ys, gl, split = BC.sorted_inputs(y, s)
        inputs = _dev((rank, ys, gl))
        good = _guarded_call(inputs, n, split, 5, (5, n), (20.0,))
        assert _same_bits(good, _run(inputs, split, 5, (5, n), (20.0,)))
        bad = _guarded_call(inputs, n, split, 5, (0, 5, n + 1, -3, n, 1 << 30), (0.0, 20.0, float("nan"), 501.0))
        assert _same_bits(bad[:5], good[:5])
        assert np.isnan(bad[5][:, [0, 2, 3, 5]]).all() and _same_bits((np.ascontiguousarray(bad[5][:, [1, 4]]),), good[5:6])
        assert np.isnan(bad[6][:, [0, 2, 3]]).all() and _same_bits((np.ascontiguousarray(bad[6][:, 1:2]),), good[6:7])
        broken = rank.copy()
        broken[::7] = np.where(np.arange(broken[::7].size) % 2 == 0, -1, n + 5)
        out = _guarded_call(_dev((broken, ys, gl)), n, split, 5, (5, n), (20.0,))
        assert (out[3] >= 0).all() and (out[3] <= n).all() and (out[2] >= 0).all()
        assert (out[5] >= 0).all() and (out[5] <= out[3][:, None]).all() and np.isfinite(out[4]).all() and np.isfinite(out[6]).all()


@pytest.mark.parametrize("n", [300, None])
def test_captured_call_follows_new_scores_cuts_and_alphas(n):
    from molkgnn_amd import evaluation as E
    from molkgnn_amd.readout import bootstrap_early
    n = _lib().BOOTSTRAP_LDS_MAX_N + 300 if n is None else n
    y = BC.labels(n, 1)
    static = _dev(BC.sorted_inputs(y, BC.scores("grid8", n, 1))[:3])
    cuts_t = torch.tensor([1, n], dtype=torch.int32, device=DEV)
    alphas_t = torch.tensor([20.0, 0.5], dtype=torch.float64, device=DEV)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        bootstrap_early(*static, n, 9, SEED, OFFSET, 0.001, 0.1, cuts_t, alphas_t)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            out = bootstrap_early(*static, n, 9, SEED, OFFSET, 0.001, 0.1, cuts_t, alphas_t)
    torch.cuda.current_stream(DEV).wait_stream(side)
    seen = []
    for seed, cuts, alphas in ((2, (7, n // 2), (160.9, 20.0)), (3, (n - 1, 2), (5.0, 80.5))):
        s = BC.scores("grid8" if seed == 2 else "distinct", n, seed)
        rank, ys, gl, split = BC.sorted_inputs(y, s)
        for dst, src in zip(static, _dev((rank, ys, gl))):
            dst.copy_(src)
        cuts_t.copy_(torch.tensor(cuts, dtype=torch.int32))
        alphas_t.copy_(torch.tensor(alphas, dtype=torch.float64))
        for o in out:
            o.fill_(0)
        graph.replay()
        got = _host(out)
        _check(got, _roc(static, n, 9), E.early_reference_sorted(rank, ys, gl, split, 9, SEED, OFFSET, cuts, alphas), ("captured", n, seed))
        seen.append(got[5].copy())
    assert not np.array_equal(seen[0], seen[1])


def test_metrics_on_cuda_against_cpu_copies():
    from molkgnn_amd import evaluation as E
    names = ("AP", "EF_0.01", "BEDROC_20")
    for n in (4097, _lib().BOOTSTRAP_LDS_MAX_N + 1):
        y, s = BC.case("grid8", n)
        yt, st = torch.from_numpy(y), torch.from_numpy(s)
        kw = dict(n_boot=32, confidence=0.9, seed=5, offset=1 << 40, early=names)
        cpu = E.bootstrap_metrics(yt, st, **kw)
        gpu = E.bootstrap_metrics(yt.to(DEV), st.to(DEV), **kw)
        assert gpu["cuts"] == cpu["cuts"] == {"EF_0.01": E.early_cut(0.01, n)} and torch.equal(gpu["n_pos"].cpu(), cpu["n_pos"])
        assert torch.equal(gpu["replicates"]["AUC"].cpu().view(torch.int64), cpu["replicates"]["AUC"].view(torch.int64))
        # EF is the exact hits through the same shared function on both routes
        assert torch.equal(gpu["replicates"]["EF_0.01"].cpu().view(torch.int64), cpu["replicates"]["EF_0.01"].view(torch.int64))
        for name in names:
            g, c = gpu["replicates"][name], cpu["replicates"][name]
            assert g.is_cuda and g.shape == (32,)
            err = float(((g.cpu() - c).abs() / c.abs()).max())
            print(f"n = {n} {name}: relative error of the replicates {err:.3g}")
            assert err <= BC.LOGAUC_TOL, (n, name, err)
            assert abs(gpu["point"][name] - cpu["point"][name]) <= BC.LOGAUC_TOL * abs(cpu["point"][name]), name
            assert abs(gpu[name]["mean"] - cpu[name]["mean"]) <= BC.LOGAUC_TOL * abs(cpu[name]["mean"]), name
            assert all(abs(a - b) <= BC.LOGAUC_TOL * abs(b) for a, b in zip(gpu[name]["ci"], cpu[name]["ci"])), name
        # without names the device route is the ROC-only call: the same first keys and values
        plain = E.bootstrap_metrics(yt.to(DEV), st.to(DEV), n_boot=32, confidence=0.9, seed=5, offset=1 << 40)
        assert set(plain) == set(gpu) - set(names) - {"cuts"}
        assert torch.equal(plain["replicates"]["logAUC"].view(torch.int64), gpu["replicates"]["logAUC"].view(torch.int64))
        r = E.bootstrap_compare(yt.to(DEV), st.to(DEV), st.to(DEV).clone(), n_boot=8, seed=5, early=names)
        assert all(bool((r[k]["diff"] == 0).all()) and r[k]["diff"].is_cuda for k in names)


def test_evaluate_resident_with_an_early_metric_and_the_bootstrap(tmp_path):
    from molkgnn_amd import evaluation as E
    from molkgnn_amd.train import evaluate_resident
    from tests._resident_library import build_library
    model, residents, _ = build_library(tmp_path, DEV, counts=(70,), shard_seed=40,
                                        labels=lambda n: (torch.arange(n) % 3 == 0).float(), model_seed=0, num_layers=3)
    plain = evaluate_resident(model, residents[0], 32, ("AUC",), bootstrap=16)
    got = evaluate_resident(model, residents[0], 32, ("AUC", "EF_0.01"), bootstrap=16)
    assert set(got) == set(plain) | {"EF_0.01"} and got["AUC"] == plain["AUC"] and torch.equal(got["pred_y"], plain["pred_y"])
    assert got["EF_0.01"] == E.calculate_enrichment_factor(got["true_y"], got["pred_y"], 0.01)
    assert "EF_0.01" not in plain["bootstrap"] and "cuts" not in plain["bootstrap"]
    block = got["bootstrap"]
    assert block["cuts"] == {"EF_0.01": 1} and block["point"]["EF_0.01"] == got["EF_0.01"]
    assert block["replicates"]["EF_0.01"].shape == (16,) and block["replicates"]["EF_0.01"].is_cuda
    assert torch.equal(block["replicates"]["AUC"].view(torch.int64), plain["bootstrap"]["replicates"]["AUC"].view(torch.int64))
    want = E.bootstrap_metrics(got["true_y"].cpu(), got["pred_y"].cpu(), n_boot=16, early=("EF_0.01",))
    assert torch.equal(block["replicates"]["EF_0.01"].cpu().view(torch.int64), want["replicates"]["EF_0.01"].view(torch.int64))
    with pytest.raises(ValueError, match="fraction"):
        evaluate_resident(model, residents[0], 32, ("EF_7",), bootstrap=16)


def test_the_c_entry_refuses_before_any_launch():
    lib = _lib().load()
    n, B = 300, 4
    y, s = BC.case("grid8", n)
    rank, ys, gl = _dev(BC.sorted_inputs(y, s)[:3])
    f64 = [torch.full((64,), 7.0, dtype=torch.float64, device=DEV) for _ in range(5)]       # auc, logauc, ap, hits, rie
    two_u = torch.full((B,), 7, dtype=torch.int64, device=DEV)
    n_pos = torch.full((B,), 7, dtype=torch.int32, device=DEV)
    cuts = torch.tensor([1, 5], dtype=torch.int32, device=DEV)
    alphas = torch.tensor([20.0, 0.5], dtype=torch.float64, device=DEV)
    ok = dict(rank=rank.data_ptr(), ys=ys.data_ptr(), gl=gl.data_ptr(), n=n, B=B, cuts=cuts.data_ptr(), J=2, alphas=alphas.data_ptr(), A=2,
              auc=f64[0].data_ptr(), logauc=f64[1].data_ptr(), two_u=two_u.data_ptr(), n_pos=n_pos.data_ptr(), ap=f64[2].data_ptr(),
              hits=f64[3].data_ptr(), rie=f64[4].data_ptr(), ws=None, wsb=0)
    big = _lib().BOOTSTRAP_LDS_MAX_N + 1
    for kw, text in ((dict(ap=None), "null pointer"), (dict(cuts=None), "null pointer"), (dict(rie=None), "null pointer"),
                     (dict(J=9), "cuts outside"), (dict(A=5), "alphas outside"), (dict(J=-1), "cuts outside"), (dict(B=4097), "replicates outside"),
                     (dict(n=(1 << 22) + 1), "rows outside"), (dict(hits=f64[3].data_ptr() + 4), "misaligned"),
                     (dict(alphas=alphas.data_ptr() + 4), "misaligned"), (dict(cuts=cuts.data_ptr() + 2), "misaligned"),
                     (dict(ap=rank.data_ptr()), "aliases rank"), (dict(hits=alphas.data_ptr()), "cuts or alphas"),
                     (dict(rie=f64[3].data_ptr() + 8), "alias each other"), (dict(ap=f64[0].data_ptr()), "alias each other"),
                     (dict(n=big), "null workspace"), (dict(n=big, ws=f64[4].data_ptr() + 256, wsb=64), "workspace of 64 bytes")):
        a = dict(ok, **kw)
        rc = lib.mkgnn_bootstrap_early(a["rank"], a["ys"], a["gl"], a["n"], a["n"], a["B"], SEED, OFFSET, 0.001, 0.1, a["cuts"], a["J"],
                                       a["alphas"], a["A"], a["auc"], a["logauc"], a["two_u"], a["n_pos"], a["ap"], a["hits"], a["rie"],
                                       a["ws"], a["wsb"], None)
        assert rc != 0 and text in lib.mkgnn_last_error().decode(), (kw, lib.mkgnn_last_error().decode())
    torch.cuda.synchronize()
    assert all(bool((t == 7).all()) for t in f64 + [two_u, n_pos])      # nothing was launched: no output was written
