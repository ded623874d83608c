"""``mkgnn_bootstrap_roc`` on the GPU against ``evaluation.bootstrap_reference``: ``two_u`` and ``n_pos`` EQUAL as integers, ``auc``
equal bit for bit, ``logauc`` within 1e-10 (about 16 (m + 2) 2^-53 < 1e-11 for the curve points of these shapes, a factor 10 over it
for the device's log10), NaN in the same places -- at both sides of every tile size and of the LDS form's boundary; the
independence of a replicate from everything but its own arguments, bit for bit; the captured call; the Python layers."""
import numpy as np
import pytest
import torch

from tests import _bootstrap_cases as BC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED, OFFSET = 11, 3


def _lib():
    from molkgnn_amd import _lib
    return _lib


def _dev(arrays):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in arrays)


def _host(out):
    torch.cuda.synchronize()
    return tuple(o.cpu().numpy() for o in out)


def _same_bits(a, b):
    """Four outputs against four outputs, bit for bit (a NaN equals the same NaN)."""
    return all(np.array_equal(x.view(np.int64) if x.dtype == np.float64 else x, y.view(np.int64) if y.dtype == np.float64 else y)
               for x, y in zip(a, b))


def _check(got, ref, what):
    auc, logauc, two_u, n_pos = got
    assert two_u.dtype == np.int64 and n_pos.dtype == np.int32 and auc.dtype == np.float64 and logauc.dtype == np.float64
    assert np.array_equal(n_pos, ref["n_pos"]), what
    assert np.array_equal(two_u, ref["two_u"]), what
    assert np.array_equal(auc.view(np.int64), ref["AUC"].view(np.int64)), what
    assert np.array_equal(np.isnan(logauc), np.isnan(ref["logAUC"])), what
    live = ~np.isnan(logauc)
    err = np.abs(logauc[live] - ref["logAUC"][live]).max(initial=0.0)
    print(f"{what}: |dlogAUC| = {err:.3g} over {int(live.sum())} defined replicates")
    assert err <= BC.LOGAUC_TOL, (what, err)


def _run(kind, n, B, window=(0.001, 0.1), stratified=False, seed=SEED, offset=OFFSET, workspace=None):
    from molkgnn_amd.readout import bootstrap_roc
    y, s = BC.case(kind, n)
    rank, ys, gl, split = BC.sorted_inputs(y, s, stratified)
    return _host(bootstrap_roc(*_dev((rank, ys, gl)), split, B, seed, offset, window[0], window[1], workspace=workspace))


def _edges():
    L = _lib()
    sizes = {1, 2, 3, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4097}
    for t in (L.BOOTSTRAP_TILE, L.BOOTSTRAP_DRAW_ROWS):
        sizes |= {t - 1, t, t + 1, 2 * t - 1, 2 * t, 2 * t + 1}
    edge = L.BOOTSTRAP_LDS_MAX_N
    sizes |= {edge - 1, edge, edge + 1}                         # the LDS form's boundary, both sides
    sizes |= {edge + L.BOOTSTRAP_TILE - 1, edge + L.BOOTSTRAP_TILE, edge + L.BOOTSTRAP_TILE + 1}      # tile edges of the workspace form
    return sorted(sizes)


@pytest.mark.parametrize("n", _edges())
def test_kernel_matches_the_definition_at_every_edge(n):
    kinds = ["distinct", "grid8", "grid1", "equal", "actives_last"] if n >= 2 else ["equal"]
    for kind in kinds:
        for stratified, window in ((False, (0.001, 0.1)), (True, (0.001, 1.0))):
            got = _run(kind, n, 7, window, stratified)
            _check(got, BC.reference(kind, n, 7, window, SEED, OFFSET, stratified), (kind, n, stratified))


@pytest.mark.parametrize("B", [1, 7, 64, 65])
def test_replicate_counts(B):
    edge = _lib().BOOTSTRAP_LDS_MAX_N
    for n in (257, edge + 1):
        _check(_run("grid8", n, B), BC.reference("grid8", n, B), ("grid8", n, B))


def test_a_tie_group_that_straddles_a_tile_edge():
    L = _lib()
    for n in (L.BOOTSTRAP_TILE + 40, L.BOOTSTRAP_LDS_MAX_N + 40):
        _check(_run("straddle", n, 16, (0.001, 1.0)), BC.reference("straddle", n, 16, (0.001, 1.0)), ("straddle", n))


def test_one_class_only_gives_nan_in_every_replicate():
    for n in (1, 300, _lib().BOOTSTRAP_LDS_MAX_N + 1):
        auc, logauc, two_u, n_pos = got = _run("one_class", n, 9)
        assert np.isnan(auc).all() and np.isnan(logauc).all() and (n_pos == 0).all() and (two_u == 0).all()
        _check(got, BC.reference("one_class", n, 9), ("one_class", n))


def test_every_split():
    """``split`` is the caller's: 0, 1, n - 1 and n rows in the first stratum, whatever the labels are."""
    from molkgnn_amd import evaluation as E
    from molkgnn_amd.readout import bootstrap_roc
    for n in (65, _lib().BOOTSTRAP_LDS_MAX_N + 1):
        y, s = BC.case("grid8", n)
        rank, ys, gl, _ = BC.sorted_inputs(y, s)
        dev = _dev((rank, ys, gl))
        for split in (0, 1, n - 1, n):
            got = _host(bootstrap_roc(*dev, split, 7, SEED, OFFSET, 0.001, 0.1))
            _check(got, E.bootstrap_reference_sorted(rank, ys, gl, split, 7, SEED, OFFSET, 0.001, 0.1), ("split", n, split))
    # split = 0 and split = n are the same single stratum
    assert _same_bits(_host(bootstrap_roc(*dev, 0, 7, SEED, OFFSET, 0.001, 0.1)), _host(bootstrap_roc(*dev, n, 7, SEED, OFFSET, 0.001, 0.1)))


def test_a_replicate_depends_on_its_own_arguments_alone():
    edge = _lib().BOOTSTRAP_LDS_MAX_N
    for n in (1025, edge + 1025):
        whole = _run("grid8", n, 65)
        # replicate b of a call at `offset` is replicate 0 of a call at `offset + b`
        for b in (1, 37, 64):
            one = _run("grid8", n, 1, offset=OFFSET + b)
            assert _same_bits(tuple(a[b:b + 1] for a in whole), one), (n, b)
        # 65 = 64 + 1
        head, tail = _run("grid8", n, 64), _run("grid8", n, 1, offset=OFFSET + 64)
        assert _same_bits(whole, tuple(np.concatenate(p) for p in zip(head, tail))), n
        # the same call twice
        assert _same_bits(whole, _run("grid8", n, 65)), n
    # a scratch sized for two replicates against the wrapper's own: 33 passes against one
    n = edge + 1025
    two = int(_lib().load().mkgnn_bootstrap_roc_workspace_bytes(n, 2))
    forced = _run("grid8", n, 65, workspace=torch.empty(two, dtype=torch.uint8, device=DEV))
    assert _same_bits(whole, forced)
    with pytest.raises(ValueError, match="workspace"):
        _run("grid8", n, 65, workspace=torch.empty(two // 2 - 64, dtype=torch.uint8, device=DEV))


def test_out_of_range_ranks_are_skipped_not_used_as_addresses():
    from molkgnn_amd.readout import bootstrap_roc
    for n in (300, _lib().BOOTSTRAP_LDS_MAX_N + 300):
        y, s = BC.case("grid8", n)
        rank, ys, gl, split = BC.sorted_inputs(y, s)
        rank = rank.copy()
        rank[::7] = np.where(np.arange(rank[::7].size) % 2 == 0, -1, n + 5)
        auc, logauc, two_u, n_pos = _host(bootstrap_roc(*_dev((rank, ys, gl)), split, 5, SEED, OFFSET, 0.001, 0.1))
        assert (n_pos >= 0).all() and (n_pos <= n).all() and (two_u >= 0).all()


@pytest.mark.parametrize("n", [300, None])
def test_captured_call_follows_new_scores(n):
    from molkgnn_amd import evaluation as E
    from molkgnn_amd.readout import bootstrap_roc
    n = _lib().BOOTSTRAP_LDS_MAX_N + 300 if n is None else n
    y = BC.labels(n, 1)
    first = BC.sorted_inputs(y, BC.scores("grid8", n, 1))
    static = _dev(first[:3])
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        bootstrap_roc(*static, n, 9, SEED, OFFSET, 0.001, 0.1)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            out = bootstrap_roc(*static, n, 9, SEED, OFFSET, 0.001, 0.1)
    torch.cuda.current_stream(DEV).wait_stream(side)
    seen = []
    for seed in (2, 3):
        s = BC.scores("grid8" if seed == 2 else "distinct", n, seed)
        for dst, src in zip(static, _dev(BC.sorted_inputs(y, s)[:3])):
            dst.copy_(src)
        for o in out:
            o.fill_(0)
        graph.replay()
        got = _host(out)
        _check(got, E.bootstrap_reference(y, s, 9, (0.001, 0.1), SEED, OFFSET), ("captured", n, seed))
        seen.append(got[2].copy())
    assert not np.array_equal(seen[0], seen[1])


@pytest.mark.parametrize("stratified", [False, True])
def test_metrics_on_cuda_against_cpu_copies(stratified):
    from molkgnn_amd import evaluation as E
    for n in (1500, _lib().BOOTSTRAP_LDS_MAX_N + 1500):
        y, s = BC.case("grid8", n)
        yt, st = torch.from_numpy(y), torch.from_numpy(s)
        kw = dict(n_boot=64, FPR_range=(0.001, 1.0), confidence=0.9, seed=5, offset=1 << 40, stratified=stratified)
        cpu = E.bootstrap_metrics(yt, st, **kw)
        gpu = E.bootstrap_metrics(yt.to(DEV), st.to(DEV), **kw)
        assert gpu["replicates"]["AUC"].is_cuda and gpu["replicates"]["logAUC"].is_cuda and gpu["n_pos"].is_cuda
        assert torch.equal(gpu["n_pos"].cpu(), cpu["n_pos"]) and gpu["n_undefined"] == cpu["n_undefined"] == 0
        assert torch.equal(gpu["replicates"]["AUC"].cpu().view(torch.int64), cpu["replicates"]["AUC"].view(torch.int64))
        assert float((gpu["replicates"]["logAUC"].cpu() - cpu["replicates"]["logAUC"]).abs().max()) <= BC.LOGAUC_TOL
        assert all(abs(gpu["point"][k] - cpu["point"][k]) <= 1e-12 for k in ("AUC", "logAUC"))       # (the existing functions' own pin)
        for name in ("AUC", "logAUC"):
            for key in ("mean", "std"):
                assert abs(gpu[name][key] - cpu[name][key]) <= BC.LOGAUC_TOL, (name, key)
            assert all(abs(a - b) <= BC.LOGAUC_TOL for a, b in zip(gpu[name]["ci"], cpu[name]["ci"])), name
        # the paired comparison on the device: the same resamples for both vectors, and a - a = 0
        other = torch.from_numpy(BC.scores("distinct", n, 8)).to(DEV)
        r = E.bootstrap_compare(yt.to(DEV), st.to(DEV), other, n_boot=16, seed=5, stratified=stratified)
        assert r["AUC"]["diff"].is_cuda and r["AUC"]["diff"].shape == (16,) and 0.0 <= r["AUC"]["p_a_better"] <= 1.0
        r = E.bootstrap_compare(yt.to(DEV), st.to(DEV), st.to(DEV).clone(), n_boot=16, seed=5, stratified=stratified)
        assert bool((r["logAUC"]["diff"] == 0).all()) and bool((r["AUC"]["diff"] == 0).all())


def test_float32_scores_and_the_raw_operator_refusals():
    from molkgnn_amd import evaluation as E
    from molkgnn_amd.readout import bootstrap_roc
    y, s = BC.case("distinct", 257)
    s32 = torch.from_numpy(s).float()
    gpu = E.bootstrap_metrics(torch.from_numpy(y).to(DEV), s32.to(DEV), n_boot=8)
    cpu = E.bootstrap_metrics(torch.from_numpy(y), s32, n_boot=8)
    assert torch.equal(gpu["replicates"]["AUC"].cpu().view(torch.int64), cpu["replicates"]["AUC"].view(torch.int64))
    rank, ys, gl = _dev(BC.sorted_inputs(y, s)[:3])
    for args, text in (((rank, ys, gl, 258, 4, 0, 0, 0.001, 0.1), "split"), ((rank, ys, gl, 257, 0, 0, 0, 0.001, 0.1), "n_boot"),
                       ((rank, ys, gl, 257, 4097, 0, 0, 0.001, 0.1), "n_boot"), ((rank, ys, gl, 257, 4, 0, 0, 0.0, 0.1), "FPR window"),
                       ((rank, ys, gl, 257, 4, 0, 0, 0.001, 1.5), "FPR window"), ((rank, ys[:-1], gl, 257, 4, 0, 0, 0.001, 0.1), "needs"),
                       ((rank, ys.cpu(), gl, 257, 4, 0, 0, 0.001, 0.1), "bootstrap_reference"), ((rank, ys, gl, 257, 4, -1, 0, 0.001, 0.1), "64-bit")):
        with pytest.raises(ValueError, match=text):
            bootstrap_roc(*args)


def test_evaluate_resident_with_bootstrap(tmp_path):
    from molkgnn_amd import evaluation as E
    from molkgnn_amd.train import evaluate_resident
    from tests._resident_library import build_library
    model, residents, _ = build_library(tmp_path, DEV, counts=(70,), shard_seed=40,
                                        labels=lambda n: (torch.arange(n) % 3 == 0).float(), model_seed=0, num_layers=3)
    model.train()
    plain = evaluate_resident(model, residents[0], 32, ("AUC",))
    assert model.training and "bootstrap" not in plain
    got = evaluate_resident(model, residents[0], 32, ("AUC",), bootstrap=64)
    assert model.training                                      # handed back in the mode it came in
    assert set(got) == set(plain) | {"bootstrap"} and got["AUC"] == plain["AUC"]
    assert torch.equal(got["pred_y"], plain["pred_y"])
    block = got["bootstrap"]
    assert block["n_boot"] == 64 and block["replicates"]["logAUC"].shape == (64,) and block["replicates"]["logAUC"].is_cuda
    assert block["point"]["AUC"] == plain["AUC"]
    want = E.bootstrap_metrics(got["true_y"].cpu(), got["pred_y"].cpu(), n_boot=64)
    assert torch.equal(block["n_pos"].cpu(), want["n_pos"])
    assert torch.equal(block["replicates"]["AUC"].cpu().view(torch.int64), want["replicates"]["AUC"].view(torch.int64))
    assert float((block["replicates"]["logAUC"].cpu() - want["replicates"]["logAUC"]).abs().nan_to_num().max()) <= BC.LOGAUC_TOL
    lo, hi = block["AUC"]["ci"]
    assert lo <= block["AUC"]["mean"] <= hi
    with pytest.raises(ValueError, match="bootstrap"):
        evaluate_resident(model, residents[0], 32, ("AUC",), bootstrap=0)
