"""``mkgnn_maxmin_pick`` on the GPU.  All five outputs against the host walk (``maxmin_pick_reference``) over ``mkgnn_embed_cosine``'s
own float32 similarities -- bits, every row, on both forms and at their edge, with the stop AT a similarity the run produced -- and
against the walk over the float64 cosine; planted hazards; a deck and excluded rows; strides, sentinels, capture; what the C ABI
rejects; the torch route beyond ``H = 64``."""
import functools

import numpy as np
import pytest
import torch

from tests import _maxmin_cases as MC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
INF = float("inf")


def _bits(t):
    return t.detach().contiguous().view(torch.int32).cpu().numpy()


def _all_sims(e):
    """``sim [n, n]`` on the host: ``mkgnn_embed_cosine`` of every row with the rows as queries, in groups of 32."""
    from molkgnn_amd.readout import embedding_cosine
    n = e.shape[0]
    out = torch.empty(n, n, dtype=torch.float32, device=e.device)
    for a in range(0, n, 32):
        out[:, a:a + 32] = embedding_cosine(e, e[a:a + 32])
    return out.cpu().numpy()


def _same_floats(got, want):
    """Equal by bit pattern apart from NaN, which only has to be NaN on both sides."""
    some = ~np.isnan(want)
    return np.array_equal(got.view(np.int32)[some], want.view(np.int32)[some]) and bool(np.isnan(got[~some]).all())


def _agree(got, sim, k, stop_sim=INF, start=None):
    """The five outputs are the host walk over ``sim``: indices equal, ``pick_sim`` and ``leader_sim`` by bit pattern apart from NaN."""
    from molkgnn_amd.screening import maxmin_pick_reference
    picks, pick_sim, n_picks, leader, leader_sim = got
    n = sim.shape[0]
    assert picks.dtype == n_picks.dtype == leader.dtype == torch.int32 and pick_sim.dtype == leader_sim.dtype == torch.float32
    assert tuple(picks.shape) == tuple(pick_sim.shape) == (k,) and tuple(n_picks.shape) == (1,)
    assert tuple(leader.shape) == tuple(leader_sim.shape) == (n,)
    wp, ws, wn, wl, wls = maxmin_pick_reference(sim, k, stop_sim, None if start is None else start.cpu().numpy())
    what = (n, k, stop_sim)
    assert int(n_picks) == wn, (what, int(n_picks), wn)
    assert np.array_equal(picks.cpu().numpy(), wp), what
    assert _same_floats(pick_sim.cpu().numpy(), ws), what
    assert np.array_equal(leader.cpu().numpy(), wl), what
    assert _same_floats(leader_sim.cpu().numpy(), wls), what
    return wp[:wn], ws[:wn], wl


@functools.lru_cache(maxsize=None)
def _cases(H):
    """Every size at width ``H``: the input on the device and ``mkgnn_embed_cosine``'s similarities, computed once."""
    cases = []
    for n in MC.SIZES:
        e = torch.from_numpy(MC.clustered(n, H, MC.seed_of(n, H))).to(DEV)
        cases.append((n, e, _all_sims(e)))
    return cases


@pytest.mark.parametrize("H", MC.WIDTHS)
def test_bits_are_the_walk_over_embed_cosines_own_similarities(H):
    from molkgnn_amd.readout import maxmin_pick
    for n, e, sim in _cases(H):
        k = min(n, 48)
        picks, taken, leader = _agree(maxmin_pick(e, k), sim, k)
        assert picks[0] == 0 and (H == 1 or len(picks) == k)       # (at width 1 every row is one of two directions)
        assert (taken[1:] >= taken[:-1]).all()
        _agree(maxmin_pick(e, 1), sim, 1)
        if n == 5:
            _agree(maxmin_pick(e, n), sim, n)
        # a stop: it decides the count, about one pick per cluster
        k = min(n, 512)
        stopped, _, leader = _agree(maxmin_pick(e, k, 0.9), sim, k, 0.9)
        if n >= MC.TILE - 1:
            assert len(stopped) < k
            if H > 1:
                assert 0.8 * n / 6 <= len(stopped) <= n / 6 + 10, (H, n, len(stopped))
                lsim = sim[np.arange(n), leader]                   # with the rows exhausted by the stop, every row lies within it
                assert (leader >= 0).all() and ((lsim >= np.float32(0.9)) | (leader == np.arange(n))).all()
        # the stop AT a pick_sim value the run produced: strict, so that pick is not made
        t = len(picks) // 2
        if t >= 1:
            at = float(taken[t])
            k = min(n, 48)
            fewer, _, _ = _agree(maxmin_pick(e, k, at), sim, k, at)
            assert 1 <= len(fewer) <= t and np.array_equal(fewer, picks[:len(fewer)])


@pytest.mark.parametrize("H", MC.F64_WIDTHS)
def test_picks_and_leaders_are_the_float64_walk(H):
    """Every case, none left out: test_maxmin_cpu.py asserts that the fixtures' pick decisions lie more than 4 error bounds apart and
    that at most 1 % of a case's rows have a leader decision that does not."""
    from molkgnn_amd.readout import maxmin_pick
    for n in MC.SIZES:
        emb, wp, wl, margin, sure, _ = MC.float64_case(n, H)
        assert margin > MC.MARGIN and (~sure).sum() <= 0.01 * n
        picks, _, n_picks, leader, _ = maxmin_pick(torch.tensor(emb, device=DEV), min(n, MC.F64_PICKS))
        assert int(n_picks) == len(wp) and np.array_equal(picks.cpu().numpy(), wp), (H, n)
        assert np.array_equal(leader.cpu().numpy()[sure], wl[sure]), (H, n)


def test_the_grid_that_fills_the_chip_takes_the_narrow_update_blocks():
    """From 2 048 blocks of 256 rows on, the update launch runs 256 threads per block instead of 1 024 (kgnn_maxmin.hip): the smallest
    such size, a few rounds, against the definition walked with ``mkgnn_embed_cosine``'s columns fetched on demand (the full matrix
    would not fit); every row finite, so every row is valid."""
    from molkgnn_amd import _lib
    from molkgnn_amd.readout import embedding_cosine, maxmin_pick
    n, H, k = 2048 * _lib.MAXMIN_ROWS + 3, 32, 5
    rng = np.random.default_rng(77)
    emb = (rng.standard_normal((64, H))[rng.integers(0, 64, n)] + 0.3 * rng.standard_normal((n, H))).astype(np.float32)
    e = torch.from_numpy(emb).to(DEV)
    picks, pick_sim, n_picks, leader, leader_sim = (t.cpu().numpy() for t in maxmin_pick(e, k))
    cur, lead, picked = np.full(n, -np.inf, dtype=np.float32), np.full(n, -1, dtype=np.int32), np.zeros(n, dtype=bool)
    for t in range(k):
        rows = np.flatnonzero(~picked)
        i = int(rows[np.argmin(cur[rows])])
        assert picks[t] == i and pick_sim[t].view(np.int32) == cur[i].view(np.int32), t
        col = embedding_cosine(e, e[i:i + 1])[:, 0].cpu().numpy()
        picked[i] = True
        meet = (~picked & (col > cur)) | (np.arange(n) == i)
        cur[meet], lead[meet] = col[meet], i
    assert int(n_picks[0]) == k and np.array_equal(leader, lead) and np.array_equal(leader_sim.view(np.int32), cur.view(np.int32))
    assert len(set(picks.tolist())) == k and picks[0] == 0


def test_planted_hazards():
    from molkgnn_amd.readout import maxmin_pick
    n, H = 300, 33
    rng = np.random.default_rng(8)
    emb = MC.clustered(n, H, 21)
    ZERO, NAN_ROW, INF_ROW, FIRST, SECOND, HUGE, TINY, OVER = 10, 20, 30, 40, 41, 50, 60, 70
    emb[ZERO] = 0.0
    emb[NAN_ROW, 7] = np.nan
    emb[INF_ROW, 32] = np.inf
    emb[FIRST] = emb[SECOND] = rng.standard_normal(H).astype(np.float32)         # a direction of its own, twice
    emb[HUGE] = (emb[HUGE] / np.abs(emb[HUGE]).max() * np.float32(1e15)).astype(np.float32)
    emb[TINY] = (np.float32(1e-41) * np.arange(1, H + 1)).astype(np.float32)      # a denormal row
    emb[OVER] = (emb[OVER] / np.abs(emb[OVER]).max() * np.float32(1e25)).astype(np.float32)      # finite, but its norm overflows
    bad = [NAN_ROW, INF_ROW, OVER]
    e = torch.from_numpy(emb).to(DEV)
    sim = _all_sims(e)
    assert np.isnan(sim[bad, bad]).all() and not np.isnan(np.delete(np.diag(sim), bad)).any()
    for k, stop in ((n, INF), (60, INF), (n, 0.99), (n, 0.0)):
        got = maxmin_pick(e, k, stop)
        picks, _, leader = _agree(got, sim, k, stop)
        lsim = got[4].cpu().numpy()
        for row in bad:                                            # never picked, leading nothing, taking no part
            assert leader[row] == -1 and np.isnan(lsim[row]) and row not in picks and not (leader == row).any()
        if stop == INF and k == n:
            assert len(picks) == n - len(bad)                      # every valid row is taken in the end, the twin too
    got = maxmin_pick(e, n, 0.99)
    picks, leader, lsim = got[0].cpu().numpy()[:int(got[2])], got[3].cpu().numpy(), got[4].cpu().numpy()
    assert FIRST in picks and SECOND not in picks                  # the duplicate: picked once (the lower row), its twin led by it
    assert leader[SECOND] == FIRST and lsim[SECOND] == sim[SECOND, FIRST] and lsim[SECOND] > 0.99
    assert ZERO in picks or leader[ZERO] == TINY                   # similarity 0 to everything: the two tie, one of them is taken
    assert leader[HUGE] >= 0 and (leader[HUGE] == HUGE or lsim[HUGE] >= 0.99)     # scale does not matter to a cosine
    # the other rows: the same result as without the bad rows
    keep = np.setdiff1d(np.arange(n), bad)
    less = maxmin_pick(e[torch.from_numpy(keep).to(DEV)].contiguous(), len(keep), 0.99)
    assert int(less[2]) == int(got[2])
    assert np.array_equal(keep[less[0].cpu().numpy()[:int(less[2])]], picks)
    assert np.array_equal(_bits(less[1]), _bits(got[1])[:len(keep)])
    assert np.array_equal(keep[less[3].cpu().numpy()], leader[keep]) and np.array_equal(_bits(less[4]), _bits(got[4])[keep])


def test_start_sim_a_deck_and_excluded_rows():
    from molkgnn_amd.readout import embedding_max_cosine, maxmin_pick
    from molkgnn_amd.screening import maxmin_pick_reference, pick_maxmin_embeddings
    n, H, k = MC.TILE + 200, 32, 64
    emb = MC.clustered(n, H, 31)
    e = torch.from_numpy(emb).to(DEV)
    sim = _all_sims(e)
    copies = [3, 500, MC.TILE + 50]
    deck = torch.from_numpy(np.concatenate([MC.clustered(47, H, 32), emb[copies]])).to(DEV)      # 50 rows, three of them copies
    start = embedding_max_cosine(e, deck)[0]
    assert not bool(torch.isnan(start).any())
    for small in (False, True):                                    # (both forms)
        m = 700 if small else n
        em, sm, st = e[:m].contiguous(), sim[:m, :m], start[:m].contiguous()
        picks, taken, leader = _agree(maxmin_pick(em, k, None, st), sm, k, INF, st)
        assert float(taken[0]) == float(st.min()) and picks[0] == int(torch.argmin(st))
        assert (leader == -1).any()                                # rows the deck stays nearer to than any pick
        free = _agree(maxmin_pick(em, k), sm, k)[0]
        assert not np.array_equal(free, picks)
    # through the screening layer: the deck, rows to leave out, ids
    exclude = torch.zeros(n, dtype=torch.bool, device=DEV)
    out_rows = [0, 7, 1030]
    exclude[out_rows] = True
    ids = torch.arange(n, device=DEV) * 3 + 5
    r = pick_maxmin_embeddings(e, k, 0.9, deck=deck, exclude=exclude, ids=ids)
    begin = start.clone()
    begin[out_rows] = float("nan")
    wp, ws, wn, wl, wls = maxmin_pick_reference(sim, k, 0.9, begin)
    assert r["n_picks"] == wn and 4 <= wn
    assert np.array_equal(r["picks"].cpu().numpy(), 3 * wp[:wn] + 5) and r["picks"].dtype == torch.int64
    assert _same_floats(r["pick_sim"].cpu().numpy(), ws[:wn])
    assert np.array_equal(r["leader"].cpu().numpy(), np.where(wl >= 0, 3 * wl + 5, -1)) and _same_floats(r["leader_sim"].cpu().numpy(), wls)
    assert np.array_equal(_bits(r["deck_sim"]), _bits(start))
    assert np.array_equal(r["cluster_size"].cpu().numpy(), np.array([(wl == p).sum() for p in wp[:wn]]))
    for row in out_rows:                                           # assigned, never picked
        assert row not in wp and not np.isnan(wls[row])
    assert (wl[out_rows] >= 0).any()
    for row in copies:                                             # what the deck holds already lies within 0.9 of it
        assert float(start[row]) > 0.99 and row not in wp[:wn]
    # without a stop and with every row allowed, a copy is picked late or not at all
    r = pick_maxmin_embeddings(e, 256, deck=deck)
    assert r["n_picks"] == 256
    place = {int(p): t for t, p in enumerate(r["picks"].cpu().tolist())}
    assert all(place.get(row, 256) >= 200 for row in copies)


def test_strides_and_sentinels():
    from molkgnn_amd.readout import maxmin_pick
    H, k = 31, 20
    for n in (MC.TILE - 24, MC.TILE + 1):                          # (both forms)
        e = torch.from_numpy(MC.clustered(n, H, 41)).to(DEV)
        start = torch.from_numpy(np.random.default_rng(n).uniform(-1, 1, n).astype(np.float32)).to(DEV)
        want = maxmin_pick(e, k, 0.95, start)
        ep = torch.full((n, H + 3), float("nan"), device=DEV)
        ep[:, :H] = e
        ibuf = torch.full((n + k + 40,), -77, dtype=torch.int32, device=DEV)
        fbuf = torch.full((n + k + 20,), -7.5, device=DEV)
        out = (ibuf[3:3 + k], fbuf[2:2 + k], ibuf[k + 10:k + 11], ibuf[k + 20:k + 20 + n], fbuf[k + 9:k + 9 + n])
        got = maxmin_pick(ep[:, :H], k, 0.95, start, out=out)
        assert all(x is y for x, y in zip(got, out))
        for a, b in zip(got, want):
            assert np.array_equal(_bits(a), _bits(b))
        used = torch.zeros_like(ibuf, dtype=torch.bool)
        used[3:3 + k] = used[k + 10] = True
        used[k + 20:k + 20 + n] = True
        assert bool((ibuf[~used] == -77).all())
        assert bool((fbuf[:2] == -7.5).all()) and bool((fbuf[2 + k:k + 9] == -7.5).all()) and bool((fbuf[k + 9 + n:] == -7.5).all())
        assert bool(torch.isnan(ep[:, H:]).all())
        count = int(got[2])
        assert 1 <= count <= k and bool((got[0][count:] == -1).all()) and bool(torch.isnan(got[1][count:]).all())
    for bad in ((out[0][:-1], out[1], out[2], out[3], out[4]), (out[0], out[1][:-1], out[2], out[3], out[4]),
                (out[0], out[1], out[2], out[3], out[4].double()), (ibuf[0:2 * k:2], out[1], out[2], out[3], out[4]),
                (out[0].long(), out[1], out[2], out[3], out[4]), (out[0], out[1], out[2], out[3][:-1], out[4]), out[:4],
                (out[0], out[0], out[2], out[3], out[4])):
        with pytest.raises(ValueError):
            maxmin_pick(e, k, out=bad)
    for bad_k in (0, n + 1):
        with pytest.raises(ValueError):
            maxmin_pick(e, bad_k)
    # no rows: nothing is launched
    p, s, c, l, ls = maxmin_pick(e[:0], 0)
    assert p.shape == s.shape == l.shape == ls.shape == (0,) and int(c) == 0
    with torch.enable_grad():
        with pytest.raises(RuntimeError):
            maxmin_pick(e.clone().requires_grad_(), k)
        with pytest.raises(RuntimeError):
            maxmin_pick(e, k, None, start.clone().requires_grad_())


def test_one_captured_call_follows_the_contents():
    from molkgnn_amd import _lib
    from molkgnn_amd.readout import maxmin_pick
    H, k = 64, 24
    n = _lib.MAXMIN_TILE + 40
    e = torch.from_numpy(MC.clustered(n, H, 1)).to(DEV)
    start = torch.zeros(n, device=DEV)
    out = (torch.empty(k, dtype=torch.int32, device=DEV), torch.empty(k, device=DEV), torch.empty(1, dtype=torch.int32, device=DEV),
           torch.empty(n, dtype=torch.int32, device=DEV), torch.empty(n, device=DEV))
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        maxmin_pick(e, k, 0.99, start, out=out)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            maxmin_pick(e, k, 0.99, start, out=out)
    torch.cuda.current_stream(DEV).wait_stream(side)
    seen = set()
    for seed in (2, 3):
        e.copy_(torch.from_numpy(MC.clustered(n, H, seed)).to(DEV))
        start.copy_(torch.from_numpy(np.random.default_rng(seed).uniform(-0.5, 0.5, n).astype(np.float32)).to(DEV))
        for o in out:
            o.fill_(-9)
        graph.replay()
        eager = maxmin_pick(e, k, 0.99, start)
        for a, b in zip(out, eager):
            assert np.array_equal(_bits(a), _bits(b))
        _agree(out, _all_sims(e), k, 0.99, start)
        seen.add(tuple(out[0].cpu().tolist()))
    assert len(seen) == 2                                          # (the two contents do give different picks)


def test_c_abi_rejects_before_any_launch():
    from molkgnn_amd import _lib
    lib = _lib.load()
    n, H, k = 40, 20, 12
    e = torch.from_numpy(MC.clustered(n, H, 9)).to(DEV)
    start = torch.zeros(n, device=DEV)
    picks = torch.full((k,), -77, dtype=torch.int32, device=DEV)
    psim = torch.full((k,), -7.5, device=DEV)
    count = torch.full((1,), -77, dtype=torch.int32, device=DEV)
    leader = torch.full((n,), -77, dtype=torch.int32, device=DEV)
    lsim = torch.full((n,), -7.5, device=DEV)
    need = lib.mkgnn_maxmin_pick_workspace_bytes(n)
    assert need == 4 * (3 * n + 2 * 4 + 72)
    ws = torch.zeros(need + 8, dtype=torch.uint8, device=DEV)
    st = _lib.stream_ptr(torch.device(DEV))

    def call(emb=e.data_ptr(), es=H, rows=n, width=H, begin=start.data_ptr(), stop=0.9, k_max=k, out_picks=picks.data_ptr(),
             out_psim=psim.data_ptr(), out_count=count.data_ptr(), out_leader=leader.data_ptr(), out_sim=lsim.data_ptr(),
             work=ws.data_ptr(), work_bytes=need):
        return lib.mkgnn_maxmin_pick(emb, es, rows, width, begin, stop, k_max, out_picks, out_psim, out_count, out_leader, out_sim,
                                     work, work_bytes, st)

    refused = (("width", dict(width=0)), ("width", dict(width=65, es=65)), ("bad shape", dict(rows=-1)), ("bad shape", dict(es=H - 1)),
               ("NaN", dict(stop=float("nan"))), ("rows", dict(rows=_lib.MAXMIN_MAX_ROWS + 1)), ("k_max", dict(k_max=0)),
               ("k_max", dict(k_max=n + 1)), ("k_max", dict(k_max=_lib.MAXMIN_MAX_PICKS + 1, rows=_lib.MAXMIN_MAX_ROWS)),
               ("null", dict(emb=None)), ("null", dict(out_picks=None)), ("null", dict(out_psim=None)), ("null", dict(out_count=None)),
               ("null", dict(out_leader=None)), ("null", dict(out_sim=None)), ("null", dict(work=None)),
               ("workspace", dict(work_bytes=need - 1)), ("aligned", dict(work=ws.data_ptr() + 1)),
               ("aliases emb", dict(out_picks=e.data_ptr())), ("aliases emb", dict(out_sim=e.data_ptr() + 4 * (n * H - 1))),
               ("aliases emb", dict(work=e.data_ptr())), ("aliases emb", dict(out_psim=start.data_ptr() + 4 * (n - 1))),
               ("aliases emb", dict(out_sim=start.data_ptr())), ("alias each other", dict(out_leader=lsim.data_ptr())),
               ("alias each other", dict(out_psim=picks.data_ptr())), ("alias each other", dict(out_count=picks.data_ptr() + 4 * (k - 1))),
               ("alias each other", dict(out_count=leader.data_ptr())), ("alias each other", dict(work=lsim.data_ptr() + 4 * (n - 1))))
    for word, kw in refused:
        assert call(**kw) != 0, kw
        assert word in lib.mkgnn_last_error().decode(), (kw, lib.mkgnn_last_error())
    assert call(rows=0, emb=None, begin=None, out_picks=None, out_psim=None, out_count=None, out_leader=None, out_sim=None, work=None,
                work_bytes=0) == 0                                 # a no-op
    torch.cuda.synchronize()
    assert bool((picks == -77).all()) and int(count) == -77 and bool((leader == -77).all())
    assert bool((lsim == -7.5).all()) and bool((psim == -7.5).all())
    sim = _all_sims(e)
    for stop in (0.9, INF, -INF):                                  # (both infinities are plain values)
        assert call(stop=stop) == 0
        _agree((picks, psim, count, leader, lsim), sim, k, stop, start)
    assert call(begin=None) == 0                                   # start_sim is the one pointer that may be null
    _agree((picks, psim, count, leader, lsim), sim, k, 0.9)
    # a poisoned workspace gives the same result: it needs no initialisation
    first = [t.clone() for t in (picks, psim, count, leader, lsim)]
    ws.fill_(0xFF)
    assert call(begin=None) == 0
    for a, b in zip((picks, psim, count, leader, lsim), first):
        assert np.array_equal(_bits(a), _bits(b))
    # ... on the form of two launches per round as well
    n2 = _lib.MAXMIN_TILE + 9
    e2 = torch.from_numpy(MC.clustered(n2, H, 10)).to(DEV)
    out2 = [torch.empty(k, dtype=torch.int32, device=DEV), torch.empty(k, device=DEV), torch.empty(1, dtype=torch.int32, device=DEV),
            torch.empty(n2, dtype=torch.int32, device=DEV), torch.empty(n2, device=DEV)]
    need2 = lib.mkgnn_maxmin_pick_workspace_bytes(n2)
    results = []
    for fill in (0x00, 0xFF):
        ws2 = torch.full((need2,), fill, dtype=torch.uint8, device=DEV)
        assert lib.mkgnn_maxmin_pick(e2.data_ptr(), H, n2, H, None, 0.9, k, *(o.data_ptr() for o in out2), ws2.data_ptr(), need2, st) == 0
        results.append([_bits(o) for o in out2])
    assert all(np.array_equal(a, b) for a, b in zip(*results))
    _agree(out2, _all_sims(e2), k, 0.9)


def test_torch_route_beyond_the_kernels_width_is_the_walk_over_its_own_similarities():
    from molkgnn_amd import readout
    H, n, k = 65, 150, 30
    assert not readout.maxmin_pick_supported(n, H, k) and readout.maxmin_pick_supported(n, 64, k)
    assert readout.maxmin_pick_supported(1 << 20, 32, 4096) and not readout.maxmin_pick_supported(1 << 20, 32, 4097)
    assert not readout.maxmin_pick_supported((1 << 20) + 1, 32, 1) and not readout.maxmin_pick_supported(5, 32, 6)
    emb = MC.clustered(n, H, 13)
    emb[17] = np.nan
    emb[19] = 0.0
    e = torch.from_numpy(emb).to(DEV)
    sim = np.empty((n, n), dtype=np.float32)                       # embedding_cosine's own torch route at this width, one column
    for i in range(n):                                             # per call: what the rounds ask for
        sim[:, i] = readout.embedding_cosine(e, e[i:i + 1])[:, 0].cpu().numpy()
    picks, _, leader = _agree(readout.maxmin_pick(e, k), sim, k)
    assert len(picks) == k and leader[17] == -1 and 17 not in picks
    start = torch.from_numpy(np.random.default_rng(5).uniform(-1, 1, n).astype(np.float32)).to(DEV)
    start[3] = float("nan")
    stopped, _, leader = _agree(readout.maxmin_pick(e, k, 0.9, start), sim, k, 0.9, start)
    assert 2 <= len(stopped) <= k and 3 not in stopped and leader[3] >= 0
    _agree(readout.maxmin_pick(e, 1), sim, 1)
