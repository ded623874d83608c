"""``mkgnn_diverse_pick`` on the GPU.  All four outputs against the host walk (``diverse_pick_reference``) over
``mkgnn_embed_cosine``'s own float32 similarities -- bits, every row, at the tile's edges, with the threshold AT a similarity and with
the list capped -- and against the walk over the float64 cosine; planted hazards; independence of the tiling; strides, sentinels,
capture; what the C ABI rejects; the torch route beyond ``H = 64``."""
import functools

import numpy as np
import pytest
import torch

from tests import _diverse_cases as DC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


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


def _agree(got, sim, max_sim, k):
    """The four outputs are the host walk over ``sim``: indices equal, ``leader_sim`` by bit pattern apart from NaN."""
    from molkgnn_amd.screening import diverse_pick_reference
    picks, n_picks, leader, leader_sim = got
    n = sim.shape[0]
    assert picks.dtype == torch.int32 and n_picks.dtype == torch.int32 and leader.dtype == torch.int32 and leader_sim.dtype == torch.float32
    assert tuple(picks.shape) == (k,) and tuple(n_picks.shape) == (1,) and tuple(leader.shape) == tuple(leader_sim.shape) == (n,)
    wp, wn, wl, ws = diverse_pick_reference(sim, max_sim, k)
    assert int(n_picks) == wn, (n, max_sim, k, int(n_picks), wn)
    assert np.array_equal(picks.cpu().numpy(), wp), (n, max_sim, k)
    assert np.array_equal(leader.cpu().numpy(), wl), (n, max_sim, k)
    some = ~np.isnan(ws)
    got_sim = leader_sim.cpu().numpy()
    assert np.array_equal(got_sim.view(np.int32)[some], ws.view(np.int32)[some]) and np.isnan(got_sim[~some]).all(), (n, max_sim, k)
    return wp[:wn], wl


@functools.lru_cache(maxsize=None)
def _cases(H):
    """Every size at width ``H``, run ONCE at the fixtures' threshold without a cap: the input, the kernel's outputs and
    ``mkgnn_embed_cosine``'s similarities."""
    from molkgnn_amd.readout import diverse_pick
    cases = []
    for n in DC.sizes(H):
        e = torch.tensor(DC.float64_case(n, H)[0], device=DEV)         # (a copy: the cached array is read-only)
        cases.append((n, e, diverse_pick(e, DC.MAX_SIM), _all_sims(e)))
    return cases


@pytest.mark.parametrize("H", DC.WIDTHS)
def test_bits_are_the_walk_over_embed_cosines_own_similarities(H):
    from molkgnn_amd.readout import diverse_pick
    for n, e, got, sim in _cases(H):
        picks, leader = _agree(got, sim, DC.MAX_SIM, n)
        # the threshold AT the float32 similarity of a covered pair: strict, so that pair is not covered any more
        covered = np.flatnonzero((leader >= 0) & (leader != np.arange(n)))
        if covered.size:
            i = int(covered[len(covered) // 2])
            p = int(leader[i])
            at = float(sim[i, p])
            assert at > np.float32(DC.MAX_SIM)
            strict = diverse_pick(e, at)
            _agree(strict, sim, at, n)
            assert int(strict[2][i]) != p
        else:
            assert n == 1 or len(picks) == n
        # the list capped: one pick, half of them, no cap
        for k in sorted({1, max(len(picks) // 2, 1), n}):
            capped = diverse_pick(e, DC.MAX_SIM, k)
            cp, cl = _agree(capped, sim, DC.MAX_SIM, k)
            assert len(cp) == min(k, len(picks)) and np.array_equal(cp, picks[:len(cp)])
            if k < len(picks):
                assert (cl == -1).any()


@pytest.mark.parametrize("H", DC.WIDTHS)
def test_picks_and_leaders_are_the_float64_walk(H):
    """Every case, none left out: test_diverse_cpu.py asserts that no similarity of these fixtures lies within 4 error bounds of the
    threshold, so float32 inside its bound decides every comparison as float64 does."""
    for n, e, (picks, n_picks, leader, leader_sim), _ in _cases(H):
        _, wp, wn, wl, margin = DC.float64_case(n, H)
        assert margin > 4
        assert int(n_picks) == wn and np.array_equal(picks.cpu().numpy(), wp) and np.array_equal(leader.cpu().numpy(), wl), (H, n)


def test_planted_hazards():
    from molkgnn_amd.readout import diverse_pick
    n, H = 300, 33
    rng = np.random.default_rng(8)
    emb = DC.clustered(n, H, 21)
    ZERO, NAN_ROW, INF_ROW, FIRST, SECOND, HUGE, TINY, OVER = 10, 20, 30, 40, 41, 50, 60, 70
    emb[ZERO] = 0.0
    emb[NAN_ROW, 7] = np.nan
    emb[INF_ROW, 32] = np.inf
    emb[FIRST] = emb[SECOND] = rng.standard_normal(H).astype(np.float32)         # a direction of its own, twice
    emb[HUGE] = (emb[HUGE] / np.abs(emb[HUGE]).max() * np.float32(1e15)).astype(np.float32)
    emb[TINY] = (np.float32(1e-41) * np.arange(1, H + 1)).astype(np.float32)
    emb[OVER] = (emb[OVER] / np.abs(emb[OVER]).max() * np.float32(1e25)).astype(np.float32)      # finite, but its norm overflows
    e = torch.from_numpy(emb).to(DEV)
    sim = _all_sims(e)
    assert np.isnan(sim[[NAN_ROW, INF_ROW, OVER], [NAN_ROW, INF_ROW, OVER]]).all() and not np.isnan(np.delete(np.diag(sim), [NAN_ROW, INF_ROW, OVER])).any()
    assert sim[OVER, 0] == 0.0                                     # (finite dot x zero inverse norm: only the NaN diagonal keeps it out)
    for max_sim in (DC.MAX_SIM, 0.0, -0.5):
        got = diverse_pick(e, max_sim)
        picks, leader = _agree(got, sim, max_sim, n)
        lsim = got[3].cpu().numpy()
        for bad in (NAN_ROW, INF_ROW, OVER):                       # never picked, never covered, covering nothing
            assert leader[bad] == -1 and np.isnan(lsim[bad]) and bad not in picks and not (leader == bad).any()
        if max_sim >= 0:
            assert leader[ZERO] == ZERO and ZERO in picks and (leader == ZERO).sum() == 1          # similarity +0.0 to everything
    got = diverse_pick(e, DC.MAX_SIM)
    leader, lsim = got[2].cpu().numpy(), got[3].cpu().numpy()
    assert leader[FIRST] == FIRST and leader[SECOND] == FIRST and lsim[SECOND] == sim[SECOND, FIRST]
    assert leader[HUGE] >= 0 and lsim[HUGE] > DC.MAX_SIM           # scale does not matter to a cosine: led by its cluster, or itself
    assert leader[TINY] == TINY and lsim[TINY] == 0.0              # squares underflow: norm clamped, similarity 0 to everything
    # the neighbours of the NaN rows: the same clustering as without those rows
    keep = np.setdiff1d(np.arange(n), [NAN_ROW, INF_ROW, OVER])
    less = diverse_pick(e[torch.from_numpy(keep).to(DEV)].contiguous(), DC.MAX_SIM)
    assert int(less[1]) == int(got[1])
    assert np.array_equal(keep[less[2].cpu().numpy()], leader[keep]) and np.array_equal(_bits(less[3]), _bits(got[3])[keep])


def test_result_does_not_depend_on_the_tiling():
    """A cluster whose members sit in three different tiles, and the same rows walked from the other end: the host walk every time."""
    from molkgnn_amd import _lib
    from molkgnn_amd.readout import diverse_pick
    H = 32
    tile = _lib.diverse_tile(H)
    n = 2 * tile + 37
    emb = DC.clustered(n, H, 5).copy()
    rng = np.random.default_rng(6)
    centre = 3.0 * rng.standard_normal(H)
    members = (5, tile + 5, 2 * tile + 5)
    for j in members:
        emb[j] = (centre + 0.08 * rng.standard_normal(H)).astype(np.float32)
    e = torch.from_numpy(emb).to(DEV)
    got = diverse_pick(e, DC.MAX_SIM)
    picks, leader = _agree(got, _all_sims(e), DC.MAX_SIM, n)
    assert [int(leader[j]) for j in members] == [5, 5, 5]
    assert len({int(p) // tile for p in picks}) >= 2
    perm = np.arange(n)[::-1].copy()                               # the walk from the other end: the members swap tiles
    e2 = torch.from_numpy(emb[perm]).to(DEV)
    got2 = diverse_pick(e2, DC.MAX_SIM)
    _, leader2 = _agree(got2, _all_sims(e2), DC.MAX_SIM, n)
    where = np.argsort(perm)                                       # row j of emb sits at where[j]
    assert len({int(leader2[where[j]]) for j in members}) == 1     # still one cluster, whoever leads it now
    assert len({int(where[j]) // tile for j in members}) == 3


def test_strides_and_sentinels():
    from molkgnn_amd.readout import diverse_pick
    H = 31
    n = DC.sizes(H)[4]
    e = torch.tensor(DC.float64_case(n, H)[0], device=DEV)
    want = diverse_pick(e, DC.MAX_SIM)
    k = int(want[1]) // 2
    want_k = diverse_pick(e, DC.MAX_SIM, k)
    ep = torch.full((n, H + 3), float("nan"), device=DEV)
    ep[:, :H] = e
    ibuf = torch.full((2 * n + k + 40,), -77, dtype=torch.int32, device=DEV)
    fbuf = torch.full((n + 9,), -7.5, device=DEV)
    out = (ibuf[3:3 + k], ibuf[k + 10:k + 11], ibuf[k + 20:k + 20 + n], fbuf[4:4 + n])
    got = diverse_pick(ep[:, :H], DC.MAX_SIM, k, out=out)
    assert all(x is y for x, y in zip(got, out))
    for a, b in zip(got, want_k):
        assert np.array_equal(_bits(a), _bits(b))
    used = torch.zeros_like(ibuf, dtype=torch.bool)
    used[3:3 + k] = used[k + 10] = True
    used[k + 20:k + 20 + n] = True
    assert bool((ibuf[~used] == -77).all()) and bool((fbuf[:4] == -7.5).all()) and bool((fbuf[4 + n:] == -7.5).all())
    assert bool(torch.isnan(ep[:, H:]).all())
    assert bool((got[0] >= 0).all()) and int(got[1]) == k          # a full list has no unused slot
    full = diverse_pick(e, DC.MAX_SIM)
    assert bool((full[0][int(full[1]):] == -1).all()) and int(full[1]) < n
    for bad in ((out[0][:-1], out[1], out[2], out[3]), (out[0], out[1], out[2], out[3].double()), (out[0], out[1], ibuf[0:2 * n:2], out[3]),
                (out[0].long(), out[1], out[2], out[3]), out[:3]):
        with pytest.raises(ValueError):
            diverse_pick(e, DC.MAX_SIM, k, out=bad)
    for bad_k in (0, n + 1):
        with pytest.raises(ValueError):
            diverse_pick(e, DC.MAX_SIM, bad_k)
    # no rows: nothing is launched
    p, c, l, s = diverse_pick(e[:0], DC.MAX_SIM)
    assert p.shape == l.shape == s.shape == (0,) and int(c) == 0
    with torch.enable_grad():
        with pytest.raises(RuntimeError):
            diverse_pick(e.clone().requires_grad_(), DC.MAX_SIM)


def test_one_captured_call_follows_the_contents():
    from molkgnn_amd import _lib
    from molkgnn_amd.readout import diverse_pick
    H = 64
    n = _lib.diverse_tile(H) + 40
    e = torch.from_numpy(DC.clustered(n, H, 1)).to(DEV)
    out = (torch.empty(n, dtype=torch.int32, device=DEV), torch.empty(1, dtype=torch.int32, device=DEV),
           torch.empty(n, dtype=torch.int32, device=DEV), torch.empty(n, device=DEV))
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        diverse_pick(e, DC.MAX_SIM, out=out)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            diverse_pick(e, DC.MAX_SIM, out=out)
    torch.cuda.current_stream(DEV).wait_stream(side)
    seen = set()
    for seed in (2, 3):
        e.copy_(torch.from_numpy(DC.clustered(n, H, seed)).to(DEV))
        for o in out:
            o.fill_(-9)
        graph.replay()
        eager = diverse_pick(e, DC.MAX_SIM)
        for a, b in zip(out, eager):
            assert np.array_equal(_bits(a), _bits(b))
        _agree(out, _all_sims(e), DC.MAX_SIM, n)
        seen.add(tuple(out[0].cpu().tolist()))
    assert len(seen) == 2                                          # (the two contents do give different picks)


def test_c_abi_rejects_before_any_launch():
    from molkgnn_amd import _lib
    lib = _lib.load()
    n, H, k = 40, 20, 12
    e = torch.from_numpy(DC.clustered(n, H, 9)).to(DEV)
    picks = torch.full((k,), -77, dtype=torch.int32, device=DEV)
    count = torch.full((1,), -77, dtype=torch.int32, device=DEV)
    leader = torch.full((n,), -77, dtype=torch.int32, device=DEV)
    lsim = torch.full((n,), -7.5, device=DEV)
    need = lib.mkgnn_diverse_pick_workspace_bytes(n)
    assert need == 4 * (2 * n + 4)
    ws = torch.zeros(need + 8, dtype=torch.uint8, device=DEV)
    st = _lib.stream_ptr(torch.device(DEV))

    def call(emb=e.data_ptr(), es=H, rows=n, width=H, max_sim=0.9, k_max=k, out_picks=picks.data_ptr(), out_count=count.data_ptr(),
             out_leader=leader.data_ptr(), out_sim=lsim.data_ptr(), work=ws.data_ptr(), work_bytes=need):
        return lib.mkgnn_diverse_pick(emb, es, rows, width, max_sim, k_max, out_picks, out_count, out_leader, out_sim, work, work_bytes, st)

    refused = (("width", dict(width=0)), ("width", dict(width=65, es=65)), ("bad shape", dict(rows=-1)), ("bad shape", dict(es=H - 1)),
               ("finite", dict(max_sim=float("nan"))), ("finite", dict(max_sim=float("inf"))), ("finite", dict(max_sim=float("-inf"))),
               ("rows", dict(rows=_lib.DIVERSE_MAX_ROWS + 1)), ("k_max", dict(k_max=0)), ("k_max", dict(k_max=n + 1)),
               ("null", dict(emb=None)), ("null", dict(out_picks=None)), ("null", dict(out_count=None)), ("null", dict(out_leader=None)),
               ("null", dict(out_sim=None)), ("null", dict(work=None)), ("workspace", dict(work_bytes=need - 1)),
               ("aligned", dict(work=ws.data_ptr() + 1)), ("aliases emb", dict(out_picks=e.data_ptr())),
               ("aliases emb", dict(out_sim=e.data_ptr() + 4 * (n * H - 1))), ("aliases emb", dict(work=e.data_ptr())),
               ("alias each other", dict(out_leader=lsim.data_ptr())), ("alias each other", dict(out_count=picks.data_ptr() + 4 * (k - 1))),
               ("alias each other", dict(out_count=leader.data_ptr())), ("alias each other", dict(work=lsim.data_ptr() + 4 * (n - 1))))
    for word, kw in refused:
        assert call(**kw) != 0, kw
        assert word in lib.mkgnn_last_error().decode(), (kw, lib.mkgnn_last_error())
    assert call(rows=0, emb=None, out_picks=None, out_count=None, out_leader=None, out_sim=None, work=None, work_bytes=0) == 0      # a no-op
    torch.cuda.synchronize()
    assert bool((picks == -77).all()) and int(count) == -77 and bool((leader == -77).all()) and bool((lsim == -7.5).all())
    assert call() == 0
    _agree((picks, count, leader, lsim), _all_sims(e), 0.9, k)
    # a poisoned workspace gives the same result: it needs no initialisation
    first = [t.clone() for t in (picks, count, leader, lsim)]
    ws.fill_(0xFF)
    assert call() == 0
    for a, b in zip((picks, count, leader, lsim), first):
        assert np.array_equal(_bits(a), _bits(b))


def test_torch_route_beyond_the_kernels_width_is_the_walk_over_its_own_similarities():
    from molkgnn_amd import readout
    H, n = 65, 150
    assert not readout.diverse_pick_supported(n, H) and readout.diverse_pick_supported(n, 64)
    assert not readout.diverse_pick_supported((1 << 20) + 1, 32) and readout.diverse_pick_supported(1 << 20, 32)
    emb = DC.clustered(n, H, 13)
    emb[17] = np.nan
    emb[19] = 0.0
    e = torch.from_numpy(emb).to(DEV)
    sim = _all_sims(e)                                             # (embedding_cosine's own torch route at this width)
    picks, leader = _agree(readout.diverse_pick(e, DC.MAX_SIM), sim, DC.MAX_SIM, n)
    assert 4 <= len(picks) < n and leader[17] == -1 and leader[19] == 19
    for k in (1, len(picks) // 2):
        _agree(readout.diverse_pick(e, DC.MAX_SIM, k), sim, DC.MAX_SIM, k)
