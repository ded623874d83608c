"""``mkgnn_embed_count_within`` on the GPU.  The counts against ``(S > t).sum(1)`` over ``mkgnn_embed_cosine``'s own float32
similarities -- every width and shape, with the threshold AT a similarity, just below it, below everything and above everything --
and against the float64 count; planted hazards; independence of position, order, split and aliasing; strides, sentinels, a caller's
workspace, capture; what the C ABI rejects; the torch route beyond ``H = 64``."""
import functools

import numpy as np
import pytest
import torch

from tests import _count_cases as CC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


_sims = CC.cosine_matrix                    # S [n, R] on the host: mkgnn_embed_cosine's own similarities, in groups of 32 queries


def _above(sim, t):
    with np.errstate(invalid="ignore"):
        return (sim > np.float32(t)).sum(axis=1)


def _count(e, r, t, **kw):
    from molkgnn_amd.readout import embedding_count_within
    got = embedding_count_within(e, r, t, **kw)
    assert got.dtype == torch.int32 and got.dim() == 1
    return got.cpu().numpy().astype(np.int64)


@functools.lru_cache(maxsize=None)
def _cases(H):
    """Every shape at width ``H``, run ONCE at the fixtures' threshold: the inputs, the kernel's counts and ``mkgnn_embed_cosine``'s
    similarities."""
    cases = []
    for n, R in CC.shapes():
        emb, refs, _, _ = CC.float64_case(n, R, H)
        e, r = torch.tensor(emb, device=DEV), torch.tensor(refs, device=DEV)          # (copies: the cached arrays are read-only)
        cases.append((n, R, e, r, _count(e, r, CC.MAX_SIM), _sims(e, r)))
    return cases


@pytest.mark.parametrize("H", CC.WIDTHS)
def test_counts_are_the_elements_of_embed_cosines_own_matrix_above_the_threshold(H):
    for n, R, e, r, got, sim in _cases(H):
        assert got.shape == (n,) and np.array_equal(got, _above(sim, CC.MAX_SIM)), (H, n, R)
        # the threshold AT a float32 similarity of the matrix: strict, so the count of its row drops by exactly the multiplicity of
        # that value in the row; at the next float32 below it those elements count again
        i = n // 2
        at = np.float32(np.sort(sim[i])[R // 2])
        below = np.nextafter(at, np.float32(-2))
        c_at, c_below = _count(e, r, float(at)), _count(e, r, float(below))
        assert np.array_equal(c_at, _above(sim, at)) and np.array_equal(c_below, _above(sim, below)), (H, n, R)
        assert c_below[i] - c_at[i] == (sim[i] == at).sum() >= 1, (H, n, R)
        # below every cosine: every non-NaN pair; above every cosine: none
        assert np.array_equal(_count(e, r, -1.5), (~np.isnan(sim)).sum(axis=1)) and (_count(e, r, -1.5) == R).all(), (H, n, R)
        assert not _count(e, r, 1.5).any(), (H, n, R)


@pytest.mark.parametrize("H", CC.WIDTHS)
def test_counts_are_the_float64_counts(H):
    """Every case, none left out: test_count_within_cpu.py asserts that no similarity of these fixtures lies within 4 error bounds of
    the threshold, so float32 inside its bound decides every comparison as float64 does."""
    for n, R, e, r, got, _ in _cases(H):
        _, _, want, margin = CC.float64_case(n, R, H)
        assert margin > 4
        assert np.array_equal(got, want), (H, n, R)


@pytest.mark.parametrize("H", CC.WIDTHS)
def test_self_join_through_one_pointer_is_the_self_join_against_a_clone(H):
    for n in CC.self_sizes():
        emb, want, margin = CC.float64_self_case(n, H)
        e = torch.tensor(emb, device=DEV)
        same, cloned = _count(e, e, CC.MAX_SIM), _count(e, e.clone(), CC.MAX_SIM)
        assert np.array_equal(same, cloned), (H, n)
        assert np.array_equal(same, _above(_sims(e, e), CC.MAX_SIM)), (H, n)
        assert margin > 4 and np.array_equal(same, want), (H, n)


def test_planted_hazards():
    n, R, H = 300, 200, 33
    rng = np.random.default_rng(8)
    pool = CC.clustered(n + R, H, 21)
    emb, refs = pool[:n].copy(), pool[n:].copy()
    ZERO, NAN_ROW, INF_ROW, TWIN, HUGE, TINY, OVER = 10, 20, 30, 40, 50, 60, 70
    emb[ZERO] = 0.0
    emb[NAN_ROW, 7] = np.nan
    emb[INF_ROW, 32] = np.inf
    emb[TWIN] = refs[5] = refs[9] = rng.standard_normal(H).astype(np.float32)          # a direction of its own: the row, and two references
    refs[15] = 3 * emb[HUGE]                                                           # (so that HUGE has a neighbour for certain)
    emb[HUGE] = (emb[HUGE] / np.abs(emb[HUGE]).max() * np.float32(1e15)).astype(np.float32)
    emb[TINY] = (np.float32(1e-41) * np.arange(1, H + 1)).astype(np.float32)           # denormal: its squares underflow
    emb[OVER] = (emb[OVER] / np.abs(emb[OVER]).max() * np.float32(1e25)).astype(np.float32)      # finite, but its norm overflows
    refs[11] = np.nan                                                                  # a NaN reference only ever fails to count
    refs[13] = 0.0
    e, r = torch.from_numpy(emb).to(DEV), torch.from_numpy(refs).to(DEV)
    sim = _sims(e, r)
    assert np.isnan(sim[[NAN_ROW, INF_ROW]]).all() and np.isnan(sim[:, 11]).all()
    assert (sim[ZERO, np.arange(R) != 11] == 0.0).all()
    assert (np.abs(np.delete(sim[TINY], 11)) < 1e-20).all()        # (its norm is clamped: denormal products times 1e8)
    assert (np.delete(sim[OVER], 11) == 0.0).all()                 # (finite dot x zero inverse norm)
    for t in (CC.MAX_SIM, 0.0, -0.5, -1.5):
        got = _count(e, r, t)
        assert np.array_equal(got, _above(sim, t)), t
        assert got[NAN_ROW] == got[INF_ROW] == 0
        assert got[ZERO] == got[OVER] == (R - 1 if t < 0 else 0) and (t == 0.0 or got[TINY] == got[ZERO])
        assert got.max() <= R - 1                                  # the NaN reference is counted by no row
    got = _count(e, r, CC.MAX_SIM)
    assert got[TWIN] == 2                                          # the duplicated reference counts twice
    assert got[HUGE] == _count(torch.from_numpy(pool[HUGE:HUGE + 1].copy()).to(DEV), r, CC.MAX_SIM)[0] >= 1          # scale does not matter
    # without the NaN reference: the same counts
    keep = np.delete(np.arange(R), 11)
    assert np.array_equal(_count(e, r[torch.from_numpy(keep).to(DEV)].contiguous(), CC.MAX_SIM), got)
    # hazards on the references' side of a self-join: the NaN rows are counted by nobody, themselves included
    self_sim = _sims(e, e)
    self_got = _count(e, e, CC.MAX_SIM)
    assert np.array_equal(self_got, _above(self_sim, CC.MAX_SIM)) and self_got[NAN_ROW] == self_got[INF_ROW] == self_got[OVER] == 0
    assert self_got[ZERO] == 0 and self_got[HUGE] >= 1


def test_result_does_not_depend_on_position_order_or_split():
    rows, tile, parts = CC.tiling()
    H = 33
    n, R = 2 * rows + 37, 9 * tile + 5
    pool = CC.clustered(n + R, H, 31)
    emb, refs = pool[:n].copy(), pool[n:].copy()
    for at in (0, 63, 64, rows - 1, rows, 2 * rows + 36):          # the same row at several places: lanes, waves, blocks
        emb[at] = pool[7]
    e, r = torch.from_numpy(emb).to(DEV), torch.from_numpy(refs).to(DEV)
    full = _count(e, r, CC.MAX_SIM)
    assert np.array_equal(full, _above(_sims(e, r), CC.MAX_SIM)) and full.max() >= 2
    assert len({int(full[at]) for at in (0, 7, 63, 64, rows - 1, rows, 2 * rows + 36)}) == 1
    # the references permuted; fewer rows, so the same rows at another place in another grid
    perm = torch.from_numpy(np.random.default_rng(2).permutation(R)).to(DEV)
    assert np.array_equal(_count(e, r[perm].contiguous(), CC.MAX_SIM), full)
    assert np.array_equal(_count(e, r, CC.MAX_SIM, n_rows=5), full[:5])
    for n_rows in (1, rows, rows + 1):
        assert np.array_equal(_count(e[:n_rows].contiguous(), r, CC.MAX_SIM), full[:n_rows])
    # counts(refs[:a]) + counts(refs[a:]) == counts(refs), at cuts inside and at the edge of a tile
    for a in (1, tile - 1, tile, 4 * tile + 3, R - 1):
        assert np.array_equal(_count(e, r[:a], CC.MAX_SIM) + _count(e, r[a:], CC.MAX_SIM), full), a
    # two tiles per part and a ragged last part against halves of one tile per part
    from molkgnn_amd import _lib
    n, R = CC.shapes()[-1]
    emb, refs, want, _ = CC.float64_case(n, R, H)
    e, r = torch.tensor(emb, device=DEV), torch.tensor(refs, device=DEV)
    a = tile * parts // 2
    assert _lib.count_within_split(n, R)[0] == 2 * tile and _lib.count_within_split(n, a)[0] == _lib.count_within_split(n, R - a)[0] == tile
    assert np.array_equal(_count(e, r[:a], CC.MAX_SIM) + _count(e, r[a:], CC.MAX_SIM), _count(e, r, CC.MAX_SIM))
    assert np.array_equal(_count(e, r, CC.MAX_SIM), want)


def test_strides_sentinels_workspace_and_out():
    from molkgnn_amd import _lib
    from molkgnn_amd.readout import embedding_count_within
    rows, tile, parts = CC.tiling()
    H, n, R = 31, rows + 1, 3 * tile
    emb, refs, _, _ = CC.float64_case(n, R, H)
    e, r = torch.tensor(emb, device=DEV), torch.tensor(refs, device=DEV)
    want = _count(e, r, CC.MAX_SIM)
    ep = torch.full((n + 6, H + 3), float("nan"), device=DEV)      # wider rows, and rows behind n_rows: NaN, never read into a count
    ep[:n, :H] = e
    rp = torch.full((R, H + 5), float("nan"), device=DEV)
    rp[:, :H] = r
    buf = torch.full((2 * n + 9,), -77, dtype=torch.int32, device=DEV)
    lib = _lib.load()
    need = lib.mkgnn_embed_count_within_workspace_bytes(n, R)
    assert need == 4 * ((R + n + 3) // 4 * 4 + 3 * n)
    ws = torch.full((need + 16,), 0xFF, dtype=torch.uint8, device=DEV)             # poisoned: it needs no initialisation
    got = embedding_count_within(ep[:, :H], rp[:, :H], CC.MAX_SIM, n_rows=n, out=buf[4:4 + n], workspace=ws)
    assert got.data_ptr() == buf[4:4 + n].data_ptr() and np.array_equal(got.cpu().numpy(), want)
    assert bool((buf[:4] == -77).all()) and bool((buf[4 + n:] == -77).all()) and bool((ws[need:] == 0xFF).all())
    assert bool(torch.isnan(ep[:, H:]).all()) and bool(torch.isnan(ep[n:]).all()) and bool(torch.isnan(rp[:, H:]).all())
    for bad in (buf[:n - 1], buf[:n].long(), buf[0:2 * n:2], buf[:n].float(), [buf[:n]]):
        with pytest.raises(ValueError):
            embedding_count_within(e, r, CC.MAX_SIM, out=bad)
    for bad in (ws[:need - 1], ws[:need].float(), ws.cpu()):
        with pytest.raises(ValueError):
            embedding_count_within(e, r, CC.MAX_SIM, workspace=bad)
    for bad_rows in (-1, n + 1):
        with pytest.raises(ValueError):
            embedding_count_within(e, r, CC.MAX_SIM, n_rows=bad_rows)
    assert tuple(embedding_count_within(e, r, CC.MAX_SIM, n_rows=0).shape) == (0,)          # no rows: nothing is launched
    assert tuple(embedding_count_within(e[:0], r, CC.MAX_SIM).shape) == (0,)
    with torch.enable_grad():
        with pytest.raises(RuntimeError):
            embedding_count_within(e.clone().requires_grad_(), r, CC.MAX_SIM)
        with pytest.raises(RuntimeError):
            embedding_count_within(e, r.clone().requires_grad_(), CC.MAX_SIM)


def test_one_captured_call_follows_the_contents_of_both_inputs():
    from molkgnn_amd.readout import embedding_count_within
    rows, tile, parts = CC.tiling()
    H, n, R = 64, rows + 40, 5 * tile + 3
    pool = CC.clustered(n + R, H, 1)
    e, r = torch.from_numpy(pool[:n].copy()).to(DEV), torch.from_numpy(pool[n:].copy()).to(DEV)
    out = torch.empty(n, dtype=torch.int32, device=DEV)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        embedding_count_within(e, r, CC.MAX_SIM, out=out)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            embedding_count_within(e, r, CC.MAX_SIM, out=out)
    torch.cuda.current_stream(DEV).wait_stream(side)
    seen = set()
    for seed_e, seed_r in ((2, 2), (2, 3), (3, 3)):                # the rows change, the references change, both do
        e.copy_(torch.from_numpy(CC.clustered(n + R, H, seed_e)[:n].copy()).to(DEV))
        r.copy_(torch.from_numpy(CC.clustered(n + R, H, seed_r)[n:].copy()).to(DEV))
        out.fill_(-9)
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), _above(_sims(e, r), CC.MAX_SIM))
        assert np.array_equal(out.cpu().numpy(), _count(e, r, CC.MAX_SIM))
        seen.add(tuple(out.cpu().tolist()))
    assert len(seen) == 3                                          # (the three contents do give different counts)


def test_c_abi_rejects_before_any_launch():
    from molkgnn_amd import _lib
    lib = _lib.load()
    rows, tile, parts = CC.tiling()
    n, R, H = 40, 2 * tile + 1, 20
    pool = CC.clustered(n + R, H, 9)
    e, r = torch.from_numpy(pool[:n].copy()).to(DEV), torch.from_numpy(pool[n:].copy()).to(DEV)
    counts = torch.full((n,), -77, dtype=torch.int32, device=DEV)
    need = lib.mkgnn_embed_count_within_workspace_bytes(n, R)
    assert need == 4 * ((R + n + 3) // 4 * 4 + 3 * n)
    ws = torch.zeros(need + 8, dtype=torch.uint8, device=DEV)
    st = _lib.stream_ptr(torch.device(DEV))

    def call(emb=e.data_ptr(), es=H, n_rows=n, width=H, refs=r.data_ptr(), rs=H, n_refs=R, min_sim=0.9, out=counts.data_ptr(),
             work=ws.data_ptr(), work_bytes=need):
        return lib.mkgnn_embed_count_within(emb, es, n_rows, width, refs, rs, n_refs, min_sim, out, work, work_bytes, st)

    refused = (("width", dict(width=0)), ("width", dict(width=65, es=65, rs=65)), ("references", dict(n_refs=0)),
               ("references", dict(n_refs=_lib.MAX_COSINE_MAX_REFS + 1)), ("bad shape", dict(n_rows=-1)), ("bad shape", dict(es=H - 1)),
               ("bad shape", dict(rs=H - 1)), ("finite", dict(min_sim=float("nan"))), ("finite", dict(min_sim=float("inf"))),
               ("finite", dict(min_sim=float("-inf"))), ("null", dict(emb=None)), ("null", dict(refs=None)), ("null", dict(out=None)),
               ("null", dict(work=None)), ("workspace", dict(work_bytes=need - 1)), ("aligned", dict(work=ws.data_ptr() + 1)),
               ("aliases an input", dict(out=e.data_ptr())), ("aliases an input", dict(out=r.data_ptr() + 4 * (R * H - 1))),
               ("aliases an input", dict(work=e.data_ptr())), ("alias each other", dict(out=ws.data_ptr() + need - 4)))
    for word, kw in refused:
        assert call(**kw) != 0, kw
        assert word in lib.mkgnn_last_error().decode(), (kw, lib.mkgnn_last_error())
    assert call(n_rows=0, emb=None, refs=None, out=None, work=None, work_bytes=0) == 0      # a no-op
    torch.cuda.synchronize()
    assert bool((counts == -77).all())
    assert call() == 0
    sim = _sims(e, r)
    assert np.array_equal(counts.cpu().numpy(), _above(sim, 0.9))
    # a poisoned workspace gives the same result: it needs no initialisation; the same pointer for both sets is a self-join
    ws.fill_(0xFF)
    assert call() == 0 and np.array_equal(counts.cpu().numpy(), _above(sim, 0.9))
    assert call(refs=e.data_ptr(), n_refs=n, work_bytes=need) == 0
    assert np.array_equal(counts.cpu().numpy(), _above(_sims(e, e), 0.9))


def test_torch_route_beyond_the_kernels_width_meets_the_float64_count():
    from molkgnn_amd import readout
    from molkgnn_amd.screening import cosine_bound, cosine_reference, count_within_reference
    H, n, R = 65, 150, 130
    assert not readout.embedding_count_within_supported(R, H) and readout.embedding_count_within_supported(R, 64)
    pool = CC.clustered(n + R, H, 13)
    emb, refs = pool[:n].copy(), pool[n:].copy()
    sim = cosine_reference(emb, refs)
    assert (np.abs(sim - CC.MAX_SIM) / cosine_bound(emb, refs)).min() > 4
    emb[17] = np.nan
    emb[19] = 0.0
    refs[3] = np.nan
    want = count_within_reference(cosine_reference(emb, refs), CC.MAX_SIM)
    e, r = torch.from_numpy(emb).to(DEV), torch.from_numpy(refs).to(DEV)
    got = _count(e, r, CC.MAX_SIM)
    assert np.array_equal(got, want) and got[17] == got[19] == 0 and got.max() >= 2
    # more than one chunk of references gives the same sum
    old = readout.MAX_COSINE_TORCH_CHUNK
    readout.MAX_COSINE_TORCH_CHUNK = 37
    try:
        assert np.array_equal(_count(e, r, CC.MAX_SIM), want)
    finally:
        readout.MAX_COSINE_TORCH_CHUNK = old
