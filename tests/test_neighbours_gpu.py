"""``mkgnn_embed_neighbours_within`` on the GPU.  The lists against ``np.nonzero(S > t)`` over ``mkgnn_embed_cosine``'s own float32
similarities -- every width and shape, with the threshold AT a similarity, just below it, below everything and above everything
-- with the similarities' bits, against the count and against the float64 lists; planted hazards; independence of position,
split and aliasing; strides, sentinels, a caller's workspace; THE GUARD -- row pointers that are too short, a capacity cut in the
middle of a row, row pointers that are not monotone; one captured count-cumsum-fill; what the C ABI rejects; the torch route
beyond ``H = 64``."""
import functools

import numpy as np
import pytest
import torch

from tests import _components_cases as CC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = -77

_sims = CC.cosine_matrix                    # S [n, R] on the host: mkgnn_embed_cosine's own similarities


def _want(sim, t):
    """``(row_ptr, nbr, nbr_sim)`` by ``np.nonzero`` over a float32 matrix."""
    with np.errstate(invalid="ignore"):
        above = sim > np.float32(t)
    row_ptr = np.zeros(sim.shape[0] + 1, dtype=np.int64)
    np.cumsum(above.sum(axis=1), out=row_ptr[1:])
    rows, cols = np.nonzero(above)
    return row_ptr, cols.astype(np.int32), sim[rows, cols]


def _lists(e, r, t, **kw):
    from molkgnn_amd.readout import embedding_neighbours_within
    row_ptr, nbr, val = embedding_neighbours_within(e, r, t, **kw)
    assert row_ptr.dtype == torch.int64 and nbr.dtype == torch.int32 and val.dtype == torch.float32
    assert row_ptr.dim() == nbr.dim() == val.dim() == 1 and nbr.shape == val.shape
    return row_ptr.cpu().numpy(), nbr.cpu().numpy(), val.cpu().numpy()


def _same(got, want):
    return np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) \
        and np.array_equal(got[2].view(np.int32), want[2].view(np.int32))            # the similarities' BITS


def _count(e, r, t, **kw):
    from molkgnn_amd.readout import embedding_count_within
    return embedding_count_within(e, r, t, **kw).cpu().numpy().astype(np.int64)


@functools.lru_cache(maxsize=None)
def _cases(H):
    """Every shape at width ``H``, run ONCE at the fixtures' threshold: the inputs, the kernel's lists and ``mkgnn_embed_cosine``'s
    similarities."""
    cases = []
    for n, R in CC.shapes():
        emb, refs, _, _ = CC.float64_case(n, R, H)
        e, r = torch.tensor(emb, device=DEV), torch.tensor(refs, device=DEV)          # (copies: the cached arrays are read-only)
        cases.append((n, R, e, r, _lists(e, r, CC.MAX_SIM), _sims(e, r)))
    return cases


@pytest.mark.parametrize("H", CC.WIDTHS)
def test_lists_are_the_elements_of_embed_cosines_own_matrix_above_the_threshold(H):
    for n, R, e, r, got, sim in _cases(H):
        assert got[0].shape == (n + 1,) and _same(got, _want(sim, CC.MAX_SIM)), (H, n, R)
        assert np.array_equal(np.diff(got[0]), _count(e, r, CC.MAX_SIM)), (H, n, R)
        # the threshold AT a float32 similarity of the matrix: strict, so that element is not listed; at the next float32 below, it is
        i = n // 2
        at = np.float32(np.sort(sim[i])[R // 2])
        below = np.nextafter(at, np.float32(-2))
        l_at, l_below = _lists(e, r, float(at)), _lists(e, r, float(below))
        assert _same(l_at, _want(sim, at)) and _same(l_below, _want(sim, below)), (H, n, R)
        assert (l_below[0][i + 1] - l_below[0][i]) - (l_at[0][i + 1] - l_at[0][i]) == (sim[i] == at).sum() >= 1, (H, n, R)
        # below every cosine: every non-NaN pair, nnz = n R; above every cosine: empty tensors
        every = _lists(e, r, -1.5)
        assert _same(every, _want(sim, -1.5)) and every[0][-1] == n * R and np.array_equal(every[1], np.tile(np.arange(R), n)), (H, n, R)
        none = _lists(e, r, 1.5)
        assert not none[0].any() and none[1].shape == none[2].shape == (0,), (H, n, R)


@pytest.mark.parametrize("H", CC.WIDTHS)
def test_lists_are_the_float64_lists(H):
    """Every case, none left out: test_count_within_cpu.py asserts that no similarity of these fixtures lies within 4 error bounds of
    the threshold, so float32 inside its bound decides every pair as float64 does."""
    from molkgnn_amd.screening import cosine_reference, neighbours_reference
    for n, R, e, r, got, _ in _cases(H):
        emb, refs, counts, margin = CC.float64_case(n, R, H)
        assert margin > 4
        row_ptr, nbr, _ = neighbours_reference(cosine_reference(emb, refs), CC.MAX_SIM)
        assert np.array_equal(got[0], row_ptr) and np.array_equal(got[1], nbr) and np.array_equal(np.diff(got[0]), counts), (H, n, R)


@pytest.mark.parametrize("H", CC.WIDTHS)
def test_self_join_through_one_pointer_is_the_self_join_against_a_clone(H):
    for n in CC.self_sizes():
        emb, counts, margin = CC.float64_self_case(n, H)
        e = torch.tensor(emb, device=DEV)
        same, cloned = _lists(e, e, CC.MAX_SIM), _lists(e, e.clone(), CC.MAX_SIM)
        assert _same(same, cloned) and _same(same, _want(_sims(e, e), CC.MAX_SIM)), (H, n)
        assert margin > 4 and np.array_equal(np.diff(same[0]), counts), (H, n)


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
    refs[11] = np.nan                                                                  # a NaN reference is on nobody's list
    refs[13] = 0.0
    e, r = torch.from_numpy(emb).to(DEV), torch.from_numpy(refs).to(DEV)
    sim = _sims(e, r)
    assert np.isnan(sim[[NAN_ROW, INF_ROW]]).all() and np.isnan(sim[:, 11]).all()
    for t in (CC.MAX_SIM, 0.0, -0.5, -1.5):
        got = _lists(e, r, t)
        assert _same(got, _want(sim, t)), t
        ptr, nbr, _ = got
        assert ptr[NAN_ROW + 1] == ptr[NAN_ROW] and ptr[INF_ROW + 1] == ptr[INF_ROW] and 11 not in nbr.tolist()
        if t < 0:                                                  # a zero row, an overflowing row: similarity 0 with everything but the NaN
            for row in (ZERO, OVER):
                assert np.array_equal(nbr[ptr[row]:ptr[row + 1]], np.delete(np.arange(R), 11))
    ptr, nbr, val = _lists(e, r, CC.MAX_SIM)
    assert nbr[ptr[TWIN]:ptr[TWIN + 1]].tolist() == [5, 9]         # the duplicated reference is listed twice, in order
    assert np.array_equal(val[ptr[TWIN]:ptr[TWIN + 1]].view(np.int32), sim[TWIN, [5, 9]].view(np.int32))
    small = _lists(torch.from_numpy(pool[HUGE:HUGE + 1].copy()).to(DEV), r, CC.MAX_SIM)
    assert 15 in nbr[ptr[HUGE]:ptr[HUGE + 1]].tolist() and np.array_equal(nbr[ptr[HUGE]:ptr[HUGE + 1]], small[1])      # scale does not matter
    # hazards on the references' side of a self-join: the NaN rows are on nobody's list, their own included
    self_got = _lists(e, e, CC.MAX_SIM)
    assert _same(self_got, _want(_sims(e, e), CC.MAX_SIM))
    for row in (NAN_ROW, INF_ROW, OVER, ZERO):
        assert self_got[0][row + 1] == self_got[0][row] and row not in self_got[1].tolist()


def _row(lists, i):
    ptr, nbr, val = lists
    return nbr[ptr[i]:ptr[i + 1]], val[ptr[i]:ptr[i + 1]].view(np.int32)


def _joined(first, second, a):
    """Per row, the list over ``refs[:a]`` followed by the list over ``refs[a:]`` with its references moved up by ``a``."""
    n = first[0].shape[0] - 1
    ptr = first[0] + second[0]
    nbr = np.concatenate([np.concatenate([_row(first, i)[0], _row(second, i)[0] + a]) for i in range(n)])
    val = np.concatenate([np.concatenate([_row(first, i)[1], _row(second, i)[1]]) for i in range(n)])
    return ptr, nbr.astype(np.int32), val.view(np.float32)


def test_result_does_not_depend_on_position_or_split():
    rows, tile, parts = CC.tiling()
    H = 33
    n, R = 2 * rows + 37, 9 * tile + 5
    pool = CC.clustered(n + R, H, 31)
    emb, refs = pool[:n].copy(), pool[n:].copy()
    places = (0, 63, 64, rows - 1, rows, 2 * rows + 36)            # the same row at several places: lanes, waves, blocks
    for at in places:
        emb[at] = pool[7]
    e, r = torch.from_numpy(emb).to(DEV), torch.from_numpy(refs).to(DEV)
    full = _lists(e, r, CC.MAX_SIM)
    assert _same(full, _want(_sims(e, r), CC.MAX_SIM)) and np.diff(full[0]).max() >= 2
    for at in places:
        assert np.array_equal(_row(full, at)[0], _row(full, 7)[0]) and np.array_equal(_row(full, at)[1], _row(full, 7)[1])
    assert len(_row(full, 7)[0]) >= 1
    # fewer rows: the same rows at another place in another grid, and another split of the references
    few = _lists(e, r, CC.MAX_SIM, n_rows=5)
    assert np.array_equal(few[0], full[0][:6]) and np.array_equal(few[1], full[1][:full[0][5]])
    for n_rows in (1, rows, rows + 1):
        part = _lists(e[:n_rows].contiguous(), r, CC.MAX_SIM)
        assert np.array_equal(part[0], full[0][:n_rows + 1]) and np.array_equal(part[1], full[1][:full[0][n_rows]])
        assert np.array_equal(part[2].view(np.int32), full[2][:full[0][n_rows]].view(np.int32))
    # lists(refs[:a]) and lists(refs[a:]) concatenate per row to lists(refs), at cuts inside and at the edge of a tile
    for a in (1, tile - 1, tile, 4 * tile + 3, R - 1):
        assert _same(_joined(_lists(e, r[:a], CC.MAX_SIM), _lists(e, r[a:], CC.MAX_SIM), a), full), a
    # two tiles per part and a ragged last part against halves of one tile per part
    from molkgnn_amd import _lib
    n, R = CC.shapes()[-1]
    emb, refs, counts, _ = CC.float64_case(n, R, H)
    e, r = torch.tensor(emb, device=DEV), torch.tensor(refs, device=DEV)
    a = tile * parts // 2
    assert _lib.count_within_split(n, R)[0] == 2 * tile and _lib.count_within_split(n, a)[0] == _lib.count_within_split(n, R - a)[0] == tile
    whole = _lists(e, r, CC.MAX_SIM)
    assert _same(_joined(_lists(e, r[:a], CC.MAX_SIM), _lists(e, r[a:], CC.MAX_SIM), a), whole)
    assert np.array_equal(np.diff(whole[0]), counts) and _same(whole, _want(_sims(e, r), CC.MAX_SIM))


def _raw(e, r, t, row_ptr, capacity, n_rows=None, pad=6, workspace=None):
    """The raw form into buffers with ``pad`` sentinels on either side: ``(nbr buffer, sim buffer, found buffer)`` on the host."""
    from molkgnn_amd.readout import embedding_neighbours_within
    n = e.shape[0] if n_rows is None else n_rows
    ref_buf = torch.full((capacity + 2 * pad,), SENTINEL, dtype=torch.int32, device=DEV)
    sim_buf = torch.full((capacity + 2 * pad,), float(SENTINEL), dtype=torch.float32, device=DEV)
    found = torch.full((n + 2 * pad,), SENTINEL, dtype=torch.int32, device=DEV)
    out = (ref_buf[pad:pad + capacity], sim_buf[pad:pad + capacity])
    got = embedding_neighbours_within(e, r, t, n_rows=n, row_ptr=torch.as_tensor(row_ptr, dtype=torch.int64).to(DEV), out=out,
                                      found=found[pad:pad + n], workspace=workspace)
    assert got[1].data_ptr() == out[0].data_ptr() and got[2].data_ptr() == out[1].data_ptr()
    torch.cuda.synchronize()
    return ref_buf.cpu().numpy(), sim_buf.cpu().numpy(), found.cpu().numpy()


def _expected_buffers(want, row_ptr, capacity, pad=6):
    """What THE GUARD lets through: row ``i`` writes the head of its true list into ``[row_ptr[i], min(row_ptr[i + 1], capacity))``
    if ``0 <= row_ptr[i]``, and nothing otherwise; everything else keeps its sentinel.  Also the slots written, to see that no two
    rows of the test's own row pointers write the same one."""
    true_ptr, nbr, val = want
    ref_buf = np.full(capacity + 2 * pad, SENTINEL, dtype=np.int32)
    sim_buf = np.full(capacity + 2 * pad, float(SENTINEL), dtype=np.float32)
    written = np.zeros(capacity, dtype=np.int64)
    for i in range(true_ptr.shape[0] - 1):
        lo, hi = int(row_ptr[i]), min(int(row_ptr[i + 1]), capacity)
        if lo < 0 or lo >= hi:
            continue
        k = min(hi - lo, int(true_ptr[i + 1] - true_ptr[i]))
        ref_buf[pad + lo:pad + lo + k] = nbr[true_ptr[i]:true_ptr[i] + k]
        sim_buf[pad + lo:pad + lo + k] = val[true_ptr[i]:true_ptr[i] + k]
        written[lo:lo + k] += 1
    assert written.max() <= 1
    return ref_buf, sim_buf, int(written.sum())


def _guarded(e, r, t, want, row_ptr, capacity, pad=6):
    ref_buf, sim_buf, found = _raw(e, r, t, row_ptr, capacity, pad=pad)
    want_ref, want_sim, n_written = _expected_buffers(want, row_ptr, capacity, pad)
    assert np.array_equal(ref_buf, want_ref) and np.array_equal(sim_buf.view(np.int32), want_sim.view(np.int32))
    assert np.array_equal(found[pad:-pad], np.diff(want[0])) and (found[:pad] == SENTINEL).all() and (found[-pad:] == SENTINEL).all()
    return n_written


def test_strides_sentinels_workspace_and_out():
    from molkgnn_amd import _lib
    from molkgnn_amd.readout import embedding_neighbours_within
    rows, tile, parts = CC.tiling()
    H, n, R = 31, rows + 1, 3 * tile
    emb, refs, _, _ = CC.float64_case(n, R, H)
    e, r = torch.tensor(emb, device=DEV), torch.tensor(refs, device=DEV)
    want = _lists(e, r, CC.MAX_SIM)
    nnz = int(want[0][-1])
    assert nnz >= n
    ep = torch.full((n + 6, H + 3), float("nan"), device=DEV)      # wider rows, and rows behind n_rows: NaN, never read into a list
    ep[:n, :H] = e
    rp = torch.full((R, H + 5), float("nan"), device=DEV)
    rp[:, :H] = r
    lib = _lib.load()
    need = lib.mkgnn_embed_neighbours_within_workspace_bytes(n, R)
    assert need == 4 * ((R + n + 3) // 4 * 4 + 3 * n) == lib.mkgnn_embed_count_within_workspace_bytes(n, R)
    ws = torch.full((need + 16,), 0xFF, dtype=torch.uint8, device=DEV)             # poisoned: it needs no initialisation
    padded = _lists(ep[:, :H], rp[:, :H], CC.MAX_SIM, n_rows=n, workspace=ws)
    assert _same(padded, want) and bool((ws[need:] == 0xFF).all())
    assert bool(torch.isnan(ep[:, H:]).all()) and bool(torch.isnan(ep[n:]).all()) and bool(torch.isnan(rp[:, H:]).all())
    # the raw form: sentinels around the lists and around found, the same poisoned workspace
    ws.fill_(0xFF)
    ref_buf, sim_buf, found = _raw(ep[:, :H], rp[:, :H], CC.MAX_SIM, want[0], nnz, n_rows=n, workspace=ws)
    want_ref, want_sim, n_written = _expected_buffers(want, want[0], nnz)
    assert n_written == nnz and np.array_equal(ref_buf, want_ref) and np.array_equal(sim_buf.view(np.int32), want_sim.view(np.int32))
    assert np.array_equal(found[6:-6], np.diff(want[0])) and (found[:6] == SENTINEL).all() and (found[-6:] == SENTINEL).all()
    assert bool((ws[need:] == 0xFF).all())
    # capacity 0 with no lists: found is still written
    found0 = torch.full((n,), SENTINEL, dtype=torch.int32, device=DEV)
    empty = (torch.empty(0, dtype=torch.int32, device=DEV), torch.empty(0, dtype=torch.float32, device=DEV))
    embedding_neighbours_within(e, r, CC.MAX_SIM, row_ptr=torch.zeros(n + 1, dtype=torch.int64, device=DEV), out=empty, found=found0)
    assert np.array_equal(found0.cpu().numpy(), np.diff(want[0]))
    ptr = torch.from_numpy(want[0]).to(DEV)
    out = (torch.empty(nnz, dtype=torch.int32, device=DEV), torch.empty(nnz, dtype=torch.float32, device=DEV))
    for bad in (dict(row_ptr=ptr[:-1]), dict(row_ptr=ptr.int()), dict(row_ptr=ptr.cpu()), dict(out=out[0]), dict(out=(out[1], out[0])),
                dict(out=(out[0], out[1][:-1])), dict(out=(out[0][::2], out[1][::2])), dict(found=found0[:-1]), dict(found=found0.long()),
                dict(found=None), dict(workspace=ws[:need - 1]), dict(workspace=ws.cpu())):
        kw = dict(row_ptr=ptr, out=out, found=found0)
        kw.update(bad)
        with pytest.raises(ValueError):
            embedding_neighbours_within(e, r, CC.MAX_SIM, **kw)
    for bad_rows in (-1, n + 1):
        with pytest.raises(ValueError):
            embedding_neighbours_within(e, r, CC.MAX_SIM, n_rows=bad_rows)
    none = _lists(e, r, CC.MAX_SIM, n_rows=0)                      # no rows: nothing is launched
    assert none[0].tolist() == [0] and none[1].shape == (0,)
    with pytest.raises(ValueError, match=f"nnz = {nnz}"):          # the cap is checked before the lists are allocated
        embedding_neighbours_within(e, r, CC.MAX_SIM, max_pairs=nnz - 1)
    assert _same(_lists(e, r, CC.MAX_SIM, max_pairs=nnz), want)
    with torch.enable_grad():
        with pytest.raises(RuntimeError):
            embedding_neighbours_within(e.clone().requires_grad_(), r, CC.MAX_SIM)


@pytest.mark.parametrize("shape", ["split", "one_part"])
def test_the_guard_keeps_every_store_inside_the_rows_segment_and_the_capacity(shape):
    """Bad row pointers are input that must be refused to write, not faults: whatever they hold, a row writes only the head of its
    list inside ``[row_ptr[i], min(row_ptr[i + 1], capacity))``, every other slot keeps its sentinel, and ``found`` is the true count."""
    from molkgnn_amd import _lib
    rows, tile, parts = CC.tiling()
    H = 33
    n, R = (2 * rows + 37, 3 * tile) if shape == "split" else (rows + 1, tile - 1)
    assert (_lib.count_within_split(n, R)[1] > 1) == (shape == "split")
    emb, refs, _, _ = CC.float64_case(n, R, H)
    e, r = torch.tensor(emb, device=DEV), torch.tensor(refs, device=DEV)
    sim = _sims(e, r)
    t = float(np.float32(np.quantile(sim[~np.isnan(sim)], 0.7)))    # about a third of all pairs: lists of many lengths
    want = _want(sim, t)
    true_ptr, nnz = want[0], int(want[0][-1])
    assert np.diff(true_ptr).max() >= 4 and _guarded(e, r, t, want, true_ptr, nnz) == nnz
    # 1. the row pointers of a HIGHER threshold's counts: every segment too short (or just right)
    short = _want(sim, float(np.float32(np.quantile(sim[~np.isnan(sim)], 0.85))))[0]
    assert (np.diff(short) <= np.diff(true_ptr)).all() and short[-1] < nnz
    assert _guarded(e, r, t, want, short, int(short[-1])) == short[-1]
    # 2. a capacity that ends in the middle of a row, and one that ends before the first slot of most rows
    longer = np.nonzero(np.diff(true_ptr) >= 2)[0]
    mid = int(longer[len(longer) // 2])
    cut = int(true_ptr[mid]) + 1
    assert _guarded(e, r, t, want, true_ptr, cut) == cut
    assert _guarded(e, r, t, want, true_ptr, 1) == 1
    # 3. row pointers that are not monotone: segments twice as long as needed (gaps keep their sentinels), two negative entries, one
    # entry above its successor, one far beyond the capacity
    wild = 2 * true_ptr.copy()
    capacity = int(wild[-1])
    wild[3] = -5                                                   # row 2 runs backwards, row 3 begins below 0
    wild[n // 3] = wild[n // 3 + 1] + 7                            # row n/3 runs backwards; row n/3 - 1 gets a longer segment
    wild[n - 4] = 1 << 40                                          # row n - 5's segment ends at the capacity, row n - 4 begins beyond it
    wild[n - 9] = -(1 << 62)
    written = _guarded(e, r, t, want, wild, capacity)
    assert 0 < written < nnz


def test_one_captured_count_cumsum_and_fill_follows_the_contents_of_both_inputs():
    from molkgnn_amd.readout import embedding_count_within, embedding_neighbours_within
    rows, tile, parts = CC.tiling()
    H, n, R = 64, rows + 40, 5 * tile + 3
    pool = CC.clustered(n + R, H, 1)
    e, r = torch.from_numpy(pool[:n].copy()).to(DEV), torch.from_numpy(pool[n:].copy()).to(DEV)
    capacity = n * R // 4
    counts = torch.empty(n, dtype=torch.int32, device=DEV)
    found = torch.empty(n, dtype=torch.int32, device=DEV)
    row_ptr = torch.zeros(n + 1, dtype=torch.int64, device=DEV)
    out = (torch.empty(capacity, dtype=torch.int32, device=DEV), torch.empty(capacity, dtype=torch.float32, device=DEV))

    def step():
        embedding_count_within(e, r, CC.MAX_SIM, out=counts)
        row_ptr[1:] = torch.cumsum(counts, dim=0, dtype=torch.int64)
        embedding_neighbours_within(e, r, CC.MAX_SIM, row_ptr=row_ptr, out=out, found=found)

    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        step()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            step()
    torch.cuda.current_stream(DEV).wait_stream(side)
    seen = set()
    for seed_e, seed_r in ((2, 2), (2, 3), (3, 3)):                # the rows change, the references change, both do
        e.copy_(torch.from_numpy(CC.clustered(n + R, H, seed_e)[:n].copy()).to(DEV))
        r.copy_(torch.from_numpy(CC.clustered(n + R, H, seed_r)[n:].copy()).to(DEV))
        for buf in (counts, found, out[0]):
            buf.fill_(-9)
        out[1].fill_(-9.0)
        graph.replay()
        torch.cuda.synchronize()
        want = _want(_sims(e, r), CC.MAX_SIM)
        nnz = int(want[0][-1])
        assert nnz <= capacity and (nnz > 0) == (seed_e == seed_r)  # (rows and references of different pools share no centre)
        got = (row_ptr.cpu().numpy(), out[0][:nnz].cpu().numpy(), out[1][:nnz].cpu().numpy())
        assert _same(got, want) and torch.equal(found, counts) and bool((out[0][nnz:] == -9).all())
        assert _same(_lists(e, r, CC.MAX_SIM), want)
        seen.add(tuple(got[1].tolist()))
    assert len(seen) == 3                                          # (the three contents do give different lists)


def test_c_abi_rejects_before_any_launch():
    from molkgnn_amd import _lib
    lib = _lib.load()
    rows, tile, parts = CC.tiling()
    n, R, H = 40, 2 * tile + 1, 20
    pool = CC.clustered(n + R, H, 9)
    e, r = torch.from_numpy(pool[:n].copy()).to(DEV), torch.from_numpy(pool[n:].copy()).to(DEV)
    sim = _sims(e, r)
    want = _want(sim, 0.9)
    cap = int(want[0][-1])
    assert cap >= 4
    ptr = torch.from_numpy(want[0]).to(DEV)
    nbr = torch.full((cap,), SENTINEL, dtype=torch.int32, device=DEV)
    val = torch.full((cap,), float(SENTINEL), dtype=torch.float32, device=DEV)
    found = torch.full((n,), SENTINEL, dtype=torch.int32, device=DEV)
    need = lib.mkgnn_embed_neighbours_within_workspace_bytes(n, R)
    assert need == 4 * ((R + n + 3) // 4 * 4 + 3 * n)
    ws = torch.zeros(need + 8, dtype=torch.uint8, device=DEV)
    st = _lib.stream_ptr(torch.device(DEV))

    def call(emb=e.data_ptr(), es=H, n_rows=n, width=H, refs=r.data_ptr(), rs=H, n_refs=R, min_sim=0.9, row_ptr=ptr.data_ptr(),
             capacity=cap, ref=nbr.data_ptr(), sims=val.data_ptr(), count=found.data_ptr(), work=ws.data_ptr(), work_bytes=need):
        return lib.mkgnn_embed_neighbours_within(emb, es, n_rows, width, refs, rs, n_refs, min_sim, row_ptr, capacity, ref, sims, count,
                                                 work, work_bytes, st)

    refused = (("width", dict(width=0)), ("width", dict(width=65, es=65, rs=65)), ("references", dict(n_refs=0)),
               ("references", dict(n_refs=_lib.MAX_COSINE_MAX_REFS + 1)), ("bad shape", dict(n_rows=-1)), ("bad shape", dict(es=H - 1)),
               ("bad shape", dict(rs=H - 1)), ("bad shape", dict(capacity=-1)), ("finite", dict(min_sim=float("nan"))),
               ("finite", dict(min_sim=float("inf"))), ("finite", dict(min_sim=float("-inf"))), ("null", dict(emb=None)),
               ("null", dict(refs=None)), ("null", dict(row_ptr=None)), ("null", dict(ref=None)), ("null", dict(sims=None)),
               ("null", dict(count=None)), ("null", dict(work=None)), ("workspace", dict(work_bytes=need - 1)),
               ("aligned", dict(work=ws.data_ptr() + 1)), ("aliases an input", dict(ref=e.data_ptr())),
               ("aliases an input", dict(sims=r.data_ptr() + 4 * (R * H - 1))), ("aliases an input", dict(count=ptr.data_ptr() + 8 * n)),
               ("aliases an input", dict(work=e.data_ptr())), ("aliases an input", dict(ref=ptr.data_ptr())),
               ("alias each other", dict(count=ws.data_ptr() + need - 4)), ("alias each other", dict(sims=nbr.data_ptr() + 4 * (cap - 1))),
               ("alias each other", dict(count=nbr.data_ptr())))
    for word, kw in refused:
        assert call(**kw) != 0, kw
        assert word in lib.mkgnn_last_error().decode(), (kw, lib.mkgnn_last_error())
    assert call(n_rows=0, emb=None, refs=None, row_ptr=None, ref=None, sims=None, count=None, work=None, work_bytes=0) == 0      # a no-op
    torch.cuda.synchronize()
    assert bool((nbr == SENTINEL).all()) and bool((found == SENTINEL).all())
    assert call() == 0
    assert _same((want[0], nbr.cpu().numpy(), val.cpu().numpy()), want) and np.array_equal(found.cpu().numpy(), np.diff(want[0]))
    # no lists at all: capacity 0 with null pointers is legal, and found is written
    found.fill_(SENTINEL)
    assert call(capacity=0, ref=None, sims=None) == 0 and np.array_equal(found.cpu().numpy(), np.diff(want[0]))
    # a poisoned workspace gives the same result; the same pointer for both sets is a self-join
    ws.fill_(0xFF)
    nbr.fill_(SENTINEL)
    assert call() == 0 and _same((want[0], nbr.cpu().numpy(), val.cpu().numpy()), want)
    self_want = _want(_sims(e, e), 0.9)
    self_cap = int(self_want[0][-1])
    self_ptr = torch.from_numpy(self_want[0]).to(DEV)
    self_nbr, self_val = torch.empty(self_cap, dtype=torch.int32, device=DEV), torch.empty(self_cap, dtype=torch.float32, device=DEV)
    self_ws = torch.zeros(lib.mkgnn_embed_neighbours_within_workspace_bytes(n, n), dtype=torch.uint8, device=DEV)
    assert call(refs=e.data_ptr(), n_refs=n, row_ptr=self_ptr.data_ptr(), capacity=self_cap, ref=self_nbr.data_ptr(),
                sims=self_val.data_ptr(), work=self_ws.data_ptr(), work_bytes=self_ws.numel()) == 0
    assert _same((self_want[0], self_nbr.cpu().numpy(), self_val.cpu().numpy()), self_want)


def test_torch_route_beyond_the_kernels_width_meets_the_float64_lists():
    from molkgnn_amd import readout
    from molkgnn_amd.screening import cosine_bound, cosine_reference, neighbours_reference
    H, n, R = 65, 150, 130
    assert not readout.embedding_neighbours_within_supported(R, H) and readout.embedding_neighbours_within_supported(R, 64)
    pool = CC.clustered(n + R, H, 13)
    emb, refs = pool[:n].copy(), pool[n:].copy()
    sim = cosine_reference(emb, refs)
    assert (np.abs(sim - CC.MAX_SIM) / cosine_bound(emb, refs)).min() > 4
    emb[17] = np.nan
    emb[19] = 0.0
    refs[3] = np.nan
    sim = cosine_reference(emb, refs)
    want = neighbours_reference(sim, CC.MAX_SIM)
    e, r = torch.from_numpy(emb).to(DEV), torch.from_numpy(refs).to(DEV)
    got = _lists(e, r, CC.MAX_SIM)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.diff(got[0]).max() >= 2
    assert got[0][18] == got[0][17] and got[0][20] == got[0][19] and 3 not in got[1].tolist()
    assert (np.abs(got[2] - want[2]) <= cosine_bound(emb, refs)[np.repeat(np.arange(n), np.diff(want[0])), want[1]]).all()
    # more than one chunk of references gives the same lists, in ascending reference order
    old = readout.MAX_COSINE_TORCH_CHUNK
    readout.MAX_COSINE_TORCH_CHUNK = 37
    try:
        chunked = _lists(e, r, CC.MAX_SIM)
    finally:
        readout.MAX_COSINE_TORCH_CHUNK = old
    assert _same(chunked, got)
    with pytest.raises(ValueError, match="nnz"):
        readout.embedding_neighbours_within(e, r, CC.MAX_SIM, max_pairs=3)
    with pytest.raises(ValueError, match="raw form"):
        readout.embedding_neighbours_within(e, r, CC.MAX_SIM, row_ptr=torch.zeros(n + 1, dtype=torch.int64, device=DEV),
                                            out=(torch.empty(4, dtype=torch.int32, device=DEV), torch.empty(4, dtype=torch.float32, device=DEV)),
                                            found=torch.empty(n, dtype=torch.int32, device=DEV))
