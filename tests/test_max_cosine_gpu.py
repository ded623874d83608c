"""``mkgnn_embed_max_cosine`` and ``mkgnn_select_rows`` on the GPU.  The nearest reference of every row against the host winner of
``mkgnn_embed_cosine``'s own similarities (bits, every row), against the float64 definition (tie-aware, within ``cosine_bound``);
NaN rows and references; independence of the row's place and of the split of the references; strides, sentinels, capture; the
compaction against ``select_rows_reference`` (bits); what the C ABI rejects; the torch route beyond ``H = 64``."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WIDTHS = (1, 31, 32, 33, 64)


def _bits(t):
    return t.detach().contiguous().view(torch.int32).cpu().numpy()


def _constants():
    from molkgnn_amd import _lib
    return _lib.MAX_COSINE_ROWS, _lib.MAX_COSINE_TILE, _lib.MAX_COSINE_MAX_PARTS


def _shapes():
    """``(n, R)``: ``n`` on either side of the rows of a block and one larger value; ``R`` = 1, 2, 33, on either side of the LDS tile,
    three one-tile parts, and -- beyond ``MAX_PARTS`` tiles, where a part holds several tiles -- on either side of a part's end."""
    from molkgnn_amd import _lib
    rows, tile, parts = _constants()
    many = tile * parts                                            # the most references whose parts are single tiles
    shapes = [(rows - 1, 1), (rows, 2), (rows + 1, 33), (17, tile - 1), (rows + 1, tile), (rows - 1, tile + 1), (1000, 3 * tile),
              (1000, 3 * tile + 1), (17, many + 1), (rows + 1, 2 * many + 5)]
    assert _lib.max_cosine_split(rows - 1, 1) == (tile, 1) and _lib.max_cosine_split(rows + 1, tile) == (tile, 1)
    assert _lib.max_cosine_split(rows - 1, tile + 1) == (tile, 2) and _lib.max_cosine_split(1000, 3 * tile) == (tile, 3)
    assert _lib.max_cosine_split(1000, 3 * tile + 1) == (tile, 4)
    assert _lib.max_cosine_split(17, many + 1) == (2 * tile, parts // 2 + 1)          # two tiles per part, the last part one reference
    assert _lib.max_cosine_split(rows + 1, 2 * many + 5) == (3 * tile, (2 * parts + 1 + 2) // 3)
    return shapes


def _inputs(n, H, R, seed):
    """float32 ``emb [n, H]`` and ``refs [R, H]`` with the hazards planted: a zero row, a row below the norm clamp, denormals, a row at
    scale 1e15, a row equal to a reference; a reference duplicated at two indices (the second and the last: in different tiles and
    parts wherever there are several), a zero reference."""
    rng = np.random.default_rng(seed)
    emb = rng.standard_normal((n, H)).astype(np.float32)
    refs = rng.standard_normal((R, H)).astype(np.float32)
    if R > 3:
        refs[2] = 0.0
    if R > 2:
        refs[R - 1] = refs[1]
    emb[0] = 0.0
    emb[1] = np.float32(3e-9) / np.sqrt(np.float32(H))
    emb[2] = (np.float32(1e-41) * np.arange(1, H + 1)).astype(np.float32)
    emb[3] *= np.float32(1e15)
    emb[4] = refs[min(1, R - 1)]
    emb[5] = -refs[0]
    return emb, refs


def _all_sims(emb, refs):
    """``sim [n, R]`` on the host: ``mkgnn_embed_cosine`` on the references in groups of 32."""
    from molkgnn_amd.readout import embedding_cosine
    out = torch.empty(emb.shape[0], refs.shape[0], dtype=torch.float32, device=emb.device)
    for a in range(0, refs.shape[0], 32):
        out[:, a:a + 32] = embedding_cosine(emb, refs[a:a + 32])
    return out.cpu().numpy()


def _host_winner(sim):
    """The stated order on float32 similarities: ``(value with its bits, index)`` per row."""
    nan = np.isnan(sim)
    clean = np.where(nan, np.float32(-np.inf), sim)
    cand = (clean == clean.max(axis=1, keepdims=True)) & ~nan      # (-0.0 == +0.0)
    arg = np.where(cand.any(axis=1), cand.argmax(axis=1), 0)
    return sim[np.arange(len(sim)), arg], arg.astype(np.int32), cand.any(axis=1)


def _agree(got_sim, got_arg, sim):
    """Bit for bit the host winner of ``sim``, for every row (a NaN winner: any NaN, index 0)."""
    want, warg, some = _host_winner(sim)
    got_sim, got_arg = got_sim.cpu().numpy(), got_arg.cpu().numpy()
    assert got_arg.dtype == np.int32 and np.array_equal(got_arg, warg)
    assert np.array_equal(got_sim.view(np.int32)[some], want.view(np.int32)[some])
    assert np.isnan(got_sim[~some]).all()


@functools.lru_cache(maxsize=None)
def _cases(H):
    """Every shape at width ``H``, run ONCE: the inputs, the kernel's outputs and ``mkgnn_embed_cosine``'s similarities."""
    from molkgnn_amd.readout import embedding_max_cosine
    cases = []
    for j, (n, R) in enumerate(_shapes()):
        emb, refs = _inputs(n, H, R, 1000 * H + j)
        e, q = torch.from_numpy(emb).to(DEV), torch.from_numpy(refs).to(DEV)
        max_sim, arg_ref = embedding_max_cosine(e, q)
        assert max_sim.shape == arg_ref.shape == (n,) and max_sim.dtype == torch.float32 and arg_ref.dtype == torch.int32
        cases.append((emb, refs, max_sim, arg_ref, _all_sims(e, q)))
    return cases


@pytest.mark.parametrize("H", WIDTHS)
def test_bits_are_those_of_embed_cosine_for_every_row(H):
    for emb, refs, max_sim, arg_ref, sim in _cases(H):
        n, R = len(emb), len(refs)
        _agree(max_sim, arg_ref, sim)
        arg = arg_ref.cpu().numpy()
        assert arg[0] == 0 and _bits(max_sim)[0] == 0              # the zero row: +0.0 everywhere, the first reference
        if R > 3 and H > 1:                                        # (H = 1: every similarity is +-1 to rounding)
            assert arg[4] == 1, (n, R)                             # equal to reference 1 and to its duplicate R - 1: the lower index


@pytest.mark.parametrize("H", WIDTHS)
def test_float64_criterion_is_tie_aware_and_leaves_no_row_out(H):
    """With ``a`` the kernel's winner and ``a64`` the float64 one: ``|sim32[a] - sim64[a]| <= bound[a]`` and ``sim32[a] >= sim32[a64] >=
    max64 - bound[a64]`` give ``|max_sim - max64| <= b`` and ``sim64[a] >= max64 - 2 b`` for ``b = max(bound[a], bound[a64])`` --
    ``cosine_bound`` at the row's two winning elements."""
    from molkgnn_amd.screening import cosine_bound, cosine_reference, max_cosine_reference
    for emb, refs, max_sim, arg_ref, _ in _cases(H):
        rows = np.arange(len(emb))
        sim64, bound = cosine_reference(emb, refs), cosine_bound(emb, refs)
        max64, arg64 = max_cosine_reference(emb, refs)
        got, arg = max_sim.cpu().numpy().astype(np.float64), arg_ref.cpu().numpy()
        assert not np.isnan(got).any() and not np.isnan(max64).any()
        b = np.maximum(bound[rows, arg], bound[rows, arg64])
        assert (np.abs(got - max64) <= b).all(), (emb.shape, refs.shape, float((np.abs(got - max64) / b).max()))
        assert (sim64[rows, arg] >= max64 - 2 * b).all(), (emb.shape, refs.shape)


def _base(H=33, n=None, R=None, seed=77):
    rows, tile, _ = _constants()
    emb, refs = _inputs(rows + 2 if n is None else n, H, 3 * tile + 1 if R is None else R, seed)
    return torch.from_numpy(emb).to(DEV), torch.from_numpy(refs).to(DEV)


def test_nan_stays_in_its_row_and_a_nan_reference_only_loses():
    from molkgnn_amd.readout import embedding_max_cosine
    e, q = _base()
    sim0, arg0 = embedding_max_cosine(e, q)
    e2 = e.clone()
    e2[9, 7] = float("nan")
    sim1, arg1 = embedding_max_cosine(e2, q)
    assert bool(torch.isnan(sim1[9])) and int(arg1[9]) == 0
    keep = np.arange(len(e)) != 9
    assert np.array_equal(_bits(sim1)[keep], _bits(sim0)[keep]) and np.array_equal(arg1.cpu().numpy()[keep], arg0.cpu().numpy()[keep])
    # a NaN reference: where it was the winner another one wins, nothing else changes; at index 0 it is skipped too
    for r in {int(arg0[7]), 0, len(q) - 1}:
        q2 = q.clone()
        q2[r, 3] = float("nan")
        sim2, arg2 = embedding_max_cosine(e, q2)
        was = arg0.cpu().numpy() == r
        assert np.array_equal(_bits(sim2)[~was], _bits(sim0)[~was]) and np.array_equal(arg2.cpu().numpy()[~was], arg0.cpu().numpy()[~was])
        assert not (arg2.cpu().numpy() == r).any() and not bool(torch.isnan(sim2).any())
        _agree(sim2, arg2, _all_sims(e, q2))
    # every reference NaN: (NaN, 0) everywhere
    sim3, arg3 = embedding_max_cosine(e, torch.full_like(q, float("nan")))
    assert bool(torch.isnan(sim3).all()) and not bool(arg3.any())


def test_result_does_not_depend_on_position_or_split():
    from molkgnn_amd import _lib
    from molkgnn_amd.readout import embedding_max_cosine
    rows, tile, _ = _constants()
    e, q = _base(H=32, n=1000, R=3 * tile)
    sim0, arg0 = embedding_max_cosine(e, q)
    perm = torch.randperm(1000, generator=torch.Generator().manual_seed(1)).to(DEV)
    sim1, arg1 = embedding_max_cosine(e[perm].contiguous(), q)
    assert np.array_equal(_bits(sim1), _bits(sim0[perm])) and np.array_equal(arg1.cpu().numpy(), arg0[perm].cpu().numpy())
    # 17 rows: another grid (one row block, as many parts as tiles), the same 17 answers; n_rows cuts the same way
    assert _lib.max_cosine_split(17, 3 * tile)[1] == 3
    for sim2, arg2 in (embedding_max_cosine(e[:17], q), embedding_max_cosine(e, q, n_rows=17)):
        assert sim2.shape == (17,) and np.array_equal(_bits(sim2), _bits(sim0[:17])) and np.array_equal(arg2.cpu().numpy(), arg0[:17].cpu().numpy())
    # the references cut in two separate calls, inside a tile and at a part's end: the host combination under the stated order
    assert _lib.max_cosine_split(1000, 3 * tile)[0] == tile
    for a in (5, tile, 2 * tile, 3 * tile - 1):
        (s1, a1), (s2, a2) = embedding_max_cosine(e, q[:a]), embedding_max_cosine(e, q[a:])
        take = ~torch.isnan(s2) & (torch.isnan(s1) | (s2 > s1))
        assert np.array_equal(_bits(torch.where(take, s2, s1)), _bits(sim0)), a
        assert np.array_equal(torch.where(take, a2 + a, a1).cpu().numpy(), arg0.cpu().numpy()), a


def test_strides_and_sentinels():
    from molkgnn_amd.readout import embedding_max_cosine
    e, q = _base(H=31)
    n, H, R = e.shape[0], 31, q.shape[0]
    sim0, arg0 = embedding_max_cosine(e, q)
    ep = torch.full((n, H + 3), float("nan"), device=DEV)
    qp = torch.full((R, H + 5), float("nan"), device=DEV)
    ep[:, :H], qp[:, :H] = e, q
    fbuf = torch.full((n + 9,), -7.5, device=DEV)
    ibuf = torch.full((n + 9,), -77, dtype=torch.int32, device=DEV)
    out = (fbuf[3:3 + n], ibuf[5:5 + n])
    sim1, arg1 = embedding_max_cosine(ep[:, :H], qp[:, :H], out=out)
    assert sim1 is out[0] and arg1 is out[1]
    assert np.array_equal(_bits(sim1), _bits(sim0)) and np.array_equal(arg1.cpu().numpy(), arg0.cpu().numpy())
    assert bool((fbuf[:3] == -7.5).all()) and bool((fbuf[3 + n:] == -7.5).all())
    assert bool((ibuf[:5] == -77).all()) and bool((ibuf[5 + n:] == -77).all())
    assert bool(torch.isnan(ep[:, H:]).all()) and bool(torch.isnan(qp[:, H:]).all())
    for bad in ((fbuf[3:3 + n], ibuf[5:4 + n]), (fbuf[3:3 + n].double(), ibuf[5:5 + n]), (fbuf[0:2 * n:2], ibuf[5:5 + n])):
        with pytest.raises(ValueError):
            embedding_max_cosine(e, q, out=bad)
    # the caller's own scratch, poisoned: the same bits (the workspace needs no initialisation); one that is too small is refused
    from molkgnn_amd import _lib
    need = int(_lib.load().mkgnn_embed_max_cosine_workspace_bytes(n, R))
    own = torch.full((need + 5,), 0xFF, dtype=torch.uint8, device=DEV)
    sim2, arg2 = embedding_max_cosine(e, q, workspace=own)
    assert np.array_equal(_bits(sim2), _bits(sim0)) and np.array_equal(arg2.cpu().numpy(), arg0.cpu().numpy())
    for bad in (own[:need - 1], own.float(), own.cpu()):
        with pytest.raises(ValueError):
            embedding_max_cosine(e, q, workspace=bad)
    # no rows: nothing is launched, nothing is written
    s, a = embedding_max_cosine(e, q, n_rows=0)
    assert s.shape == a.shape == (0,)
    with torch.enable_grad():
        with pytest.raises(RuntimeError):
            embedding_max_cosine(e.clone().requires_grad_(), q)


def test_one_captured_call_follows_both_inputs():
    from molkgnn_amd.readout import embedding_max_cosine
    e, q = _base(H=64)
    n = e.shape[0]
    out = (torch.empty(n, device=DEV), torch.empty(n, dtype=torch.int32, device=DEV))
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        embedding_max_cosine(e, q, out=out)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            embedding_max_cosine(e, q, out=out)
    torch.cuda.current_stream(DEV).wait_stream(side)
    gen = torch.Generator(device=DEV).manual_seed(5)
    for scale in (1.0, 1e-3, 1e4):
        e.copy_(torch.randn(e.shape, generator=gen, device=DEV))
        q.copy_(torch.randn(q.shape, generator=gen, device=DEV) * scale)         # (another norm scale: the norms are the call's own)
        graph.replay()
        sim1, arg1 = embedding_max_cosine(e, q)
        assert np.array_equal(_bits(out[0]), _bits(sim1)) and np.array_equal(out[1].cpu().numpy(), arg1.cpu().numpy())
        _agree(out[0], out[1], _all_sims(e, q))


def _select_inputs(B, seed):
    rng = np.random.default_rng(seed)
    scores = rng.standard_normal(B).astype(np.float32)
    key = rng.uniform(-1, 1, B).astype(np.float32)
    key[rng.integers(0, B, max(B // 9, 1))] = np.nan
    scores[0] = np.float32(-0.0)
    if B > 2:
        scores[2] = np.nan
        key[1] = 0.25
    ids = rng.permutation(B).astype(np.int32)
    return scores, ids, key


@pytest.mark.parametrize("B", [1, 63, 64, 65, 1025, 4096])
def test_select_rows_is_the_reference_by_bits(B):
    from molkgnn_amd.readout import select_rows
    from molkgnn_amd.screening import select_rows_reference
    scores, ids, key = _select_inputs(B, B)
    real = np.sort(key[~np.isnan(key)]) if (~np.isnan(key)).any() else np.array([0.0], dtype=np.float32)
    lo, hi = float(real[len(real) // 4]), float(real[(3 * len(real)) // 4])       # bounds AT keys' exact values
    s, i, k = (torch.from_numpy(a).to(DEV) for a in (scores, ids, key))
    for n_valid in (0, 1, B - 1, B, B + 5, -3):
        for a, b in ((lo, hi), (-np.inf, hi), (lo, np.inf), (-np.inf, np.inf), (hi, lo) if hi > lo else (1.0, -1.0)):
            out = (torch.full((B,), -7.5, device=DEV), torch.full((B,), -77, dtype=torch.int32, device=DEV),
                   torch.full((1,), -5, dtype=torch.int32, device=DEV))
            bounds = torch.tensor([a, b], dtype=torch.float32, device=DEV)
            got = select_rows(s, i, k, n_valid, bounds, out=out)
            assert all(x is y for x, y in zip(got, out))
            ws, wi, wn = select_rows_reference(scores, ids, key, n_valid, a, b)
            assert int(out[2]) == wn, (n_valid, a, b)
            assert np.array_equal(_bits(out[0][:wn]), ws.view(np.int32)) and np.array_equal(out[1][:wn].cpu().numpy(), wi)
            assert bool((out[0][wn:] == -7.5).all()) and bool((out[1][wn:] == -77).all())         # slots past n_kept keep their sentinel
    # the count as a device scalar, and fresh outputs
    nv = torch.tensor([B], dtype=torch.int32, device=DEV)
    os_, oi, nk = select_rows(s, i, k, nv, torch.tensor([lo, hi], device=DEV))
    ws, wi, wn = select_rows_reference(scores, ids, key, B, lo, hi)
    assert int(nk) == wn and np.array_equal(_bits(os_[:wn]), ws.view(np.int32)) and np.array_equal(oi[:wn].cpu().numpy(), wi)


def test_one_captured_select_follows_count_and_bounds():
    from molkgnn_amd.readout import select_rows
    from molkgnn_amd.screening import select_rows_reference
    B = 1500
    scores, ids, key = _select_inputs(B, 3)
    s, i, k = (torch.from_numpy(a).to(DEV) for a in (scores, ids, key))
    nv = torch.zeros(1, dtype=torch.int32, device=DEV)
    bounds = torch.zeros(2, device=DEV)
    out = (torch.empty(B, device=DEV), torch.empty(B, dtype=torch.int32, device=DEV), torch.empty(1, dtype=torch.int32, device=DEV))
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            select_rows(s, i, k, nv, bounds, out=out)
    torch.cuda.current_stream(DEV).wait_stream(side)
    for n_valid, lo, hi in ((B, -0.5, 0.5), (1100, 0.25, np.inf), (0, -1.0, 1.0), (B + 7, -np.inf, 0.25), (3, -np.inf, np.inf)):
        nv.fill_(n_valid)
        bounds.copy_(torch.tensor([lo, hi]))
        out[0].fill_(-7.5)
        graph.replay()
        ws, wi, wn = select_rows_reference(scores, ids, key, n_valid, lo, hi)
        assert int(out[2]) == wn and np.array_equal(_bits(out[0][:wn]), ws.view(np.int32)) and np.array_equal(out[1][:wn].cpu().numpy(), wi)
        assert bool((out[0][wn:] == -7.5).all())


def test_c_abi_rejects_before_any_launch():
    from molkgnn_amd import _lib
    lib = _lib.load()
    n, H, R = 40, 20, 50
    e, q = _base(H=H, n=n, R=R)
    sim = torch.full((n,), -7.5, device=DEV)
    arg = torch.full((n,), -77, dtype=torch.int32, device=DEV)
    need = lib.mkgnn_embed_max_cosine_workspace_bytes(n, R)
    assert need > 0
    ws = torch.zeros(need, dtype=torch.uint8, device=DEV)
    st = _lib.stream_ptr(torch.device(DEV))

    def call(emb=e.data_ptr(), es=H, rows=n, width=H, refs=q.data_ptr(), rs=H, count=R, out_sim=sim.data_ptr(), out_arg=arg.data_ptr(),
             work=ws.data_ptr(), work_bytes=need):
        return lib.mkgnn_embed_max_cosine(emb, es, rows, width, refs, rs, count, out_sim, out_arg, work, work_bytes, st)

    refused = (("outside", dict(width=0)), ("outside", dict(width=65, es=65, rs=65)), ("references outside", dict(count=0)),
               ("references outside", dict(count=_lib.MAX_COSINE_MAX_REFS + 1)), ("bad shape", dict(rows=-1)), ("bad shape", dict(es=H - 1)),
               ("bad shape", dict(rs=H - 1)), ("null", dict(emb=None)), ("null", dict(refs=None)), ("null", dict(out_sim=None)),
               ("null", dict(out_arg=None)), ("null", dict(work=None)), ("workspace", dict(work_bytes=need - 1)),
               ("aligned", dict(work=ws.data_ptr() + 1, work_bytes=need)), ("rows", dict(rows=1 << 31)))
    for word, kw in refused:
        assert call(**kw) != 0, kw
        assert word in lib.mkgnn_last_error().decode(), (kw, lib.mkgnn_last_error())
    assert call(rows=0, emb=None, refs=None, out_sim=None, out_arg=None, work=None, work_bytes=0) == 0       # a no-op
    torch.cuda.synchronize()
    assert bool((sim == -7.5).all()) and bool((arg == -77).all())          # nothing was launched
    assert call() == 0
    _agree(sim, arg, _all_sims(e, q))
    # mkgnn_select_rows
    B = 10
    s, k = torch.randn(B, device=DEV), torch.randn(B, device=DEV)
    i = torch.arange(B, dtype=torch.int32, device=DEV)
    nv, bounds = torch.tensor([B], dtype=torch.int32, device=DEV), torch.tensor([-1.0, 1.0], device=DEV)
    os_, oi = torch.full((B,), -7.5, device=DEV), torch.full((B,), -77, dtype=torch.int32, device=DEV)
    nk = torch.full((1,), -5, dtype=torch.int32, device=DEV)
    good = [s.data_ptr(), i.data_ptr(), k.data_ptr(), B, nv.data_ptr(), bounds.data_ptr(), os_.data_ptr(), oi.data_ptr(), nk.data_ptr(), st]
    for word, at, value in [("at least one", 3, 0), ("at least one", 3, -4)] + [("null", j, None) for j in (0, 1, 2, 4, 5, 6, 7, 8)] + \
            [("alias", 6, s.data_ptr()), ("alias", 7, i.data_ptr()), ("alias", 6, k.data_ptr() + 4), ("alias", 7, os_.data_ptr()),
             ("alias", 8, nv.data_ptr()), ("alias", 8, bounds.data_ptr() + 4), ("alias", 8, os_.data_ptr() + 8)]:
        args = list(good)
        args[at] = value
        assert lib.mkgnn_select_rows(*args) != 0, (word, at)
        assert word in lib.mkgnn_last_error().decode(), (word, at, lib.mkgnn_last_error())
    torch.cuda.synchronize()
    assert bool((os_ == -7.5).all()) and bool((oi == -77).all()) and int(nk) == -5
    assert lib.mkgnn_select_rows(*good) == 0
    assert int(nk) == int(((k >= -1) & (k <= 1)).sum())


def test_torch_route_beyond_the_kernels_width_meets_the_float64_criterion():
    from molkgnn_amd import readout
    from molkgnn_amd.screening import cosine_bound, cosine_reference, max_cosine_reference
    H, n, R = 80, 50, 70
    assert not readout.embedding_max_cosine_supported(R, H) and readout.embedding_max_cosine_supported(R, 64)
    assert not readout.embedding_max_cosine_supported((1 << 20) + 1, 32) and not readout.embedding_max_cosine_supported(0, 32)
    emb, refs = _inputs(n, H, R, 11)
    refs[7] = np.nan
    chunk = readout.MAX_COSINE_TORCH_CHUNK
    readout.MAX_COSINE_TORCH_CHUNK = 32                            # three chunks, so the combination across chunks runs
    try:
        max_sim, arg_ref = readout.embedding_max_cosine(torch.from_numpy(emb).to(DEV), torch.from_numpy(refs).to(DEV))
    finally:
        readout.MAX_COSINE_TORCH_CHUNK = chunk
    rows = np.arange(n)
    sim64, bound = cosine_reference(emb, refs), cosine_bound(emb, refs)
    max64, arg64 = max_cosine_reference(emb, refs)
    got, arg = max_sim.cpu().numpy().astype(np.float64), arg_ref.cpu().numpy()
    assert arg_ref.dtype == torch.int32 and not (arg == 7).any() and arg[4] == 1
    b = np.maximum(bound[rows, arg], bound[rows, arg64])
    assert (np.abs(got - max64) <= b).all() and (sim64[rows, arg] >= max64 - 2 * b).all()
