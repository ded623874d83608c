"""``mkgnn_embed_cosine`` (``readout.embedding_cosine``): the cosine similarity of every embedding row with every query.  Every
element within ``screening.cosine_bound`` of ``screening.cosine_reference`` (float64), the special rows by bits, NaN confinement,
strides and both output layouts, position independence by bits, one captured launch serving new contents, rejections, and the
torch route beyond the kernel's limits."""
from functools import lru_cache

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
R = 16                                  # HEAD_ROWS: the kernel's rows per block
ROWS = (1, R - 1, R, R + 1, 2 * R + 1, 1000)


def _L():
    from molkgnn_amd import _lib
    return _lib


def _bits(t):
    return t.detach().contiguous().view(torch.int32).cpu().numpy()


def _cos(emb, q, **kw):
    from molkgnn_amd.readout import embedding_cosine
    return embedding_cosine(emb, q, **kw)


@lru_cache(maxsize=None)
def _queries(Q, H):
    """float32 CPU ``[Q, H]`` (never written to): query 0 has no positive value (a zero row's products with it are all -0.0);
    query 3, where there is one, is zero."""
    g = torch.Generator().manual_seed(100 * Q + H)
    q = torch.randn(Q, H, generator=g)
    q[0] = -q[0].abs() - 0.1
    if Q > 3:
        q[3] = 0.0
    return q


@lru_cache(maxsize=None)
def _rows(n, H, Q):
    """float32 CPU ``[n, H]`` (never written to) whose LAST rows are planted, as many as fit -- from the end: zeros; norm 3e-9
    (clamped); the last query; the negative of query 0; denormals; scale 1e15."""
    q = _queries(Q, H)
    g = torch.Generator().manual_seed(1000 * n + 10 * H + Q)
    e = torch.randn(n, H, generator=g) * 2
    planted = [torch.zeros(H), torch.full((H,), 3e-9 / H ** 0.5), q[Q - 1].clone(), -q[0], 1e-41 * torch.arange(1, H + 1),
               torch.randn(H, generator=g) * 1e15]
    for j, row in enumerate(planted[:n]):
        e[n - 1 - j] = row
    return e


@pytest.mark.parametrize("Q", [1, 9, 32])
@pytest.mark.parametrize("H", [1, 31, 32, 33, 64])
def test_every_element_within_the_bound_of_the_float64_reference(H, Q):
    from molkgnn_amd.screening import cosine_bound, cosine_reference
    q_c = _queries(Q, H)
    q = q_c.to(DEV)
    worst = 0.0
    for n in ROWS:
        e_c = _rows(n, H, Q)
        sim = _cos(e_c.to(DEV), q)
        assert sim.shape == (n, Q) and sim.dtype == torch.float32 and sim.is_contiguous()
        got = sim.cpu().numpy()
        err = np.abs(got.astype(np.float64) - cosine_reference(e_c, q_c))
        bound = cosine_bound(e_c, q_c)
        worst = max(worst, float((err / bound).max()))
        assert (err <= bound).all(), (n, H, Q, float((err / bound).max()), np.argwhere(err > bound)[:4].tolist())
        assert (got[n - 1].view(np.int32) == 0).all(), (n, H, Q)          # the zero row: +0.0 by bits, against negative queries too
        if Q > 3:
            assert (got[:, 3].view(np.int32) == 0).all(), (n, H, Q)       # the zero query
        if n >= 6:
            # a row equal to a query and the negative of one: 1 and -1 to within the bound (never exactly promised)
            assert abs(float(got[n - 3, Q - 1]) - 1.0) <= bound[n - 3, Q - 1] and abs(float(got[n - 4, 0]) + 1.0) <= bound[n - 4, 0]
    print(f"H={H} Q={Q}: worst error / bound = {worst:.3f}")


def test_a_nan_stays_in_its_row_and_its_column():
    n, H, Q = 40, 33, 9
    e, q = _rows(n, H, Q).clone(), _queries(Q, H).clone()
    clean = _cos(e.to(DEV), q.to(DEV))
    e[17, 32], q[4, 0] = float("nan"), float("nan")                       # (column 32: the second value of lane 0)
    sim = _cos(e.to(DEV), q.to(DEV))
    want = torch.zeros(n, Q, dtype=torch.bool)
    want[17, :], want[:, 4] = True, True
    assert torch.equal(torch.isnan(sim).cpu(), want)
    keep = ~want
    assert np.array_equal(_bits(sim.cpu()[keep]), _bits(clean.cpu()[keep]))


def _padded(a, pad):
    """The same rows with ``pad`` NaN columns behind them: a row stride larger than the width."""
    n, H = a.shape
    store = torch.full((n, H + pad), float("nan"), dtype=torch.float32, device=DEV)
    store[:, :H] = a
    return store[:, :H]


@pytest.mark.parametrize("n,H,Q", [(2 * R + 1, 33, 9), (250, 64, 32), (R, 31, 1), (1, 1, 1)])
def test_strides_both_layouts_and_nothing_else_is_written(n, H, Q):
    e, q = _rows(n, H, Q).to(DEV), _queries(Q, H).to(DEV)
    rows = _cos(e, q)
    # input strides larger than H, NaN in the padding
    assert np.array_equal(_bits(_cos(_padded(e, 3), _padded(q, 5))), _bits(rows))
    by_query = _cos(e, q, query_major=True)
    assert by_query.shape == (Q, n) and np.array_equal(_bits(by_query.t()), _bits(rows))
    # into the middle of larger, sentinel-filled buffers, the leading n - 1 rows only: every other cell keeps the sentinel
    m = max(n - 1, 1)
    sentinel = np.float32(-777.25).view(np.int32)
    big_r = torch.full((n + 2, Q + 3), -777.25, device=DEV)
    got = _cos(e, q, n_rows=m, out=big_r[1:1 + m, 2:2 + Q])
    assert got.data_ptr() == big_r[1:, 2:].data_ptr()
    big_q = torch.full((Q + 2, n + 5), -777.25, device=DEV)
    _cos(e, q, n_rows=m, out=big_q[1:1 + Q, 3:3 + m], query_major=True)
    inside = torch.zeros_like(big_r, dtype=torch.bool)
    inside[1:1 + m, 2:2 + Q] = True
    assert (_bits(big_r[~inside]) == sentinel).all() and np.array_equal(_bits(big_r[1:1 + m, 2:2 + Q]), _bits(rows[:m]))
    inside = torch.zeros_like(big_q, dtype=torch.bool)
    inside[1:1 + Q, 3:3 + m] = True
    assert (_bits(big_q[~inside]) == sentinel).all() and np.array_equal(_bits(big_q[1:1 + Q, 3:3 + m].t()), _bits(rows[:m]))


@pytest.mark.parametrize("H", [33, 64, 7])
def test_an_elements_bits_depend_on_its_row_and_its_query_alone(H):
    n, Q = 1000, 32
    e, q = _rows(n, H, Q).to(DEV), _queries(Q, H).to(DEV)
    full = _cos(e, q)
    # Q and q's index: column q of the Q = 32 call is the Q = 1 call with that query alone; a reversed query order reverses columns
    for j in (0, 3, 8, 9, 31):
        assert np.array_equal(_bits(_cos(e, q[j:j + 1])[:, 0]), _bits(full[:, j])), j
    assert np.array_equal(_bits(_cos(e, q[:9])), _bits(full[:, :9]))
    assert np.array_equal(_bits(_cos(e, q.flip(0).contiguous())), _bits(full.flip(1)))
    # the row's place in block and grid: permuted rows give permuted output
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(H)).to(DEV)
    assert np.array_equal(_bits(_cos(e[perm].contiguous(), q)), _bits(full[perm]))
    # n_rows: 1000 and 17 agree on their common rows
    assert np.array_equal(_bits(_cos(e[:17].contiguous(), q)), _bits(full[:17]))
    assert np.array_equal(_bits(_cos(e, q, n_rows=17)), _bits(full[:17]))


def test_one_captured_launch_serves_new_contents_of_rows_and_queries():
    n, H, Q = 100, 33, 9
    e = torch.zeros(n, H, device=DEV)
    q = torch.zeros(Q, H, device=DEV)
    out = torch.full((n, Q), float("nan"), device=DEV)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side), torch.cuda.graph(graph, stream=side):
        _cos(e, q, out=out)
    torch.cuda.current_stream().wait_stream(side)
    assert bool(torch.isnan(out).all())                                   # a capture launches nothing
    for seed in (1, 2):
        g = torch.Generator().manual_seed(seed)
        e.copy_(torch.randn(n, H, generator=g))
        q.copy_(torch.randn(Q, H, generator=g) * 10.0 ** seed)            # (another norm: nothing of the queries was prepared)
        graph.replay()
        assert np.array_equal(_bits(out), _bits(_cos(e.clone(), q.clone()))), seed


def test_rejections_and_the_empty_call():
    L = _L()
    lib = L.load()
    n, H, Q = 16, 8, 3
    e, q = torch.zeros(n, H, device=DEV), torch.zeros(Q, H, device=DEV)
    sim = torch.full((n, 40), -777.25, device=DEV)
    stream = L.stream_ptr(torch.device(DEV))

    def call(emb=e.data_ptr(), es=H, n=n, H=H, qry=q.data_ptr(), qs=H, Q=Q, out=sim.data_ptr(), rs=40, cs=1):
        return lib.mkgnn_embed_cosine(emb, es, n, H, qry, qs, Q, out, rs, cs, stream)

    for change, word in ((dict(Q=0), b"queries"), (dict(Q=33), b"queries"), (dict(H=0), b"width"), (dict(H=65), b"width"),
                         (dict(n=-1), b"shape"), (dict(es=H - 1), b"shape"), (dict(qs=H - 1), b"shape"),
                         (dict(emb=None), b"null"), (dict(qry=None), b"null"), (dict(out=None), b"null"),
                         (dict(rs=2, cs=1), b"share"), (dict(rs=1, cs=n - 1), b"share"), (dict(rs=0, cs=1), b"share"),
                         (dict(rs=40, cs=-1), b"share")):
        assert call(**change) != 0 and word in lib.mkgnn_last_error(), change
    assert call(n=0) == 0                                                 # no rows: a no-op
    assert call(n=0, emb=None, out=None) == 0
    torch.cuda.synchronize()
    assert (_bits(sim) == np.float32(-777.25).view(np.int32)).all()      # nothing was launched by any of them
    assert call() == 0                                                    # (and the call they were variations of is taken)
    torch.cuda.synchronize()
    assert (_bits(sim[:, :Q]) == 0).all() and (_bits(sim[:, Q:]) == np.float32(-777.25).view(np.int32)).all()


@pytest.mark.parametrize("Q,H", [(33, 32), (9, 65)])
def test_torch_route_beyond_the_limits_meets_the_same_bound(Q, H):
    from molkgnn_amd.readout import embedding_cosine_supported
    from molkgnn_amd.screening import cosine_bound, cosine_reference
    assert not embedding_cosine_supported(Q, H) and embedding_cosine_supported(32, 64)
    n = 37
    e_c, q_c = _rows(n, H, Q), _queries(Q, H)
    sim = _cos(e_c.to(DEV), q_c.to(DEV))
    by_query = _cos(e_c.to(DEV), q_c.to(DEV), query_major=True)
    assert sim.shape == (n, Q) and np.array_equal(_bits(by_query.t()), _bits(sim))
    err = np.abs(sim.cpu().numpy().astype(np.float64) - cosine_reference(e_c, q_c))
    assert (err <= cosine_bound(e_c, q_c)).all(), float((err / cosine_bound(e_c, q_c)).max())


def test_python_wrapper_refuses_a_recorded_gradient_and_wrong_shapes():
    e, q = torch.zeros(4, 8, device=DEV), torch.zeros(3, 8, device=DEV)
    with pytest.raises(RuntimeError):
        _cos(e.clone().requires_grad_(), q)
    with pytest.raises(RuntimeError):
        _cos(e, q.clone().requires_grad_())
    with torch.no_grad():
        assert _cos(e.clone().requires_grad_(), q).shape == (4, 3)
    assert _cos(e, q, n_rows=0).shape == (0, 3)
    for bad in (dict(n_rows=5), dict(out=torch.zeros(3, 4, device=DEV)), dict(out=torch.zeros(4, 3))):
        with pytest.raises(ValueError):
            _cos(e, q, **bad)
    with pytest.raises(ValueError):
        _cos(torch.zeros(4, 7, device=DEV), q)
    with pytest.raises(ValueError):
        _cos(e, q.cpu())
