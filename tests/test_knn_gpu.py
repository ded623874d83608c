"""``mkgnn_embed_knn_update`` on the GPU: fused cosine and top-k for any number of queries.  The lists against the host definition
(``mkgnn_embed_cosine``'s similarities in groups of at most 32 queries, ``topk_update_tasks_reference``'s order) by bits at every
shape; running lists and the full tie-break; ``n_valid`` as a device scalar; capture; NaN; independence of ``Q``, the strides and
the split of the candidates; the routes that exist (``rank_embeddings``, ``nearest``); the float64 criterion; what the C ABI
rejects; the torch route beyond ``H = 64``."""
import functools

import numpy as np
import pytest
import torch

from tests import _knn_cases as KC
from tests._resident_library import build_library

pytestmark = pytest.mark.gpu
DEV = KC.DEV


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _update(emb, queries, lists, **kw):
    from molkgnn_amd.readout import embedding_knn_update
    embedding_knn_update(emb if torch.is_tensor(emb) else _dev(emb), queries if torch.is_tensor(queries) else _dev(queries), *lists, **kw)
    return KC.host_of(lists)


@functools.lru_cache(maxsize=None)
def _cases():
    """Every shape, run ONCE from empty lists: the inputs, the kernel's lists and the host definition's."""
    out = []
    for j, (n, Q, K, H) in enumerate(KC.shapes()):
        emb, queries = KC.inputs(n, H, Q, 100 + j)
        got = _update(emb, queries, KC.device_lists(Q, K))
        want = KC.host_update(KC.empty_lists(Q, K), emb, queries)
        out.append(((n, Q, K, H), emb, queries, got, want))
    return out


@pytest.mark.parametrize("j", range(14))
def test_lists_from_empty_are_the_host_definition_by_bits(j):
    assert len(KC.shapes()) == 14
    (n, Q, K, H), emb, queries, got, want = _cases()[j]
    assert got[0].shape == got[1].shape == got[2].shape == (Q, K)
    assert KC.same_lists(got, want), (n, Q, K, H)
    occupied = min(n, K)
    assert (got[1][:, :occupied] == 0).all() and (got[1][:, occupied:] == -1).all() and (got[2][:, occupied:] == -1).all()
    assert (KC.bits(got[0][:, occupied:]) == KC.bits([-np.inf])[0]).all()              # fewer candidates than K: empty slots at the end


def test_running_lists_and_the_full_tie_break():
    n, Q, K, H = 300, 5, 16, 33
    emb, queries = KC.inputs(n, H, Q, 7)
    ids = (1000 + np.random.default_rng(1).permutation(n)).astype(np.int32)
    lists = KC.device_lists(Q, K)
    got = _update(emb, queries, lists, ids=_dev(ids), shard_tag=5)
    want = KC.host_update(KC.empty_lists(Q, K), emb, queries, ids, tag=5)
    assert KC.same_lists(got, want)
    # a second call with another tag and lower ids: other candidates and, among them, copies of the first call's rows
    emb2, _ = KC.inputs(200, H, Q, 8)
    emb2[50:60] = emb[20:30]
    ids2 = np.arange(200, dtype=np.int32)
    got = _update(emb2, queries, lists, ids=_dev(ids2), shard_tag=3)
    want = KC.host_update(want, emb2, queries, ids2, tag=3)
    assert KC.same_lists(got, want)
    assert (got[1] == 3).any() and (got[1] == 5).any()
    # a candidate whose similarity EQUALS the last entry's bit for bit -- the same embedding -- decides by (shard, id) alone
    last_shard, last_mol = int(got[1][0, K - 1]), int(got[2][0, K - 1])
    row = emb[np.flatnonzero(ids == last_mol)[0]] if last_shard == 5 else emb2[last_mol]
    one = np.ascontiguousarray(row[None, :])
    for shard, mol, enters in ((last_shard, last_mol + 1, False), (last_shard + 1, 0, False), (last_shard, last_mol - 1, True),
                               (last_shard - 1, 1 << 30, True)):
        before = KC.host_of(lists)
        got = _update(one, queries, lists, ids=_dev(np.array([mol], dtype=np.int32)), shard_tag=shard)
        want = KC.host_update(before, one, queries, [mol], tag=shard)
        assert KC.same_lists(got, want), (shard, mol)
        changed = not KC.same_lists(tuple(a[:1] for a in got), tuple(a[:1] for a in before))
        assert changed == enters, (shard, mol)
        if enters:                                                 # (with the similarity the last entry had, and that entry is gone)
            at = list(zip(got[1][0].tolist(), got[2][0].tolist())).index((shard, mol))
            assert KC.bits(got[0][0, at]) == KC.bits(before[0][0, K - 1])
    # an entry equal to the last one in similarity, shard and id does not displace its equal: the one that was there stays
    before = KC.host_of(lists)
    got = _update(one, queries[:1], tuple(t[:1] for t in lists), ids=_dev(np.array([int(before[2][0, K - 1])], dtype=np.int32)),
                  shard_tag=int(before[1][0, K - 1]))
    assert KC.same_lists(got, tuple(a[:1] for a in before))


@pytest.mark.parametrize("n_valid", [0, 1, 199, -4, 1000])
def test_n_valid_is_read_on_the_device_and_rows_behind_it_never_enter(n_valid):
    n, Q, K, H = 200, 3, 8, 32
    emb, queries = KC.inputs(n, H, Q, 21)
    poisoned = emb.copy()
    live = min(max(n_valid, 0), n)
    poisoned[live:] = np.float32(1e30)
    poisoned[live::2] = np.nan
    nv = torch.tensor([n_valid], dtype=torch.int32, device=DEV)
    got = _update(poisoned, queries, KC.device_lists(Q, K), n_valid=nv)                   # ids = NULL: the row indices
    want = KC.host_update(KC.empty_lists(Q, K), emb, queries, None, n_valid)
    assert KC.same_lists(got, want)
    assert not np.isnan(got[0]).any() and (got[2] < live).all()
    assert ((got[1] == 0).sum(axis=1) == min(live, K)).all()


def test_one_captured_call_follows_every_input():
    from molkgnn_amd import _lib
    from molkgnn_amd.readout import embedding_knn_update
    n, Q, K, H = 300, 6, 9, 64
    assert _lib.knn_split(n, Q)[1] > 1                             # (the merge launch is captured as well)
    emb, queries = (_dev(a) for a in KC.inputs(n, H, Q, 31))
    ids = torch.arange(n, dtype=torch.int32, device=DEV)
    nv = torch.tensor([n], dtype=torch.int32, device=DEV)
    tag = torch.zeros(1, dtype=torch.int32, device=DEV)
    lists = KC.device_lists(Q, K)
    ws = torch.empty(int(_lib.load().mkgnn_embed_knn_workspace_bytes(n, Q, K)), dtype=torch.uint8, device=DEV)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        embedding_knn_update(emb, queries, *lists, ids=ids, n_valid=nv, shard_tag=tag, workspace=ws)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            embedding_knn_update(emb, queries, *lists, ids=ids, n_valid=nv, shard_tag=tag, workspace=ws)
    torch.cuda.current_stream(DEV).wait_stream(side)
    for t, a in zip(lists, KC.empty_lists(Q, K)):                  # (the eager call filled them)
        t.copy_(_dev(a))
    want = KC.empty_lists(Q, K)
    gen = torch.Generator(device=DEV).manual_seed(5)
    for step, (count, shard, scale) in enumerate(((n, 4, 1.0), (123, 2, 1e-3), (0, 9, 1.0), (n - 1, 0, 1e4))):
        emb.copy_(torch.randn(emb.shape, generator=gen, device=DEV))
        queries.copy_(torch.randn(queries.shape, generator=gen, device=DEV) * scale)
        ids.copy_(torch.randperm(n, generator=gen, device=DEV).to(torch.int32) + 10 * step)
        nv.fill_(count)
        tag.fill_(shard)
        if step == 2:                                              # (new queries: the running lists start over)
            for t, a in zip(lists, KC.empty_lists(Q, K)):
                t.copy_(_dev(a))
            want = KC.empty_lists(Q, K)
        graph.replay()
        want = KC.host_update(want, emb, queries, ids, count, shard)
        assert KC.same_lists(KC.host_of(lists), want), step


def test_nan_rows_rank_last_and_a_nan_query_keeps_to_its_own_list():
    n, Q, K, H = 150, 4, 64, 33
    emb, queries = KC.inputs(n, H, Q, 41)
    queries[3] = 0.0                                               # a zero query
    base = _update(emb, queries, KC.device_lists(Q, K))
    assert KC.same_lists(base, KC.host_update(KC.empty_lists(Q, K), emb, queries))
    assert np.array_equal(base[2][3], np.arange(K)) and (KC.bits(base[0][3]) == 0).all()  # the K lowest ids, +0.0 by bits
    # NaN rows among 40 candidates for 64 slots: every list holds them all, behind every non-NaN entry
    few = emb[:40].copy()
    few[[7, 20, 39], 5] = np.nan
    got = _update(few, queries, KC.device_lists(Q, K))
    assert KC.same_lists(got, KC.host_update(KC.empty_lists(Q, K), few, queries))
    for q in range(Q):
        assert not np.isnan(got[0][q, :37]).any() and np.isnan(got[0][q, 37:40]).all() and got[2][q, 37:40].tolist() == [7, 20, 39]
        assert (got[1][q, 40:] == -1).all()
    # a NaN row never displaces a non-NaN entry of a full list
    many = emb.copy()
    many[11, 0] = np.nan
    got = _update(many, queries, KC.device_lists(Q, K))
    assert KC.same_lists(got, KC.host_update(KC.empty_lists(Q, K), many, queries)) and not np.isnan(got[0]).any()
    # a NaN query: its list is NaN entries in (shard, id) order; no other list changes
    q2 = queries.copy()
    q2[1, 2] = np.nan
    got = _update(emb, q2, KC.device_lists(Q, K))
    assert np.isnan(got[0][1]).all() and np.array_equal(got[2][1], np.arange(K)) and (got[1][1] == 0).all()
    keep = [0, 2, 3]
    assert KC.same_lists(tuple(a[keep] for a in got), tuple(a[keep] for a in base))


def test_a_list_does_not_depend_on_q_strides_or_the_split():
    from molkgnn_amd import _lib
    n, H, K = 1000, 31, 32
    emb, queries = KC.inputs(n, H, 70, 51)
    alone = _update(emb, queries[40:41], KC.device_lists(1, K))
    assert KC.same_lists(alone, KC.host_update(KC.empty_lists(1, K), emb, queries[40:41]))
    among = _update(emb, queries, KC.device_lists(70, K))
    assert KC.same_lists(tuple(a[40:41] for a in among), alone)
    # so many queries that the candidates are not split at all: another launch shape, the same list
    Q = 4 * _lib.KNN_TARGET_BLOCKS
    assert _lib.knn_split(n, 1)[1] > 1 and _lib.knn_split(n, Q)[1] == 1
    crowd = np.ascontiguousarray(np.tile(queries, (-(-Q // 70), 1))[:Q])
    assert KC.same_lists(tuple(a[40:41] for a in _update(emb, crowd, KC.device_lists(Q, K))), alone)
    # padded strides, NaN in the padding
    ep = torch.full((n, H + 3), float("nan"), device=DEV)
    qp = torch.full((70, H + 5), float("nan"), device=DEV)
    ep[:, :H], qp[:, :H] = _dev(emb), _dev(queries)
    assert KC.same_lists(_update(ep[:, :H], qp[:, :H], KC.device_lists(70, K)), among)
    # the candidates in two calls cut at an odd row, and in permuted row order with their ids carried
    lists = KC.device_lists(1, K)
    _update(emb[:333], queries[40:41], lists, ids=_dev(np.arange(333, dtype=np.int32)))
    two = _update(emb[333:], queries[40:41], lists, ids=_dev(np.arange(333, n, dtype=np.int32)))
    assert KC.same_lists(two, alone)
    perm = np.random.default_rng(2).permutation(n)
    assert KC.same_lists(_update(emb[perm], queries[40:41], KC.device_lists(1, K), ids=_dev(perm.astype(np.int32))), alone)


def test_nearest_embeddings_is_rank_embeddings_by_bits():
    from molkgnn_amd.screening import NearestLists, TopKTasks, nearest_embeddings, rank_embeddings
    n, H, Q, K = 5000, 32, 32, 64
    emb, queries = (_dev(a) for a in KC.inputs(n, H, Q, 61))
    ids = _dev((np.random.default_rng(3).permutation(n) + 7).astype(np.int32))
    for use_ids in (None, ids):
        old = TopKTasks(K, Q, DEV)
        rank_embeddings(emb, queries, old, ids=use_ids, shard_tag=2)
        new = NearestLists(K, Q, DEV)
        nearest_embeddings(emb, queries, new, ids=use_ids, shard_tag=2)
        assert KC.same_lists(KC.host_of(new.result()[:3]), KC.host_of(old.result()[:3]))
        assert new.result()[3].tolist() == [K] * Q
    # the lists run on over a second matrix; reset() empties them
    nearest_embeddings(emb[:100] * 2, queries, new, shard_tag=1)
    rank_embeddings(emb[:100] * 2, queries, old, shard_tag=1)
    assert KC.same_lists(KC.host_of(new.result()[:3]), KC.host_of(old.result()[:3]))
    new.reset()
    assert new.result()[3].tolist() == [0] * Q
    for bad in (TopKTasks(K, Q, DEV), NearestLists(K, Q + 1, DEV), None):
        with pytest.raises(ValueError, match="NearestLists"):
            nearest_embeddings(emb, queries, bad)
    with pytest.raises(ValueError, match="ids"):
        nearest_embeddings(emb, queries, new, ids=ids[:-1])
    with pytest.raises(ValueError):
        new.update(emb, queries[:5])


@pytest.fixture(scope="module")
def library(tmp_path_factory):
    """The two-shard library of test_nearest_gpu.py (70 and 33 synthetic molecules, batch 32) and its nine-task model, left in
    training mode."""
    model, residents, _ = build_library(tmp_path_factory.mktemp("library_knn"), DEV, counts=(70, 33), shard_seed=40,
                                        labels=lambda n: (torch.arange(n) % 3 == 0).float(), model_seed=9, num_layers=3, task_dim=9)
    model.train()
    return model, residents


def test_nearest_many_is_nearest_and_goes_beyond_32_queries(library):
    from molkgnn_amd.screening import NearestLists, embed_resident, nearest, nearest_many, nearest_many_resident
    model, residents = library
    embeds = [embed_resident(model, r, 32) for r in residents]
    G = embeds[0].shape[1]
    five = torch.stack([embeds[0][0], embeds[0][7], embeds[0][69], embeds[1][32], torch.zeros(G, device=DEV)]).contiguous()
    old = nearest(model, five, residents, 16, 32)
    new = nearest_many(model, five, (r for r in residents), 16, 32)                      # (a generator: shards one at a time)
    assert model.training                                          # handed back in the mode it came in
    assert sorted(new) == ["n_occupied", "n_searched", "query_emb", "top_mol", "top_shard", "top_sim"]
    assert new["top_sim"].shape == new["top_shard"].shape == new["top_mol"].shape == (5, 16)
    assert KC.same_lists(*(KC.host_of((r["top_sim"], r["top_shard"], r["top_mol"])) for r in (new, old)))
    assert new["n_occupied"].tolist() == old["n_occupied"].tolist() == [16] * 5 and new["n_searched"] == 103
    assert new["query_emb"] is five
    # 40 queries: the host definition built from embed_resident's embeddings
    forty = embeds[0][:40].contiguous()
    r = nearest_many(model, forty, residents, 64, 32)
    want = KC.empty_lists(40, 64)
    for tag, e in enumerate(embeds):
        want = KC.host_update(want, e, forty, tag=tag)
    assert KC.same_lists(KC.host_of((r["top_sim"], r["top_shard"], r["top_mol"])), want)
    assert r["n_occupied"].tolist() == [64] * 40 and model.training
    # the queries as a shard of more than 32 molecules: embedded first
    by_shard = nearest_many(model, residents[1], residents, 8, 32)
    assert np.array_equal(KC.bits(by_shard["query_emb"]), KC.bits(embeds[1])) and by_shard["top_sim"].shape == (33, 8)
    want = KC.empty_lists(33, 8)
    for tag, e in enumerate(embeds):
        want = KC.host_update(want, e, embeds[1], tag=tag)
    assert KC.same_lists(KC.host_of((by_shard["top_sim"], by_shard["top_shard"], by_shard["top_mol"])), want)
    # one shard pass returns the shard's embeddings; the lists are checked before a launch
    lists = NearestLists(8, 40, DEV)
    model.eval()
    emb = nearest_many_resident(model, residents[1], forty, 32, lists=lists, shard_tag=1)
    assert not model.training and np.array_equal(KC.bits(emb), KC.bits(embeds[1]))
    assert KC.same_lists(KC.host_of(lists.result()[:3]), KC.host_update(KC.empty_lists(40, 8), embeds[1], forty, tag=1))
    model.train()
    for bad in (NearestLists(8, 39, DEV), None):
        with pytest.raises(ValueError, match="NearestLists"):
            nearest_many_resident(model, residents[1], forty, 32, lists=bad)
    with pytest.raises(ValueError, match="at least one shard"):
        nearest_many(model, forty, [], 8, 32)


def _float64_criterion(emb, queries, got, n_valid=None):
    """Tie-aware, no list left out: every listed similarity lies within ``cosine_bound`` of ``cosine_reference`` for its pair, and no
    unlisted candidate's float64 similarity exceeds the list's last float64 similarity by more than the two bounds involved --
    ``sim32[unlisted] <= sim32[last]`` by the order, and each float32 value lies within its own bound of its float64 one."""
    from molkgnn_amd.screening import cosine_bound, cosine_reference
    sim64, bound = cosine_reference(emb, queries).T, cosine_bound(emb, queries).T         # [Q, n]
    n = emb.shape[0] if n_valid is None else n_valid
    for q in range(queries.shape[0]):
        mol = got[2][q]
        occupied = mol >= 0
        assert occupied.sum() == min(n, len(mol))
        listed = mol[occupied]
        err = np.abs(got[0][q][occupied].astype(np.float64) - sim64[q, listed])
        assert (err <= bound[q, listed]).all(), (q, float((err / bound[q, listed]).max()))
        unlisted = np.setdiff1d(np.arange(n), listed)
        if len(unlisted):
            last = listed[-1]
            assert (sim64[q, unlisted] <= sim64[q, last] + bound[q, last] + bound[q, unlisted]).all(), q


def test_float64_criterion_is_tie_aware_and_leaves_no_list_out():
    for (n, Q, K, H), emb, queries, got, _ in _cases():
        _float64_criterion(emb, queries, got)


def test_c_abi_rejects_before_any_launch_and_writes_the_lists_alone():
    from molkgnn_amd import _lib
    lib = _lib.load()
    n, H, Q, K = 300, 20, 5, 7
    assert _lib.knn_split(n, Q)[1] > 1
    emb, queries = (_dev(a) for a in KC.inputs(n, H, Q, 71))
    ids = torch.arange(n, dtype=torch.int32, device=DEV)
    nv = torch.tensor([n], dtype=torch.int32, device=DEV)
    tag = torch.tensor([3], dtype=torch.int32, device=DEV)
    pad = 11
    fbuf = torch.full((Q * K + 2 * pad,), -7.5, device=DEV)
    hbuf = torch.full((Q * K + 2 * pad,), -77, dtype=torch.int32, device=DEV)
    mbuf = torch.full((Q * K + 2 * pad,), -78, dtype=torch.int32, device=DEV)
    lists = tuple(b[pad:pad + Q * K].view(Q, K) for b in (fbuf, hbuf, mbuf))
    for t, a in zip(lists, KC.empty_lists(Q, K)):
        t.copy_(_dev(a))
    need = lib.mkgnn_embed_knn_workspace_bytes(n, Q, K)
    assert need > 0
    ws = torch.full((need,), 0xFF, dtype=torch.uint8, device=DEV)                         # (poisoned: it needs no initialisation)
    st = _lib.stream_ptr(torch.device(DEV))

    def call(e=emb.data_ptr(), es=H, rows=n, width=H, i=ids.data_ptr(), v=nv.data_ptr(), t=tag.data_ptr(), q=queries.data_ptr(), qs=H,
             count=Q, k=K, s=lists[0].data_ptr(), h=lists[1].data_ptr(), m=lists[2].data_ptr(), work=ws.data_ptr(), work_bytes=need):
        return lib.mkgnn_embed_knn_update(e, es, rows, width, i, v, t, q, qs, count, k, s, h, m, work, work_bytes, st)

    refused = (("width", dict(width=0)), ("width", dict(width=65, es=65, qs=65)), ("queries outside", dict(count=0)),
               ("queries outside", dict(count=_lib.KNN_MAX_QUERIES + 1)), ("K = ", dict(k=0)), ("K = ", dict(k=65)),
               ("rows outside", dict(rows=-1)), ("rows outside", dict(rows=_lib.KNN_MAX_ROWS + 1)), ("stride", dict(es=H - 1)),
               ("stride", dict(qs=H - 1)), ("null", dict(e=None)), ("null", dict(q=None)), ("null", dict(s=None)), ("null", dict(h=None)),
               ("null", dict(m=None)), ("null", dict(work=None)), ("workspace", dict(work_bytes=need - 1)),
               ("aligned", dict(work=ws.data_ptr() + 1, work_bytes=need)), ("alias", dict(s=emb.data_ptr())),
               ("alias", dict(h=queries.data_ptr() + 4)), ("alias", dict(m=ids.data_ptr())), ("alias", dict(h=nv.data_ptr())),
               ("alias", dict(m=tag.data_ptr())), ("alias", dict(h=lists[0].data_ptr() + 4)), ("alias", dict(m=lists[1].data_ptr())),
               ("alias", dict(s=ws.data_ptr())))
    for word, kw in refused:
        assert call(**kw) != 0, kw
        assert word in lib.mkgnn_last_error().decode(), (kw, lib.mkgnn_last_error())
    assert call(rows=0, e=None, q=None, s=None, h=None, m=None, work=None, work_bytes=0) == 0          # a no-op
    torch.cuda.synchronize()
    assert KC.same_lists(KC.host_of(lists), KC.empty_lists(Q, K))                         # nothing was launched
    assert bool((ws == 0xFF).all())
    assert call() == 0
    want = KC.host_update(KC.empty_lists(Q, K), emb, queries, ids, n, 3)
    assert KC.same_lists(KC.host_of(lists), want)
    for buf, fill in ((fbuf, -7.5), (hbuf, -77), (mbuf, -78)):     # the lists, bracketed by sentinels, are the only memory written
        assert bool((buf[:pad] == fill).all()) and bool((buf[pad + Q * K:] == fill).all())
    # ids, n_valid and shard_tag as NULL: the row index, every row, tag 0; a clean workspace gives the same lists
    for t, a in zip(lists, KC.empty_lists(Q, K)):
        t.copy_(_dev(a))
    ws.zero_()
    assert call(i=None, v=None, t=None) == 0
    assert KC.same_lists(KC.host_of(lists), KC.host_update(KC.empty_lists(Q, K), emb, queries))


def test_torch_route_beyond_the_kernels_width_meets_the_float64_criterion():
    from molkgnn_amd import readout
    n, Q, K, H = 150, 5, 8, 65
    assert not readout.embedding_knn_supported(H, K) and readout.embedding_knn_supported(64, K)
    emb, queries = KC.inputs(n, H, Q, 81)
    chunk = readout.KNN_TORCH_CHUNK
    readout.KNN_TORCH_CHUNK = 64                                   # three chunks, so the running lists run on across chunks
    try:
        got = _update(emb, queries, KC.device_lists(Q, K))
        _float64_criterion(emb, queries, got)
        nv = torch.tensor([70], dtype=torch.int32, device=DEV)
        poisoned = emb.copy()
        poisoned[70:] = np.nan
        got = _update(poisoned, queries, KC.device_lists(Q, K), n_valid=nv, shard_tag=4)
        assert (got[1] == 4).all() and (got[2] < 70).all()
        _float64_criterion(emb[:70], queries, got)
        few = _update(emb[:3], queries, KC.device_lists(Q, K), n_valid=2)
        assert (few[2][:, :2] >= 0).all() and (few[2][:, 2:] == -1).all() and (few[1][:, 2:] == -1).all()
        assert (KC.bits(few[0][:, 2:]) == KC.bits([-np.inf])[0]).all()
    finally:
        readout.KNN_TORCH_CHUNK = chunk
    with pytest.raises(ValueError, match="rank_embeddings"):
        _update(emb, queries, KC.device_lists(Q, 65))
    with torch.enable_grad():
        with pytest.raises(RuntimeError):
            readout.embedding_knn_update(_dev(emb).requires_grad_(), _dev(queries), *KC.device_lists(Q, K))
