"""Monte Carlo dropout on the forward-only tail (csrc/kgnn_tail_mc.hip ``tail_mc_kernel``, ``mkgnn_tail_score_mc``,
``readout.tail_score_mc``, ``GNNModel.predict_mc``, ``screening.score_resident_mc`` / ``screen_acquisition``).  ``pytest -m gpu``.

The kernel is pinned to the training tail: sample ``s`` is BIT FOR BIT the ``pred`` that ``mkgnn_tail_fused_readout_dropout`` writes
for generator state ``{seed, offset + s}``; ``pred`` / ``emb`` are ``mkgnn_tail_score``'s bits; the statistics are
``readout.mc_statistics_reference``'s bits.  Like the other tail tests it is also held to the float64 formula of the reference, with
the masks of the host mirror (``tests._philox``), within 2e-5 of the result's scale.  Both entry points are called through the C ABI
with buffers of the test's own.

(A group of the work distribution holds at most 8 molecules -- ``tail_group_size`` -- so a chunk never holds the 12 its window has
room for, and only batches beyond 768 molecules put more than one molecule into a chunk: the 4 096-molecule case.)
"""
import ctypes

import numpy as np
import pytest
import torch

from tests import _philox as PH
from tests import _topologies as T
from tests.test_score_tail import LS, PATTERN, _Call, _bits, _close, _modules, _patterned, _reference_f64, _targets
from tests.test_tail import _block_rows

pytestmark = pytest.mark.gpu

SEED, OFFSET = 1234, 7
PROBS = [(0.25, 0.2), (0.25, 0.0), (0.0, 0.5)]


def _dev():
    assert torch.cuda.is_available(), "pytest -m gpu needs the MI355X"
    return torch.device("cuda:0")


class _Case:
    """A batch, its plan and segments, random block rows and the modules: what every call of a test shares."""

    def __init__(self, b, n_rows, seed, dev, mods=None, seg=None):
        from molkgnn_amd import readout as R
        from molkgnn_amd.plan import plan_from_data
        self.b, self.dev, self.n_rows = b, dev, n_rows
        self.plan = plan_from_data(b)
        self.seg = R.molecule_segments(b.batch, b.num_graphs) if seg is None else seg
        self.sim0, self.inblock = _block_rows(b, self.plan, LS, dev, seed)
        self.mods = _modules(dev, seed) if mods is None else mods
        self.y, self.kind = _targets("docking_score", n_rows, dev, seed)

    def call(self):
        return _Call(self.sim0, self.plan, self.seg, self.mods, self.n_rows, self.y, self.kind, self.dev)


def _synthetic(n_mols, dev, mods=None):
    from molkgnn_amd.synthetic import make_batch
    b = make_batch(n_mols, seed=900 + n_mols, target="docking_score").to(dev)
    b.num_graphs = n_mols
    return _Case(b, n_mols, 900 + n_mols, dev, mods)


class _Mc:
    """One ``mkgnn_tail_score_mc`` call on a ``_Call``'s argument block: every output starts out as a pattern; ``rc`` is the return
    code, ``guard`` the bytes behind the stated workspace size."""

    def __init__(self, c, p_head, p_ro, S, alpha=1.0, beta=0.0, samples=True, pred=True, pair=(SEED, OFFSET), stride=None,
                 short_ws=False, null_pair=False, check=True):
        from molkgnn_amd import _lib
        lib = _lib.load()
        dev, n = c.dev, c.pred.numel()
        rows = max(S, 1)
        self.stride = rows if stride is None else stride
        self.samples = _patterned((n, max(self.stride, rows)), dev).view(torch.float32)
        self.mean, self.std, self.acq = (_patterned((n,), dev).view(torch.float32) for _ in range(3))
        self.pair = torch.tensor(list(pair), dtype=torch.int64, device=dev)
        self.c = c
        c.a.dropout_p = float(p_head)
        if not pred:
            c.a.pred, c.a.emb = None, None
        out = _lib.TailMcOut()
        out.samples, out.samples_stride = (self.samples.data_ptr() if samples else None), self.stride
        out.mean, out.std, out.acq = self.mean.data_ptr(), self.std.data_ptr(), self.acq.data_ptr()
        out.alpha, out.beta = alpha, beta
        need = int(lib.mkgnn_tail_score_mc_workspace_bytes(*c.dims))
        assert 0 < need <= int(lib.mkgnn_tail_workspace_bytes(*c.dims))
        ws = torch.full((need + 4096,), 0x5A, dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            self.rc = lib.mkgnn_tail_score_mc(ctypes.byref(c.a), float(p_ro), S, None if null_pair else self.pair.data_ptr(),
                                              ctypes.byref(out), ws.data_ptr(), need - 256 if short_ws else need, _lib.stream_ptr(dev))
        torch.cuda.synchronize()
        self.guard, self.ws = ws[need:], ws
        if check:
            _lib.check(self.rc, "mkgnn_tail_score_mc")
            assert bool((self.guard == 0x5A).all()), "bytes behind mkgnn_tail_score_mc_workspace_bytes were written"
            assert self.pair.tolist() == list(pair), "the generator pair is read, never advanced"
            c.untouched()

    def all_patterned(self):
        return all(bool((_bits(t) == PATTERN).all()) for t in (self.samples, self.mean, self.std, self.acq, self.c.pred, self.c.emb))


def _training_pred(case, p_head, p_ro, offset):
    """``pred`` of ``mkgnn_tail_fused_readout_dropout`` for the generator state ``{SEED, offset}``."""
    from molkgnn_amd import _lib
    lib = _lib.load()
    c = case.call()
    c.a.dropout_p = float(p_head)
    c.rng.copy_(torch.tensor([SEED, offset], dtype=torch.int64))
    ws = torch.empty(int(lib.mkgnn_tail_workspace_bytes(*c.dims)), dtype=torch.uint8, device=case.dev)
    with torch.cuda.device(case.dev):
        _lib.check(lib.mkgnn_tail_fused_readout_dropout(ctypes.byref(c.a), float(p_ro), ws.data_ptr(), ws.numel(),
                                                        _lib.stream_ptr(case.dev)), "mkgnn_tail_fused_readout_dropout")
    torch.cuda.synchronize()
    if p_head > 0 or p_ro > 0:
        assert c.rng_used.tolist() == [SEED, offset] and c.rng.tolist() == [SEED, offset + 1]
    return c.pred


def _samples_f64(case, p_head, p_ro, S, n_mols=None):
    """``_reference_f64``'s formula with the host mirror's masks: the readout's behind the swish, the head's on the embedding --
    ``[n_mols, S]`` in float64."""
    b, dev = case.b, case.dev
    lin1, lin2, ffn = case.mods
    n_mols = case.seg.size if n_mols is None else n_mols
    H, G = lin1.weight.shape[0], lin2.weight.shape[0]
    dense = torch.where(case.inblock, case.sim0, torch.zeros((), device=dev)).double()
    src, dst = b.edge_index[0], b.edge_index[1]
    h = torch.zeros_like(dense).index_add_(0, dst, dense[src])
    z = h @ lin1.weight.double().t() + lin1.bias.double()
    z = (z * torch.sigmoid(z)).detach()
    N = z.shape[0]
    cols = []
    for s in range(S):
        zs = z
        if p_ro > 0:
            zs = z * torch.from_numpy(PH.readout_mask(SEED, OFFSET + s, N, H, p_ro)).to(dev).double()
        e = zs @ lin2.weight.double().t() + lin2.bias.double()
        emb = torch.zeros(n_mols, G, dtype=torch.float64, device=dev).index_add_(0, b.batch, e)
        if p_head > 0:
            emb = emb * torch.from_numpy(PH.head_mask(SEED, OFFSET + s, n_mols, G, p_head)).to(dev).double()
        pred = emb @ ffn.weight.double().t()
        if ffn.bias is not None:
            pred = pred + ffn.bias.double()
        cols.append(pred.view(-1).detach())
    return torch.stack(cols, dim=1)


def _close_all(got, want, rel=2e-5):
    """The project's tail criterion: max |got - want| <= 2e-5 * max(max |want|, 1e-6)."""
    err, scale = float((got.double() - want.double()).abs().max()), max(float(want.abs().max()), 1e-6)
    print(f"max error {err:.3e} at scale {scale:.3e} (bound {rel * scale:.3e})")
    assert err <= rel * scale, (err, scale)


# ------------------------------------------------------------------------- 1, 4: the samples are the training tail's --
@pytest.mark.parametrize("p_head,p_ro", PROBS)
@pytest.mark.parametrize("n_mols", [1, 2, 300])
def test_samples_are_the_training_tail_bit_for_bit(n_mols, p_head, p_ro):
    dev = _dev()
    case = _synthetic(n_mols, dev)
    score = case.call()
    score.score()
    want = {}
    for S in (1, 5, 64):
        mc = _Mc(case.call(), p_head, p_ro, S)
        for s in sorted({0, 1, S - 1} & set(range(S))):
            if s not in want:
                want[s] = _training_pred(case, p_head, p_ro, OFFSET + s)
            assert torch.equal(_bits(mc.samples[:, s]), _bits(want[s])), (S, s, float((mc.samples[:, s] - want[s]).abs().max()))
        assert torch.equal(_bits(mc.c.pred), _bits(score.pred)) and torch.equal(_bits(mc.c.emb), _bits(score.emb))
        again = _Mc(case.call(), p_head, p_ro, S)
        assert torch.equal(_bits(again.samples), _bits(mc.samples))
        for name in ("mean", "std", "acq"):
            assert torch.equal(_bits(getattr(again, name)), _bits(getattr(mc, name))), name


def test_samples_of_4096_molecules_where_a_workgroup_walks_several_groups():
    dev = _dev()
    case = _synthetic(4096, dev)
    score = case.call()
    score.score()
    p_head, p_ro, S = 0.25, 0.2, 3
    mc = _Mc(case.call(), p_head, p_ro, S)
    for s in range(S):
        assert torch.equal(_bits(mc.samples[:, s]), _bits(_training_pred(case, p_head, p_ro, OFFSET + s))), s
    assert torch.equal(_bits(mc.c.pred), _bits(score.pred)) and torch.equal(_bits(mc.c.emb), _bits(score.emb))
    _close_all(mc.samples, _samples_f64(case, p_head, p_ro, S))
    head_only = _Mc(case.call(), p_head, 0.0, S)
    for s in range(S):
        assert torch.equal(_bits(head_only.samples[:, s]), _bits(_training_pred(case, p_head, 0.0, OFFSET + s))), s


def test_both_probabilities_zero_give_the_score_tail_in_every_column():
    dev = _dev()
    case = _synthetic(300, dev)
    score = case.call()
    score.score()
    mc = _Mc(case.call(), 0.0, 0.0, 5, beta=2.0)
    for s in range(5):
        assert torch.equal(_bits(mc.samples[:, s]), _bits(score.pred)), s
    assert torch.equal(_bits(mc.c.pred), _bits(score.pred)) and torch.equal(_bits(mc.c.emb), _bits(score.emb))


# ----------------------------------------------------------------------------------- 2: float64 with the host's masks --
@pytest.mark.parametrize("p_head,p_ro", PROBS)
@pytest.mark.parametrize("H,G", [(32, 32), (30, 7)])
def test_samples_against_float64_with_the_masks_of_the_host_mirror(H, G, p_head, p_ro):
    from molkgnn_amd import readout as R
    dev = _dev()
    assert R.tail_supported(110, H, G, LS)
    case = _synthetic(300, dev, mods=_modules(dev, 5, True, 110, H, G))
    S = 5
    mc = _Mc(case.call(), p_head, p_ro, S)
    _close_all(mc.samples, _samples_f64(case, p_head, p_ro, S))
    for s in (0, S - 1):                                   # (the unaligned keep path and the j >= G lanes, against the training tail too)
        assert torch.equal(_bits(mc.samples[:, s]), _bits(_training_pred(case, p_head, p_ro, OFFSET + s))), s
    want_pred, want_emb = _reference_f64(case.b, case.inblock, case.sim0, case.mods, 300, dev)
    _close(mc.c.pred, want_pred)
    _close(mc.c.emb, want_emb)


# ------------------------------------------------------------------------------------------------------ 3: statistics --
@pytest.mark.parametrize("S,alpha,beta", [(64, 1.0, 0.0), (64, 1.0, 1.5), (7, -1.0, 2.0), (1, 1.0, 1.5)])
def test_statistics_are_the_reference_bit_for_bit(S, alpha, beta):
    from molkgnn_amd.readout import mc_statistics_reference
    dev = _dev()
    case = _synthetic(300, dev)
    mc = _Mc(case.call(), 0.25, 0.2, S, alpha, beta)
    want = mc_statistics_reference(mc.samples[:, :S], alpha, beta)
    for name, w in zip(("mean", "std", "acq"), want):
        got = getattr(mc, name).cpu().numpy()
        assert np.array_equal(got.view(np.int32), w.view(np.int32)), (name, float(np.abs(got - w).max()))
    if S == 1:
        assert bool((mc.std == 0).all()) and torch.equal(_bits(mc.mean), _bits(mc.samples[:, 0]))
    bare = _Mc(case.call(), 0.25, 0.2, S, alpha, beta, samples=False, pred=False)       # no [n, S] buffer, no pred, no emb
    assert bool((_bits(bare.samples) == PATTERN).all())
    for name in ("mean", "std", "acq"):
        assert torch.equal(_bits(getattr(bare, name)), _bits(getattr(mc, name))), name


# ------------------------------------------------------------------------------------------------------ 5: chunk edges --
def test_a_molecule_at_the_limit_single_atoms_and_twelve_small_ones():
    from molkgnn_amd import _lib
    from molkgnn_amd import readout as R
    dev = _dev()
    b = T.batch_of([T.tree(10)] * 12 + [T.circulant(_lib.TAIL_MAX_ATOMS), T.single(), T.tree(30)], seed=21).to(dev)
    case = _Case(b, b.num_graphs, 21, dev)
    assert R._tail_limits_ok(case.seg, case.plan) and max(T.molecule_sizes(b)) == _lib.TAIL_MAX_ATOMS
    score = case.call()
    score.score()
    for p_head, p_ro in PROBS:
        S = 5
        mc = _Mc(case.call(), p_head, p_ro, S)
        _close_all(mc.samples, _samples_f64(case, p_head, p_ro, S))
        for s in (0, S - 1):
            assert torch.equal(_bits(mc.samples[:, s]), _bits(_training_pred(case, p_head, p_ro, OFFSET + s))), s
        assert torch.equal(_bits(mc.c.pred), _bits(score.pred)) and torch.equal(_bits(mc.c.emb), _bits(score.emb))


def test_a_padded_batch_gives_the_real_molecules_the_unpadded_batch_s_bits():
    """padding.pad_batch with fewer than 64 padding atoms: most of the 64 padding molecules are empty, and a chunk of empty
    molecules has A == 0 (as test_score_tail_on_padded_batches_equals_the_unpadded_batch builds it)."""
    from molkgnn_amd import padding as P
    from molkgnn_amd import readout as R
    from molkgnn_amd.receptive_field import attach_receptive_fields
    from molkgnn_amd.synthetic import make_batch
    dev = _dev()
    B = 700
    raw = make_batch(B, seed=4100, with_receptive_fields=False)
    shape = P.fixed_shape([P.degree_histogram(raw)])
    n_pad = shape["atoms"] - raw.x.shape[0]
    assert 0 < n_pad < 64, n_pad
    plain = attach_receptive_fields(raw.to(dev))
    plain.num_graphs = B
    padded = attach_receptive_fields(P.pad_batch(raw, shape, B).to(dev), sizes=[shape[f"n{d}"] for d in range(1, 5)])
    mods = _modules(dev, 5)
    case0 = _Case(plain, B, 77, dev, mods)
    seg1 = R.MoleculeSegments.from_tensors(padded.mol_ptr, padded.atom_mol, padded.max_mol_atoms, padded.max_mol_edges)
    assert seg1.size == B + P.PAD_MOLECULES
    case1 = _Case(padded, B, 78, dev, mods, seg=seg1)
    n_real = plain.x.shape[0]
    assert torch.equal(case1.inblock[:n_real], case0.inblock)
    case1.sim0[:n_real] = case0.sim0                       # the real atoms' rows; the padding atoms keep random ones
    for p_head, p_ro in PROBS:
        m0 = _Mc(case0.call(), p_head, p_ro, 5, 1.0, 1.0)
        m1 = _Mc(case1.call(), p_head, p_ro, 5, 1.0, 1.0)
        assert m1.samples.shape == (B, 5) and torch.equal(_bits(m1.samples), _bits(m0.samples))
        for name in ("mean", "std", "acq"):
            assert torch.equal(_bits(getattr(m1, name)), _bits(getattr(m0, name))), name
        assert torch.equal(_bits(m1.c.pred), _bits(m0.c.pred)) and torch.equal(_bits(m1.c.emb[:B]), _bits(m0.c.emb))
        _close_all(m0.samples, _samples_f64(case0, p_head, p_ro, 5))


def test_an_oversize_molecule_is_loud_in_every_output_of_its_row():
    from molkgnn_amd import readout as R
    dev = _dev()
    b = T.batch_of([T.tree(12), T.circulant(130), T.tree(30)], seed=14).to(dev)
    case = _Case(b, 3, 14, dev)
    assert not R._tail_limits_ok(case.seg, case.plan)
    for p_head, p_ro in PROBS:
        mc = _Mc(case.call(), p_head, p_ro, 5, 1.0, 1.0)
        for t in (mc.samples[1], mc.mean[1], mc.std[1], mc.acq[1], mc.c.pred[1], mc.c.emb[1]):
            assert bool(torch.isnan(t).all())
        _close_all(mc.samples[[0, 2]], _samples_f64(case, p_head, p_ro, 5)[[0, 2]])
        assert bool(torch.isfinite(mc.mean[[0, 2]]).all()) and bool(torch.isfinite(mc.acq[[0, 2]]).all())


# ---------------------------------------------------------------------------------------------------- 6: unbiasedness --
def _unbiased(mean, pred, std, what):
    """|mean - pred| <= 6 std / 8 for every molecule with std > 0; at most 1 % may have std == 0.  (The standard error of a mean of
    64 samples is std / 8: six of them.)"""
    mean, pred, std = (t.double().reshape(-1) for t in (mean, pred, std))
    live = std > 0
    excluded = int((~live).sum())
    ratio = ((mean - pred).abs()[live] / (std[live] / 8.0))
    print(f"{what}: {excluded} excluded, max |mean - pred| / (std / 8) = {float(ratio.max()):.3f}")
    assert excluded <= mean.numel() // 100, (what, excluded)
    assert bool((ratio <= 6.0).all()), (what, float(ratio.max()))


def test_the_sample_mean_is_an_unbiased_estimate_of_the_point_score():
    dev = _dev()
    case = _synthetic(300, dev)
    p_head, p_ro, S = 0.25, 0.2, 64
    ref = _samples_f64(case, p_head, p_ro, S)
    want_pred, _ = _reference_f64(case.b, case.inblock, case.sim0, case.mods, 300, dev)
    _unbiased(ref.mean(dim=1), want_pred, ref.std(dim=1, unbiased=True), "float64 reference")
    mc = _Mc(case.call(), p_head, p_ro, S)
    _close_all(mc.samples, ref)
    _unbiased(mc.mean, mc.c.pred, mc.std, "kernel")


# -------------------------------------------------------------------------------------------------------- 7: refusals --
@pytest.mark.parametrize("bad", ["no_samples", "too_many_samples", "head_p_one", "readout_p_one", "short_stride", "null_pair",
                                 "short_workspace", "null_out"])
def test_the_c_abi_refuses_before_any_launch(bad):
    from molkgnn_amd import _lib
    dev = _dev()
    case = _synthetic(20, dev)
    kw = dict(p_head=0.25, p_ro=0.2, S=4, check=False)
    if bad == "no_samples":
        kw["S"] = 0
    elif bad == "too_many_samples":
        kw["S"] = 65
    elif bad == "head_p_one":
        kw["p_head"] = 1.0
    elif bad == "readout_p_one":
        kw["p_ro"] = 1.0
    elif bad == "short_stride":
        kw["stride"] = 3
    elif bad == "null_pair":
        kw["null_pair"] = True
    elif bad == "short_workspace":
        kw["short_ws"] = True
    if bad == "null_out":
        lib = _lib.load()
        c = case.call()
        pair = torch.tensor([SEED, OFFSET], dtype=torch.int64, device=dev)
        ws = torch.full((1 << 20,), 0x5A, dtype=torch.uint8, device=dev)
        rc = lib.mkgnn_tail_score_mc(ctypes.byref(c.a), 0.2, 4, pair.data_ptr(), None, ws.data_ptr(), ws.numel(), _lib.stream_ptr(dev))
        torch.cuda.synchronize()
        assert rc != 0 and bool((ws == 0x5A).all()) and bool((_bits(c.pred) == PATTERN).all())
        return
    mc = _Mc(case.call(), **kw)
    assert mc.rc != 0, bad
    print(_lib.load().mkgnn_last_error().decode())
    assert mc.all_patterned(), "a refused call wrote an output"
    assert bool((mc.ws == 0x5A).all()), "a refused call wrote its workspace"
    mc.c.untouched()


def test_tail_score_mc_refuses_to_drop_a_gradient_and_advances_only_its_own_generator():
    from molkgnn_amd import readout as R
    dev = _dev()
    case = _synthetic(20, dev)
    lin1, lin2, ffn = case.mods
    with pytest.raises(RuntimeError, match="forward only"):
        R.tail_score_mc(case.sim0, case.plan, LS, lin1, lin2, ffn, case.seg, 4, 0.25, 0.2)
    R.reset_head_rng(dev, seed=SEED)
    R.head_rng_state(dev)[1] = OFFSET
    pair = torch.tensor([SEED, OFFSET], dtype=torch.int64, device=dev)
    with torch.no_grad():
        with pytest.raises(ValueError, match="n_samples"):
            R.tail_score_mc(case.sim0, case.plan, LS, lin1, lin2, ffn, case.seg, 65, 0.25, 0.2)
        own = R.tail_score_mc(case.sim0, case.plan, LS, lin1, lin2, ffn, case.seg, 4, 0.25, 0.2, n_rows=17, beta=1.0,
                              return_samples=True, return_pred=True)
        assert R.head_rng_state(dev).tolist() == [SEED, OFFSET + 4]
        given = R.tail_score_mc(case.sim0, case.plan, LS, lin1, lin2, ffn, case.seg, 4, 0.25, 0.2, n_rows=17, beta=1.0,
                                rng_pair=pair, return_samples=True)
        assert R.head_rng_state(dev).tolist() == [SEED, OFFSET + 4] and pair.tolist() == [SEED, OFFSET]
    assert set(own) == {"mean", "std", "acq", "samples", "pred", "emb"} and set(given) == {"mean", "std", "acq", "samples"}
    assert own["samples"].shape == (17, 4) and own["pred"].shape == (17,) and own["emb"].shape == (20, 32)
    for k in given:
        assert torch.equal(_bits(own[k]), _bits(given[k])), k
    _close_all(own["samples"], _samples_f64(case, 0.25, 0.2, 4)[:17])


# ----------------------------------------------------------------------------------------------------- 8: model level --
def _mc_model(dev, seed=1798, **kw):
    from tests._resident_library import eval_model
    kw.setdefault("dropout_ratio", 0.2)
    kw.setdefault("ffn_dropout_rate", 0.25)
    return eval_model(dev, seed, **kw)


def _spy(monkeypatch, R, name):
    calls = []
    real = getattr(R, name)
    monkeypatch.setattr(R, name, lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    return calls


def _model_batch(n, seed, dev):
    from molkgnn_amd.synthetic import make_batch
    b = make_batch(n, seed=seed, target="docking_score").to(dev)
    b.num_graphs = n
    return b


def test_predict_mc_takes_the_kernel_and_changes_nothing_but_the_generator(monkeypatch):
    from molkgnn_amd import readout as R
    dev = _dev()
    model = _mc_model(dev)
    b = _model_batch(300, 61, dev)
    S = 64
    want_pred = model.predict(b)[0].reshape(-1).clone()
    state0 = {k: v.clone() for k, v in model.state_dict().items()}
    R.reset_head_rng(dev, seed=4321)
    assert R.head_rng_state(dev).tolist() == [4321, 0]
    calls = _spy(monkeypatch, R, "tail_score_mc")
    r = model.predict_mc(b, S, alpha=-1.0, beta=2.0, return_samples=True)
    torch.cuda.synchronize()
    assert len(calls) == 1, "predict_mc takes the kernel route"
    assert R.head_rng_state(dev).tolist() == [4321, S], "the head generator advances by exactly n_samples"
    assert set(r) == {"pred", "mean", "std", "acq", "samples"}
    assert r["samples"].shape == (300, S) and all(r[k].shape == (300,) for k in ("pred", "mean", "std", "acq"))
    assert torch.equal(_bits(r["pred"]), _bits(want_pred))
    want = R.mc_statistics_reference(r["samples"], -1.0, 2.0)
    for name, w in zip(("mean", "std", "acq"), want):
        assert np.array_equal(r[name].cpu().numpy().view(np.int32), w.view(np.int32)), name
    _unbiased(r["mean"], r["pred"], r["std"], "predict_mc")
    assert not model.training and not any(m.training for m in model.modules())
    state1 = model.state_dict()
    for k, v in state0.items():
        assert torch.equal(v, state1[k]), k
    without = model.predict_mc(b, S)
    assert set(without) == {"pred", "mean", "std", "acq"} and R.head_rng_state(dev).tolist() == [4321, 2 * S]
    assert not torch.equal(_bits(without["mean"]), _bits(r["mean"])), "the next call draws other masks"


def test_predict_mc_inside_a_captured_graph_draws_fresh_masks_on_every_replay(monkeypatch):
    from molkgnn_amd import readout as R
    dev = _dev()
    model = _mc_model(dev)
    b = _model_batch(300, 61, dev)
    S = 8
    want_pred = model.predict(b)[0].reshape(-1).clone()
    R.reset_head_rng(dev, seed=99)
    calls = _spy(monkeypatch, R, "tail_score_mc")
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        model.predict_mc(b, S, return_samples=True)            # (eager once: lazily made buffers exist before the capture)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            out = model.predict_mc(b, S, return_samples=True)
    torch.cuda.current_stream(dev).wait_stream(side)
    assert len(calls) == 2, "the captured call takes the kernel route too"
    seen = []
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        seen.append((out["samples"].clone(), out["pred"].clone(), R.head_rng_state(dev).tolist()))
    assert seen[0][2] == [99, 2 * S] and seen[1][2] == [99, 3 * S]
    assert not torch.equal(_bits(seen[0][0]), _bits(seen[1][0])), "two replays give different samples"
    assert torch.equal(_bits(seen[0][1]), _bits(want_pred)) and torch.equal(_bits(seen[1][1]), _bits(want_pred))


@pytest.mark.parametrize("why", ["switch", "three_tasks", "oversize_molecule"])
def test_predict_mc_on_the_torch_route(why, monkeypatch):
    from molkgnn_amd import readout as R
    dev = _dev()
    S = 64
    torch.manual_seed(7)
    if why == "three_tasks":
        model = _mc_model(dev, task_dim=3)
        b = _model_batch(300, 61, dev)
        want_pred = model.predict_tasks(b)[0].clone()
        shape = (300, 3)
    elif why == "oversize_molecule":
        model = _mc_model(dev)
        b = T.batch_of([T.tree(12), T.circulant(130), T.tree(30)] + [T.tree(20)] * 8, seed=15).to(dev)
        want_pred = model.predict(b)[0].reshape(-1).clone()
        shape = (11,)
    else:
        model = _mc_model(dev)
        monkeypatch.setattr(R, "_SCORE_MC", False)
        b = _model_batch(300, 61, dev)
        want_pred = model.predict(b)[0].reshape(-1).clone()
        shape = (300,)
    calls = _spy(monkeypatch, R, "tail_score_mc")
    rng0 = R.head_rng_state(dev).clone()
    r = model.predict_mc(b, S, alpha=1.0, beta=1.0, return_samples=True)
    torch.cuda.synchronize()
    assert not calls, "the kernel route was taken"
    assert torch.equal(R.head_rng_state(dev), rng0)
    assert set(r) == {"pred", "mean", "std", "acq", "samples"}
    assert all(tuple(r[k].shape) == shape for k in ("pred", "mean", "std", "acq"))
    assert tuple(r["samples"].shape) == (shape[0], S, *shape[1:])
    assert torch.equal(_bits(r["pred"]), _bits(want_pred))
    assert bool(torch.isfinite(r["samples"]).all())
    _unbiased(r["mean"], r["pred"], r["std"], f"torch route ({why})")
    assert not model.training


# ------------------------------------------------------------------------------------------------------- 9: screening --
@pytest.fixture(scope="module")
def library(tmp_path_factory):
    from tests._resident_library import build_library
    model, residents, _ = build_library(tmp_path_factory.mktemp("mc-library"), "cuda:0", counts=(70,), shard_seed=40,
                                        labels=lambda n: (torch.arange(n) % 3 == 0).float(), model_seed=0, num_layers=3,
                                        dropout_ratio=0.2, ffn_dropout_rate=0.25)
    return model, residents


def test_score_resident_mc_is_reproducible_for_a_seed_and_keeps_the_point_score(library):
    from molkgnn_amd.screening import score_resident, score_resident_mc
    model, residents = library
    shard = residents[0]                                   # 70 molecules in batches of 32: a short last batch of 6
    first = [t.clone() for t in score_resident_mc(model, shard, 32, 16, alpha=-1.0, beta=2.0, seed=11)]
    second = score_resident_mc(model, shard, 32, 16, alpha=-1.0, beta=2.0, seed=11)
    assert len(first) == 4 and all(t.shape == (70,) for t in first)
    for a, b in zip(first, second):
        assert torch.equal(_bits(a), _bits(b))
    other = score_resident_mc(model, shard, 32, 16, alpha=-1.0, beta=2.0, seed=12)
    assert not torch.equal(_bits(other[1]), _bits(first[1]))
    pred, mean, std, acq = first
    assert torch.equal(_bits(pred), _bits(score_resident(model, shard, 32)))
    assert bool(torch.isfinite(mean).all()) and bool((std > 0).all())
    one = np.float32(-1.0) * mean.cpu().numpy() + np.float32(2.0) * std.cpu().numpy()
    assert np.array_equal(acq.cpu().numpy().view(np.int32), one.astype(np.float32).view(np.int32))
    assert not model.training
    with pytest.raises(ValueError, match="n_samples"):
        score_resident_mc(model, shard, 32, 0)


@pytest.mark.parametrize("k", [5, 100])
def test_screen_acquisition_ranks_by_the_acquisition_value(library, k):
    from molkgnn_amd.screening import empty_top, score_resident_mc, screen_acquisition, topk_update_reference
    model, residents = library
    pred, mean, std, acq = (t.clone() for t in score_resident_mc(model, residents[0], 32, 16, alpha=-1.0, beta=1.0, seed=5))
    r = screen_acquisition(model, (s for s in residents), k, 32, 16, alpha=-1.0, beta=1.0, seed=5)
    assert set(r) == {"top_score", "top_pred", "top_mean", "top_std", "top_shard", "top_mol", "n_scored"} and r["n_scored"] == 70
    want = topk_update_reference(empty_top(k), acq.cpu().numpy(), np.arange(70, dtype=np.int32), 70, 0)
    occupied = min(k, 70)
    got = (r["top_score"].cpu().numpy(), r["top_shard"].cpu().numpy(), r["top_mol"].cpu().numpy())
    for g, w in zip(got, want):
        assert g.shape == (occupied,) and np.array_equal(g.view(np.int32), w[:occupied].view(np.int32))
    at = r["top_mol"].long()
    for name, vector in (("top_pred", pred), ("top_mean", mean), ("top_std", std)):
        assert torch.equal(_bits(r[name]), _bits(vector[at])), name
