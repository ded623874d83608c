"""The any-shape convolution kernels against float64 at every width edge.  ``pytest -m gpu``.

``kc_forward_generic``, ``kc_backward_rows``, ``kc_backward_bank``, ``kc_backward_bank_reduce``, ``kc_backward_gather``
(csrc/kgnn_generic.hip) and ``bank_prepare_task`` (csrc/kgnn_prepare.h) serve every shape the C ABI admits (F = 1..256, E = 1..64, any
kernel counts) and are the ``variant="generic"`` reference of the A/B switches.  Every case of ``tests/_conv_f64.CASES`` -- one per
side of every branch those kernels take on the row width, the bond width, the kernel counts and the atoms per bucket; the CPU
module proves each reaches its edge and that the fp32 oracle passes the same bound -- runs under the any-shape kernels and under
the automatic dispatch:

* forward by the tie-aware criterion, zeros outside an atom's own degree block, nothing non-finite;
* the three scores the kernels keep for backward against the float64 oracle at the build's permutation (``tests/_f64.check``), the
  chirality sign exactly;
* grad x, every parameter gradient and the score weights per element within ``32 * 2^-24 * sum |terms|`` of the float64 closed form;
* which kernels ran: the streamed launch counters, and under the automatic dispatch at F <= 160 the family of every degree
  (``mkgnn_debug_conv_dispatch`` against ``tests/_conv_f64.AUTO_DISPATCH``).

Beside the table: banks prepared ahead (``prepare_banks``, direct and deferred) give the same bits, two runs give the same bits,
and shapes outside the ABI's limits are refused before anything is written.
"""
import copy

import pytest
import torch

from tests import _conv_f64 as C

pytestmark = pytest.mark.gpu

NAMES = [c.name for c in C.CASES]
PATH_IDS = ["generic", "auto"]


def _dev():
    assert torch.cuda.is_available(), "pytest -m gpu needs the MI355X"
    return torch.device("cuda:0")


@pytest.mark.parametrize("path", C.PATHS, ids=PATH_IDS)
@pytest.mark.parametrize("name", NAMES)
def test_case_against_float64(name, path):
    dev = _dev()
    built = C.build(name)
    case = built.case
    res = C.run_build(built, dev, *path)
    tag = (name, path[0])
    worst, oracle = C.check_against_float64(built, res, tag)
    # ---- which kernels ran
    if path[0] == "generic":
        assert res.streamed == (0, 0, 0) and res.backward == "generic", (tag, res.streamed)
    elif case.F > C.STREAM_MAX_F:
        assert res.streamed == (0, 0, 0) and res.backward == "auto", (tag, res.streamed)
    else:
        # the automatic dispatch where the fast kernels exist: the families the plan functions name for this case, and the streamed
        # launch counters' agreement with them (a case meant for the fast path that lands on the any-shape kernels fails here)
        assert res.dispatch == C.AUTO_DISPATCH[name], (tag, res.dispatch)
        C.check_streamed_counters(res.dispatch, res.streamed, tag)
    C.record({"case": name, "edge": case.edge, "path": path[0], "backward": res.backward, "streamed": list(res.streamed),
              "worst": worst, **C.worst_by_group(res.gx, res.grads, oracle)})


DETERMINISM = ["width_f129", "width_f256", "bond_e64_f129", "counts_129_1_0_17_f130", "atoms_n4_257", "clamp_f256", "chirality_f129"]


@pytest.mark.parametrize("path", C.PATHS, ids=PATH_IDS)
@pytest.mark.parametrize("name", DETERMINISM)
def test_two_runs_give_the_same_bits(name, path):
    """Fixed-order sums and no float atomics: every output of a second run is bit-identical."""
    dev = _dev()
    built = C.build(name)
    a, b = C.run_build(built, dev, *path), C.run_build(built, dev, *path)
    assert torch.equal(a.out, b.out) and torch.equal(a.gx, b.gx)
    for u, v in zip(a.idx + a.scores + a.chir, b.idx + b.scores + b.chir):
        assert (u is None) == (v is None) and (u is None or torch.equal(u, v))
    assert a.grads.keys() == b.grads.keys()
    for k in a.grads:
        assert torch.equal(a.grads[k], b.grads[k]), k


PREPARED = [(28, (10, 20, 30, 50)), (128, (3, 2, 4, 2)), (129, (5, 1, 7, 17)), (161, (2, 9, 3, 6)), (256, (4, 3, 2, 5))]


@pytest.mark.parametrize("variant", ["generic", "auto"])
def test_banks_prepared_ahead_give_the_same_bits(variant):
    """``prepare_banks`` over five calls of different widths and counts (two launches: four calls each at most), launched directly
    and left pending for ``prepare_flush``: forward and every gradient bit-identical to the calls that prepare their own bank --
    on both sides of ``width <= 128`` and of ``bank_pitch``, the last call in the last layer (its chirality table)."""
    from molkgnn_amd import functional as Fn
    from molkgnn_amd.kernels import KernelSetConv
    from molkgnn_amd.plan import plan_from_data
    dev = _dev()
    cpu = C.build("width_f64").cpu
    bd = cpu.to(dev)
    plan = plan_from_data(bd)
    n = cpu.x.shape[0]
    torch.manual_seed(17)
    layers = [KernelSetConv(*counts, D=3, node_attr_dim=F, edge_attr_dim=7).to(dev) for F, counts in PREPARED]
    Fs = [F for F, _ in PREPARED]
    g = torch.Generator().manual_seed(18)
    stores = []
    for F in Fs:
        st = torch.zeros(n, F + (-F) % 4, device=dev)
        st[:, :F] = torch.randn(n, F, generator=g).to(dev)
        stores.append(st)
    cots = [torch.randn(n, sum(counts), generator=g).to(dev) for _, counts in PREPARED]
    pl = [layer._bank_params("train", stores[0])[0] for layer in layers]

    def run(k, prep):
        x = stores[k][:, :Fs[k]].detach().requires_grad_(True)
        for p in pl[k]:
            p.grad = None
        out = Fn.kernelsetconv(x, plan, k == 4, pl[k], 7, variant, prepared=prep)
        (out * cots[k]).sum().backward()
        torch.cuda.synchronize()
        return out.detach().clone(), x.grad.clone(), [None if p.grad is None else p.grad.clone() for p in pl[k]]

    plain = [run(k, None) for k in range(5)]

    def same(k, prep):
        assert prep.key == Fn._prepared_key(pl[k], Fs[k], 7, n, plan.n_slots)          # (the call will take it: not stale)
        o, gx, gp = run(k, prep)
        assert torch.equal(o, plain[k][0]) and torch.equal(gx, plain[k][1]), (variant, k)
        assert all((a is None and c is None) or torch.equal(a, c) for a, c in zip(gp, plain[k][2])), (variant, k)

    direct = Fn.prepare_banks(pl, Fs, 7, n, plan.n_slots)
    assert len(direct) == 5
    for k in range(5):
        same(k, direct[k])
    # left pending (at most four calls): the widths on both sides of both thresholds, launched by the flush
    pending = Fn.prepare_banks(pl[1:], Fs[1:], 7, n, plan.n_slots, defer=True)
    Fn.prepare_flush(dev)
    for k in range(1, 5):
        same(k, pending[k - 1])
    # five calls with defer=True: more than a pending preparation holds -- the wrapper launches them at once; a flush finds nothing
    five = Fn.prepare_banks(pl, Fs, 7, n, plan.n_slots, defer=True)
    Fn.prepare_flush(dev)
    for k in range(5):
        same(k, five[k])


SENTINEL = 1234.5


@pytest.mark.parametrize("F,E", [(257, 7), (64, 65), (0, 7), (64, 0)])
def test_shapes_outside_the_limits_are_refused_before_any_launch(F, E):
    """F = 1..256 and E = 1..64 are the ABI's limits: beyond them both entry points answer with an error from the host-side check
    -- output, workspace, input gradient and bank gradients of the test's own keep their sentinel bits, and no streamed kernel is
    launched.  (The calls carry valid buffers of a 64-wide case: only the two widths are out of range.)"""
    from molkgnn_amd import _lib
    from molkgnn_amd import functional as Fn
    from molkgnn_amd._lib import MolKGNNLibraryError
    from molkgnn_amd.plan import plan_from_data
    dev = _dev()
    built = C.build("width_f64")
    lib = _lib.load()
    bd = built.cpu.to(dev)
    plan = plan_from_data(bd)
    n, F0 = built.x.shape
    layer = copy.deepcopy(built.layer).to(dev)
    x = built.x.to(dev).contiguous()
    params, E0 = layer._bank_params("train", x)
    params = [p.detach() for p in params]
    banks, Ls, keep = Fn._banks(params, F0, E0)
    buckets = Fn._buckets(plan, E0, False)
    inv = Fn.row_inv_norm(x)
    K = sum(Ls)
    out = torch.full((n, K), SENTINEL, device=dev)
    ws = torch.full((Fn.workspace_bytes(Ls, F0, E0, n, plan.n_slots) // 4 + 1,), SENTINEL, device=dev)
    gx = torch.full((n, F0), SENTINEL, device=dev)
    gout = torch.randn(n, K, device=dev)
    gbuf = [torch.full((p.numel() + 3,), SENTINEL, device=dev) for p in params]
    grads = _lib.BankGrads4()
    for i in range(4):
        gxc, gxs, ges, _, gts, gtc, gte = gbuf[7 * i:7 * i + 7]
        grads[i].x_center, grads[i].x_support, grads[i].edge_attr_support = gxc.data_ptr(), gxs.data_ptr(), ges.data_ptr()
        grads[i].support_attr_sc_weight, grads[i].center_attr_sc_weight, grads[i].edge_attr_support_sc_weight = \
            gts.data_ptr(), gtc.data_ptr(), gte.data_ptr()
    rowptr, rows = plan.scatter
    saved = _lib.Saved4()
    torch.cuda.synchronize()
    before = C.streamed_launches()
    st = _lib.stream_ptr(dev)
    for variant in (0, 1):
        with pytest.raises(MolKGNNLibraryError, match="outside 1.."):
            _lib.check(lib.mkgnn_kernelsetconv_forward(banks, buckets, x.data_ptr(), F0, inv.data_ptr(), n, F, E, 0, out.data_ptr(), K,
                                                       saved, ws.data_ptr(), ws.numel() * 4, variant, st), "mkgnn_kernelsetconv_forward")
        with pytest.raises(MolKGNNLibraryError, match="outside 1.."):
            _lib.check(lib.mkgnn_kernelsetconv_backward(banks, buckets, x.data_ptr(), F0, inv.data_ptr(), n, F, E, 0, gout.data_ptr(), K,
                                                        saved, rowptr.data_ptr(), rows.data_ptr(), gx.data_ptr(), F0, grads,
                                                        ws.data_ptr(), ws.numel() * 4, 0, variant, st), "mkgnn_kernelsetconv_backward")
    torch.cuda.synchronize()
    assert C.streamed_launches() == before
    for t in [out, ws, gx] + gbuf:
        assert bool((t == SENTINEL).all())
    # ... and through the operator: kernels of the refused width, an error before the convolution
    if F > 0 and E > 0:
        from molkgnn_amd.kernels import KernelSetConv
        wide = KernelSetConv(3, 2, 4, 2, D=3, node_attr_dim=F, edge_attr_dim=E).to(dev)
        cpu = C.T.batch_of(C._base(), F=F, E=E, seed=3)
        with pytest.raises(MolKGNNLibraryError, match="outside 1.."):
            wide._run(cpu.x.to(dev), plan_from_data(cpu.to(dev)), False)
