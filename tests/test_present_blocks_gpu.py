"""Present blocks of d loss / d h (``MKGNN_GRAD_BLOCKS``; csrc/kgnn_launch.h GradBlocks, functional.mark_grad_blocks).  ``pytest -m gpu``.

Between two layers ``h = propagate(sim_sc)`` is structurally zero outside the column blocks of every atom's bond partners' degrees,
and the layer below reads ``d loss / d h`` in exactly those blocks.  The gather of the layer that reads a tagged ``h`` skips every
other 16-byte chunk of the contribution rows, of ``h`` and of the gradient.  What must hold, against the same kernels with the
switch off:

* loss, every parameter gradient and the input gradient are BIT FOR BIT the same, eagerly and in a replayed graph, and the masked
  kernels really ran (``mkgnn_debug_grad_blocks_launches``);
* nothing absent is read or written: with the contribution rows and the gradient buffers filled with NaN beforehand, the results
  are finite and unchanged and the absent chunks of ``d loss / d h`` are still NaN;
* the chunk tables hold where block boundaries fall inside a chunk, where all blocks share one chunk, with several column parts,
  and at forty chunks per row;
* a tensor without a valid tag gets the whole gradient from the plain kernels.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

REF = (10, 20, 30, 50)


def _dev():
    assert torch.cuda.is_available(), "pytest -m gpu needs the MI355X"
    return torch.device("cuda:0")


def _gnn(hop1=REF, hopn=REF, layers=3, seed=5):
    from molkgnn_amd.KernelLayer import MolGCN
    torch.manual_seed(seed)
    names = {f"num_kernel{d}_1hop": hop1[d - 1] for d in range(1, 5)}
    names.update({f"num_kernel{d}_Nhop": hopn[d - 1] for d in range(1, 5)})
    return MolGCN(num_layers=layers, x_dim=28, p_dim=3, edge_attr_dim=7, **names).to(_dev())


def _kwargs(b):
    kw = {f"{nm}_deg{d}": getattr(b, f"{nm}_deg{d}")
          for nm in ("p_focal", "nei_p", "nei_edge_attr", "selected_index", "nei_index") for d in range(1, 5)}
    return dict(edge_index=b.edge_index, edge_attr=b.edge_attr, p=b.p, save_score=False, **kw)


class _Case:
    """A network, a batch (48 to 64 molecules: the per-operator path), an input and a cotangent of the last layer's h."""

    def __init__(self, hop1=REF, hopn=REF, n_mol=56, seed=41, layers=3):
        from molkgnn_amd.synthetic import make_batch
        self.gnn = _gnn(hop1, hopn, layers)
        self.b = make_batch(n_mol, seed=seed).to(_dev())
        g = torch.Generator().manual_seed(seed)
        self.x0 = torch.randn(self.b.x.shape[0], 28, generator=g).to(_dev())
        self.cot = torch.randn(self.b.x.shape[0], sum(hopn), generator=g).to(_dev())
        self.kw = _kwargs(self.b)
        self.x = self.x0.clone().requires_grad_(True)
        self.after_forward = None                         # called between the forward and the backward

    def step(self):
        for p in self.gnn.parameters():
            p.grad = None
        self.x.grad = None
        h = self.gnn(x=self.x, **self.kw)
        loss = (h * self.cot).sum()
        if self.after_forward is not None:
            self.after_forward()
        loss.backward()
        return loss

    def results(self, loss):
        torch.cuda.synchronize()
        return (loss.detach().clone(), self.x.grad.clone(),
                {n: p.grad.clone() for n, p in self.gnn.named_parameters() if p.grad is not None})


def _same(a, c):
    assert torch.equal(a[0], c[0]), (float(a[0]), float(c[0]))
    assert torch.equal(a[1], c[1]), "input gradient"
    assert set(a[2]) == set(c[2]) and len(a[2]) >= 16
    for n in a[2]:
        assert torch.equal(a[2][n], c[2][n]), n
        assert bool(torch.isfinite(a[2][n]).all()), n


def _counted(fn):
    from molkgnn_amd import functional as Fn
    n0 = Fn.debug_grad_blocks_launches()
    out = fn()
    torch.cuda.synchronize()
    return out, Fn.debug_grad_blocks_launches() - n0


def _plain(case, monkeypatch):
    """The step with MKGNN_GRAD_BLOCKS=0's behaviour: nobody tags, nobody takes a tag."""
    from molkgnn_amd import functional as Fn
    with monkeypatch.context() as m:
        m.setattr(Fn, "GRAD_BLOCKS", False)
        loss, counts = _counted(case.step)
        assert counts == 0, counts
        return case.results(loss)


def test_step_is_bit_equal_with_and_without_present_blocks(monkeypatch):
    case = _Case()
    want = _plain(case, monkeypatch)
    loss, counts = _counted(case.step)
    assert counts == 2, counts                            # the masked gather of each of the two N-hop layers
    _same(case.results(loss), want)


def test_captured_step_replayed_three_times_is_bit_equal(monkeypatch):
    case = _Case(seed=43)
    want = _plain(case, monkeypatch)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            case.step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    (loss, counts) = (None, None)
    with torch.cuda.graph(graph):
        loss, counts = _counted_nosync(case.step)
    assert counts == 2, counts
    for _ in range(3):
        case.x.grad.zero_()
        for p in case.gnn.parameters():
            if p.grad is not None:
                p.grad.zero_()
        graph.replay()
        _same(case.results(loss), want)


def _counted_nosync(fn):
    from molkgnn_amd import functional as Fn
    n0 = Fn.debug_grad_blocks_launches()
    out = fn()
    return out, Fn.debug_grad_blocks_launches() - n0


def _chunk_blocks(Ls, width):
    """[chunks] the blocks (bit d - 1) that meet columns 4 c .. 4 c + 3."""
    off = np.concatenate([[0], np.cumsum(Ls)])
    out = np.zeros((width + 3) // 4, dtype=np.int64)
    for c in range(out.shape[0]):
        for d in range(4):
            if Ls[d] > 0 and 4 * c + 3 >= off[d] and 4 * c < off[d + 1]:
                out[c] |= 1 << d
    return out


def _spy_tagged_gradients(monkeypatch, case, seen):
    """``seen`` receives (d loss / d h, plan, blocks) of every tagged h of ``case``'s next step.  The hooks are put on AFTER the
    forward: a tensor that carries a hook when its reader's forward runs has another reader, and gets whole rows
    (functional.grad_blocks_of) -- here the point is to look at what the masked kernels left."""
    from molkgnn_amd import functional as Fn
    real, tagged = Fn.mark_grad_blocks, []

    def spy(h, plan, blocks):
        out = real(h, plan, blocks)
        if h.requires_grad:
            tagged.append((h, plan, tuple(int(v) for v in blocks)))
        return out

    def hook_all():
        for h, plan, blocks in tagged:
            h.register_hook(lambda g, plan=plan, blocks=blocks: seen.append((g.detach().clone(), plan, blocks)))
        tagged.clear()
    monkeypatch.setattr(Fn, "mark_grad_blocks", spy)
    case.after_forward = hook_all


def test_nothing_absent_is_read_or_written(monkeypatch):
    from molkgnn_amd import functional as Fn
    case = _Case(seed=47)
    want = case.results(case.step())
    seen = []
    _spy_tagged_gradients(monkeypatch, case, seen)
    Fn.debug_poison_backward(True)
    try:
        loss, counts = _counted(case.step)
        got = case.results(loss)
    finally:
        Fn.debug_poison_backward(False)
    assert counts == 2, counts
    _same(got, want)
    assert bool(torch.isfinite(got[1]).all())
    assert len(seen) == 2                                 # d loss / d h of the two inner h's
    for g, plan, blocks in seen:
        present = plan.present8.cpu().numpy().astype(np.int64) & 15
        chunks = _chunk_blocks(blocks, g.shape[1])
        keep = (present[:, None] == 0) | ((present[:, None] & chunks[None, :]) != 0)       # [atoms, chunks]
        cols = np.repeat(keep, 4, axis=1)[:, :g.shape[1]]
        nan = torch.isnan(g).cpu().numpy()
        assert 0.3 < cols.mean() < 0.7, cols.mean()       # (the benchmark's batch: 41 % of the chunks are present)
        assert not nan[cols].any()                        # every present chunk was written, with numbers
        assert nan[~cols].all()                           # ... and nothing else was


EDGES = {
    "boundaries_inside_a_chunk": ((5, 10, 15, 25), (5, 10, 15, 25)),
    "all_blocks_in_one_chunk": ((1, 1, 1, 1), (1, 1, 1, 1)),
    # (two layers: the layer that reads the tagged h has F = 110 and banks of up to seven column tiles, so its contribution rows
    # are the sums of four launches of the plain rows kernel before the masked gather reads them; a third layer would have to
    # take its 274 columns as input, more than any kernel does)
    "several_column_parts": (REF, (40, 70, 100, 64)),
    "forty_chunks": ((16, 32, 48, 64), (16, 32, 48, 64)),
}


@pytest.mark.parametrize("name", list(EDGES))
def test_edges_of_the_chunk_tables(name, monkeypatch):
    hop1, hopn = EDGES[name]
    case = _Case(hop1, hopn, n_mol=48, seed=53, layers=2 if name == "several_column_parts" else 3)
    want = _plain(case, monkeypatch)
    seen = []
    _spy_tagged_gradients(monkeypatch, case, seen)
    loss, counts = _counted(case.step)
    _same(case.results(loss), want)
    tagged = len(seen)
    if name == "several_column_parts":
        # h of the first layer is tagged; one masked gather reads it
        assert tagged == 1 and counts == 1, (tagged, counts)
    elif name == "forty_chunks":
        # 160 columns, 40 chunks: taken or refused (then whole rows), the same for both layers
        assert tagged == 2 and counts in (0, 2), (tagged, counts)
    else:
        assert tagged == 2 and counts == 2, (tagged, counts)


def _two_layers(banks=REF):
    """A 28 -> K layer that makes a tagged h and the K -> 110 layer that reads it, on a batch of 48 molecules."""
    from molkgnn_amd.kernels import KernelSetConv
    from molkgnn_amd.plan import plan_from_data
    from molkgnn_amd.synthetic import make_batch
    dev = _dev()
    torch.manual_seed(7)
    b = make_batch(48, seed=59).to(dev)
    plan = plan_from_data(b)
    first = KernelSetConv(*banks, D=3, node_attr_dim=28, edge_attr_dim=7).to(dev)
    second = KernelSetConv(*REF, D=3, node_attr_dim=sum(banks), edge_attr_dim=7).to(dev)
    g = torch.Generator().manual_seed(61)
    x = torch.randn(b.x.shape[0], 28, generator=g).to(dev)
    cot = torch.randn(b.x.shape[0], 110, generator=g).to(dev)
    return b, plan, first, second, x, cot


def _read(second, h, plan, cot, backward_variant=None):
    """The second layer on ``h`` with poisoned buffers: (counter deltas, d loss / d h as the layer wrote it)."""
    from molkgnn_amd import functional as Fn
    p2, E = second._bank_params("train", h)
    got = []
    Fn.debug_poison_backward(True)
    try:
        def run():
            out = Fn.kernelsetconv(h, plan, False, p2, E, "auto", block_rows=True, propagate=True, backward_variant=backward_variant)
            h.register_hook(lambda g: got.append(g.detach().clone()))        # (after the forward: see _spy_tagged_gradients)
            (out * cot).sum().backward()
        _, counts = _counted(run)
    finally:
        Fn.debug_poison_backward(False)
    return counts, got[0]


def _tagged_h(first, x, plan):
    from molkgnn_amd import functional as Fn
    p1, E = first._bank_params("train", x)
    return Fn.kernelsetconv(x.clone().requires_grad_(True), plan, False, p1, E, "auto", block_rows=True, propagate=True,
                            grad_blocks=True)


def test_tag_hygiene():
    from molkgnn_amd import functional as Fn
    b, plan, first, second, x, cot = _two_layers()
    # the tag as MolGCN.forward uses it: masked kernels, absent chunks untouched
    h = _tagged_h(first, x, plan)
    assert Fn.grad_blocks_of(h, plan) == REF
    counts, g = _read(second, h, plan, cot)
    assert counts == 1 and bool(torch.isnan(g).any())
    # a tagged h that is detached and made a leaf: a new tensor, no tag -- the plain kernels, the whole gradient
    h2 = _tagged_h(first, x, plan).detach().requires_grad_(True)
    assert Fn.grad_blocks_of(h2, plan) is None
    counts, full = _read(second, h2, plan, cot)
    assert counts == 0 and bool(torch.isfinite(full).all())
    # ... of which the masked gradient above is every chunk it wrote
    wrote = ~torch.isnan(g)
    assert torch.equal(g[wrote], full[wrote])
    # a tagged h that carries a hook when its reader's forward runs: somebody else reads the gradient -- whole rows
    h3 = _tagged_h(first, x, plan)
    h3.register_hook(lambda g: None)
    assert Fn.grad_blocks_of(h3, plan) is None
    counts, g3 = _read(second, h3, plan, cot)
    assert counts == 0 and torch.equal(g3, full)
    # a dense random leaf of width 110
    leaf = torch.zeros(b.x.shape[0], 112, device=_dev())[:, :110]
    leaf.copy_(torch.randn(b.x.shape[0], 110, generator=torch.Generator().manual_seed(3)))
    leaf.requires_grad_(True)
    counts, gl = _read(second, leaf, plan, cot)
    assert counts == 0 and bool(torch.isfinite(gl).all())
    # a reader on the generic backward kernels does not understand the tag: the whole gradient, equal to the default's to the
    # tolerance of the variant tests (tests/test_scale_parity.py holds either variant's grad x to the oracle with atol 3e-5, rtol 1e-3)
    counts, gg = _read(second, _tagged_h(first, x, plan), plan, cot, backward_variant="generic")
    assert counts == 0 and bool(torch.isfinite(gg).all())
    assert torch.allclose(gg, full, atol=3e-5, rtol=1e-3), float((gg - full).abs().max())


def test_tagged_h_modified_in_place_loses_the_tag():
    """(Banks of 112 columns: an h whose storage rows need no padding is no view of its storage, so autograd lets it be modified.)"""
    from molkgnn_amd import functional as Fn
    banks = (10, 20, 30, 52)
    b, plan, first, second, x, cot = _two_layers(banks)
    h = _tagged_h(first, x, plan)
    assert Fn.grad_blocks_of(h, plan) == banks
    counts, g = _read(second, h, plan, cot)
    assert counts == 1 and bool(torch.isnan(g).any())
    h = _tagged_h(first, x, plan)
    with torch.no_grad():
        h.add_(0.0)
    assert Fn.grad_blocks_of(h, plan) is None
    counts, full = _read(second, h, plan, cot)
    assert counts == 0 and bool(torch.isfinite(full).all())
    wrote = ~torch.isnan(g)
    assert torch.equal(g[wrote], full[wrote])


def test_dense_propagate_sets_no_tag(monkeypatch):
    """MKGNN_DENSE_PROPAGATE=1 (zero-filled rows, dense sums whose backward reads whole rows): no h is tagged."""
    from molkgnn_amd import KernelLayer
    from molkgnn_amd import functional as Fn
    monkeypatch.setattr(KernelLayer, "_BLOCK_ROWS", False)
    monkeypatch.setattr(KernelLayer, "_FUSE_PROPAGATE", False)
    monkeypatch.setattr(KernelLayer, "_ROWS_SPLIT", False)
    tags = []
    real = Fn.mark_grad_blocks
    monkeypatch.setattr(Fn, "mark_grad_blocks", lambda h, plan, blocks: (tags.append(1), real(h, plan, blocks))[1])
    case = _Case(n_mol=48, seed=67)
    loss, counts = _counted(case.step)
    assert counts == 0 and tags == []
    got = case.results(loss)
    assert bool(torch.isfinite(got[1]).all())


def test_library_switch_off_ignores_the_hint():
    """``MKGNN_GRAD_BLOCKS=0`` is read once per process, by the package and by the library: a child process with the variable set,
    in which the package's half is forced back on so that tags are set and hints are sent -- the library must ignore them: no masked
    launch, whole rows of d loss / d h (tests/_present_blocks_child.py)."""
    import os
    import subprocess
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MKGNN_GRAD_BLOCKS="0")
    out = subprocess.run([sys.executable, "-m", "tests._present_blocks_child"], cwd=repo, env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "hints sent 2, masked launches 0, whole rows 2" in out.stdout, out.stdout[-500:]
