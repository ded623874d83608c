"""``mkgnn_flat_copy`` (``flat_copy_kernel``, csrc/kgnn_optim.hip) at the edges of its table: around the 120 items of one launch,
item ends around the 256-lane passes and the 1024-element blocks, a three-block item on each side of every launch boundary -- called
directly, and through ``dp.FlatGradAllReduce._fill`` with more than 120 parameters, empty ones and ``None`` gradients.  A copy is exact:
everything is compared bit for bit.  ``pytest -m gpu``."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

GUARD = 1024
SRC_GAP = 8                 # sentinel floats between two sources
SENTINEL = 1234567.0
EDGE_SIZES = (1, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 4097)


def _dev():
    assert torch.cuda.is_available(), "pytest -m gpu needs the MI355X"
    return torch.device("cuda:0")


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def item_sizes(n_items):
    """1 .. 5 elements, the block-edge sizes spread over the table, and 2049 on each side of every 120-item boundary."""
    sizes = [1 + (7 * i) % 5 for i in range(n_items)]
    for k, n in enumerate(EDGE_SIZES):
        if 3 + 10 * k < n_items:
            sizes[3 + 10 * k] = n
    for pos in (0, 119, 120, 239, 240):
        if pos < n_items:
            sizes[pos] = 2049
    return sizes


class _Copy:
    """Sources cut out of one buffer with sentinels between them; destinations the adjacent slots of a flat buffer between two guards."""

    def __init__(self, dev, sizes, seed):
        from molkgnn_amd import _lib
        self._lib, self.lib, self.dev, self.sizes = _lib, _lib.load(), dev, sizes
        g = torch.Generator().manual_seed(seed)
        self.soff, o = [], SRC_GAP
        for n in sizes:
            self.soff.append(o)
            o += n + SRC_GAP
        src = torch.full((o,), SENTINEL)
        for off, n in zip(self.soff, sizes):
            src[off:off + n] = torch.randn(n, generator=g)
        self.src_host, self.src = src, src.to(dev)
        self.doff, o = [], GUARD
        for n in sizes:
            self.doff.append(o)
            o += n
        self.dst = torch.full((o + GUARD,), SENTINEL, device=dev)
        self.table = (_lib.CopyItem * len(sizes))()
        for e, so, do, n in zip(self.table, self.soff, self.doff, sizes):
            e.dst, e.src, e.numel = self.dst.data_ptr() + 4 * do, self.src.data_ptr() + 4 * so, n
        torch.cuda.synchronize()

    def run(self):
        with torch.cuda.device(self.dev):
            rc = self.lib.mkgnn_flat_copy(C.cast(self.table, C.c_void_p), len(self.sizes), self._lib.stream_ptr(self.dev))
        torch.cuda.synchronize()
        return rc

    def expected(self, upto=None):
        """The destination buffer with the first ``upto`` items (default: all) copied and nothing else touched."""
        want = torch.full((self.dst.numel(),), SENTINEL)
        for so, do, n in list(zip(self.soff, self.doff, self.sizes))[:upto]:
            want[do:do + n] = self.src_host[so:so + n]
        return want


@pytest.mark.parametrize("n_items", [1, 119, 120, 121, 240, 241])
def test_direct_copy_at_table_edges(n_items):
    c = _Copy(_dev(), item_sizes(n_items), seed=n_items)
    assert c.run() == 0
    assert torch.equal(_bits(c.dst.cpu()), _bits(c.expected()))          # every slot, and both guards
    assert torch.equal(_bits(c.src.cpu()), _bits(c.src_host))


def test_every_block_edge_size_is_in_the_direct_tables():
    sizes = item_sizes(241)
    assert set(EDGE_SIZES) <= set(sizes) and [sizes[i] for i in (0, 119, 120, 239, 240)] == [2049] * 5
    assert set(EDGE_SIZES) <= set(item_sizes(119))


@pytest.mark.parametrize("bad,what", [(122, "null src"), (121, "numel 0"), (120, "null dst")])
def test_a_bad_item_of_the_second_launch_is_refused_by_its_index(bad, what):
    """The item's index is in ``mkgnn_last_error``; its slot and every later one keep their bytes, and so do the guards."""
    c = _Copy(_dev(), item_sizes(125), seed=7)
    if what == "null src":
        c.table[bad].src = None
    elif what == "null dst":
        c.table[bad].dst = None
    else:
        c.table[bad].numel = 0
    assert c.run() != 0
    assert f"item {bad}:".encode() in c.lib.mkgnn_last_error()
    got = c.dst.cpu()
    lo = c.doff[bad]
    assert torch.equal(_bits(got[lo:]), _bits(torch.full((got.numel() - lo,), SENTINEL)))
    assert torch.equal(_bits(got[:GUARD]), _bits(torch.full((GUARD,), SENTINEL)))
    # what the launch before it wrote is exactly its items
    assert torch.equal(_bits(got[:c.doff[120]]), _bits(c.expected(upto=120)[:c.doff[120]]))


def _param_sizes():
    sizes = [1 + (7 * i) % 5 for i in range(130)]
    for i in (4, 50, 125):
        sizes[i] = 0
    for i in (0, 60, 119, 120, 121, 129):
        sizes[i] = 2049
    sizes[30], sizes[90] = 1025, 1023
    return sizes


def test_fill_of_more_than_120_parameters_is_foreach_copy_bit_for_bit():
    """``FlatGradAllReduce._fill``: 130 parameters (three of them empty) and the flags make 128 items, two launches; ``None`` gradients
    -- some on 2049-element parameters -- are filled from the resident zeros; the same pattern a second time takes the cached table."""
    from molkgnn_amd import dp
    dev = _dev()
    torch.manual_seed(11)
    params = [torch.nn.Parameter(torch.randn(n, device=dev)) for n in _param_sizes()]
    red = dp.FlatGradAllReduce(params)
    assert len(red.params) == 130
    used = []
    hip = red._hip_copy
    counted = lambda d, s: (used.append(1), hip(d, s))[1]                  # noqa: E731

    def fill(grads, native):
        red._buf.fill_(7.0)                                  # (a slot without a gradient must be zeroed, a flag written)
        red._hip_copy = counted if native else (lambda d, s: False)
        red._fill(grads)
        torch.cuda.synchronize()
        return red._buf.clone()
    none_a, none_b = (0, 7, 60, 120, 128), (1, 119, 121, 129)
    static = [torch.empty_like(p) for p in red.params]       # (a step's gradients live in the same tensors: the table is keyed by pointers)
    for rnd, none in enumerate((none_a, none_a, none_b)):
        grads = [None if i in none else g.normal_() for i, g in enumerate(static)]
        got = fill(grads, True)
        assert len(used) == rnd + 1, "the HIP copy was not taken"
        assert len(red._copy_tables) == (1 if rnd < 2 else 2)
        want = fill(grads, False)
        assert torch.equal(_bits(got), _bits(want)), rnd
        assert red.flags.tolist() == [0.0 if i in none else 1.0 for i in range(130)]
        for i in none:
            assert float(red.views[i].abs().max()) == 0.0
        assert all(torch.equal(v, g) for v, g in zip(red.views, grads) if g is not None)
