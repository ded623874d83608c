"""The case table of the any-shape convolution kernels' float64 leg (tests/_conv_f64.py), checked without a GPU: every case
reaches the edge it is named for, and the yardstick passes its own test -- the fp32 oracle (autograd of the reference-faithful
form at its own permutation choices) lies within the per-element bound of the float64 closed form on every case, before a
kernel is asked to."""
import pytest
import torch

from tests import _conv_f64 as C

NAMES = [c.name for c in C.CASES]
SMALL = [c.name for c in C.CASES if c.oracle_on_cpu]


def test_the_table_holds_every_edge_of_the_issue():
    """Both sides of every width / count / chunk threshold the kernels branch on are in the table."""
    widths = sorted(c.F for c in C.CASES if c.edge == "row width")
    assert widths == [1, 2, 3, 63, 64, 65, 127, 128, 129, 160, 161, 191, 192, 193, 255, 256]
    assert all(c.E == 7 and c.counts == (3, 2, 4, 2) for c in C.CASES if c.edge == "row width")
    for k in range(6):                                   # every branch has widths on both of its sides (part[8][256]: F = 256 itself)
        sides = {C.WIDTH_SIDES[F][k] for F in widths}
        assert sides == ({True} if k == 4 else {True, False}), k
    assert sorted((c.E, c.F) for c in C.CASES if c.edge == "bond width") == sorted((E, F) for E in (1, 8, 9, 63, 64) for F in (20, 129))
    counts = {(c.counts, c.F) for c in C.CASES if c.edge == "kernel counts"}
    for F in (5, 130):
        assert {((63, 64, 65, 6), F), ((129, 1, 0, 17), F), ((0, 0, 0, 5), F), ((1, 1, 1, 1), F)} <= counts
    assert sorted(c.counts[3] for c in C.CASES if c.name.startswith("table_l4_") and c.last) == [5, 6, 16, 17]
    assert [c.name for c in C.CASES if c.edge == "the grid-stride loop"] == ["grid_stride_last0", "grid_stride_last1"]
    assert sorted(c.F for c in C.CASES if c.edge == "the clamp") == [129, 256]
    assert sorted(c.F for c in C.CASES if c.edge == "chirality at width") == [65, 129, 256]
    assert all(c.bound == C.F64_BOUND for c in C.CASES)  # (no case needed a constant of its own)


@pytest.mark.parametrize("name", NAMES)
def test_case_reaches_its_edge(name):
    built = C.build(name)
    info = built.info
    assert built.case.proves(info), (name, vars(info))
    assert built.x.shape == (sum(info.n), built.case.F) and built.cot.shape == (sum(info.n), sum(built.case.counts))
    for d in range(1, 5):
        e = getattr(built.cpu, f"nei_edge_attr_deg{d}")
        assert e.numel() == info.n[d - 1] * d * built.case.E
    # no row anywhere near the epsilon: the fp32 clamp flag and the float64 oracle's agree by construction
    assert info.margins_ok, name
    assert (info.clamped_rows > 0) == (built.case.tweak == "clamp"), (name, info.clamped_rows)
    if built.case.edge != "the grid-stride loop":         # the only case above about 1 500 atoms
        assert built.case.oracle_on_cpu and sum(info.n) <= 1500, sum(info.n)


@pytest.mark.parametrize("name", SMALL)
def test_fp32_oracle_is_within_the_bound_of_the_float64_oracle(name):
    built = C.build(name)
    idx = C.oracle_choices(built)
    gx, grads = C.oracle_gradients_fp32(built, idx)
    oracle = C.oracle_gradients_f64(built, idx)
    assert torch.isfinite(oracle[0]).all() and torch.isfinite(gx).all()
    worst = C._check_gradients_f64(gx, grads, oracle, name, bound=built.case.bound, expect=C.expected_gradients(built))
    print(f"{name}: fp32 oracle worst err / lim = {worst:.3f}")
    # ... and the three scores a kernel keeps, by the network-level bound's own form (the fp32 oracle is its yardstick: trivially
    # within it here; what this pins is that the float64 evaluation exists for every degree that has atoms and kernels)
    s32, s64 = C.pair_scores(built, idx, torch.float32), C.pair_scores(built, idx, torch.float64)
    for d in range(4):
        has = built.info.n[d] > 0 and built.info.counts[d] > 0
        assert (s64[d] is not None) == has and (s32[d] is not None) == has
        if has and built.case.last and d == 3:
            assert torch.equal(s32[d]["chirality"].double(), s64[d]["chirality"])
