"""The float64 AdamW reference of ``tests/_adamw_f64.py`` checked WITHOUT a GPU: against ``torch.optim.AdamW`` run on float64
parameters over the hyper-parameter grid of ``tests/test_adamw_f64.py``, that a skipped tensor's state stands still, and what
carrying the hyper-parameters as float32 costs.  A wrong reference would bless a wrong kernel; this is what keeps it right."""
import math

import pytest
import torch

from tests import _adamw_f64 as A

REL = 1e-12
SIZES = [3, 1025, 1, 5, 257, 2]
STEPS = 12


def _close(a, b, tag):
    a, b = a.detach().double().reshape(-1), b.detach().double().reshape(-1)
    assert a.shape == b.shape, tag
    err, scale = float((a - b).abs().max()), max(float(b.abs().max()), 1e-300)
    assert err <= REL * scale, (tag, err, scale)


def _same_trajectory(group_of, groups, grads, active=None, state0=None, tag=""):
    params0 = A.make_params(SIZES, seed=21)
    ps, sts = A.run_f64(params0, group_of, groups, grads, active, state0)
    pt, stt = A.run_torch(params0, group_of, groups, grads, active, state0, dtype=torch.float64)
    for i in range(len(SIZES)):
        _close(ps[i], pt[i], (tag, "param", i))
        _close(sts[i].exp_avg, stt[i].exp_avg, (tag, "exp_avg", i))
        _close(sts[i].exp_avg_sq, stt[i].exp_avg_sq, (tag, "exp_avg_sq", i))
        assert sts[i].step == stt[i].step, (tag, "step", i)
    return ps, sts


@pytest.mark.parametrize("rounded", [False, True])
@pytest.mark.parametrize("edge", sorted(A.HYPER_EDGES))
def test_reference_is_torch_adamw_in_float64_at_every_hyper_parameter_edge(edge, rounded):
    G = A.HYPER_EDGES[edge]
    groups = [A.as_launched(G) if rounded else G]
    grads = A.make_grads(SIZES, STEPS, seed=5)
    ps, sts = _same_trajectory([0] * len(SIZES), groups, grads, tag=edge)
    assert all(st.step == STEPS for st in sts)
    if edge == "lr_0_weight_decay_0":
        assert all(torch.equal(p, q.double()) for p, q in zip(ps, A.make_params(SIZES, seed=21)))
        assert all(float(st.exp_avg.abs().max()) > 0.0 and float(st.exp_avg_sq.abs().max()) > 0.0 for st in sts)


@pytest.mark.parametrize("rounded", [False, True])
def test_reference_is_torch_adamw_in_float64_over_four_groups_with_a_moving_lr(rounded):
    groups = A.launched(A.four_groups_at) if rounded else A.four_groups_at
    grads = A.make_grads(SIZES, STEPS, seed=6)
    for s in (1, 4, 5):                                    # tensors without a gradient on some steps
        grads[s][1] = None
        grads[s][3] = None
    _, sts = _same_trajectory([i % 4 for i in range(len(SIZES))], groups, grads, tag="four groups")
    assert [st.step for st in sts] == [12, 9, 12, 9, 12, 12]


def test_reference_resumes_a_state_at_a_large_step_count():
    moments = A.make_moments(SIZES, seed=8)
    state0 = [(m, v, 1_000_000) for m, v in moments]
    grads = A.make_grads(SIZES, 2, seed=9)
    _, sts = _same_trajectory([0] * len(SIZES), [A.as_launched(A.group(lr=2e-3))], grads, state0=state0, tag="resumed")
    assert all(st.step == 1_000_002 for st in sts)
    assert A.bias_corrections_fp32((A.fp32(0.9), A.fp32(0.999)), 1_000_001) == (1.0, 1.0)


def test_a_skipped_tensor_stands_still():
    """None gradient or an active flag of 0: parameter, both moments and the step count are bit-identical across the step; the
    others move.  The flags are the same as None gradients to ``torch.optim.AdamW``."""
    grads = A.make_grads(SIZES, 6, seed=10)
    active = [[1.0] * len(SIZES) for _ in range(6)]
    active[2][1] = 0.0
    active[3][1] = 0.0
    active[3][4] = 0.0
    grads[4][0] = None
    groups = [A.group(lr=1e-2, weight_decay=0.1)]
    snaps = A.run_f64(A.make_params(SIZES, seed=21), [0] * len(SIZES), groups, grads, active, snapshots=True)
    skipped = {(2, 1), (3, 1), (3, 4), (4, 0)}
    for s in range(1, 6):
        (p0, s0), (p1, s1) = snaps[s - 1], snaps[s]
        for i in range(len(SIZES)):
            same = torch.equal(p0[i], p1[i]) and torch.equal(s0[i].exp_avg, s1[i].exp_avg) and torch.equal(s0[i].exp_avg_sq, s1[i].exp_avg_sq)
            if (s, i) in skipped:
                assert same and s1[i].step == s0[i].step, (s, i)
            else:
                assert not same and s1[i].step == s0[i].step + 1, (s, i)
    assert [st.step for st in snaps[-1][1]] == [5, 4, 6, 6, 5, 6]
    _same_trajectory([0] * len(SIZES), groups, grads, active, tag="skipped")


def test_one_step_by_hand():
    """The definition on one element, written out: p = 2, g = 3 scaled by 1/2 and maximised."""
    G = A.group(lr=0.1, betas=(0.5, 0.75), eps=0.25, weight_decay=0.5, maximize=True, grad_scale=0.5)
    p, st = torch.tensor([2.0], dtype=torch.float64), A.State((1,))
    A.step([(p, torch.tensor([3.0]), 0)], [G], [st])
    g = -1.5
    m, v = 0.5 * g, 0.25 * g * g
    want = 2.0 * (1 - 0.1 * 0.5) - 0.1 * (m / 0.5) / (math.sqrt(v / 0.25) + 0.25)
    assert st.step == 1 and float(st.exp_avg) == m and float(st.exp_avg_sq) == v
    assert abs(float(p) - want) <= 1e-15 * abs(want)


def test_what_float32_hyper_parameters_cost():
    """Why the GPU module hands every leg the float32 values: ``mkgnn_adamw_group`` carries beta2 as a float32, and ``1 - fp32(0.999)``
    is 1.29e-5 away from 0.001 relatively -- the first ``exp_avg_sq`` of ANY float32-carried 0.999 is that far from the one of the
    decimal 0.999, most of ``_f64.R`` = 1.53e-5, whatever the arithmetic after it."""
    g = torch.tensor([3.0])
    a, b = A.State((1,)), A.State((1,))
    A.step([(torch.zeros(1, dtype=torch.float64), g, 0)], [A.group()], [a])
    A.step([(torch.zeros(1, dtype=torch.float64), g, 0)], [A.as_launched(A.group())], [b])
    rel = abs(float(b.exp_avg_sq) - float(a.exp_avg_sq)) / float(a.exp_avg_sq)
    assert 1.2e-5 < rel < 1.4e-5
    assert A.state_floats(1) == 6 and A.state_floats(1024) == 2052 and A.state_floats(1025) == 2055


def test_the_tables_of_the_gpu_module():
    for n in (1, 79, 80, 81, 160, 161):
        sizes = A.table_sizes(n)
        assert len(sizes) == n and all(1 <= k <= 5 or k in (1025, 2049) for k in sizes)
        assert [i for i, k in enumerate(sizes) if k > 5] == [p for p in (0, 79, 80, 159, 160) if p < n]
    sizes = A.table_sizes(161)
    assert (sizes[79], sizes[80], sizes[159], sizes[160]) == (1025, 2049, 1025, 2049)
    # pairwise different in every field
    for k in ("lr", "betas", "eps", "weight_decay", "grad_scale"):
        assert len({str(G[k]) for G in A.FOUR_GROUPS}) == 4, k
    assert sorted(G["maximize"] for G in A.FOUR_GROUPS) == [False, False, True, True]
    grads = A.make_grads([5, 1025], 4, seed=1)
    mags = sorted({round(math.log10(float(t.abs().max()))) for row in A.make_grads([4097] * 10, 10, seed=1) for t in row})
    assert mags[0] <= -5 and mags[-1] >= 3
    assert all(float(row[1][512]) == 0.0 for row in grads) and float(grads[1][0][0]) == 0.0 and float(grads[0][0][0]) != 0.0
