"""Float64 reference of ``torch.nn.BatchNorm1d`` on a 2-D input, written from the definition, and the input families the batch
norm kernels (``csrc/kgnn_batchnorm.hip``: ``bn_block_stats``, ``bn_total_m2``, ``bn_pass_vec`` / ``bn_pass_col``, the
statistics-only companion) are fed in ``tests/test_batch_norm_f64.py``.  CPU only: nothing here imports the package.

The fp32 inputs are cast up exactly, so ``reference`` is the exact answer *for the inputs the kernel saw* (up to float64
rounding, 2^-53 per operation).  ``tests/test_bn_reference_cpu.py`` pins it to ``torch.nn.BatchNorm1d`` run in float64.
"""
from __future__ import annotations

import math

import numpy as np
import torch

ROW_EPS = 1e-8          # torch.nn.CosineSimilarity's clamp (MKGNN_EPS): inv_norm = 1 / max(|row|, ROW_EPS)
BN_BLOCKS = 256         # blocks of the batch norm's own passes (kgnn_batchnorm.hip BN_MAIN_BLOCKS)


def _f64(t):
    return None if t is None else t.detach().cpu().to(torch.float64)


def reference(x, weight, bias, running_mean, running_var, momentum, eps, training, n_valid=None, cot=None):
    """Batch norm of ``x`` [n, C] in float64 on the CPU -> dict of ``out, save_mean, save_invstd, running_mean, running_var,
    grad_x, grad_weight, grad_bias, inv_norm`` (gradients only with a cotangent ``cot`` of ``out``; ``None`` where an input is
    ``None``).  ``training``: batch statistics (mean and BIASED variance over the counted rows; the running buffers move by
    ``momentum`` towards the batch mean and the UNBIASED variance); else the running buffers are the statistics and stand still.
    ``running_mean=None`` with ``training``: batch statistics, no buffers.  ``save_invstd = 1 / sqrt(var + eps)``;
    ``inv_norm = 1 / max(|out row|, 1e-8)``.

    ``n_valid`` (padded batches): only rows ``[0, n_valid)`` are counted; the padding rows behind them are normalised with the
    same statistics.  The cotangent is taken as ZERO on the padding rows -- that is what a padded step guarantees: padding atoms
    belong to molecules the loss leaves out -- so ``grad_weight`` / ``grad_bias`` are sums over the counted rows and ``grad_x``
    of a padding row is zero here.  The kernels promise nothing about ``grad_x`` of padding rows (no reader exists): compare
    ``grad_x[:n_valid]`` only."""
    x64 = _f64(x).requires_grad_(cot is not None)
    n, C = x64.shape
    nv = n if n_valid is None else int(n_valid)
    assert 1 <= nv <= n
    w = None if weight is None else _f64(weight).requires_grad_(cot is not None)
    b = None if bias is None else _f64(bias).requires_grad_(cot is not None)
    rm, rv = _f64(running_mean), _f64(running_var)
    if training:
        xc = x64[:nv]
        mean = xc.sum(0) / nv
        var = ((xc - mean) ** 2).sum(0) / nv
        if rm is not None:
            rm = rm + momentum * (mean.detach() - rm)
        if rv is not None:
            unbiased = var.detach() * (nv / (nv - 1.0)) if nv > 1 else var.detach()
            rv = rv + momentum * (unbiased - rv)
    else:
        mean, var = rm, rv
    invstd = 1.0 / torch.sqrt(var + eps)
    out = (x64 - mean) * invstd
    if w is not None:
        out = out * w
    if b is not None:
        out = out + b
    res = {"out": out.detach(), "save_mean": mean.detach(), "save_invstd": invstd.detach(), "running_mean": rm, "running_var": rv,
           "grad_x": None, "grad_weight": None, "grad_bias": None,
           "inv_norm": 1.0 / out.detach().norm(dim=1).clamp_min(ROW_EPS)}
    if cot is not None:
        c64 = _f64(cot).clone()
        c64[nv:] = 0.0
        (out * c64).sum().backward()
        res["grad_x"] = x64.grad
        res["grad_weight"] = None if w is None else w.grad
        res["grad_bias"] = None if b is None else b.grad
    return res


def masked_statistics(x, keep, running_mean, running_var, momentum):
    """The statistics-only companion in float64: what ``bn(x[keep])`` does to the running buffers in training mode (``keep``: a
    boolean row mask or ``None``).  Fewer than two counted rows: nothing moves (BatchNorm1d raises; ``bn_side_final`` leaves the
    buffers and the counter where they are).  -> (running_mean, running_var, moved)"""
    x64 = _f64(x)
    if keep is not None:
        x64 = x64[keep.cpu()]
    rm, rv = _f64(running_mean), _f64(running_var)
    cnt = x64.shape[0]
    if cnt < 2:
        return rm, rv, False
    mean = x64.sum(0) / cnt
    unbiased = ((x64 - mean) ** 2).sum(0) / (cnt - 1.0)
    return rm + momentum * (mean - rm), rv + momentum * (unbiased - rv), True


# ------------------------------------------------------------------------------------------- input families --
def plain(n, C, g):
    """The existing tests' input: well-conditioned."""
    return torch.randn(n, C, generator=g) * 3 + 1.5


def offset(n, C, g):
    """|mean| >> std: 1e3 against 1e-1 (the fp32 merge ``cnt * d * d`` works on differences of numbers with an ulp of 6e-5)."""
    return (torch.randn(n, C, generator=g, dtype=torch.float64) * 0.1 + 1e3).float()


def sorted_columns(n, C, g):
    """Every column ascending: block means differ as much as they can (atoms ARE sorted by molecule)."""
    return plain(n, C, g).sort(dim=0).values.contiguous()


def scales(n, C, g):
    """Column c scaled by 10 ** linspace(-6, 6): magnitudes 1e-6 .. 1e+6 side by side."""
    s = torch.tensor(10.0 ** np.linspace(-6.0, 6.0, C), dtype=torch.float64)
    return (torch.randn(n, C, generator=g, dtype=torch.float64) * s).float()


def spike(n, C, g):
    """Zero except for one row per column."""
    x = torch.zeros(n, C)
    rows = torch.randint(0, n, (C,), generator=g)
    x[rows, torch.arange(C)] = 1.0
    return x


DYADIC = (0.5, 3.0, -1.25, 2.0, -0.75, 6.0, 0.125, -5.0)


def constant_exact(n, C, g=None):
    """Every column one dyadic value (at most three significant bits): every partial sum a kernel can form is j * v with j <= n
    <= 2^21, exact in fp32, so every mean is exactly v, the variance exactly 0 and the normalised column exactly ``bias``."""
    v = torch.tensor([DYADIC[c % len(DYADIC)] for c in range(C)])
    return v.repeat(n, 1).contiguous()


def mean_rows_zero_rows(n):
    """The all-zero rows of ``mean_rows(n, ...)``: three or four (so that the others are an even number), spread over the rows."""
    assert n >= 8
    z = 4 if n % 2 == 0 else 3
    return [(k * n) // z + n // (2 * z) for k in range(z)]


def mean_rows(n, C, g):
    """Every column as many +1 as -1 in shuffled rows, plus a few all-zero rows: every fp32 partial sum is a small integer, the
    batch mean exactly 0; with bias 0 the zero rows come out as exactly zero rows (``inv_norm`` at its clamp, 1 / 1e-8)."""
    zero = mean_rows_zero_rows(n)
    live = torch.tensor([r for r in range(n) if r not in set(zero)], dtype=torch.int64)
    m = live.numel()
    assert m % 2 == 0 and m >= 2, (n, zero)
    x = torch.zeros(n, C)
    half = torch.cat([torch.ones(m // 2), -torch.ones(m // 2)])
    for c in range(C):
        x[live, c] = half[torch.randperm(m, generator=g)]
    return x


FAMILIES = {"plain": plain, "offset": offset, "sorted": sorted_columns, "scales": scales, "spike": spike,
            "constant_exact": constant_exact, "mean_rows": mean_rows}


def make(family, n, C, seed=0):
    g = torch.Generator().manual_seed(1000 * seed + 7 * n + C)
    return FAMILIES[family](n, C, g)


def shares(nv, nblk=BN_BLOCKS):
    """``bn_share``: the counted rows [0, nv) dealt to ``nblk`` blocks in equal runs of ceil(nv / nblk) -> [(lo, hi)]."""
    per = (nv + nblk - 1) // nblk
    out = []
    for b in range(nblk):
        lo = per * b
        hi = min(lo + per, nv)
        out.append((min(lo, hi), hi))
    return out


def fp32_inv_clamp():
    """``1.f / 1e-8f`` as fp32 arithmetic gives it: the handed norm of a zero row."""
    return float(np.float32(1.0) / np.float32(ROW_EPS))


assert math.isfinite(fp32_inv_clamp())
