// The batch norm in front of the kernel-convolution stack (the readout behind it: kgnn_readout.hip):
//
//   batch norm  BatchNorm1d over the atom rows                      reference MolKGNNNet.py:115
//
// Batch norm.  Tall and skinny ([1e5, 28]): three short launches (column sums, centred squares, apply),
// every block re-deriving the column statistics from the per-block partials in a fixed order.
#include <hip/hip_runtime.h>
#include <atomic>
#include <cstdint>
#include <cstdlib>
#include "kgnn_common.h"

#include "kgnn_launch.h"
#include "kgnn_prepare.h"
#include "kgnn_split.h"
#include "../../include/molkgnn_hip.h"

namespace mkgnn {

typedef mkgnn_f32x4 f32x4;

// ------------------------------------------------------------------------------------ batch norm ----
// Statistics-only companion of a batch norm (mkgnn_bn_stats): the reference runs edge_batch_norm(data.edge_attr) in every
// forward (MolKGNNNet.py:116) although its output never reaches the kernel convolution; what remains of the
// call is its side effect in training mode -- running_mean / running_var / num_batches_tracked move.  The rows are summed
// by extra blocks of the node batch norm's own two launches (no launch of their own in a step), or by
// mkgnn_batchnorm_update_stats alone.  part: [3][nblk][C] = column sums | squares about the block's own means | counted rows.
#ifndef MKGNN_BN_BLOCKS                  // (A/B builds)
#define MKGNN_BN_BLOCKS 256
#endif
// Attribution builds (their results are WRONG, they exist to be timed): make VARIANT=... EXTRA=-DMKGNN_BN_AB=n with
// 1: the apply launch takes the saved statistics instead of merging the partials; 2: the apply launch without its row pass;
// 3: the statistics launch without pass B
#ifndef MKGNN_BN_AB
#define MKGNN_BN_AB 0
#endif
constexpr int BN_MAIN_BLOCKS = MKGNN_BN_BLOCKS;       // (= BN_BLOCKS: the grid of the batch norm's own passes)
constexpr int BN_SIDE_BLOCKS = 1024;                   // companion blocks at most (one loop trip per pass each where that is enough)
struct BnSide {
    const float* x; int64_t xs; int64_t n; int C, CL, nblk;
    int flat;                                          // contiguous narrow rows: the 16-byte form (bn_side_block_stats_flat)
    float *running_mean, *running_var; float momentum;
    int64_t* nbt;
    const int64_t* key; const int64_t* key_limit;      // both or neither: row r counts iff key[r] < *key_limit
    float* part;
    int merge;                                         // the totals from one set of loads where they fit (bn_merge_on)
};

struct BnArgs {
    const float* x; int64_t xs; int64_t n; int C;
    const float *weight, *bias;
    float *running_mean, *running_var;
    float momentum, eps; int training;
    float* out; int64_t os;
    float *save_mean, *save_invstd;
    float* part1; float* part2;    // [nblk, C] each
    float* part3;                  // forward statistics: the blocks' residual sums about their own (rounded) means
    // backward
    const float* gout; int64_t gos;
    float* gx; int64_t gxs;
    float *gweight, *gbias;
    float* inv_out;                // forward: 1 / max(|out row|, eps) for the convolution that reads out next (17 <= C <= 32)
    int split_out;                 // ... and the rows themselves written PRE-SPLIT for it (kgnn_split.h; MKGNN_BN_SPLIT_ROWS)
    int touch_first;               // blocks from here on of the statistics launch read `touch` and throw it away (mkgnn_touch_hint)
    TouchArgs touch;
    int64_t* nbt;                  // forward, training: BatchNorm1d.num_batches_tracked, incremented
    const int64_t* nvalid;         // device scalar or null: only rows [0, *nvalid) enter the batch statistics (padded batches)
    int merge;                     // the block partials merged out of registers where they fit (bn_merge_on; 0: the loop form)
    BnSide side;                   // statistics-only companion (blocks gridDim.x - side.nblk .. of the same launches); nblk = 0: none
};

// blocks that work on the batch norm's own rows: the grid, less the companion's extra blocks (BnSide) behind them
__device__ __forceinline__ int bn_nblk() { return (int)gridDim.x < BN_MAIN_BLOCKS ? (int)gridDim.x : BN_MAIN_BLOCKS; }

// rows that count for the statistics: all of them, or the leading *nvalid (the rest is padding: normalised like any
// row, excluded from every sum)
__device__ __forceinline__ int64_t bn_valid(const BnArgs& a) {
    if (!a.nvalid) return a.n;
    const int64_t v = *a.nvalid;
    return v < 1 ? 1 : (v < a.n ? v : a.n);
}

// rows of this block: [lo, hi)
__device__ __forceinline__ void bn_rows(const BnArgs& a, int64_t& lo, int64_t& hi) {
    const int64_t per = (a.n + bn_nblk() - 1) / bn_nblk();
    lo = per * blockIdx.x;
    hi = lo + per < a.n ? lo + per : a.n;
    if (lo > hi) lo = hi;
}

// ---- round 6: statistics in ONE launch, 16-byte row passes ------------------------------------------------------------------
// Rounds 1-5 took the batch statistics in two launches (column sums; then, with the batch mean known, centred squares) and
// applied them in a third; every row pass was 4-byte loads, eight in flight per thread -- 8.6 + 8.9 + 14.2 us for an 11.5 MB
// tensor at batch 4096, bound by load latency times loop trips.  Now a block sums its share of the counted rows (pass A), takes
// ITS OWN mean, and sums the squares about that (pass B: the rows the block has just pulled into L2).  The batch statistics
// follow exactly from the block triples (count_b, sum_b, M2_b):
//     mean = (sum_b sum_b) / n,     M2 = sum_b [ M2_b + count_b (sum_b / count_b - mean)^2 ]          (Chan, Golub, LeVeque 1979)
// evaluated in a fixed order by every block of the apply launch -- centred sums throughout, like the two-pass form over the
// whole batch it replaces; one launch less, and the mean itself is bit for bit the old one (the same partial sums).  Rows that
// are 16-byte aligned with C a multiple of 4 are read as float4, BN_U rows in flight per thread.
constexpr int BN_U = 16;                               // float4 row loads in flight per thread (statistics passes)
constexpr int BN_UA = 8;                               // ... in the passes that also write rows

__device__ __forceinline__ float bn_shfl_xor(float v, int o) { return __shfl_xor(v, o, 64); }
__device__ __forceinline__ f32x4 bn_shfl_xor(f32x4 v, int o) {
    return f32x4{__shfl_xor(v[0], o, 64), __shfl_xor(v[1], o, 64), __shfl_xor(v[2], o, 64), __shfl_xor(v[3], o, 64)};
}
__device__ __forceinline__ void bn_zero(float& v) { v = 0.f; }
__device__ __forceinline__ void bn_zero(f32x4& v) { v = f32x4{0.f, 0.f, 0.f, 0.f}; }

// Sum of v over the threads of the block that share threadIdx.x % LW (LW a power of two, 1 .. 256), in a fixed order: an xor
// tree over the lanes of a wave, then the waves (or row lanes) in ascending order.  Valid in threads < LW.  shv: 256 V's.
template <typename V> __device__ __forceinline__ V bn_reduce_rows(V v, int LW, V* shv) {
    const int t = threadIdx.x;
    for (int o = 32; o >= LW; o >>= 1) v = v + bn_shfl_xor(v, o);
    __syncthreads();                                     // (shv may still be read from an earlier reduction)
    int parts;
    if (LW <= 64) {
        if ((t & 63) < LW) shv[(t >> 6) * LW + (t & 63)] = v;
        parts = 4;
    } else {
        shv[t] = v;
        parts = 256 / LW;
    }
    __syncthreads();
    V r;
    bn_zero(r);
    if (t < LW)
        for (int k = 0; k < parts; ++k) r = r + shv[k * LW + t];
    return r;
}

// rows of block b of nblk, the counted rows [0, nv) dealt in equal runs: [lo, hi)
__device__ __forceinline__ void bn_share(int64_t nv, int nblk, int b, int64_t& lo, int64_t& hi) {
    const int64_t per = (nv + nblk - 1) / nblk;
    lo = per * b;
    hi = lo + per < nv ? lo + per : nv;
    if (lo > hi) lo = hi;
}

// One pass over rows [lo, hi) of x (and g): per-thread partial sums.  MODE 0: s0 += x;  1: s0 += (x - mu)^2, s1 += x - mu;  2: s0 += g,
// s1 += g (x - mu) is.  VEC: thread = (row lane rsub of RS, column group col .. col + 3), float4 loads; else one column c.
// All loads of a trip are issued before anything is consumed (clamped addresses, masked use).
template <int MODE, int U>
__device__ __forceinline__ void bn_pass_vec(const float* x, int64_t xs, const float* g, int64_t gs, int64_t lo, int64_t hi, int rsub, int RS,
                                            int col, f32x4 mu, f32x4 is, f32x4& s0, f32x4& s1) {
    for (int64_t r0 = lo + rsub; r0 < hi; r0 += (int64_t)U * RS) {
        f32x4 v[U], gg[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t rr = r0 + (int64_t)u * RS < hi ? r0 + (int64_t)u * RS : hi - 1;
            v[u] = *(const f32x4*)(x + rr * xs + col);
            if (MODE == 2) gg[u] = *(const f32x4*)(g + rr * gs + col);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (r0 + (int64_t)u * RS < hi) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    if (MODE == 0) s0[e] += v[u][e];
                    if (MODE == 1) { const float d = v[u][e] - mu[e]; s0[e] = fmaf(d, d, s0[e]); s1[e] += d; }
                    if (MODE == 2) { s0[e] += gg[u][e]; s1[e] = fmaf(gg[u][e], (v[u][e] - mu[e]) * is[e], s1[e]); }
                }
            }
        }
    }
}
template <int MODE>
__device__ __forceinline__ void bn_pass_col(const float* x, int64_t xs, const float* g, int64_t gs, int64_t lo, int64_t hi, int rsub, int RS,
                                            int c, float mu, float is, float& s0, float& s1) {
    for (int64_t r0 = lo + rsub; r0 < hi; r0 += 8 * RS) {
        float v[8], gg[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int64_t rr = r0 + u * RS < hi ? r0 + u * RS : hi - 1;
            v[u] = x[rr * xs + c];
            if (MODE == 2) gg[u] = g[rr * gs + c];
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            if (r0 + u * RS < hi) {
                if (MODE == 0) s0 += v[u];
                if (MODE == 1) { const float d = v[u] - mu; s0 = fmaf(d, d, s0); s1 += d; }
                if (MODE == 2) { s0 += gg[u]; s1 = fmaf(gg[u], (v[u] - mu) * is, s1); }
            }
        }
    }
}

// can the rows of a [*, C] tensor be read as float4?
static inline bool bn_vec_rows(const void* p, int64_t stride, int C) { return p && C % 4 == 0 && stride % 4 == 0 && ((uintptr_t)p & 15) == 0; }

// Forward statistics of block blockIdx.x: part1[b][c] = column sums of its counted rows, part2[b][c] = squares about the
// block's own column means, part3[b][c] = the sum of the same centred values.  The block's mean is an fp32 number: for a column
// with |mean| >> std (1e3 against 1e-1) it is off the true block mean by up to half an ulp of the MEAN, and that sum -- zero for the
// true mean -- is what the merge needs to stay exact about the pivot actually used (bn_total_m2).  sh: 1024 floats.
template <bool VEC>
__device__ __forceinline__ void bn_block_stats(const BnArgs& a, int CL, float* sh) {
    __shared__ float bmean[256];
    const int t = threadIdx.x;
    int64_t lo, hi;
    // the block's share of the rows that COUNT (not of all rows): the partial sums, and with them the statistics, are then
    // bit for bit those of the same batch without its padding rows -- a padded batch (molkgnn_amd.padding) reproduces the
    // unpadded forward exactly, which matters more than it looks: an ulp in x decides thousands of mathematically tied
    // neighbour orders the other way two layers later
    bn_share(bn_valid(a), bn_nblk(), blockIdx.x, lo, hi);
    const float cnt = (float)(hi - lo);
    float* const p1 = a.part1 + (int64_t)blockIdx.x * a.C;
    float* const p2 = a.part2 + (int64_t)blockIdx.x * a.C;
    float* const p3 = a.part3 + (int64_t)blockIdx.x * a.C;
    if constexpr (VEC) {
        const int LW = CL >= 4 ? CL / 4 : 1, g = t % LW, rsub = t / LW, RS = 256 / LW, col = 4 * g;
        const bool act = col < a.C;
        const int cb = act ? col : 0;
        const f32x4 z = {0.f, 0.f, 0.f, 0.f};
        f32x4 s0 = z, s1 = z;
        bn_pass_vec<0, BN_U>(a.x, a.xs, nullptr, 0, lo, hi, rsub, RS, cb, z, z, s0, s1);
        const f32x4 tot = bn_reduce_rows(s0, LW, (f32x4*)sh);
        if (t < LW && act) {
#pragma unroll
            for (int e = 0; e < 4; ++e) { p1[col + e] = tot[e]; bmean[col + e] = cnt > 0.f ? tot[e] / cnt : 0.f; }
        }
        __syncthreads();
        const f32x4 mu = {bmean[cb], bmean[cb + 1], bmean[cb + 2], bmean[cb + 3]};
        s0 = z;
        if (MKGNN_BN_AB != 3) bn_pass_vec<1, BN_U>(a.x, a.xs, nullptr, 0, lo, hi, rsub, RS, cb, mu, z, s0, s1);
        const f32x4 m2 = bn_reduce_rows(s0, LW, (f32x4*)sh);
        const f32x4 m1 = bn_reduce_rows(s1, LW, (f32x4*)sh);
        if (t < LW && act) {
#pragma unroll
            for (int e = 0; e < 4; ++e) { p2[col + e] = m2[e]; p3[col + e] = m1[e]; }
        }
    } else {
        const int c = t & (CL - 1), rsub = t / CL, RS = 256 / CL;
        const bool act = c < a.C;
        const int cc = act ? c : 0;
        float s0 = 0.f, s1 = 0.f;
        bn_pass_col<0>(a.x, a.xs, nullptr, 0, lo, hi, rsub, RS, cc, 0.f, 0.f, s0, s1);
        const float tot = bn_reduce_rows(s0, CL, sh);
        if (t < CL && act) { p1[c] = tot; bmean[c] = cnt > 0.f ? tot / cnt : 0.f; }
        __syncthreads();
        const float mu = bmean[cc];
        s0 = 0.f;
        bn_pass_col<1>(a.x, a.xs, nullptr, 0, lo, hi, rsub, RS, cc, mu, 0.f, s0, s1);
        const float m2 = bn_reduce_rows(s0, CL, sh);
        const float m1 = bn_reduce_rows(s1, CL, sh);
        if (t < CL && act) { p2[c] = m2; p3[c] = m1; }
    }
}

// sum over blocks b of term(b, c) for every column c, identically in every block (fixed order), result in sh_out[c];
// sh: 256 floats
template <typename Term>
__device__ __forceinline__ void bn_total_of(int nblk, int C, int CL, float* sh, float* sh_out, Term&& term) {
    const int c = threadIdx.x & (CL - 1), rsub = threadIdx.x / CL, RS = 256 / CL;
    float s = 0.f;
    if (c < C) {
        // eight terms in flight (every block repeats this sum: serial loads made it the slowest part of the pass)
        float v[8], t[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        for (int b = rsub; b < nblk; b += 8 * RS) {
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = term(b + u * RS < nblk ? b + u * RS : b, c);
#pragma unroll
            for (int u = 0; u < 8; ++u) if (b + u * RS < nblk) t[u] += v[u];
        }
        s = ((t[0] + t[1]) + (t[2] + t[3])) + ((t[4] + t[5]) + (t[6] + t[7]));
    }
    __syncthreads();
    sh[threadIdx.x] = s;
    __syncthreads();
    if (rsub == 0 && c < C) {
        float t = 0.f;
        for (int k = 0; k < RS; ++k) t += sh[k * CL + c];
        sh_out[c] = t;
    }
    __syncthreads();
}
__device__ __forceinline__ void bn_total(const float* part, int nblk, int C, int CL, float* sh, float* sh_out) {
    bn_total_of(nblk, C, CL, sh, sh_out, [&](int b, int c) { return part[(int64_t)b * C + c]; });
}
// squares about the BATCH mean (mean[c]) out of the blocks' (count, sum, squares and sum about their own means).  With m_b the
// pivot block b used -- the fp32 quotient sum_b / count_b, formed here by the same division -- r_b = sum (x - m_b) and d = m_b - mean:
//     sum (x - mean)^2 = sum (x - m_b)^2 + 2 d r_b + count_b d^2 = M2_b + d (2 r_b + count_b d)
// exactly, whatever m_b is.  Without the r_b term (until this change) the rounding of m_b entered as 2 d r_b: 2e-5 of invstd for
// a column of 1e3 +- 1e-1 in shares of two rows, ten times what the bound of tests/test_batch_norm_f64.py allows.
__device__ __forceinline__ void bn_total_m2(const float* part1, const float* part2, const float* part3, int nblk, int64_t nv, int C, int CL,
                                            const float* mean, float* sh, float* sh_out) {
    const int64_t per = (nv + nblk - 1) / nblk;          // (one 64-bit division per thread, not one per term)
    const float mu = mean[(threadIdx.x & (CL - 1)) < C ? (threadIdx.x & (CL - 1)) : 0];
    bn_total_of(nblk, C, CL, sh, sh_out, [&](int b, int c) {
        int64_t left = nv - per * b;                     // rows of block b: what bn_share deals it
        left = left < 0 ? 0 : (left > per ? per : left);
        // (both loads unconditional: a load under a condition would be issued -- and waited for -- on its own, term after term)
        const float p1 = part1[(int64_t)b * C + c], p2 = part2[(int64_t)b * C + c], p3 = part3[(int64_t)b * C + c];
        const float cnt = (float)left;
        const float d = left > 0 ? p1 / cnt - mu : 0.f;  // (an empty block: nothing)
        return fmaf(d, fmaf(cnt, d, 2.f * p3), p2);
    });
}

// ---- the totals out of registers ---------------------------------------------------------------------------------------------
// bn_total_of asks memory for eight terms, waits, adds, and asks again; a second total starts when the first is through LDS.  At
// 256 blocks and CL = 32 that is four dependent trips per total, eight for the mean and the squares -- in every block of the apply
// launch, in front of its first row load, with nothing beside them to hide the latency.  Where a thread's terms are 8 KT <= 32
// (nblk * CL <= 8192) it holds them all: the loads of every plane are issued at once, and the sums are formed from the registers IN
// bn_total_of's ORDER -- accumulator t[u] takes the terms b = rsub + RS (u + 8 k) for k ascending, the eight combine as a tree, the
// row lanes in ascending order through LDS -- so every total is the loop form's, bit for bit.  Wider rows keep the loop form.
template <int KT>
__device__ __forceinline__ void bn_load_terms(const float* part, int nblk, int C, int cc, int rsub, int RS, float (&v)[8 * KT]) {
#pragma unroll
    for (int j = 0; j < 8 * KT; ++j) {                   // (unconditional, clamped: a term past the end is loaded and not added)
        const int b = rsub + RS * j;
        v[j] = part[(int64_t)(b < nblk ? b : nblk - 1) * C + cc];
    }
}
template <int KT>
__device__ __forceinline__ float bn_sum_terms(const float (&v)[8 * KT], int nblk, int rsub, int RS) {
    float t[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < KT; ++k)
#pragma unroll
        for (int u = 0; u < 8; ++u)
            if (rsub + RS * (u + 8 * k) < nblk) t[u] += v[8 * k + u];
    return ((t[0] + t[1]) + (t[2] + t[3])) + ((t[4] + t[5]) + (t[6] + t[7]));
}
// the row lanes' sums of a column, in ascending order: the result in the threads rsub == 0, c < C.  sh: 256 floats nobody still reads
__device__ __forceinline__ float bn_sum_lanes(float s, int C, int CL, float* sh) {
    const int c = threadIdx.x & (CL - 1), rsub = threadIdx.x / CL, RS = 256 / CL;
    sh[threadIdx.x] = s;
    __syncthreads();
    float t = 0.f;
    if (rsub == 0 && c < C)
        for (int k = 0; k < RS; ++k) t += sh[k * CL + c];
    return t;
}
// ... two columns' worth behind one barrier.  sh: 512 floats
__device__ __forceinline__ void bn_sum_lanes2(float& s0, float& s1, int C, int CL, float* sh) {
    const int c = threadIdx.x & (CL - 1), rsub = threadIdx.x / CL, RS = 256 / CL;
    sh[threadIdx.x] = s0;
    sh[256 + threadIdx.x] = s1;
    __syncthreads();
    s0 = 0.f;
    s1 = 0.f;
    if (rsub == 0 && c < C)
        for (int k = 0; k < RS; ++k) { s0 += sh[k * CL + c]; s1 += sh[256 + k * CL + c]; }
}
// how many trips of eight terms a thread's share of nblk partials is; 0: more than four, the loop form
__device__ __forceinline__ int bn_term_trips(int merge, int nblk, int CL) {
    if (!merge || nblk * CL > 4 * 2048) return 0;
    return nblk * CL <= 2048 ? 1 : (nblk * CL <= 2 * 2048 ? 2 : 4);
}

// The forward merge: mean[c] = batch mean, m2[c] = squares about it (bn_total, the division, bn_total_m2) from one set of loads.
// The rows of block b are `per` up to the last block that has any, whose count is what is left, and none behind it (bn_share):
// two float constants and two comparisons per term where bn_total_m2 multiplies and clamps in 64 bits.  sh: 512 floats
template <int KT>
__device__ __forceinline__ void bn_merge_held(const BnArgs& a, int nblk, int CL, float* sh, float* mean, float* m2) {
    const int c = threadIdx.x & (CL - 1), rsub = threadIdx.x / CL, RS = 256 / CL, cc = c < a.C ? c : 0;
    float p1[8 * KT], p2[8 * KT], p3[8 * KT];
    bn_load_terms<KT>(a.part1, nblk, a.C, cc, rsub, RS, p1);
    bn_load_terms<KT>(a.part2, nblk, a.C, cc, rsub, RS, p2);
    bn_load_terms<KT>(a.part3, nblk, a.C, cc, rsub, RS, p3);
    const int64_t nv = bn_valid(a);
    const int64_t per = (nv + nblk - 1) / nblk, full = nv / per;         // blocks [0, full) hold `per` rows, block `full` the rest
    const float cnt_full = (float)per, cnt_last = (float)(nv - per * full);
    __syncthreads();                                     // (sh may still be read)
    const float tot = bn_sum_lanes(bn_sum_terms<KT>(p1, nblk, rsub, RS), a.C, CL, sh);
    if (rsub == 0 && c < a.C) mean[c] = tot / (float)nv;
    __syncthreads();
    const float mu = mean[cc];
#pragma unroll
    for (int j = 0; j < 8 * KT; ++j) {
        const int b = rsub + RS * j;
        const float cnt = b < full ? cnt_full : (b == full ? cnt_last : 0.f);
        const float d = cnt > 0.f ? p1[j] / cnt - mu : 0.f;              // (an empty block: nothing)
        p2[j] = fmaf(d, fmaf(cnt, d, 2.f * p3[j]), p2[j]);
    }
    const float q = bn_sum_lanes(bn_sum_terms<KT>(p2, nblk, rsub, RS), a.C, CL, sh + 256);
    if (rsub == 0 && c < a.C) m2[c] = q;                 // (read back by the thread that wrote it: t == c)
}

// two plain totals (the backward's column sums of dy and of dy xhat) from one set of loads.  sh: 512 floats
template <int KT>
__device__ __forceinline__ void bn_total_pair_held(const float* pa, const float* pb, int nblk, int C, int CL, float* sh, float* out_a, float* out_b) {
    const int c = threadIdx.x & (CL - 1), rsub = threadIdx.x / CL, RS = 256 / CL, cc = c < C ? c : 0;
    float va[8 * KT], vb[8 * KT];
    bn_load_terms<KT>(pa, nblk, C, cc, rsub, RS, va);
    bn_load_terms<KT>(pb, nblk, C, cc, rsub, RS, vb);
    float sa = bn_sum_terms<KT>(va, nblk, rsub, RS), sb = bn_sum_terms<KT>(vb, nblk, rsub, RS);
    __syncthreads();                                     // (sh may still be read)
    bn_sum_lanes2(sa, sb, C, CL, sh);
    if (rsub == 0 && c < C) { out_a[c] = sa; out_b[c] = sb; }
    __syncthreads();
}

// Companion statistics, block `blk` of s.nblk: plane 0 column sums, plane 1 squares about the block's own column means,
// plane 2 counted rows (every column of the plane holds the count).  Fixed order everywhere.  sh: 1024 floats
__device__ __forceinline__ void bn_side_block_stats(const BnSide& s, int blk, float* sh) {
    __shared__ float smean[256];
    const int CL = s.CL, t = threadIdx.x, c = t & (CL - 1), rsub = t / CL, RS = 256 / CL;
    const bool act = c < s.C;
    const int cc = act ? c : 0;
    int64_t lo, hi;
    bn_share(s.n, s.nblk, blk, lo, hi);
    const int64_t lim = s.key ? *s.key_limit : 0;
    float mu = 0.f, m2 = 0.f;
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
        float s0 = 0.f, cnt = 0.f;
        for (int64_t r0 = lo + rsub; r0 < hi; r0 += 8 * RS) {
            float v[8];
            bool ok[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int64_t rr = r0 + u * RS < hi ? r0 + u * RS : hi - 1;
                v[u] = s.x[rr * s.xs + cc];
                ok[u] = r0 + u * RS < hi && (!s.key || s.key[rr] < lim);
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                if (ok[u]) {
                    if (pass == 0) { s0 += v[u]; cnt += 1.f; }
                    else { const float d = v[u] - mu; s0 = fmaf(d, d, s0); }
                }
            }
        }
        const float tot = bn_reduce_rows(s0, CL, sh);
        if (pass == 0) {
            const float n_b = bn_reduce_rows(cnt, CL, sh);          // counts: exact below 2^24 rows per block
            if (t < CL && act) {
                s.part[((size_t)0 * s.nblk + blk) * s.C + c] = tot;
                s.part[((size_t)2 * s.nblk + blk) * s.C + c] = n_b;
                smean[c] = n_b > 0.f ? tot / n_b : 0.f;
            }
            __syncthreads();
            mu = smean[cc];
        } else {
            m2 = tot;
            if (t < CL && act) s.part[((size_t)1 * s.nblk + blk) * s.C + c] = m2;
        }
    }
}

// The same for narrow contiguous rows (x_stride == C <= 8, 16-byte aligned base: the reference's bond rows, [n, 7]): four rows
// are C whole float4s, so a thread takes groups of four rows with C 16-byte loads each, SIDE_G groups in flight -- 4 096 rows per
// block and loop trip where the column-per-thread form above takes 256 (a batch of 4 096 molecules has 216 k bond rows: 53
// blocks of one trip per pass instead of 844, and a final merge over 53 partials instead of 844).
constexpr int SIDE_G = 4;
constexpr int SIDE_FLAT_ROWS = 256 * 4 * SIDE_G;       // rows per block and loop trip
template <int C>
__device__ __forceinline__ void bn_side_block_stats_flat(const BnSide& s, int blk, float* sh) {
    __shared__ float smean[8];
    const int t = threadIdx.x;
    int64_t lo, hi;
    bn_share(s.n / 4, s.nblk, blk, lo, hi);              // in units of four rows: the whole groups; the last n % 4 rows below
    const int64_t lim = s.key ? *s.key_limit : 0;
    float mu[C];
#pragma unroll
    for (int c = 0; c < C; ++c) mu[c] = 0.f;
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
        float acc[C], cnt = 0.f;
#pragma unroll
        for (int c = 0; c < C; ++c) acc[c] = 0.f;
        for (int64_t q0 = lo + t; q0 - t < hi && lo < hi; q0 += 256 * SIDE_G) {
            f32x4 v[SIDE_G][C];
            bool ok[SIDE_G][4];
#pragma unroll
            for (int g = 0; g < SIDE_G; ++g) {
                const int64_t q = q0 + 256 * g;                       // rows 4 q .. 4 q + 3
                const int64_t qc = q < hi ? q : hi - 1;
#pragma unroll
                for (int c = 0; c < C; ++c) v[g][c] = *(const f32x4*)(s.x + 4 * qc * C + 4 * c);      // (all loads unconditional)
#pragma unroll
                for (int r = 0; r < 4; ++r) ok[g][r] = q < hi && (!s.key || s.key[4 * qc + r] < lim);
            }
#pragma unroll
            for (int g = 0; g < SIDE_G; ++g)
#pragma unroll
                for (int e = 0; e < 4 * C; ++e) {                     // element e of the group: row e / C, column e % C
                    if (ok[g][e / C]) {
                        const float x = v[g][e / 4][e % 4];
                        if (pass == 0) { acc[e % C] += x; if (e % C == 0) cnt += 1.f; }
                        else { const float d = x - mu[e % C]; acc[e % C] = fmaf(d, d, acc[e % C]); }
                    }
                }
        }
        if (blk == s.nblk - 1 && t == 0) {                            // the tensor's last n % 4 rows: a few scalar loads of one thread
            for (int64_t row = s.n / 4 * 4; row < s.n; ++row) {
                if (s.key && !(s.key[row] < lim)) continue;
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    const float x = s.x[row * C + c];
                    if (pass == 0) acc[c] += x;
                    else { const float d = x - mu[c]; acc[c] = fmaf(d, d, acc[c]); }
                }
                if (pass == 0) cnt += 1.f;
            }
        }
        // every thread holds every column: an xor tree over the wave, the four waves in order -- all C + 1 sums behind ONE pair of
        // barriers (one reduction per column cost more than the row pass itself)
        float tot[C], n_b = cnt;
#pragma unroll
        for (int c = 0; c < C; ++c) tot[c] = acc[c];
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
#pragma unroll
            for (int c = 0; c < C; ++c) tot[c] += __shfl_xor(tot[c], o, 64);
            n_b += __shfl_xor(n_b, o, 64);
        }
        __syncthreads();
        if ((t & 63) == 0) {
#pragma unroll
            for (int c = 0; c < C; ++c) sh[(t >> 6) * 16 + c] = tot[c];
            sh[(t >> 6) * 16 + 8] = n_b;
        }
        __syncthreads();
        if (t == 0) {
#pragma unroll
            for (int c = 0; c < C; ++c) tot[c] = ((sh[c] + sh[16 + c]) + sh[32 + c]) + sh[48 + c];
            n_b = ((sh[8] + sh[24]) + sh[40]) + sh[56];
        }
        if (t == 0) {
#pragma unroll
            for (int c = 0; c < C; ++c) {
                if (pass == 0) {
                    s.part[((size_t)0 * s.nblk + blk) * C + c] = tot[c];
                    s.part[((size_t)2 * s.nblk + blk) * C + c] = n_b;
                    smean[c] = n_b > 0.f ? tot[c] / n_b : 0.f;
                } else {
                    s.part[((size_t)1 * s.nblk + blk) * C + c] = tot[c];
                }
            }
        }
        __syncthreads();
        if (pass == 0) {
#pragma unroll
            for (int c = 0; c < C; ++c) mu[c] = smean[c];
        }
    }
}
__device__ __forceinline__ bool bn_side_is_flat(const BnSide& s) { return s.flat != 0; }
__device__ __forceinline__ void bn_side_stats_any(const BnSide& s, int blk, float* sh) {
    if (!bn_side_is_flat(s)) { bn_side_block_stats(s, blk, sh); return; }
    switch (s.C) {
        case 1: bn_side_block_stats_flat<1>(s, blk, sh); break;
        case 2: bn_side_block_stats_flat<2>(s, blk, sh); break;
        case 3: bn_side_block_stats_flat<3>(s, blk, sh); break;
        case 4: bn_side_block_stats_flat<4>(s, blk, sh); break;
        case 5: bn_side_block_stats_flat<5>(s, blk, sh); break;
        case 6: bn_side_block_stats_flat<6>(s, blk, sh); break;
        case 7: bn_side_block_stats_flat<7>(s, blk, sh); break;
        default: bn_side_block_stats_flat<8>(s, blk, sh); break;
    }
}

// the companion's three totals from one set of loads (the loop form: bn_side_final's last branch); returns the counted rows.
// sh: 512 floats
template <int KT>
__device__ __forceinline__ float bn_side_totals_held(const BnSide& s, const float* sums, const float* sqs, const float* cnts, float* sh,
                                                     float* tot_sh, float* cnt_sh, float* mu_sh, float* sq_sh) {
    const int CL = s.CL, c = threadIdx.x & (CL - 1), rsub = threadIdx.x / CL, RS = 256 / CL, cc = c < s.C ? c : 0;
    float s_b[8 * KT], n_b[8 * KT], q_b[8 * KT];
    bn_load_terms<KT>(sums, s.nblk, s.C, cc, rsub, RS, s_b);
    bn_load_terms<KT>(cnts, s.nblk, s.C, cc, rsub, RS, n_b);
    bn_load_terms<KT>(sqs, s.nblk, s.C, cc, rsub, RS, q_b);
    float tot = bn_sum_terms<KT>(s_b, s.nblk, rsub, RS), n = bn_sum_terms<KT>(n_b, s.nblk, rsub, RS);
    __syncthreads();                                     // (sh may still be read)
    bn_sum_lanes2(tot, n, s.C, CL, sh);
    if (rsub == 0 && c < s.C) { tot_sh[c] = tot; cnt_sh[c] = n; }
    __syncthreads();
    const float cnt = cnt_sh[0];
    if ((int)threadIdx.x < s.C) mu_sh[threadIdx.x] = cnt > 0.f ? tot_sh[threadIdx.x] / cnt : 0.f;
    __syncthreads();
    const float mu = mu_sh[cc];
#pragma unroll
    for (int j = 0; j < 8 * KT; ++j) {
        const float d = s_b[j] / fmaxf(n_b[j], 1.f) - mu;
        q_b[j] = fmaf(n_b[j] * d, d, q_b[j]);
    }
    const float q = bn_sum_lanes(bn_sum_terms<KT>(q_b, s.nblk, rsub, RS), s.C, CL, sh);
    if (rsub == 0 && c < s.C) sq_sh[c] = q;              // (read back by the thread that wrote it)
    return cnt;
}

// running <- running + momentum (batch - running), unbiased variance, counter + 1 (one block)
template <bool HELD = true>
__device__ __forceinline__ void bn_side_final(const BnSide& s, float* sh) {
    __shared__ float tot_sh[256], sq_sh[256], cnt_sh[256], mu_sh[256];
    const float* const sums = s.part;
    const float* const sqs = s.part + (size_t)s.nblk * s.C;
    const float* const cnts = s.part + (size_t)2 * s.nblk * s.C;
    const int col = threadIdx.x;
    const int trips = HELD ? bn_term_trips(s.merge, s.nblk, s.CL) : 0;
    float cnt;
    if (trips == 1) cnt = bn_side_totals_held<1>(s, sums, sqs, cnts, sh, tot_sh, cnt_sh, mu_sh, sq_sh);
    else if (trips == 2) cnt = bn_side_totals_held<2>(s, sums, sqs, cnts, sh, tot_sh, cnt_sh, mu_sh, sq_sh);
    else if (trips == 4) cnt = bn_side_totals_held<4>(s, sums, sqs, cnts, sh, tot_sh, cnt_sh, mu_sh, sq_sh);
    else {
        bn_total(sums, s.nblk, s.C, s.CL, sh, tot_sh);
        bn_total(cnts, s.nblk, s.C, s.CL, sh, cnt_sh);
        cnt = cnt_sh[0];
        if (col < s.C) mu_sh[col] = cnt > 0.f ? tot_sh[col] / cnt : 0.f;
        __syncthreads();
        bn_total_of(s.nblk, s.C, s.CL, sh, sq_sh, [&](int b, int c) {
            const float n_b = cnts[(size_t)b * s.C + c], s_b = sums[(size_t)b * s.C + c], q_b = sqs[(size_t)b * s.C + c];     // (unconditional loads)
            const float d = s_b / fmaxf(n_b, 1.f) - mu_sh[c];
            return fmaf(n_b * d, d, q_b);
        });
    }
    // (BatchNorm1d raises on fewer than two values per channel in training mode; a kernel cannot: such a degenerate batch -- a
    // padded batch without a single real bond -- leaves the statistics AND the counter where they are: ADVICE round 5)
    if (col < s.C && cnt > 1.f) {
        const float mu = mu_sh[col], var = sq_sh[col] / cnt;
        if (s.running_mean) s.running_mean[col] = fmaf(s.momentum, mu - s.running_mean[col], s.running_mean[col]);
        if (s.running_var) {
            const float unbiased = cnt > 1.f ? var * (cnt / (cnt - 1.f)) : var;
            s.running_var[col] = fmaf(s.momentum, unbiased - s.running_var[col], s.running_var[col]);
        }
    }
    if (threadIdx.x == 0 && s.nbt && cnt > 1.f) s.nbt[0] += 1;
}

// the companion alone: two launches (phase 0: block statistics, phase 2: totals), or -- one block's worth of rows -- one (phase 3)
__global__ void __launch_bounds__(256) bn_side_kernel(BnSide s, int phase) {
    __shared__ float sh[1024];
    if (phase == 0 || phase == 3) bn_side_stats_any(s, blockIdx.x, sh);
    if (phase == 3) __syncthreads();                     // (one block: its own global stores are visible to it behind a barrier)
    if (phase == 2 || phase == 3) bn_side_final(s, sh);
}

// what rides behind the statistics launch's own blocks: [touch_first, prep_first) read the hinted arrays (mkgnn_touch_hint),
// [prep_first, grid) run a pending bank preparation (mkgnn_bank_prepare_deferred) -- both independent of the batch norm, both
// otherwise paid for on the chain in front of the first convolution
template <bool VEC>
__global__ void __launch_bounds__(256) bn_stats_kernel(BnArgs a, int CL) {
    __shared__ float sh[1024];
    if (a.touch.count > 0 && (int)blockIdx.x >= a.touch_first) {     // (behind the batch norm's and the companion's own blocks)
        touch_body(a.touch, blockIdx.x - a.touch_first, gridDim.x - a.touch_first);
        return;
    }
    if (blockIdx.x >= BN_MAIN_BLOCKS) {
        bn_side_stats_any(a.side, blockIdx.x - BN_MAIN_BLOCKS, sh);
        if (a.side.nblk == 1) {                          // a companion of one block's worth of rows: all of it here, in this launch
            __syncthreads();                             // (its own global stores are visible to the block behind a barrier)
            bn_side_final<false>(a.side, sh);            // (one partial: the loop form is one trip; the launch keeps its registers)
        }
        return;
    }
    bn_block_stats<VEC>(a, CL, sh);
}

template <bool VEC>
__global__ void __launch_bounds__(256) bn_stats_prep_kernel(BnArgs a, int CL, PrepManyArgs pm, int prep_first) {
    __shared__ float sh[1024];
    if ((int)blockIdx.x >= prep_first) { bank_prepare_many_block(pm, blockIdx.x - prep_first); return; }
    if ((int)blockIdx.x >= a.touch_first) {
        touch_body(a.touch, blockIdx.x - a.touch_first, prep_first - a.touch_first);
        return;
    }
    if (blockIdx.x >= BN_MAIN_BLOCKS) {
        bn_side_stats_any(a.side, blockIdx.x - BN_MAIN_BLOCKS, sh);
        if (a.side.nblk == 1) {
            __syncthreads();
            bn_side_final<false>(a.side, sh);
        }
        return;
    }
    bn_block_stats<VEC>(a, CL, sh);
}

// Round 6, second step: ONE launch for the training forward, one for the backward -- statistics | grid-wide barrier | apply.  The
// two phases need every block's partial sums, which until now meant a kernel boundary (~5 us in a captured graph on this chip,
// for kernels that take 14 and 17).  All blocks of these launches are resident at once (at most 256 + 54 blocks of 256 threads and
// a few KB of LDS on 256 CUs), so a counter in device memory does: a block's thread 0 releases its partials (__threadfence),
// adds 1, spins until the count is the grid's size, acquires; the last block to LEAVE resets the counters.  The spin is bounded: a
// grid that is not resident within ~a second falls through (its output is then wrong, but it ends).
// MEASURED (batch 4096, profiles/r06 notes in DESIGN 4.4): 47 us for the fused forward against 14 + 17 for the two launches, the step
// 0.723 against 0.708 ms -- the agent-scope release / acquire around the counter writes back and invalidates the L2 of every XCD (the
// apply phase then re-reads from memory the rows the statistics phase had just pulled in), and 310 waves polling one counter across
// eight XCDs are slow to see it move.  Correct (the 56 batch-norm / network tests pass with it on), not faster: opt-in only,
// MKGNN_BN_ONE_LAUNCH=1.
__device__ unsigned g_bn_barrier[8];                   // {arrived, left} of the forward launch, of the backward launch
__device__ __forceinline__ void bn_grid_barrier(unsigned* ctr) {
    __syncthreads();
    if (threadIdx.x == 0) {
        __threadfence();
        atomicAdd(&ctr[0], 1u);
        for (unsigned spins = 0; atomicAdd(&ctr[0], 0u) < gridDim.x && spins < (1u << 24); ++spins) __builtin_amdgcn_s_sleep(1);
        __threadfence();
        if (atomicAdd(&ctr[1], 1u) == gridDim.x - 1) { atomicExch(&ctr[0], 0u); atomicExch(&ctr[1], 0u); }      // (everybody has seen the count)
    }
    __syncthreads();
}

__device__ __forceinline__ void bn_apply_body(const BnArgs& a, int CL, float* sh) {
    __shared__ float mean[256], invstd[256], scale[256], shift[256];
    const int t = threadIdx.x;
    if (a.training) {
        const int64_t nv = bn_valid(a);
        const int trips = bn_term_trips(a.merge, bn_nblk(), CL);
        if (MKGNN_BN_AB == 1) {
            if (t < a.C) { mean[t] = a.save_mean[t]; invstd[t] = a.save_invstd[t]; }
        } else if (trips == 1) {
            bn_merge_held<1>(a, bn_nblk(), CL, sh, mean, invstd);
        } else if (trips == 2) {
            bn_merge_held<2>(a, bn_nblk(), CL, sh, mean, invstd);
        } else if (trips == 4) {
            bn_merge_held<4>(a, bn_nblk(), CL, sh, mean, invstd);
        } else {
            bn_total(a.part1, bn_nblk(), a.C, CL, sh, mean);
            if (t < a.C) mean[t] = mean[t] / (float)nv;
            __syncthreads();
            bn_total_m2(a.part1, a.part2, a.part3, bn_nblk(), nv, a.C, CL, mean, sh, invstd);
        }
        if (t < a.C) {
            const float mu = mean[t], var = invstd[t] / (float)nv;
            invstd[t] = 1.f / sqrtf(var + a.eps);
            if (blockIdx.x == 0) {
                a.save_mean[t] = mu;
                a.save_invstd[t] = invstd[t];
                if (a.running_mean) a.running_mean[t] = fmaf(a.momentum, mu - a.running_mean[t], a.running_mean[t]);
                if (a.running_var) {
                    const float unbiased = nv > 1 ? var * ((float)nv / (float)(nv - 1)) : var;
                    a.running_var[t] = fmaf(a.momentum, unbiased - a.running_var[t], a.running_var[t]);
                }
            }
        }
    } else if (t < a.C) {
        mean[t] = a.running_mean[t];
        invstd[t] = 1.f / sqrtf(a.running_var[t] + a.eps);
        if (blockIdx.x == 0 && a.save_mean) { a.save_mean[t] = mean[t]; a.save_invstd[t] = invstd[t]; }
    }
    __syncthreads();
    if (t < a.C) {
        const float w = a.weight ? a.weight[t] : 1.f, b = a.bias ? a.bias[t] : 0.f;
        scale[t] = invstd[t] * w;
        shift[t] = b;
    }
    __syncthreads();
    int64_t lo, hi;
    bn_rows(a, lo, hi);
    if (MKGNN_BN_AB == 2) hi = lo;
    const int c = t & (CL - 1), rsub = t / CL, RS = 256 / CL;       // same thread layout as the column sums
    if (blockIdx.x == 0 && t == 0 && a.nbt && a.training) a.nbt[0] += 1;
    if (a.inv_out) {
        // also the row norms of the output, for the kernel convolution that reads it next.  Thread layout of
        // row_inv_norm_aligned_kernel<8> (kgnn_csr.hip): eight lanes per row, four consecutive channels each (16-byte
        // loads and stores; the host checks the alignment), the same FMA chain and xor tree on the stored values --
        // bit-identical to mkgnn_row_inv_norm on `out`.
        const int l = t & 7, rs8 = t >> 3, col = 4 * l;
        const bool act = col < a.C;                       // (C is a multiple of 4 here: a lane's four channels exist or do not)
        const int cb = act ? col : 0;
        f32x4 mu4, sc4, sh4;
#pragma unroll
        for (int e = 0; e < 4; ++e) { mu4[e] = mean[cb + e]; sc4[e] = scale[cb + e]; sh4[e] = shift[cb + e]; }
        for (int64_t r0 = lo + rs8; r0 - rs8 < hi; r0 += BN_UA * 32) {
            f32x4 v[BN_UA];
#pragma unroll
            for (int u = 0; u < BN_UA; ++u) v[u] = *(const f32x4*)(a.x + (r0 + u * 32 < hi ? r0 + u * 32 : hi - 1) * a.xs + cb);
#pragma unroll
            for (int u = 0; u < BN_UA; ++u) {
                const bool ok = r0 + u * 32 < hi;
                f32x4 o;
#pragma unroll
                for (int e = 0; e < 4; ++e) o[e] = act ? fmaf(v[u][e] - mu4[e], sc4[e], sh4[e]) : 0.f;
                float ss = o[0] * o[0];
                ss = fmaf(o[1], o[1], ss); ss = fmaf(o[2], o[2], ss); ss = fmaf(o[3], o[3], ss);
                ss += __shfl_xor(ss, 4, 64); ss += __shfl_xor(ss, 2, 64); ss += __shfl_xor(ss, 1, 64);
                const float inv = 1.f / fmaxf(sqrtf(ss), MKGNN_EPS);      // (every lane of the row holds the sum)
                if (ok && l == 0) a.inv_out[r0 + u * 32] = inv;
                if (ok && act) *(f32x4*)(a.out + (r0 + u * 32) * a.os + col) = a.split_out ? split_row_store(o, inv) : o;
            }
        }
    } else if (c < a.C) {
        const float mu = mean[c], sc = scale[c], sh0 = shift[c];
        for (int64_t r0 = lo + rsub; r0 < hi; r0 += 8 * RS) {
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = a.x[(r0 + u * RS < hi ? r0 + u * RS : hi - 1) * a.xs + c];
#pragma unroll
            for (int u = 0; u < 8; ++u)
                if (r0 + u * RS < hi) a.out[(r0 + u * RS) * a.os + c] = fmaf(v[u] - mu, sc, sh0);
        }
    }
}

__global__ void __launch_bounds__(256) bn_apply_kernel(BnArgs a, int CL) {
    __shared__ float sh[1024];
    if (blockIdx.x >= BN_MAIN_BLOCKS) { bn_side_final(a.side, sh); return; }      // (one extra block, training mode only)
    bn_apply_body(a, CL, sh);
}

// statistics | barrier | apply: the grid is BN_MAIN_BLOCKS + the companion's blocks (its first block does the companion's totals)
template <bool VEC>
__global__ void __launch_bounds__(256) bn_forward_fused_kernel(BnArgs a, int CL) {
    __shared__ float sh[1024];
    const bool side = blockIdx.x >= BN_MAIN_BLOCKS;
    if (side) {
        bn_side_stats_any(a.side, blockIdx.x - BN_MAIN_BLOCKS, sh);
        if (a.side.nblk == 1) { __syncthreads(); bn_side_final(a.side, sh); }
    } else {
        bn_block_stats<VEC>(a, CL, sh);
    }
    bn_grid_barrier(&g_bn_barrier[0]);
    if (side) {
        if (blockIdx.x == BN_MAIN_BLOCKS && a.side.nblk > 1) bn_side_final(a.side, sh);
        return;
    }
    bn_apply_body(a, CL, sh);
}

// backward: per-block column sums of dy and dy * xhat over the block's counted rows -> part1, part2
template <bool VEC>
__device__ __forceinline__ void bn_bwd_partial_body(const BnArgs& a, int CL, float* sh) {
    const int t = threadIdx.x;
    int64_t lo, hi;
    bn_share(bn_valid(a), bn_nblk(), blockIdx.x, lo, hi);
    float* const p1 = a.part1 + (int64_t)blockIdx.x * a.C;
    float* const p2 = a.part2 + (int64_t)blockIdx.x * a.C;
    if constexpr (VEC) {
        const int LW = CL >= 4 ? CL / 4 : 1, g = t % LW, rsub = t / LW, RS = 256 / LW, col = 4 * g;
        const bool act = col < a.C;
        const int cb = act ? col : 0;
        const f32x4 mu = {a.save_mean[cb], a.save_mean[cb + 1], a.save_mean[cb + 2], a.save_mean[cb + 3]};
        const f32x4 is = {a.save_invstd[cb], a.save_invstd[cb + 1], a.save_invstd[cb + 2], a.save_invstd[cb + 3]};
        f32x4 s0 = {0.f, 0.f, 0.f, 0.f}, s1 = {0.f, 0.f, 0.f, 0.f};
        bn_pass_vec<2, BN_UA>(a.x, a.xs, a.gout, a.gos, lo, hi, rsub, RS, cb, mu, is, s0, s1);
        const f32x4 t0 = bn_reduce_rows(s0, LW, (f32x4*)sh);
        const f32x4 t1 = bn_reduce_rows(s1, LW, (f32x4*)sh);
        if (t < LW && act) {
#pragma unroll
            for (int e = 0; e < 4; ++e) { p1[col + e] = t0[e]; p2[col + e] = t1[e]; }
        }
    } else {
        const int c = t & (CL - 1), rsub = t / CL, RS = 256 / CL;
        const bool act = c < a.C;
        const int cc = act ? c : 0;
        float s0 = 0.f, s1 = 0.f;
        bn_pass_col<2>(a.x, a.xs, a.gout, a.gos, lo, hi, rsub, RS, cc, a.save_mean[cc], a.save_invstd[cc], s0, s1);
        const float t0 = bn_reduce_rows(s0, CL, sh);
        const float t1 = bn_reduce_rows(s1, CL, sh);
        if (t < CL && act) { p1[c] = t0; p2[c] = t1; }
    }
}

template <bool VEC>
__global__ void __launch_bounds__(256) bn_bwd_partial_kernel(BnArgs a, int CL) {
    __shared__ float sh[1024];
    bn_bwd_partial_body<VEC>(a, CL, sh);
}

template <bool VEC>
__device__ __forceinline__ void bn_bwd_final_body(const BnArgs& a, int CL, int nblk_part, float* sh) {
    __shared__ float sdy[256], sdyx[256];
    const int trips = bn_term_trips(a.merge, nblk_part, CL);
    if (trips == 1) bn_total_pair_held<1>(a.part1, a.part2, nblk_part, a.C, CL, sh, sdy, sdyx);
    else if (trips == 2) bn_total_pair_held<2>(a.part1, a.part2, nblk_part, a.C, CL, sh, sdy, sdyx);
    else if (trips == 4) bn_total_pair_held<4>(a.part1, a.part2, nblk_part, a.C, CL, sh, sdy, sdyx);
    else {
        bn_total(a.part1, nblk_part, a.C, CL, sh, sdy);
        bn_total(a.part2, nblk_part, a.C, CL, sh, sdyx);
    }
    const int t = threadIdx.x;
    if (blockIdx.x == 0 && t < a.C) {
        if (a.gbias) a.gbias[t] = sdy[t];
        if (a.gweight) a.gweight[t] = sdyx[t];
    }
    if (!a.gx) return;
    int64_t lo, hi;
    bn_rows(a, lo, hi);
    const float invn = 1.f / (float)bn_valid(a);
    if constexpr (VEC) {
        const int LW = CL >= 4 ? CL / 4 : 1, g = t % LW, rsub = t / LW, RS = 256 / LW, col = 4 * g;
        const bool act = col < a.C;
        const int cb = act ? col : 0;
        f32x4 k0, is, mu, s0, s1;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float w = a.weight ? a.weight[cb + e] : 1.f;
            is[e] = a.save_invstd[cb + e]; mu[e] = a.save_mean[cb + e];
            k0[e] = w * is[e]; s0[e] = sdy[cb + e] * invn; s1[e] = sdyx[cb + e] * invn;
        }
        for (int64_t r0 = lo + rsub; r0 < hi; r0 += (int64_t)BN_UA * RS) {
            f32x4 dy[BN_UA], xv[BN_UA];
#pragma unroll
            for (int u = 0; u < BN_UA; ++u) {
                const int64_t rr = r0 + (int64_t)u * RS < hi ? r0 + (int64_t)u * RS : hi - 1;
                dy[u] = *(const f32x4*)(a.gout + rr * a.gos + cb);
                xv[u] = *(const f32x4*)(a.x + rr * a.xs + cb);
            }
#pragma unroll
            for (int u = 0; u < BN_UA; ++u) {
                if (r0 + (int64_t)u * RS < hi && act) {
                    f32x4 o;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float xh = (xv[u][e] - mu[e]) * is[e];
                        o[e] = a.training ? k0[e] * (dy[u][e] - (s0[e] + xh * s1[e])) : k0[e] * dy[u][e];
                    }
                    *(f32x4*)(a.gx + (r0 + (int64_t)u * RS) * a.gxs + col) = o;
                }
            }
        }
    } else {
        const int c = t & (CL - 1), rsub = t / CL, RS = 256 / CL;
        if (c < a.C) {
            const float w = a.weight ? a.weight[c] : 1.f;
            const float is = a.save_invstd[c], mu = a.save_mean[c];
            const float k0 = w * is, s0 = sdy[c] * invn, s1 = sdyx[c] * invn;
            for (int64_t r0 = lo + rsub; r0 < hi; r0 += 4 * RS) {
                float dy[4], xv[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int64_t rr = r0 + u * RS < hi ? r0 + u * RS : hi - 1;
                    dy[u] = a.gout[rr * a.gos + c];
                    xv[u] = a.x[rr * a.xs + c];
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    if (r0 + u * RS < hi) {
                        const float xh = (xv[u] - mu) * is;
                        a.gx[(r0 + u * RS) * a.gxs + c] = a.training ? k0 * (dy[u] - (s0 + xh * s1)) : k0 * dy[u];
                    }
                }
            }
        }
    }
}

template <bool VEC>
__global__ void __launch_bounds__(256) bn_bwd_final_kernel(BnArgs a, int CL, int nblk_part) {
    __shared__ float sh[1024];
    bn_bwd_final_body<VEC>(a, CL, nblk_part, sh);
}

// partial sums | barrier | gradient rows   (grad_x wanted: every block has rows to write)
template <bool VEC>
__global__ void __launch_bounds__(256) bn_backward_fused_kernel(BnArgs a, int CL) {
    __shared__ float sh[1024];
    bn_bwd_partial_body<VEC>(a, CL, sh);
    bn_grid_barrier(&g_bn_barrier[2]);
    bn_bwd_final_body<VEC>(a, CL, (int)gridDim.x, sh);
}

}  // namespace mkgnn

using namespace mkgnn;

// ================================================================== C ABI ==========================
static constexpr int BN_BLOCKS = BN_MAIN_BLOCKS;

// MKGNN_BN_MERGE=0 and mkgnn_debug_set_bn_merge(0) (tests; it wins over the environment) keep the loop form of every merge at every
// width: the in-process reference of the register forms.  The results are the same bits either way.
static std::atomic<int> g_bn_merge_override{-1};
extern "C" int mkgnn_debug_set_bn_merge(int32_t on) {
    g_bn_merge_override.store(on < 0 ? -1 : (on ? 1 : 0));           // negative: back to the default
    return 0;
}
static inline int bn_merge_on() {
    const int forced = g_bn_merge_override.load();
    return forced >= 0 ? forced : (switches().bn_merge ? 1 : 0);
}

extern "C" {

size_t mkgnn_batchnorm_workspace_bytes(int32_t C) { return C > 0 ? (size_t)3 * BN_BLOCKS * C * 4 : 0; }

static int bn_common(const char* who, int64_t n, int32_t C, int& CL) {
    if (C < 1 || C > 256) return api_fail("%s: channel count C=%d outside 1..256", who, C);
    if (n < 1) return api_fail("%s: batch norm needs at least one row", who);
    CL = 1;
    while (CL < C) CL <<= 1;
    return 0;
}

size_t mkgnn_batchnorm_stats_workspace_bytes(int32_t C) { return C > 0 ? (size_t)3 * BN_SIDE_BLOCKS * C * 4 : 0; }

// checks a companion and turns it into the kernels' form; s.nblk blocks
static int bn_side_setup(const char* who, const mkgnn_bn_stats* c, void* ws, size_t ws_bytes, BnSide& s) {
    if (!c->x || c->n_rows < 1 || c->C < 1 || c->C > 256 || c->x_stride < c->C) return api_fail("%s: bad companion tensor", who);
    if ((c->row_key != nullptr) != (c->key_limit != nullptr)) return api_fail("%s: row_key and key_limit come together", who);
    if (!ws || ws_bytes < mkgnn_batchnorm_stats_workspace_bytes(c->C)) return api_fail("%s: companion workspace too small", who);
    s.x = c->x; s.xs = c->x_stride; s.n = c->n_rows; s.C = c->C;
    s.CL = 1;
    while (s.CL < s.C) s.CL <<= 1;
    s.running_mean = c->running_mean; s.running_var = c->running_var; s.momentum = c->momentum; s.nbt = c->num_batches_tracked;
    s.key = c->row_key; s.key_limit = c->key_limit; s.part = (float*)ws; s.merge = bn_merge_on();
    s.flat = (c->C <= 8 && c->x_stride == c->C && ((uintptr_t)c->x & 15) == 0) ? 1 : 0;
    const int64_t rows_per_pass = s.flat ? SIDE_FLAT_ROWS : 8 * (256 / s.CL);      // rows a block takes per loop trip
    int64_t nb = (c->n_rows + rows_per_pass - 1) / rows_per_pass;
    s.nblk = (int)(nb < 1 ? 1 : (nb > BN_SIDE_BLOCKS ? BN_SIDE_BLOCKS : nb));
    return 0;
}

int mkgnn_batchnorm_update_stats(const mkgnn_bn_stats* c, void* ws, size_t ws_bytes, void* stream) {
    const char* who = "mkgnn_batchnorm_update_stats";
    if (!c) return api_fail("%s: null argument", who);
    BnSide s{};
    if (int rc = bn_side_setup(who, c, ws, ws_bytes, s)) return rc;
    hipStream_t st = (hipStream_t)stream;
    if ((int64_t)c->n_rows * s.CL <= 64 * 1024) {         // one block does all three steps in one launch
        s.nblk = 1;
        bn_side_kernel<<<1, 256, 0, st>>>(s, 3);
    } else {
        bn_side_kernel<<<s.nblk, 256, 0, st>>>(s, 0);
        bn_side_kernel<<<1, 256, 0, st>>>(s, 2);
    }
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : api_hip_fail(who, e);
}

int mkgnn_batchnorm_forward(const float* x, int64_t x_stride, int64_t n_rows, int32_t C, const float* weight,
                            const float* bias, float* running_mean, float* running_var, float momentum, float eps,
                            int32_t training, float* out, int64_t out_stride, float* save_mean, float* save_invstd,
                            float* inv_norm, int64_t* num_batches_tracked, const int64_t* n_valid_rows, void* ws, size_t ws_bytes,
                            void* stream) {
    return mkgnn_batchnorm_forward_with_stats(x, x_stride, n_rows, C, weight, bias, running_mean, running_var, momentum, eps, training,
                                              out, out_stride, save_mean, save_invstd, inv_norm, num_batches_tracked, n_valid_rows,
                                              ws, ws_bytes, nullptr, nullptr, 0, stream);
}

int mkgnn_batchnorm_forward_with_stats(const float* x, int64_t x_stride, int64_t n_rows, int32_t C, const float* weight,
                            const float* bias, float* running_mean, float* running_var, float momentum, float eps,
                            int32_t training, float* out, int64_t out_stride, float* save_mean, float* save_invstd,
                            float* inv_norm, int64_t* num_batches_tracked, const int64_t* n_valid_rows, void* ws, size_t ws_bytes,
                            const mkgnn_bn_stats* companion, void* companion_ws, size_t companion_ws_bytes, void* stream) {
    int CL;
    if (int rc = bn_common("mkgnn_batchnorm_forward", n_rows, C, CL)) return rc;
    const bool split_rows = (training & MKGNN_BN_SPLIT_ROWS) != 0;       // out is written pre-split (kgnn_split.h)
    training &= 1;
    if (split_rows && !inv_norm) return api_fail("mkgnn_batchnorm_forward: MKGNN_BN_SPLIT_ROWS needs inv_norm");
    if (companion && !training) return api_fail("mkgnn_batchnorm_forward: a statistics companion needs training mode (nothing moves in eval mode)");
    if (!x || !out || x_stride < C || out_stride < C) return api_fail("mkgnn_batchnorm_forward: bad x/out");
    if (training && (!save_mean || !save_invstd)) return api_fail("mkgnn_batchnorm_forward: save_mean/save_invstd is null");
    if (!training && (!running_mean || !running_var)) return api_fail("mkgnn_batchnorm_forward: eval mode needs running statistics");
    if (training && (!ws || ws_bytes < mkgnn_batchnorm_workspace_bytes(C))) return api_fail("mkgnn_batchnorm_forward: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    BnArgs a{};
    a.x = x; a.xs = x_stride; a.n = n_rows; a.C = C; a.weight = weight; a.bias = bias;
    a.running_mean = running_mean; a.running_var = running_var; a.momentum = momentum; a.eps = eps; a.training = training;
    a.out = out; a.os = out_stride; a.save_mean = save_mean; a.save_invstd = save_invstd;
    if (inv_norm && (C > 32 || C % 4 || x_stride % 4 || out_stride % 4 || ((uintptr_t)x & 15) || ((uintptr_t)out & 15)))
        return api_fail("mkgnn_batchnorm_forward: inv_norm needs C <= 32, a multiple of 4, and 16-byte aligned rows of x and out (C=%d)", C);
    a.inv_out = inv_norm; a.split_out = split_rows ? 1 : 0; a.nbt = num_batches_tracked; a.nvalid = n_valid_rows; a.merge = bn_merge_on();
    a.part1 = (float*)ws; a.part2 = a.part1 ? a.part1 + (size_t)BN_BLOCKS * C : nullptr;
    a.part3 = a.part1 ? a.part1 + (size_t)2 * BN_BLOCKS * C : nullptr;
    static_assert(BN_BLOCKS == BN_MAIN_BLOCKS, "the companion's blocks sit behind the batch norm's own");
    bool side_single = false;
    if (companion) {
        if (int rc = bn_side_setup("mkgnn_batchnorm_forward", companion, companion_ws, companion_ws_bytes, a.side)) return rc;
        if ((int64_t)companion->n_rows * a.side.CL <= 64 * 1024) { a.side.nblk = 1; side_single = true; }
    }
    const bool one_launch = switches().bn_one_launch;    // (opt-in: it lost)
    if (training && one_launch) {                        // statistics | grid barrier | apply  (MKGNN_BN_ONE_LAUNCH=0: two launches)
        if (bn_vec_rows(x, x_stride, C)) bn_forward_fused_kernel<true><<<BN_BLOCKS + a.side.nblk, 256, 0, st>>>(a, CL);
        else bn_forward_fused_kernel<false><<<BN_BLOCKS + a.side.nblk, 256, 0, st>>>(a, CL);
    } else {
        if (training) {                                  // block statistics (the companion's blocks behind the batch norm's own)
            // ... and behind those the blocks of a pending mkgnn_touch_hint: this launch is bound by the latency of its two passes
            // over 11 MB, not by bandwidth -- the batch's index arrays are read beside them for nothing
            a.touch.count = 0;
            a.touch_first = BN_BLOCKS + a.side.nblk;
            const int extra = take_touch_hint(a.touch) ? TOUCH_BLOCKS : 0;
            PrepManyArgs pm;
            if (take_pending_prepare(pm)) {              // ... and behind those a pending bank preparation's tasks
                pm.touch.count = 0;
                const int prep_first = a.touch_first + extra;
                if (bn_vec_rows(x, x_stride, C)) bn_stats_prep_kernel<true><<<prep_first + pm.prep_blocks, 256, 0, st>>>(a, CL, pm, prep_first);
                else bn_stats_prep_kernel<false><<<prep_first + pm.prep_blocks, 256, 0, st>>>(a, CL, pm, prep_first);
            } else if (bn_vec_rows(x, x_stride, C)) bn_stats_kernel<true><<<BN_BLOCKS + a.side.nblk + extra, 256, 0, st>>>(a, CL);
            else bn_stats_kernel<false><<<BN_BLOCKS + a.side.nblk + extra, 256, 0, st>>>(a, CL);
            a.touch.count = 0;
        }
        bn_apply_kernel<<<BN_BLOCKS + ((a.side.nblk && !side_single) ? 1 : 0), 256, 0, st>>>(a, CL);
    }
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : api_hip_fail("mkgnn_batchnorm_forward", e);
}

int mkgnn_batchnorm_backward(const float* grad_out, int64_t grad_out_stride, const float* x, int64_t x_stride,
                             int64_t n_rows, int32_t C, const float* weight, const float* save_mean,
                             const float* save_invstd, int32_t training, float* grad_x, int64_t grad_x_stride, float* grad_weight, float* grad_bias,
                             const int64_t* n_valid_rows, void* ws, size_t ws_bytes, void* stream) {
    int CL;
    if (int rc = bn_common("mkgnn_batchnorm_backward", n_rows, C, CL)) return rc;
    if (!grad_out || !x || grad_out_stride < C || x_stride < C) return api_fail("mkgnn_batchnorm_backward: bad grad_out/x");
    if (!save_mean || !save_invstd) return api_fail("mkgnn_batchnorm_backward: saved statistics are null");
    if (grad_x && grad_x_stride < C) return api_fail("mkgnn_batchnorm_backward: bad grad_x stride");
    if (!ws || ws_bytes < mkgnn_batchnorm_workspace_bytes(C)) return api_fail("mkgnn_batchnorm_backward: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    BnArgs a{};
    a.x = x; a.xs = x_stride; a.n = n_rows; a.C = C; a.weight = weight;
    a.training = training;
    a.save_mean = (float*)save_mean; a.save_invstd = (float*)save_invstd;
    a.part1 = (float*)ws; a.part2 = a.part1 + (size_t)BN_BLOCKS * C;
    a.gout = grad_out; a.gos = grad_out_stride; a.gx = grad_x; a.gxs = grad_x_stride;
    a.gweight = grad_weight; a.gbias = grad_bias; a.nvalid = n_valid_rows; a.merge = bn_merge_on();
    const bool one_launch = switches().bn_one_launch;    // (opt-in: it lost)
    const bool vec = bn_vec_rows(x, x_stride, C) && bn_vec_rows(grad_out, grad_out_stride, C) && (!grad_x || bn_vec_rows(grad_x, grad_x_stride, C));
    if (one_launch && grad_x) {                          // partial sums | grid barrier | gradient rows
        if (vec) bn_backward_fused_kernel<true><<<BN_BLOCKS, 256, 0, st>>>(a, CL);
        else bn_backward_fused_kernel<false><<<BN_BLOCKS, 256, 0, st>>>(a, CL);
    } else if (vec) {
        bn_bwd_partial_kernel<true><<<BN_BLOCKS, 256, 0, st>>>(a, CL);
        bn_bwd_final_kernel<true><<<grad_x ? BN_BLOCKS : 1, 256, 0, st>>>(a, CL, BN_BLOCKS);
    } else {
        bn_bwd_partial_kernel<false><<<BN_BLOCKS, 256, 0, st>>>(a, CL);
        bn_bwd_final_kernel<false><<<grad_x ? BN_BLOCKS : 1, 256, 0, st>>>(a, CL, BN_BLOCKS);
    }
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : api_hip_fail("mkgnn_batchnorm_backward", e);
}

}  // extern "C"
