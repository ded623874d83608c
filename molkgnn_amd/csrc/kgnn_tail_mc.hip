// Monte Carlo dropout on the fused tail (mkgnn_tail_score_mc, kgnn_readout.hip): S stochastic predictions of every molecule
// from ONE run of everything in front of the two dropouts, and their mean, spread and acquisition value.
//
// Both dropouts of the model sit behind the last convolution (the readout's between swish(lin1(h)) and lin2, MolKGNNNet.py:144-146;
// the head's on the graph embedding, model.py:147-150), so propagate, lin1 and swish are the same for every sample: S samples
// differ only from the point where a chunk of molecules already sits in LDS inside the tail's middle kernel.  The masks are
// counter-based (kgnn_philox.h), nothing is stored, and sample s is DEFINED as what a training step with generator state
// {seed, offset + s} would have predicted: samples[g][s] is bit for bit the pred[g] of mkgnn_tail_fused_readout_dropout.
//
// The kernel is the forward-only form of kgnn_tail.hip (tail_middle_kernel<.., FWD>) -- its prologue, window, P1 and P3, in its own
// statements -- with the unmasked swish rows kept in registers (sw) and, per chunk,
//     RO (readout dropout):  per sample -- image = sw * readout keep(offset + s); barrier; P4's pool / lin2 / head with the head's
//                            keep(offset + s) into the chunk's [molecule][s] LDS slots; barrier (the next sample overwrites the image)
//     !RO:                   image = sw once; pool and lin2 once per molecule; per sample only the head's keep and its row sum --
//                            a row slot works on its own molecule, so the loop needs no barrier
// then the statistics of every molecule from its S slots (one thread per molecule, sample order, single IEEE operations), and the
// slots themselves to memory when asked for.  pred / emb, when asked for, come from one more pass without masks: mkgnn_tail_score's
// bits.  No atomics, one writer per output.  Work distribution: the training form's groups and grid -- though no bit of a
// molecule's outputs depends on them: its samples are sums over its own atoms in a fixed order with masks that are functions of
// (seed, offset + s, atom row, h) and (seed, offset + s, molecule, j).
#include <hip/hip_runtime.h>
#include <cstdint>
#include <math.h>

#include "kgnn_common.h"
#include "kgnn_launch.h"
#include "kgnn_philox.h"
#include "kgnn_sigmoid.h"
#include "kgnn_tail_shared.h"
#include "../../include/molkgnn_hip.h"

namespace mkgnn {
namespace tail {

constexpr int SMAX = MKGNN_TAIL_MC_MAX_SAMPLES;
constexpr int LDS_INTS_MC = (AC + 1) + EC + 2 * (MC + 1) + 4;
static_assert(SMAX % 16 == 0, "the statistics read the sample slots sixteen at a time");

// pool, lin2: emb[j] of the molecule whose swish rows are rows b0 .. b1_ - 1 of the image (P4 of tail_middle_kernel, its statements)
__device__ __forceinline__ float pool_lin2(const float* dzb, const float* W2s, const float* vec, int b0, int b1_, int j) {
    float e = 0.f;
    for (int at = b0; at < b1_; at += 8) {               // (eight reads in flight; the order of the sum stays atom by atom)
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = dzb[(at + u < b1_ ? at + u : b1_ - 1) * HP + j];
#pragma unroll
        for (int u = 0; u < 8; ++u) if (at + u < b1_) e += v[u];
    }
    const float cnt = (float)(b1_ - b0);
    float emb = vec[32 + j] * cnt;
#pragma unroll
    for (int k = 0; k < 32; ++k) emb = fmaf(W2s[j * WP + k], lane_of(e, k), emb);
    return emb;
}

// mean, unbiased standard deviation and acquisition value of x[0 .. S - 1], in sample order, every step ONE IEEE round-to-nearest
// float32 operation (readout.mc_statistics_reference mirrors it in numpy).  Written with plain operators under contract(off):
// this compiler's __fadd_rn / __fmul_rn are those operators and may be fused into an fma, its __fsqrt_rn is the approximate
// square root; '/' and __builtin_sqrtf are the correctly rounded ones (no fast-math flag in this build).
__device__ __forceinline__ void mc_statistics(const float* x, int S, float alpha, float beta, float& mean, float& sd, float& acq) {
#pragma clang fp contract(off)
    float sum = 0.f;
    for (int s0 = 0; s0 < S; s0 += 16) {                 // (sixteen reads in flight; the adds stay in sample order)
        float v[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) v[u] = x[s0 + u < S ? s0 + u : S - 1];
#pragma unroll
        for (int u = 0; u < 16; ++u) if (s0 + u < S) sum = sum + v[u];
    }
    mean = sum / (float)S;
    float q = 0.f;
    for (int s0 = 0; s0 < S; s0 += 16) {
        float v[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) v[u] = x[s0 + u < S ? s0 + u : S - 1];
#pragma unroll
        for (int u = 0; u < 16; ++u) if (s0 + u < S) { const float d = v[u] - mean; const float dd = d * d; q = q + dd; }
    }
    sd = 0.f;
    if (S > 1) { const float var = q / (float)(S - 1); sd = __builtin_sqrtf(var); }
    const float am = alpha * mean, bs = beta * sd;
    acq = am + bs;
}

template <bool RO>
__global__ void __launch_bounds__(NT, 3) tail_mc_kernel(TailMcArgs q) {
    const TailMidArgs& a = q.m;
    __shared__ __align__(16) float lds[LDS_FLOATS_FWD + MC * SMAX + LDS_INTS_MC];
    float* const W2s = lds;                              // [32][WP]
    float* const dzb = W2s + 32 * WP;                    // [AC][HP]: z, then the (masked) swish rows
    float* const vec = dzb + AC * HP;                    // b1 | b2 | wh
    float* const smp = vec + 96;                         // [MC][SMAX]: the chunk's samples
    int* const rpin = (int*)(smp + MC * SMAX);           // [AC + 1] local edge offsets, by target
    int* const ecin = rpin + AC + 1;                     // [EC] local source of every in-edge (-1: outside the chunk)
    int* const mptr = ecin + EC;                         // [MC + 1] first atom of every molecule of the window
    int* const mein = mptr + MC + 1;                     // [MC + 1] first in-edge
    int* const ctl = mein + MC + 1;                      // [0] molecules of this chunk
    const int t = threadIdx.x, j = t & 31, slot = t >> 5;      // the per-molecule phase: (row slot of 8, hidden unit)
    const int l = t & 7, as = t >> 3;                          // the per-atom phases: (atom slot of 32, 16-byte lane of 8)
    const int H = a.H, G = a.G, S = q.S;

    // ---- once: the weights (tail_middle_kernel's prologue)
    float w2r[4], vr = 0.f;
#pragma unroll
    for (int u = 0; u < 4; ++u) { const int i = t + NT * u; w2r[u] = a.w2[i < G * H ? i : 0]; }
    {
        const float* vp = t < 32 ? a.b1 : (t < 64 ? a.b2 : a.wh);
        const int lim = t < 32 ? H : G, k = t & 31;
        if (t < 96 && vp && k < lim) vr = vp[k];
    }
    const float bh = a.bh ? a.bh[0] : 0.f;
    const bool drop = a.drop_p > 0.f;
    const uint64_t seed = (uint64_t)a.rng[0], offset = (uint64_t)a.rng[1];
    const bool want_eval = a.pred != nullptr || a.emb != nullptr;      // the pass without masks: mkgnn_tail_score's outputs
    for (int i = t; i < 32 * WP; i += NT) W2s[i] = 0.f;
    if (t < 96) vec[t] = vr;
    __syncthreads();
#pragma unroll
    for (int u = 0; u < 4; ++u) { const int i = t + NT * u; if (i < G * H) { const int r = i / H, c = i - r * H; W2s[r * WP + c] = w2r[u]; } }

    const int MG = a.mg;
    const int64_t n_groups = (a.n_mols + MG - 1) / MG;
    int64_t grp = blockIdx.x;
    int64_t m_next = grp * MG;
    int64_t m_hi = m_next + MG < a.n_mols ? m_next + MG : a.n_mols;
    if (grp >= n_groups) m_next = m_hi = 0;

    __syncthreads();
    while (true) {
        if (m_next >= m_hi) {                            // (block-uniform) this group is done: the next one of this workgroup
            grp += gridDim.x;
            if (grp >= n_groups) break;
            m_next = grp * MG;
            m_hi = m_next + MG < a.n_mols ? m_next + MG : a.n_mols;
        }
        const int64_t m0 = m_next;
        // ---- the window: first atom and first edge of the next MC + 1 molecules
        if (t <= MC) {
            const int64_t m = m0 + t < a.n_mols ? m0 + t : a.n_mols;
            const int at = a.mol_ptr[m];
            mptr[t] = at;
            mein[t] = a.rin[at];
        }
        __syncthreads();
        if (t == 0) {
            int nm = 0;
            const int lim = (int)(m_hi - m0 < MC ? m_hi - m0 : MC);
            while (nm < lim && mptr[nm + 1] - mptr[0] <= AC && mein[nm + 1] - mein[0] <= EC) ++nm;
            ctl[0] = nm;
        }
        __syncthreads();
        const int nm = ctl[0];
        if (nm == 0) {                                   // (block-uniform) one molecule beyond a chunk: NaN in every output of its row
            const float nan = __builtin_nanf("");
            if (m0 < a.n_loss) {
                if (q.samples && t < S) q.samples[m0 * q.ss + t] = nan;
                if (t == 0) {
                    if (q.mean) q.mean[m0] = nan;
                    if (q.std) q.std[m0] = nan;
                    if (q.acq) q.acq[m0] = nan;
                    if (a.pred) a.pred[m0] = nan;
                }
            }
            if (a.emb && t < G) a.emb[m0 * a.es + t] = nan;
            m_next = m0 + 1;
            __syncthreads();
            continue;
        }
        m_next = m0 + nm;
        const int a0 = mptr[0], A = mptr[nm] - a0;
        const int ein0 = mein[0], nin = mein[nm] - ein0;
        // (A == 0: a chunk of empty molecules only -- see tail_middle_kernel: no load below leaves the arrays)
        // ---- P1: edge offsets; the z rows; the in-edges' sources
        if (t <= A) rpin[t] = a.rin[a0 + t] - ein0;
        {
            f32x4 zr[AC / 32];
            const int zlast = A > 0 ? a0 + A - 1 : 0;
#pragma unroll
            for (int u = 0; u < AC / 32; ++u) { const int at = as + 32 * u; zr[u] = *(const f32x4*)(a.z + (int64_t)(at < A ? a0 + at : zlast) * 32 + 4 * l); }
#pragma unroll
            for (int u = 0; u < AC / 32; ++u) { const int at = as + 32 * u; if (at < A) *(f32x4*)(dzb + at * HP + 4 * l) = zr[u]; }
        }
        {
            int ci[EC / NT];
#pragma unroll
            for (int u = 0; u < EC / NT; ++u) { const int i = t + NT * u; ci[u] = a.cin[nin > 0 ? ein0 + (i < nin ? i : 0) : 0]; }
#pragma unroll
            for (int u = 0; u < EC / NT; ++u) {
                const int i = t + NT * u;
                if (i < nin) { const int s = ci[u] - a0; ecin[i] = (s >= 0 && s < A) ? s : -1; }
            }
        }
        __syncthreads();
        // ---- P3: pre = b1 + sum of z over the in-edges; swish -- WITHOUT a mask, kept in registers for every sample
        f32x4 sw[AC / 32];
        {
            const f32x4 b1v = *(const f32x4*)(vec + 4 * l);
            f32x4 p[AC / 32];
            gather_rows<AC / 32>(rpin, ecin, dzb, as, A, l, p);
#pragma unroll
            for (int u = 0; u < AC / 32; ++u) {
                const int at = as + 32 * u;
                const f32x4 pv = b1v + p[u];
                sw[u] = f32x4{0.f, 0.f, 0.f, 0.f};
                if (at < A) {
#pragma unroll
                    for (int c = 0; c < 4; ++c) sw[u][c] = pv[c] * sigmoidf_(pv[c]);
                }
            }
        }
        __syncthreads();                                 // (everybody has read the z rows: the image may take their place)
        const float wv = vec[64 + j];
        if constexpr (RO) {
            // ---- per sample (s = -1: the pass without masks): the masked image, then P4 up to the prediction
            for (int s = want_eval ? -1 : 0; s < S; ++s) {
#pragma unroll
                for (int u = 0; u < AC / 32; ++u) {
                    const int at = as + 32 * u;
                    if (at < A) {
                        f32x4 v = sw[u];
                        if (s >= 0) {
                            float ks[4];
                            readout_keep4(seed, offset + (uint64_t)s, (int64_t)a0 + at, H, l, a.rdrop_p, ks);
#pragma unroll
                            for (int c = 0; c < 4; ++c) v[c] *= ks[c];
                        }
                        *(f32x4*)(dzb + at * HP + 4 * l) = v;
                    }
                }
                __syncthreads();
                for (int g = slot; g < nm; g += 8) {
                    const float emb = pool_lin2(dzb, W2s, vec, mptr[g] - a0, mptr[g + 1] - a0, j);
                    const int64_t gi = m0 + g;
                    const bool counted = gi < a.n_loss;
                    if (s < 0) {
                        if (a.emb && j < G) a.emb[gi * a.es + j] = emb;
                        const float ks = 1.f;
                        const float x = half_sum(j < G ? emb * ks * wv : 0.f) + bh;
                        if (a.pred && counted && j == 0) a.pred[gi] = x;
                    } else {
                        const float ks = (drop && j < G) ? keep_scale_of(seed, offset + (uint64_t)s, (uint64_t)(counted ? gi : 0) * G + j, a.drop_p) : 1.f;
                        const float x = half_sum(j < G ? emb * ks * wv : 0.f) + bh;
                        if (j == 0) smp[g * SMAX + s] = x;
                    }
                }
                // (the image is free for the next sample, and the slots are written, once everybody's LDS operations are done: a
                // barrier that does not wait for the stores to memory)
                asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
            }
        } else {
            // ---- the image once; per molecule pool and lin2 once, per sample the head's keep and its row sum
#pragma unroll
            for (int u = 0; u < AC / 32; ++u) { const int at = as + 32 * u; if (at < A) *(f32x4*)(dzb + at * HP + 4 * l) = sw[u]; }
            __syncthreads();
            for (int g = slot; g < nm; g += 8) {
                const float emb = pool_lin2(dzb, W2s, vec, mptr[g] - a0, mptr[g + 1] - a0, j);
                const int64_t gi = m0 + g;
                const bool counted = gi < a.n_loss;
                if (a.emb && j < G) a.emb[gi * a.es + j] = emb;
                if (a.pred) {
                    const float ks = 1.f;
                    const float x = half_sum(j < G ? emb * ks * wv : 0.f) + bh;
                    if (counted && j == 0) a.pred[gi] = x;
                }
                const uint64_t e0 = (uint64_t)(counted ? gi : 0) * G + j;
                for (int s = 0; s < S; ++s) {
                    const float ks = (drop && j < G) ? keep_scale_of(seed, offset + (uint64_t)s, e0, a.drop_p) : 1.f;
                    const float x = half_sum(j < G ? emb * ks * wv : 0.f) + bh;
                    if (j == 0) smp[g * SMAX + s] = x;
                }
            }
            asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
        }
        // ---- the chunk's outputs: the slots as they are (a run of S per molecule), and a thread per molecule for the statistics.
        // (the next chunk writes its first slot behind three more barriers)
        if (q.samples) {
            for (int i = t; i < nm * S; i += NT) {
                const int g = i / S, s = i - g * S;
                const int64_t gi = m0 + g;
                if (gi < a.n_loss) q.samples[gi * q.ss + s] = smp[g * SMAX + s];
            }
        }
        if (t < nm && m0 + t < a.n_loss && (q.mean || q.std || q.acq)) {
            float mean, sd, acq;
            mc_statistics(smp + t * SMAX, S, q.alpha, q.beta, mean, sd, acq);
            const int64_t gi = m0 + t;
            if (q.mean) q.mean[gi] = mean;
            if (q.std) q.std[gi] = sd;
            if (q.acq) q.acq[gi] = acq;
        }
    }
}

}  // namespace tail

hipError_t launch_tail_score_mc(const TailMcArgs& a, int nb, hipStream_t st) {
    if (a.m.mg < tail::MG_MIN || a.m.mg > tail::MG_MAX || a.m.mg > tail::MC) return hipErrorInvalidValue;
    if (a.S < 1 || a.S > tail::SMAX || !a.m.rng) return hipErrorInvalidValue;
    if (a.m.rdrop_p > 0.f) tail::tail_mc_kernel<true><<<nb, tail::NT, 0, st>>>(a);
    else tail::tail_mc_kernel<false><<<nb, tail::NT, 0, st>>>(a);
    return hipGetLastError();
}

}  // namespace mkgnn
