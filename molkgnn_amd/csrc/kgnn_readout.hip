// The readout behind the kernel-convolution stack (the batch norm in front of it: kgnn_batchnorm.hip):
//
//   readout     pool_g( lin2( dropout( swish( lin1(h) ) ) ) )      reference MolKGNNNet.py:144-146
//
// Readout.  lin2 and the add-pool are both linear, so the molecule sum is taken first and lin2 is
// applied to one row per molecule: out_g = W2 (sum_{n in g} keep_n * swish(W1 h_n + b1)) + |g| b2.
// That removes the [N, H] x [H, G] product and its two gradients; what is left per atom is the
// [16 atoms x F] x [F x H] tile product, which runs on the fp32 matrix cores
// (v_mfma_f32_16x16x4_f32), fed straight from global memory with 16-byte loads: an MFMA's k index may
// be any permutation as long as both operands use the same one, so lane (row r, k-slot q) takes the
// four consecutive columns 16 j + 4 q .. + 3 of its row for the four k-steps of chunk j.
//
// Backward per 16-atom tile: dpre = dA[mol] * keep * swish'(pre) in registers, then two tile products,
// dh = dpre W1 (stored) and dW1 += dpre^T h (kept in accumulators for the whole kernel), followed by a
// fixed-order reduction block -> slab -> parameter.  No float atomics anywhere: results are reproducible.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "kgnn_common.h"
#include <mutex>

#include "kgnn_launch.h"
#include "kgnn_philox.h"
#include "../../include/molkgnn_hip.h"

namespace mkgnn {

typedef mkgnn_f32x4 f32x4;

struct ReadoutArgs {
    const float* h; int64_t hs; int64_t n;
    const int32_t* mol_ptr; const int32_t* atom_mol; int64_t nmol;
    const float *w1, *b1, *w2, *b2;
    int F, H, G;
    const float* keep;             // [n, H] dropout multipliers or null
    float* pre;                    // [n, HP]
    float* pooled;                 // [nmol, HP]
    float* out; int64_t os;
    const float* gout; int64_t gos;
    float* dA;                     // [nmol, HP]
    float* gh; int64_t ghs;
    float* slab_atoms; int slab_atoms_stride; int nblk_atoms;
    float* slab_mol; int slab_mol_stride; int nblk_mol;
    // block-row readout (mkgnn_readout_blocks_*): `pre` holds propagate(W1 sim) WITHOUT the bias, added where it is read
    const float* pre_bias;         // b1 (or null: pre includes it)
    float* gsum;                   // [nmol, HP] or null.  Forward (pool kernel): `pre` is OVERWRITTEN with the gate keep * swish'(pre + b1)
                                   // the backward multiplies by, gsum receives its per-molecule sums; backward (mol kernel): db1 from it
};

__device__ __forceinline__ float sigmoid_f(float p) { return 1.f / (1.f + expf(-p)); }

// A [rows, cols] row-major weight matrix -> LDS image [rows_pad][ld] (zero outside), eight loads in flight per thread.
// (Written as "for (i ...) lds[i] = ok ? w[...] : 0" the compiler keeps one conditional load in flight at a time:
// 16 dependent round trips ahead of readout_pre_kernel's first tile, ~10 of its 21 us.)
template <int NTHREADS>
__device__ __forceinline__ void weights_to_lds(float* lds, int total, int ld, const float* w, int rows, int cols, int tid) {
    for (int base = 0; base < total; base += NTHREADS * 8) {
        float tmp[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int i = base + tid + NTHREADS * k;
            const int ic = i < total ? i : total - 1;
            const int r = ic / ld, c = ic - r * ld;
            const bool ok = r < rows && c < cols;
            const float v = w[ok ? r * cols + c : 0];          // unconditional load, masked after
            tmp[k] = ok ? v : 0.f;
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int i = base + tid + NTHREADS * k;
            if (i < total) lds[i] = tmp[k];
        }
    }
}

// ------------------------------------------------------------------ forward: pre = h W1^T + b1 ----
template <int NT, int NJ>
__global__ void __launch_bounds__(256) readout_pre_kernel(ReadoutArgs a) {
    constexpr int HP = 16 * NT, FP = 16 * NJ, LDW = FP + 4;
    __shared__ __attribute__((aligned(16))) float w1s[HP * LDW];
    weights_to_lds<256>(w1s, HP * LDW, LDW, a.w1, a.H, a.F, threadIdx.x);
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane & 15, q = lane >> 4;
    float bias[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) bias[t] = (a.b1 && 16 * t + r < a.H) ? a.b1[16 * t + r] : 0.f;
    const int64_t ntiles = (a.n + 15) / 16;
    for (int64_t tile = (int64_t)blockIdx.x * 4 + wave; tile < ntiles; tile += (int64_t)gridDim.x * 4) {
        int64_t atom = tile * 16 + r;
        if (atom >= a.n) atom = a.n - 1;
        const float* row = a.h + atom * a.hs;
        f32x4 v[NJ];
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int col = 16 * j + 4 * q;
            v[j] = *(const f32x4*)(row + (col < a.F ? col : 0));
        }
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int col = 16 * j + 4 * q;
#pragma unroll
            for (int c = 0; c < 4; ++c) v[j][c] = (col + c < a.F) ? v[j][c] : 0.f;   // row padding may hold anything
        }
        f32x4 acc[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const f32x4 w = *(const f32x4*)&w1s[(16 * t + r) * LDW + 16 * j + 4 * q];
#pragma unroll
                for (int c = 0; c < 4; ++c) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(v[j][c], w[c], acc[t], 0, 0, 0);
            }
        }
#pragma unroll
        for (int t = 0; t < NT; ++t) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int64_t ao = tile * 16 + 4 * q + i;
                if (ao < a.n) a.pre[ao * HP + 16 * t + r] = acc[t][i] + bias[t];
            }
        }
    }
}

// -------------------------------------- forward: pooled_g = sum keep*swish(pre); out_g = W2 pooled_g + |g| b2 ----
__global__ void __launch_bounds__(256) readout_pool_kernel(ReadoutArgs a, int HP) {
    __shared__ float w2s[64 * 65];
    __shared__ float scr[4][64];
    const int H = a.H, G = a.G;
    weights_to_lds<256>(w2s, G * (H + 1), H + 1, a.w2, G, H, threadIdx.x);
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int groups = 64 / HP, c = lane & (HP - 1), gid = lane / HP;
    const bool kc = a.keep && c < H;
    const float pb = (a.pre_bias && c < H) ? a.pre_bias[c] : 0.f;
    for (int64_t mol = (int64_t)blockIdx.x * 4 + wave; mol < a.nmol; mol += (int64_t)gridDim.x * 4) {
        const int lo = a.mol_ptr[mol], hi = a.mol_ptr[mol + 1];
        float s = 0.f, gs = 0.f;
        for (int at0 = lo + gid; at0 < hi; at0 += 4 * groups) {
            float p[4], k[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int at = at0 + u * groups;
                const int atc = at < hi ? at : hi - 1;
                p[u] = a.pre[(int64_t)atc * HP + c] + pb;
                k[u] = kc ? a.keep[(int64_t)atc * H + c] : 1.f;
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const float sg = sigmoid_f(p[u]);
                const float v = p[u] * sg * k[u];
                if (at0 + u * groups < hi) {
                    s += v;
                    if (a.gsum) {                                // (wave-uniform) training: leave the backward's gate in place of pre
                        const float gate = c < H ? k[u] * (sg * fmaf(p[u], 1.f - sg, 1.f)) : 0.f;
                        a.pre[(int64_t)(at0 + u * groups) * HP + c] = gate;
                        gs += gate;
                    }
                }
            }
        }
        if (groups == 2) { s += __shfl_xor(s, 32, 64); gs += __shfl_xor(gs, 32, 64); }
        else if (groups == 4) { s += __shfl_xor(s, 16, 64); s += __shfl_xor(s, 32, 64); gs += __shfl_xor(gs, 16, 64); gs += __shfl_xor(gs, 32, 64); }
        if (gid == 0) { a.pooled[mol * HP + c] = s; scr[wave][c] = s; if (a.gsum) a.gsum[mol * HP + c] = gs; }
        __builtin_amdgcn_wave_barrier();
        if (lane < G) {
            float z = 0.f;
            for (int cc = 0; cc < H; ++cc) z = fmaf(w2s[lane * (H + 1) + cc], scr[wave][cc], z);
            if (a.b2) z = fmaf((float)(hi - lo), a.b2[lane], z);
            a.out[mol * a.os + lane] = z;
        }
        __builtin_amdgcn_wave_barrier();
    }
}

// ------------------- backward, per molecule: dA_g = dz_g W2; partial dW2 = dz^T pooled, db2 = sum |g| dz_g ----
__global__ void __launch_bounds__(256) readout_bwd_mol_kernel(ReadoutArgs a, int HP) {
    constexpr int MC = 16;
    __shared__ float w2s[64 * 65];
    __shared__ float dzs[MC][64];
    __shared__ float As[MC][64];
    __shared__ float nat[MC];
    const int H = a.H, G = a.G, tid = threadIdx.x;
    weights_to_lds<256>(w2s, G * (H + 1), H + 1, a.w2, G, H, tid);
    const int64_t per = (a.nmol + gridDim.x - 1) / gridDim.x;
    const int64_t m_lo = per * blockIdx.x, m_hi = (m_lo + per < a.nmol) ? m_lo + per : a.nmol;
    float accw[16];
    int po[16], pc[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        accw[k] = 0.f;
        int p = tid + 256 * k;
        if (p >= G * H) p = 0;
        po[k] = p / H; pc[k] = p - po[k] * H;
    }
    float accb = 0.f, accb1 = 0.f;
    for (int64_t m0 = m_lo; m0 < m_hi; m0 += MC) {
        __syncthreads();
        {   // MC * 64 = 4 * 256 entries: all loads first (unconditional, clamped), then the LDS stores
            float dz[4], av[4];
            int p0[4], p1[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int i = tid + 256 * k, m = i >> 6, o = i & 63;
                const int64_t mc = m0 + m < m_hi ? m0 + m : m_hi - 1;
                dz[k] = a.gout[mc * a.gos + (o < G ? o : 0)];
                av[k] = a.pooled[mc * HP + (o < H ? o : 0)];
                p0[k] = a.mol_ptr[mc]; p1[k] = a.mol_ptr[mc + 1];
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int i = tid + 256 * k, m = i >> 6, o = i & 63;
                const bool ok = m0 + m < m_hi;
                dzs[m][o] = (ok && o < G) ? dz[k] : 0.f;
                As[m][o] = (ok && o < H) ? av[k] : 0.f;
                if (o == 0) nat[m] = ok ? (float)(p1[k] - p0[k]) : 0.f;
            }
        }
        __syncthreads();
        for (int m = 0; m < MC; ++m) {
#pragma unroll
            for (int k = 0; k < 16; ++k)
                if (256 * k < G * H) accw[k] = fmaf(dzs[m][po[k]], As[m][pc[k]], accw[k]);      // (uniform: G * H = 1024 uses 4 of 16)
            if (tid < G) accb = fmaf(nat[m], dzs[m][tid], accb);
        }
        for (int i = tid; i < MC * HP; i += 256) {
            const int m = i / HP, c = i - m * HP;
            if (m0 + m < m_hi) {
                float v = 0.f;
                if (c < H)
                    for (int o = 0; o < G; ++o) v = fmaf(dzs[m][o], w2s[o * (H + 1) + c], v);
                a.dA[(m0 + m) * HP + c] = v;
                // block-row readout: db1 = sum_n dpre[n] = sum_mol dA[mol] * (sum of the molecule's gates); a thread's column
                // c = tid % HP is fixed (HP divides 256)
                if (a.gsum && c < H) accb1 = fmaf(v, a.gsum[(m0 + m) * HP + c], accb1);
            }
        }
    }
    float* slab = a.slab_mol + (int64_t)blockIdx.x * a.slab_mol_stride;
#pragma unroll
    for (int k = 0; k < 16; ++k) { const int p = tid + 256 * k; if (p < G * H) slab[p] = accw[k]; }
    if (tid < G) slab[G * H + tid] = accb;
    if (a.gsum) {                                            // db1 partial of this block: the 256 / HP thread groups in a fixed order
        __syncthreads();
        float* red = &dzs[0][0];                             // (MC * 64 >= 256 floats)
        red[tid] = accb1;
        __syncthreads();
        if (tid < HP) {
            float t = 0.f;
            for (int k = 0; k < 256 / HP; ++k) t += red[k * HP + tid];
            slab[G * H + G + tid] = t;
        }
    }
}

// ----------------------------------- backward, per atom tile: dpre, dh = dpre W1, dW1 += dpre^T h, db1 += dpre ----
template <int NT, int NU>
__global__ void __launch_bounds__(512) readout_bwd_atoms_kernel(ReadoutArgs a) {
    constexpr int NJ = 4 * NU, HP = 16 * NT, FP = 16 * NJ, LDW = FP + 4, LDP = HP + 4;
    constexpr int NW = NT == 4 ? 4 : 8;                               // two waves per SIMD where the 64 KB of static LDS allow it
    __shared__ __attribute__((aligned(16))) float w1s[HP * LDW];      // [hidden][feature]; reused for the block reduction
    __shared__ __attribute__((aligned(16))) float dps[NW][16 * LDP];  // per wave: dpre tile [atom][hidden]
    weights_to_lds<64 * NW>(w1s, HP * LDW, LDW, a.w1, a.H, a.F, threadIdx.x);
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane & 15, q = lane >> 4;
    float* dpw = dps[wave];
    f32x4 accw[NT][NJ];
    f32x4 colsum[NT];
#pragma unroll
    for (int mt = 0; mt < NT; ++mt) {
        colsum[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int t = 0; t < NJ; ++t) accw[mt][t] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    const int64_t ntiles = (a.n + 15) / 16;
    for (int64_t tile = (int64_t)blockIdx.x * NW + wave; tile < ntiles; tile += (int64_t)gridDim.x * NW) {
        // operand of the weight product: h rows 4 s + q, columns 64 u + 4 r .. + 3 (issued first: longest latency)
        f32x4 hv[4][NU];
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            int64_t ra = tile * 16 + 4 * s + q;
            if (ra >= a.n) ra = a.n - 1;
#pragma unroll
            for (int u = 0; u < NU; ++u) {
                const int col = 64 * u + 4 * r;
                hv[s][u] = *(const f32x4*)(a.h + ra * a.hs + (col < a.F ? col : 0));
            }
        }
        const int64_t atom = tile * 16 + r;
        const bool valid = atom < a.n;
        const int64_t atomc = valid ? atom : a.n - 1;
        const int mol = a.atom_mol[atomc];
        f32x4 dp[NT];
#pragma unroll
        for (int jj = 0; jj < NT; ++jj) {
            const int c0 = 16 * jj + 4 * q;
            const f32x4 p = *(const f32x4*)(a.pre + atomc * HP + c0);
            const f32x4 g = *(const f32x4*)(a.dA + (int64_t)mol * HP + c0);
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const float sg = sigmoid_f(p[c]);
                float d = g[c] * (sg * fmaf(p[c], 1.f - sg, 1.f));
                if (a.keep) d *= (c0 + c < a.H) ? a.keep[atomc * a.H + c0 + c] : 0.f;
                dp[jj][c] = valid ? d : 0.f;
            }
            colsum[jj] += dp[jj];
            *(f32x4*)&dpw[r * LDP + c0] = dp[jj];
        }
        // dh tile = dpre [16 x HP] . W1 [HP x FP]
        if (a.gh) {
            f32x4 acch[NJ];
#pragma unroll
            for (int t = 0; t < NJ; ++t) acch[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int jj = 0; jj < NT; ++jj) {
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const float* wrow = &w1s[(16 * jj + 4 * q + c) * LDW + r];
#pragma unroll
                    for (int t = 0; t < NJ; ++t)
                        acch[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(dp[jj][c], wrow[16 * t], acch[t], 0, 0, 0);
                }
            }
#pragma unroll
            for (int t = 0; t < NJ; ++t) {
                const int col = 16 * t + r;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int64_t ao = tile * 16 + 4 * q + i;
                    if (ao < a.n && col < a.F) a.gh[ao * a.ghs + col] = acch[t][i];
                }
            }
        }
        __builtin_amdgcn_wave_barrier();
        // dW1 += dpre^T [HP x 16 atoms] . h [16 atoms x FP]
#pragma unroll
        for (int s = 0; s < 4; ++s) {
#pragma unroll
            for (int u = 0; u < NU; ++u) {
                const int col = 64 * u + 4 * r;
#pragma unroll
                for (int c = 0; c < 4; ++c) hv[s][u][c] = (col + c < a.F) ? hv[s][u][c] : 0.f;
            }
#pragma unroll
            for (int mt = 0; mt < NT; ++mt) {
                const float at = dpw[(4 * s + q) * LDP + 16 * mt + r];
#pragma unroll
                for (int u = 0; u < NU; ++u)
#pragma unroll
                    for (int c = 0; c < 4; ++c)
                        accw[mt][4 * u + c] = __builtin_amdgcn_mfma_f32_16x16x4f32(at, hv[s][u][c], accw[mt][4 * u + c], 0, 0, 0);
            }
        }
        __builtin_amdgcn_wave_barrier();
    }
    // block reduction in wave order, then one slab row per block
    float* red = w1s;
#pragma unroll
    for (int jj = 0; jj < NT; ++jj)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            float v = colsum[jj][c];
            v += __shfl_xor(v, 1, 64); v += __shfl_xor(v, 2, 64); v += __shfl_xor(v, 4, 64); v += __shfl_xor(v, 8, 64);
            colsum[jj][c] = v;
        }
    // LDS image in lane order -- value k of lane l at red[k * 64 + l]: conflict-free.  (Indexed by (hidden, feature) the
    // lanes of an access were 512 bytes apart: 8-way bank conflicts.)  Cycle stamps of this kernel at batch 4096: weight
    // copy 3.5 k, three tiles of 14-20 k each, a fourth for one wave in eight (6412 tiles over 2048 waves) that the
    // rest of its block waits for at the barrier below, reduction + slab 5 k.
    // The (hidden, feature) mapping is applied once, on the way to the slab.
    constexpr int NV = NT * NJ * 4;                    // weight-gradient values per lane
    for (int w = 0; w < NW; ++w) {
        __syncthreads();
        if (wave == w) {
#pragma unroll
            for (int mt = 0; mt < NT; ++mt)
#pragma unroll
                for (int t = 0; t < NJ; ++t)
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int idx = ((mt * NJ + t) * 4 + i) * 64 + lane;
                        red[idx] = (w == 0) ? accw[mt][t][i] : red[idx] + accw[mt][t][i];
                    }
            if (r == 0) {
#pragma unroll
                for (int jj = 0; jj < NT; ++jj)
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        const int idx = NV * 64 + 16 * jj + 4 * q + c;
                        red[idx] = (w == 0) ? colsum[jj][c] : red[idx] + colsum[jj][c];
                    }
            }
        }
    }
    __syncthreads();
    float* slab = a.slab_atoms + (int64_t)blockIdx.x * a.slab_atoms_stride;
    for (int e = threadIdx.x; e < NV * 64; e += 64 * NW) {
        const int k = e >> 6, ln = e & 63, rr = ln & 15, qq = ln >> 4;
        const int i = k & 3, t = (k >> 2) % NJ, mt = (k >> 2) / NJ;
        const int hid = 16 * mt + 4 * qq + i, feat = 64 * (t >> 2) + 4 * rr + (t & 3);
        slab[hid * FP + feat] = red[e];
    }
    for (int e = threadIdx.x; e < HP; e += 64 * NW) slab[HP * FP + e] = red[NV * 64 + e];
}

// ------------------------------------------------ fixed-order sum of per-block slabs into the parameters ----
struct SlabSeg {
    const float* src; int stride; int count;    // count slabs, `stride` floats apart
    int src_cols, dst_rows, dst_cols;           // 2-D window [dst_rows, dst_cols] of a [*, src_cols] slab image
    float* dst;
    int blk_start;
    int dst_stride;                             // row stride of dst (0: dst_cols -- contiguous)
};
struct SlabReduceArgs {
    SlabSeg seg[12]; int nseg;
    float drop_p; int64_t* rng; int64_t* rng_used;      // the fused tail: the head's dropout generator advances here, once per step
};

// (blk == 0: none) mkgnn_tail_args.defer_reduce.  Per DEVICE, not per thread: the forward that leaves it runs on the caller's
// thread, the backward that takes it on autograd's.  (The header's rule -- one host thread per device inside these calls at a
// time -- is what orders the two; the mutex only keeps the slot itself whole.)
struct PendingReduce { SlabReduceArgs r; int blk; };
static PendingReduce g_pending_reduce_dev[16];
static std::mutex g_pending_reduce_mutex;
static PendingReduce* pending_reduce_slot() {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) dev = 0;
    return &g_pending_reduce_dev[dev];
}

__global__ void __launch_bounds__(256) slab_reduce_kernel(SlabReduceArgs a) {
    __shared__ float part[8][32];
    int si = 0;
    for (int s = 1; s < a.nseg; ++s) if ((int)blockIdx.x >= a.seg[s].blk_start) si = s;
    const SlabSeg g = a.seg[si];
    const int e = (blockIdx.x - g.blk_start) * 32 + (threadIdx.x & 31), p = threadIdx.x >> 5;
    const int total = g.dst_rows * g.dst_cols;
    const int ec = e < total ? e : total - 1;
    const int row = ec / g.dst_cols, col = ec - row * g.dst_cols;
    const float* src = g.src + row * g.src_cols + col;
    const int per = (g.count + 7) / 8;
    const int b0 = p * per, b1 = (b0 + per < g.count) ? b0 + per : g.count;
    float s = 0.f;
    for (int b = b0; b < b1; b += 8) {
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = src[(int64_t)(b + u < b1 ? b + u : b1 - 1) * g.stride];
#pragma unroll
        for (int u = 0; u < 8; ++u) if (b + u < b1) s += v[u];
    }
    part[p][threadIdx.x & 31] = s;
    __syncthreads();
    if (p == 0 && e < total) {
        float t = part[0][threadIdx.x];
#pragma unroll
        for (int k = 1; k < 8; ++k) t += part[k][threadIdx.x];
        g.dst[g.dst_stride ? (size_t)row * g.dst_stride + col : (size_t)e] = t;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0 && a.drop_p > 0.f && a.rng) {      // (as behind mkgnn_bce_head_fused)
        const int64_t seed = a.rng[0], offset = a.rng[1];
        a.rng_used[0] = seed; a.rng_used[1] = offset;
        a.rng[1] = offset + 1;
    }
}

// ---------------------------------------------------------------------- block-row readout (round 3) ----
// d loss / d z = propagate^T(dpre), dpre[t] = dA[mol(t)] * gate[t] taken on the fly (gate = keep * swish'(pre + b1), left
// in place of pre by the forward's pool kernel): row n of dz is the sum of dpre over n's neighbours t (the CSR of the edges by
// source) -- the [N x H] dpre array is never written or read.  CPR lanes per row (16-byte chunks of the HP-wide rows),
// 256 / CPR rows per pass; the first four neighbours' loads are all in flight at once (atoms have at most four neighbours
// but for a handful: the rest of such a row follows serially).
struct DzArgs {
    const float* dA; const float* gate; const int32_t* atom_mol;
    const int32_t* rowptr; const int32_t* col; int64_t n;
    float* dz;
};
constexpr int DZ_BLOCKS = 2048;

template <int CPR>
__global__ void __launch_bounds__(256) readout_dz_gather_kernel(DzArgs a) {
    constexpr int HP = 4 * CPR, RPB = 256 / CPR;
    const int tid = threadIdx.x, l = tid % CPR, rs = tid / CPR, c0 = 4 * l;
    for (int64_t r = (int64_t)blockIdx.x * RPB + rs; r < a.n; r += (int64_t)gridDim.x * RPB) {
        const int e0 = a.rowptr[r], e1 = a.rowptr[r + 1];
        int64_t t[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) t[j] = e0 + j < e1 ? (int64_t)a.col[e0 + j] : r;         // (clamped loads, masked below)
        int m[4];
        f32x4 g4[4], d4[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) { m[j] = a.atom_mol[t[j]]; g4[j] = *(const f32x4*)(a.gate + t[j] * HP + c0); }
#pragma unroll
        for (int j = 0; j < 4; ++j) d4[j] = *(const f32x4*)(a.dA + (int64_t)m[j] * HP + c0);
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < 4; ++j) if (e0 + j < e1) acc += d4[j] * g4[j];
        for (int e = e0 + 4; e < e1; ++e) {                                                  // (more than four neighbours)
            const int64_t tt = a.col[e];
            acc += *(const f32x4*)(a.dA + (int64_t)a.atom_mol[tt] * HP + c0) * *(const f32x4*)(a.gate + tt * HP + c0);
        }
        *(f32x4*)(a.dz + r * HP + c0) = acc;
    }
}

// The last kernel convolution's output sim goes nowhere but into  h = propagate(sim)  and  pre = W1 h + b1  (reference
// KernelLayer.py:119-123, MolKGNNNet.py:144-146).  Both are linear, and row n of sim is non-zero only in the column block
// of atom n's degree: project first, z[n] = W1[:, block(n)] sim[n, block(n)]  (H numbers from L_d), then propagate the
// H-wide rows instead of the K-wide ones, pre = propagate(z) (+ b1 where it is read).  Same sums, re-associated.  Removes a
// 45 MB dense h, its 45 MB gradient and the [N x K] x [K x H] tile products from the step.
struct BlockProjArgs {
    const float* sim; int64_t ss; int64_t n;
    const float* w1; int H, K, HP;
    int off[MKGNN_MAX_DEGREE], L[MKGNN_MAX_DEGREE];
    float* z;                                   // forward: [n, HP]
    // backward
    const float* dz;                            // [n, HP] = propagate^T(dpre)
    const int64_t* sel[MKGNN_MAX_DEGREE]; int64_t cnt[MKGNN_MAX_DEGREE];
    float* dsim; int64_t dss;                   // [n, K] block rows (only every atom's own block is written)
    float* slab; int slab_stride; int FP;       // per block: dW1 image [HP][FP]
};

// Both kernels work on TILES OF ONE DEGREE BUCKET (16 atoms of degree d in selected_index order, so the block [off, off + L)
// is the same for the whole tile) on the fp32 matrix cores; a block's four waves take four consecutive tiles of one bucket
// and share that degree's slice of W1 in LDS ([HP][LP], rows 16-byte aligned, zero beyond H / L).
//
// Lane layout of a tile (r = lane & 15, q = lane >> 4), as in readout_pre_kernel: lane (r, q) holds, of atom r's row, the four
// consecutive columns 16 j + 4 q .. + 3 of chunk j -- an MFMA's k index may be any permutation as long as both operands use
// the same one.
struct BlockTile { int di; int64_t t; int64_t cnt; int L, off, nj; };
__device__ __forceinline__ bool block_tile_of(const BlockProjArgs& a, int64_t blk, int wave, BlockTile& T) {
    // blocks are numbered bucket by bucket: bucket d has ceil(ceil(cnt_d / 16) / 4) of them
    int64_t b0 = 0;
    for (int di = 0; di < MKGNN_MAX_DEGREE; ++di) {
        const int64_t tiles = (a.cnt[di] + 15) / 16, nb = a.L[di] > 0 ? (tiles + 3) / 4 : 0;
        if (blk < b0 + nb) {
            T.di = di; T.t = (blk - b0) * 4 + wave; T.cnt = a.cnt[di]; T.L = a.L[di]; T.off = a.off[di]; T.nj = (a.L[di] + 15) / 16;
            return true;
        }
        b0 += nb;
    }
    return false;
}
// four consecutive floats of a row whose alignment (in floats, mod 4) is wave-uniform: one, two or four loads
__device__ __forceinline__ f32x4 load4_at(const float* p, int align4) {
    f32x4 v;
    if (align4 == 0) v = *(const f32x4*)p;
    else if (align4 == 2) { const float2 lo = *(const float2*)p, hi = *(const float2*)(p + 2); v = f32x4{lo.x, lo.y, hi.x, hi.y}; }
    else v = f32x4{p[0], p[1], p[2], p[3]};
    return v;
}
// this degree's slice of W1 -> LDS [HP][LP] (LP = 16 nj + 4), zero beyond H and L
__device__ __forceinline__ void w1_block_to_lds(float* w1s, const BlockProjArgs& a, int HP, int L, int off, int LP, int tid) {
    for (int i = tid; i < HP * LP; i += 256) {
        const int hid = i / LP, l = i - hid * LP;
        w1s[i] = (hid < a.H && l < L) ? a.w1[(size_t)hid * a.K + off + l] : 0.f;
    }
}

// z[n] = W1[:, block(n)] sim[n, block(n)]  for the atoms of the degree buckets: [16 atoms x L] . [L x HP] per tile
template <int NT>
__global__ void __launch_bounds__(256) block_project_mfma_kernel(BlockProjArgs a) {
    constexpr int HP = 16 * NT, LZ = HP + 4;
    extern __shared__ __align__(16) float lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, q = lane >> 4;
    BlockTile T;
    if (!block_tile_of(a, blockIdx.x, wave, T)) return;
    const int LP = 16 * T.nj + 4;
    float* const w1s = lds;
    float* const zt = lds + HP * 68 + wave * 16 * LZ;             // this wave's [16][LZ] transpose image
    w1_block_to_lds(w1s, a, HP, T.L, T.off, LP, tid);
    // the tile's rows while the weights arrive: lane (r, q) <- atom r, columns 16 j + 4 q .. + 3
    const int64_t p = T.t * 16 + r, pc = p < T.cnt ? p : T.cnt - 1;
    const bool tile_ok = T.t * 16 < T.cnt;
    const int64_t id = tile_ok ? a.sel[T.di][pc] : 0;
    const float* row = a.sim + id * a.ss + T.off;
    const int al = T.off & 3;                                      // (row bases are 16-byte aligned: the block's offset decides)
    f32x4 v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int col = 16 * j + 4 * q;
        v[j] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (j < T.nj && tile_ok) {
            if (col + 3 < T.L) v[j] = load4_at(row + col, al);
            else {                                                 // the block's last, partial chunk: element by element
#pragma unroll
                for (int c = 0; c < 4; ++c) v[j][c] = col + c < T.L ? row[col + c] : 0.f;
            }
        }
    }
    __syncthreads();
    f32x4 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (j < T.nj) {
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const f32x4 w = *(const f32x4*)&w1s[(16 * t + r) * LP + 16 * j + 4 * q];
#pragma unroll
                for (int c = 0; c < 4; ++c) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(v[j][c], w[c], acc[t], 0, 0, 0);
            }
        }
    }
    // acc[t][i] = z[atom 4 q + i][16 t + r]: through the wave's LDS image to whole 16-byte chunks of the z rows
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int i = 0; i < 4; ++i) zt[(4 * q + i) * LZ + 16 * t + r] = acc[t][i];
    __builtin_amdgcn_wave_barrier();
    constexpr int CPRZ = HP / 4;                                   // chunks per z row (8 or 16)
#pragma unroll
    for (int c0 = 0; c0 < 16 * CPRZ; c0 += 64) {
        const int cidx = c0 + lane, at = cidx / CPRZ, ch = cidx - at * CPRZ;
        const int64_t ida = __shfl(id, at, 64);                    // (lane `at` holds atom at's id: r = at, q = 0)
        if (T.t * 16 + at < T.cnt) *(f32x4*)(a.z + ida * HP + 4 * ch) = *(const f32x4*)&zt[at * LZ + 4 * ch];
    }
}

// Backward per tile:  dsim[n, block] = dz[n] W1[:, block]  ([16 x HP] . [HP x L]),  dW1[:, block] += dz^T sim  ([HP x 16] . [16 x L],
// accumulators in registers over the block's tiles, then block -> slab -> fixed-order reduction, one slab image per block
// holding only its degree's columns).
template <int NT>
__global__ void __launch_bounds__(256) block_project_bwd_mfma_kernel(BlockProjArgs a, int tiles_per_wave) {
    constexpr int HP = 16 * NT, LZ = HP + 4;
    extern __shared__ __align__(16) float lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, q = lane >> 4;
    // blocks bucket by bucket; a block takes 4 * tiles_per_wave consecutive tiles of its bucket
    int di = -1; int64_t blk_in = 0;
    {
        int64_t b0 = 0;
        for (int k = 0; k < MKGNN_MAX_DEGREE; ++k) {
            const int64_t tiles = (a.cnt[k] + 15) / 16, per = 4 * (int64_t)tiles_per_wave;
            const int64_t nb = a.L[k] > 0 ? (tiles + per - 1) / per : 0;
            if (di < 0 && (int64_t)blockIdx.x < b0 + nb) { di = k; blk_in = blockIdx.x - b0; }
            b0 += nb;
        }
    }
    if (di < 0) return;
    const int L = a.L[di], off = a.off[di], nj = (L + 15) / 16, LP = 16 * nj + 4;
    const int64_t cnt = a.cnt[di];
    float* const w1s = lds;                                        // [HP][LP]
    float* const dzs = lds + HP * 68 + wave * (16 * LZ + 16 * 68); // per wave: dz tile [16][LZ] | sim tile [16][68]
    float* const sms = dzs + 16 * LZ;
    w1_block_to_lds(w1s, a, HP, L, off, LP, tid);
    __syncthreads();
    const int al = off & 3;
    f32x4 accw[NT][4];
#pragma unroll
    for (int mt = 0; mt < NT; ++mt)
#pragma unroll
        for (int t = 0; t < 4; ++t) accw[mt][t] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int it = 0; it < tiles_per_wave; ++it) {
        const int64_t tile = (blk_in * 4 + wave) * tiles_per_wave + it;
        if (tile * 16 >= cnt) break;                               // (wave-uniform)
        const int64_t p = tile * 16 + r, pc = p < cnt ? p : cnt - 1;
        const int64_t id = a.sel[di][pc];
        const bool valid = p < cnt;
        // dz rows as the A operand of the dsim product (k = hidden unit 16 jh + 4 q + c); sim blocks for the dW1 product
        f32x4 dzv[NT], sv[4];
#pragma unroll
        for (int jh = 0; jh < NT; ++jh) dzv[jh] = *(const f32x4*)(a.dz + id * HP + 16 * jh + 4 * q);
        const float* row = a.sim + id * a.ss + off;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int col = 16 * j + 4 * q;
            sv[j] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (j < nj) {
                if (col + 3 < L) sv[j] = load4_at(row + col, al);
                else {
#pragma unroll
                    for (int c = 0; c < 4; ++c) sv[j][c] = col + c < L ? row[col + c] : 0.f;
                }
            }
        }
#pragma unroll
        for (int jh = 0; jh < NT; ++jh) {
            if (!valid) dzv[jh] = f32x4{0.f, 0.f, 0.f, 0.f};       // (a padding atom of the last tile contributes nothing)
            *(f32x4*)&dzs[r * LZ + 16 * jh + 4 * q] = dzv[jh];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) if (j < nj) *(f32x4*)&sms[r * 68 + 16 * j + 4 * q] = sv[j];
        __builtin_amdgcn_wave_barrier();
        // ---- dsim tile
        if (a.dsim) {
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                if (t < nj) {
                    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int jh = 0; jh < NT; ++jh)
#pragma unroll
                        for (int c = 0; c < 4; ++c)
                            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(dzv[jh][c], w1s[(16 * jh + 4 * q + c) * LP + 16 * t + r], acc, 0, 0, 0);
                    const int col = 16 * t + r;
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int at = 4 * q + i;
                        const int64_t ida = __shfl(id, at, 64);
                        if (tile * 16 + at < cnt && col < L) a.dsim[ida * a.dss + off + col] = acc[i];
                    }
                }
            }
        }
        // ---- dW1 += dz^T . sim  (k = atom 4 s + q)
#pragma unroll
        for (int s4 = 0; s4 < 4; ++s4) {
            float av[NT], bv[4];
#pragma unroll
            for (int mt = 0; mt < NT; ++mt) av[mt] = dzs[(4 * s4 + q) * LZ + 16 * mt + r];
#pragma unroll
            for (int t = 0; t < 4; ++t) bv[t] = t < nj ? sms[(4 * s4 + q) * 68 + 16 * t + r] : 0.f;
#pragma unroll
            for (int mt = 0; mt < NT; ++mt)
#pragma unroll
                for (int t = 0; t < 4; ++t)
                    if (t < nj) accw[mt][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[mt], bv[t], accw[mt][t], 0, 0, 0);
        }
        __builtin_amdgcn_wave_barrier();
    }
    // ---- block reduction of the four waves' accumulators (fixed order), one hidden tile at a time, then this block's slab:
    // [HP][FP], only its degree's columns
    float* const red = lds + HP * 68;                              // reuses the waves' tile images: [4 waves][4 column tiles][256]
    float* slab = a.slab + (size_t)blockIdx.x * a.slab_stride;
#pragma unroll
    for (int mt = 0; mt < NT; ++mt) {
        __syncthreads();
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int i = 0; i < 4; ++i) red[(wave * 4 + t) * 256 + i * 64 + lane] = accw[mt][t][i];
        __syncthreads();
        for (int e = tid; e < 4 * 256; e += 256) {
            const int t = e >> 8, i = (e & 255) >> 6, ln = e & 63;
            if (t < nj) {
                const float sum = (red[(0 * 4 + t) * 256 + (e & 255)] + red[(1 * 4 + t) * 256 + (e & 255)]) +
                                  (red[(2 * 4 + t) * 256 + (e & 255)] + red[(3 * 4 + t) * 256 + (e & 255)]);
                // accumulator element (i, lane): row (hidden) 16 mt + 4 (ln >> 4) + i, column 16 t + (ln & 15)
                const int hid = 16 * mt + 4 * (ln >> 4) + i, col = 16 * t + (ln & 15);
                if (col < L) slab[(size_t)hid * a.FP + off + col] = sum;
            }
        }
    }
}

}  // namespace mkgnn

using namespace mkgnn;

// ================================================================== C ABI ==========================
namespace {

struct ReadoutDims { int NT, NU, HP, FP; };

bool readout_dims(int F, int H, int G, ReadoutDims& d) {
    if (F < 1 || F > 128 || H < 1 || H > 64 || G < 1 || G > 64) return false;
    d.NT = H <= 32 ? 2 : 4;
    d.NU = F <= 64 ? 1 : 2;
    d.HP = 16 * d.NT;
    d.FP = 64 * d.NU;
    return true;
}

constexpr int RO_ATOM_BLOCKS = 256;
constexpr int RO_MOL_BLOCKS = 256;      // 16 molecules per block at batch 4096: one LDS chunk each

struct ReadoutWs { size_t dA, slab_atoms, slab_mol, total; int slab_atoms_stride, slab_mol_stride; };

ReadoutWs readout_ws(const ReadoutDims& d, int H, int G, int64_t nmol) {
    ReadoutWs w;
    auto up = [](size_t v) { return (v + 255) / 256 * 256; };
    w.slab_atoms_stride = d.HP * d.FP + d.HP;
    w.slab_mol_stride = G * H + G + d.HP;              // (+ the db1 partial of the block-row readout)
    w.dA = 0;
    w.slab_atoms = up(w.dA + (size_t)nmol * d.HP * 4);
    w.slab_mol = up(w.slab_atoms + (size_t)2 * RO_ATOM_BLOCKS * w.slab_atoms_stride * 4);   // (block-row readout: up to 2 x)
    w.total = up(w.slab_mol + (size_t)RO_MOL_BLOCKS * w.slab_mol_stride * 4);
    return w;
}

int check_readout(const char* who, const mkgnn_readout_params* p, const float* h, int64_t h_stride, int64_t n_atoms,
                  const int32_t* mol_ptr, int64_t n_mols, ReadoutDims& d) {
    if (!p) return api_fail("%s: params is null", who);
    if (!readout_dims(p->F, p->H, p->G, d))
        return api_fail("%s: shape F=%d H=%d G=%d outside F<=128, H<=64, G<=64", who, p->F, p->H, p->G);
    if (!p->lin1_weight || !p->lin2_weight) return api_fail("%s: weight pointer is null", who);
    if (n_atoms < 0 || n_mols < 0 || n_atoms >= (int64_t)1 << 31) return api_fail("%s: bad sizes", who);
    if (h_stride < (p->F + 3) / 4 * 4 || h_stride % 4 || ((uintptr_t)h & 15))
        return api_fail("%s: h rows must be 16-byte aligned with stride >= F rounded up to 4 (stride %lld)", who,
                        (long long)h_stride);
    if (n_atoms && (!h || !mol_ptr)) return api_fail("%s: h/mol_ptr is null", who);
    return 0;
}

ReadoutArgs readout_args(const mkgnn_readout_params* p, const float* h, int64_t hs, int64_t n, const int32_t* mol_ptr,
                         const int32_t* atom_mol, int64_t nmol, const float* keep, float* pre, float* pooled) {
    ReadoutArgs a{};
    a.h = h; a.hs = hs; a.n = n; a.mol_ptr = mol_ptr; a.atom_mol = atom_mol; a.nmol = nmol;
    a.w1 = p->lin1_weight; a.b1 = p->lin1_bias; a.w2 = p->lin2_weight; a.b2 = p->lin2_bias;
    a.F = p->F; a.H = p->H; a.G = p->G;
    a.keep = keep; a.pre = pre; a.pooled = pooled;
    return a;
}

}  // namespace

extern "C" {

int32_t mkgnn_readout_hidden_stride(int32_t H) { return H <= 32 ? 32 : 64; }

size_t mkgnn_readout_workspace_bytes(int32_t F, int32_t H, int32_t G, int64_t n_atoms, int64_t n_mols) {
    ReadoutDims d;
    if (!readout_dims(F, H, G, d) || n_mols < 0) return 0;
    (void)n_atoms;
    return readout_ws(d, H, G, n_mols).total;
}

int mkgnn_readout_forward(const mkgnn_readout_params* p, const float* h, int64_t h_stride, int64_t n_atoms,
                          const int32_t* mol_ptr, int64_t n_mols, const float* keep_scale, float* pre, float* pooled,
                          float* out, int64_t out_stride, void* stream) {
    ReadoutDims d;
    if (int rc = check_readout("mkgnn_readout_forward", p, h, h_stride, n_atoms, mol_ptr, n_mols, d)) return rc;
    if (n_mols && (!out || !pooled || out_stride < p->G)) return api_fail("mkgnn_readout_forward: bad out/pooled");
    if (n_atoms && !pre) return api_fail("mkgnn_readout_forward: pre is null");
    hipStream_t st = (hipStream_t)stream;
    ReadoutArgs a = readout_args(p, h, h_stride, n_atoms, mol_ptr, nullptr, n_mols, keep_scale, pre, pooled);
    a.out = out; a.os = out_stride;
    if (n_atoms) {
        const int64_t ntiles = (n_atoms + 15) / 16;
        const int grid = (int)((ntiles + 3) / 4 < 1024 ? (ntiles + 3) / 4 : 1024);
        if (d.NT == 2 && d.NU == 1) readout_pre_kernel<2, 4><<<grid, 256, 0, st>>>(a);
        else if (d.NT == 2) readout_pre_kernel<2, 8><<<grid, 256, 0, st>>>(a);
        else if (d.NU == 1) readout_pre_kernel<4, 4><<<grid, 256, 0, st>>>(a);
        else readout_pre_kernel<4, 8><<<grid, 256, 0, st>>>(a);
    }
    if (n_mols) {
        const int grid = (int)((n_mols + 3) / 4 < 2048 ? (n_mols + 3) / 4 : 2048);
        readout_pool_kernel<<<grid, 256, 0, st>>>(a, d.HP);
    }
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : api_hip_fail("mkgnn_readout_forward", e);
}

int mkgnn_readout_backward(const mkgnn_readout_params* p, const float* h, int64_t h_stride, int64_t n_atoms,
                           const int32_t* mol_ptr, const int32_t* atom_mol, int64_t n_mols, const float* keep_scale,
                           const float* pre, const float* pooled, const float* grad_out, int64_t grad_out_stride,
                           float* grad_h, int64_t grad_h_stride, float* grad_lin1_weight, float* grad_lin1_bias,
                           float* grad_lin2_weight, float* grad_lin2_bias, void* ws, size_t ws_bytes, void* stream) {
    ReadoutDims d;
    if (int rc = check_readout("mkgnn_readout_backward", p, h, h_stride, n_atoms, mol_ptr, n_mols, d)) return rc;
    if (n_atoms == 0 || n_mols == 0) return api_fail("mkgnn_readout_backward: empty batch");
    if (!atom_mol || !pre || !pooled || !grad_out || grad_out_stride < p->G)
        return api_fail("mkgnn_readout_backward: null pointer or bad grad_out stride");
    if (grad_h && grad_h_stride < p->F) return api_fail("mkgnn_readout_backward: bad grad_h stride");
    const ReadoutWs w = readout_ws(d, p->H, p->G, n_mols);
    if (!ws || ws_bytes < w.total) return api_fail("mkgnn_readout_backward: workspace too small (%zu < %zu)", ws_bytes, w.total);
    hipStream_t st = (hipStream_t)stream;
    ReadoutArgs a = readout_args(p, h, h_stride, n_atoms, mol_ptr, atom_mol, n_mols, keep_scale, (float*)pre, (float*)pooled);
    a.gout = grad_out; a.gos = grad_out_stride;
    a.dA = (float*)((char*)ws + w.dA);
    a.gh = grad_h; a.ghs = grad_h_stride;
    a.slab_atoms = (float*)((char*)ws + w.slab_atoms); a.slab_atoms_stride = w.slab_atoms_stride;
    a.slab_mol = (float*)((char*)ws + w.slab_mol); a.slab_mol_stride = w.slab_mol_stride;
    const int64_t ntiles = (n_atoms + 15) / 16;
    const int nw = d.NT == 4 ? 4 : 8;                // waves per block of readout_bwd_atoms_kernel
    a.nblk_atoms = (int)((ntiles + nw - 1) / nw < RO_ATOM_BLOCKS ? (ntiles + nw - 1) / nw : RO_ATOM_BLOCKS);
    a.nblk_mol = (int)((n_mols + 15) / 16 < RO_MOL_BLOCKS ? (n_mols + 15) / 16 : RO_MOL_BLOCKS);
    readout_bwd_mol_kernel<<<a.nblk_mol, 256, 0, st>>>(a, d.HP);
    if (d.NT == 2 && d.NU == 1) readout_bwd_atoms_kernel<2, 1><<<a.nblk_atoms, 512, 0, st>>>(a);
    else if (d.NT == 2) readout_bwd_atoms_kernel<2, 2><<<a.nblk_atoms, 512, 0, st>>>(a);
    else if (d.NU == 1) readout_bwd_atoms_kernel<4, 1><<<a.nblk_atoms, 256, 0, st>>>(a);
    else readout_bwd_atoms_kernel<4, 2><<<a.nblk_atoms, 256, 0, st>>>(a);
    SlabReduceArgs r{};
    int blk = 0;
    auto add = [&](const float* src, int stride, int count, int src_cols, int rows, int cols, float* dst) {
        if (!dst) return;
        SlabSeg& s = r.seg[r.nseg++];
        s.src = src; s.stride = stride; s.count = count; s.src_cols = src_cols; s.dst_rows = rows; s.dst_cols = cols;
        s.dst = dst; s.blk_start = blk;
        blk += (rows * cols + 31) / 32;
    };
    add(a.slab_atoms, a.slab_atoms_stride, a.nblk_atoms, d.FP, p->H, p->F, grad_lin1_weight);
    add(a.slab_atoms + d.HP * d.FP, a.slab_atoms_stride, a.nblk_atoms, d.HP, 1, p->H, grad_lin1_bias);
    add(a.slab_mol, a.slab_mol_stride, a.nblk_mol, p->H, p->G, p->H, grad_lin2_weight);
    add(a.slab_mol + p->G * p->H, a.slab_mol_stride, a.nblk_mol, p->G, 1, p->G, grad_lin2_bias);
    if (blk) slab_reduce_kernel<<<blk, 256, 0, st>>>(r);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : api_hip_fail("mkgnn_readout_backward", e);
}

// ---- block-row readout: see block_project_mfma_kernel.  Its own limits: H, G <= 64 (the pool / per-molecule kernels), K <= 255
// and every block <= 64 kernels; K may exceed the 128 columns of the dense tile-product kernels (they are not used here).
static bool blocks_dims(int K, int H, int G, ReadoutDims& d) {
    if (K < 1 || K > 255 || H < 1 || H > 64 || G < 1 || G > 64) return false;
    d.NT = H <= 32 ? 2 : 4;
    d.HP = 16 * d.NT;
    d.FP = (K + 63) / 64 * 64;
    d.NU = d.FP / 64;
    return true;
}

static int check_blocks(const char* who, const mkgnn_readout_params* p, const int32_t num_kernels[MKGNN_MAX_DEGREE],
                        const mkgnn_degree_bucket buckets[MKGNN_MAX_DEGREE], int64_t n_atoms, int64_t sim_stride, const float* sim,
                        BlockProjArgs& b, const ReadoutDims& d, int64_t* n_focal) {
    if (!num_kernels || !buckets) return api_fail("%s: num_kernels / buckets is null", who);
    int K = 0;
    int64_t n_bucketed = 0;
    *n_focal = 0;
    for (int i = 0; i < MKGNN_MAX_DEGREE; ++i) {
        if (num_kernels[i] < 0 || num_kernels[i] > 64) return api_fail("%s: num_kernels[%d] = %d outside 0..64", who, i, num_kernels[i]);
        b.off[i] = K; b.L[i] = num_kernels[i]; K += num_kernels[i];
        b.cnt[i] = buckets[i].count; b.sel[i] = buckets[i].selected_index;
        if (b.cnt[i] < 0 || (b.cnt[i] > 0 && !b.sel[i])) return api_fail("%s: degree %d bucket has no selected_index", who, i + 1);
        n_bucketed += b.cnt[i];
        if (num_kernels[i] > 0) *n_focal += b.cnt[i];        // (a bucket with atoms but no kernels launches no projection tile:
    }                                                        //  its z rows count as unwritten, the caller zero-fills)
    if (K != p->F) return api_fail("%s: lin1 takes %d columns, the blocks hold %d", who, p->F, K);
    if (sim_stride < K || sim_stride % 4 || !sim || ((uintptr_t)sim & 15)) return api_fail("%s: sim rows must be 16-byte aligned", who);
    if (n_bucketed > n_atoms) return api_fail("%s: the buckets hold more atoms than the batch", who);
    b.w1 = p->lin1_weight; b.H = p->H; b.K = K; b.HP = d.HP; b.FP = d.FP;
    return 0;
}

// z = W1[:, block] sim[block] for the blocks check_blocks filled in (d.NT = 2: H <= 32)
static hipError_t project_blocks(BlockProjArgs& b, const ReadoutDims& d, int64_t n_focal, const float* sim, int64_t sim_stride,
                                 int64_t n_atoms, float* z, hipStream_t st) {
    b.sim = sim; b.ss = sim_stride; b.n = n_atoms; b.z = z;
    if (n_focal < n_atoms) {                             // atoms in no bucket: their sim row is zero, and so is their z row
        const hipError_t e = hipMemsetAsync(z, 0, (size_t)n_atoms * d.HP * 4, st);
        if (e != hipSuccess) return e;
    }
    int64_t grid = 0;
    for (int i = 0; i < MKGNN_MAX_DEGREE; ++i) if (b.L[i] > 0) grid += ((b.cnt[i] + 15) / 16 + 3) / 4;
    if (grid > 0) {
        const size_t lds = ((size_t)d.HP * 68 + 4 * 16 * (d.HP + 4)) * 4;
        if (d.NT == 2) block_project_mfma_kernel<2><<<(unsigned)grid, 256, lds, st>>>(b);
        else block_project_mfma_kernel<4><<<(unsigned)grid, 256, lds, st>>>(b);
    }
    return hipSuccess;
}

size_t mkgnn_readout_blocks_workspace_bytes(int32_t K, int32_t H, int32_t G, int64_t n_mols) {
    ReadoutDims d;
    if (!blocks_dims(K, H, G, d) || n_mols < 0) return 0;
    return readout_ws(d, H, G, n_mols).total;
}

int mkgnn_readout_blocks_supported(int32_t F, int32_t H, int32_t G, const int32_t num_kernels[MKGNN_MAX_DEGREE]) {
    ReadoutDims d;
    if (!num_kernels || !blocks_dims(F, H, G, d)) return 0;
    int K = 0;
    for (int i = 0; i < MKGNN_MAX_DEGREE; ++i) { if (num_kernels[i] < 0 || num_kernels[i] > 64) return 0; K += num_kernels[i]; }
    return K == F;
}

int mkgnn_readout_blocks_forward(const mkgnn_readout_params* p, const float* sim, int64_t sim_stride,
                                 const int32_t num_kernels[MKGNN_MAX_DEGREE], const mkgnn_degree_bucket buckets[MKGNN_MAX_DEGREE],
                                 int64_t n_atoms, const int32_t* in_rowptr, const int32_t* in_col, const int32_t* mol_ptr,
                                 int64_t n_mols, const float* keep_scale, float* z, float* pre, float* pooled, float* gate_sum,
                                 float* out, int64_t out_stride, void* stream) {
    const char* who = "mkgnn_readout_blocks_forward";
    ReadoutDims d;
    if (!p || !blocks_dims(p->F, p->H, p->G, d)) return api_fail("%s: shape outside K<=255, H<=64, G<=64", who);
    if (!p->lin1_weight || !p->lin2_weight) return api_fail("%s: weight pointer is null", who);
    if (n_atoms < 1 || n_mols < 1 || n_atoms >= (int64_t)1 << 31) return api_fail("%s: bad sizes", who);
    if (!in_rowptr || !in_col || !mol_ptr || !z || !pre || !pooled || !out || out_stride < p->G)
        return api_fail("%s: null pointer or bad out stride", who);
    BlockProjArgs b{};
    int64_t n_focal = 0;
    if (int rc = check_blocks(who, p, num_kernels, buckets, n_atoms, sim_stride, sim, b, d, &n_focal)) return rc;
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = project_blocks(b, d, n_focal, sim, sim_stride, n_atoms, z, st);
    if (e != hipSuccess) return api_hip_fail(who, e);
    // pre = propagate(z): the propagate step on H-wide rows (+ b1 where pre is read)
    e = launch_segment_sum(z, d.HP, in_rowptr, in_col, n_atoms, d.HP, pre, d.HP, nullptr, st);
    if (e != hipSuccess) return api_hip_fail(who, e);
    ReadoutArgs a = readout_args(p, nullptr, 0, n_atoms, mol_ptr, nullptr, n_mols, keep_scale, pre, pooled);
    a.out = out; a.os = out_stride; a.pre_bias = p->lin1_bias; a.gsum = gate_sum;
    const int pgrid = (int)((n_mols + 3) / 4 < 2048 ? (n_mols + 3) / 4 : 2048);
    readout_pool_kernel<<<pgrid, 256, 0, st>>>(a, d.HP);
    e = hipGetLastError();
    return e == hipSuccess ? 0 : api_hip_fail(who, e);
}

int mkgnn_readout_blocks_backward(const mkgnn_readout_params* p, const float* sim, int64_t sim_stride,
                                  const int32_t num_kernels[MKGNN_MAX_DEGREE], const mkgnn_degree_bucket buckets[MKGNN_MAX_DEGREE],
                                  int64_t n_atoms, const int32_t* out_rowptr, const int32_t* out_col, const int32_t* mol_ptr,
                                  const int32_t* atom_mol, int64_t n_mols, const float* gate, const float* gate_sum,
                                  const float* pooled, const float* grad_out, int64_t grad_out_stride, float* dz,
                                  float* grad_sim, int64_t grad_sim_stride, float* grad_lin1_weight, float* grad_lin1_bias,
                                  float* grad_lin2_weight, float* grad_lin2_bias, void* ws, size_t ws_bytes, void* stream) {
    const char* who = "mkgnn_readout_blocks_backward";
    ReadoutDims d;
    if (!p || !blocks_dims(p->F, p->H, p->G, d)) return api_fail("%s: shape outside K<=255, H<=64, G<=64", who);
    if (n_atoms < 1 || n_mols < 1 || n_atoms >= (int64_t)1 << 31) return api_fail("%s: bad sizes", who);
    if (!out_rowptr || !out_col || !mol_ptr || !atom_mol || !gate || !gate_sum || !pooled || !grad_out || grad_out_stride < p->G || !dz)
        return api_fail("%s: null pointer or bad grad_out stride", who);
    BlockProjArgs b{};
    int64_t n_focal = 0;
    if (int rc = check_blocks(who, p, num_kernels, buckets, n_atoms, sim_stride, sim, b, d, &n_focal)) return rc;
    if (grad_sim && grad_sim_stride < b.K) return api_fail("%s: bad grad_sim stride", who);
    const ReadoutWs w = readout_ws(d, p->H, p->G, n_mols);
    if (!ws || ws_bytes < w.total) return api_fail("%s: workspace too small (%zu < %zu)", who, ws_bytes, w.total);
    hipStream_t st = (hipStream_t)stream;
    ReadoutArgs a = readout_args(p, nullptr, 0, n_atoms, mol_ptr, atom_mol, n_mols, nullptr, (float*)gate, (float*)pooled);
    a.gsum = (float*)gate_sum;
    a.gout = grad_out; a.gos = grad_out_stride;
    a.dA = (float*)((char*)ws + w.dA);
    a.slab_atoms = (float*)((char*)ws + w.slab_atoms); a.slab_atoms_stride = w.slab_atoms_stride;
    a.slab_mol = (float*)((char*)ws + w.slab_mol); a.slab_mol_stride = w.slab_mol_stride;
    a.nblk_mol = (int)((n_mols + 15) / 16 < RO_MOL_BLOCKS ? (n_mols + 15) / 16 : RO_MOL_BLOCKS);
    readout_bwd_mol_kernel<<<a.nblk_mol, 256, 0, st>>>(a, d.HP);
    // d loss / d z = propagate^T (d loss / d pre), d loss / d pre taken on the fly (readout_dz_gather_kernel)
    DzArgs z{};
    z.dA = a.dA; z.gate = gate; z.atom_mol = atom_mol; z.rowptr = out_rowptr; z.col = out_col; z.n = n_atoms; z.dz = dz;
    const int rpb = 256 / (d.HP / 4);
    const int nb_dz = (int)((n_atoms + rpb - 1) / rpb < DZ_BLOCKS ? (n_atoms + rpb - 1) / rpb : DZ_BLOCKS);
    if (d.NT == 2) readout_dz_gather_kernel<8><<<nb_dz, 256, 0, st>>>(z);
    else readout_dz_gather_kernel<16><<<nb_dz, 256, 0, st>>>(z);
    hipError_t e = hipSuccess;
    b.sim = sim; b.ss = sim_stride; b.n = n_atoms; b.dz = dz; b.dsim = grad_sim; b.dss = grad_sim_stride;
    // blocks bucket by bucket, 4 * tiles_per_wave tiles each; at most 2 * RO_ATOM_BLOCKS blocks (the slab capacity)
    int64_t tiles_all = 0;
    for (int i = 0; i < MKGNN_MAX_DEGREE; ++i) if (b.L[i] > 0) tiles_all += (b.cnt[i] + 15) / 16;
    int tpw = (int)((tiles_all + 4 * (2 * RO_ATOM_BLOCKS - 4) - 1) / (4 * (2 * RO_ATOM_BLOCKS - 4)));
    if (tpw < 1) tpw = 1;
    int64_t nb_of[MKGNN_MAX_DEGREE], nb = 0;
    for (int i = 0; i < MKGNN_MAX_DEGREE; ++i) {
        const int64_t tiles = (b.cnt[i] + 15) / 16, per = 4 * (int64_t)tpw;
        nb_of[i] = b.L[i] > 0 ? (tiles + per - 1) / per : 0;
        nb += nb_of[i];
    }
    if (nb > 2 * RO_ATOM_BLOCKS) return api_fail("%s: internal: %lld blocks for %d slabs", who, (long long)nb, 2 * RO_ATOM_BLOCKS);
    b.slab = a.slab_atoms; b.slab_stride = a.slab_atoms_stride;
    if (nb > 0) {
        const size_t img = (size_t)4 * (16 * (d.HP + 4) + 16 * 68);
        const size_t lds = ((size_t)d.HP * 68 + (img > 4096 ? img : 4096)) * 4;
        if (d.NT == 2) block_project_bwd_mfma_kernel<2><<<(unsigned)nb, 256, lds, st>>>(b, tpw);
        else block_project_bwd_mfma_kernel<4><<<(unsigned)nb, 256, lds, st>>>(b, tpw);
    }
    SlabReduceArgs r{};
    int blk = 0;
    auto add = [&](const float* src, int stride, int count, int src_cols, int rows, int cols, float* dst, int dst_stride) {
        if (!dst || count < 1 || rows * cols < 1) return;
        SlabSeg& sg = r.seg[r.nseg++];
        sg.src = src; sg.stride = stride; sg.count = count; sg.src_cols = src_cols; sg.dst_rows = rows; sg.dst_cols = cols;
        sg.dst = dst; sg.blk_start = blk; sg.dst_stride = dst_stride;
        blk += (rows * cols + 31) / 32;
    };
    // dW1: per degree, the column window [H x L_d] of its blocks' slab images -> columns [off_d, off_d + L_d) of grad_lin1_weight
    bool absent = false;
    {
        int64_t b0 = 0;
        for (int i = 0; i < MKGNN_MAX_DEGREE; ++i) {
            if (b.L[i] > 0 && nb_of[i] == 0) absent = true;
            if (nb_of[i] > 0)
                add(a.slab_atoms + (size_t)b0 * a.slab_atoms_stride + b.off[i], a.slab_atoms_stride, (int)nb_of[i], d.FP, p->H, b.L[i],
                    grad_lin1_weight ? grad_lin1_weight + b.off[i] : nullptr, b.K);
            b0 += nb_of[i];
        }
    }
    if (absent && grad_lin1_weight) {                    // a degree without atoms: its columns of the gradient are zero
        e = hipMemsetAsync(grad_lin1_weight, 0, (size_t)p->H * b.K * 4, st);
        if (e != hipSuccess) return api_hip_fail(who, e);
    }
    add(a.slab_mol + p->G * p->H + p->G, a.slab_mol_stride, a.nblk_mol, d.HP, 1, p->H, grad_lin1_bias, 0);
    add(a.slab_mol, a.slab_mol_stride, a.nblk_mol, p->H, p->G, p->H, grad_lin2_weight, 0);
    add(a.slab_mol + p->G * p->H, a.slab_mol_stride, a.nblk_mol, p->G, 1, p->G, grad_lin2_bias, 0);
    if (blk > 0) slab_reduce_kernel<<<blk, 256, 0, st>>>(r);
    e = hipGetLastError();
    return e == hipSuccess ? 0 : api_hip_fail(who, e);
}

// (on == false: none) mkgnn_tail_defer_projection: step (3) of a fused tail call, left to the last convolution's backward -- its
// coefficient pre-pass forms d sim itself and the dW1 half runs on the helper stream (launch_pending_tail_projection) -- or to
// whoever flushes first.  Per device and under the pending reduction's mutex, for its reasons.
struct PendingProject { BlockProjArgs b; int tpw; int64_t nb; size_t lds; bool on; };
static PendingProject g_pending_project_dev[16];
static bool g_defer_projection_dev[16];                  // the one-shot request of mkgnn_tail_defer_projection
static int pending_device() {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) dev = 0;
    return dev;
}
// blocks of block_project_bwd_mfma_kernel for the buckets in b: 4 * tiles_per_wave tiles each, at most 2 * RO_ATOM_BLOCKS (the slabs)
static int64_t project_bwd_blocks(const BlockProjArgs& b, int* tpw_out, int64_t nb_of[MKGNN_MAX_DEGREE]) {
    int64_t tiles_all = 0;
    for (int i = 0; i < MKGNN_MAX_DEGREE; ++i) if (b.L[i] > 0) tiles_all += (b.cnt[i] + 15) / 16;
    int tpw = (int)((tiles_all + 4 * (2 * RO_ATOM_BLOCKS - 4) - 1) / (4 * (2 * RO_ATOM_BLOCKS - 4)));
    if (tpw < 1) tpw = 1;
    int64_t nb = 0;
    for (int i = 0; i < MKGNN_MAX_DEGREE; ++i) {
        const int64_t tiles = (b.cnt[i] + 15) / 16, per = 4 * (int64_t)tpw;
        nb_of[i] = b.L[i] > 0 ? (tiles + per - 1) / per : 0;
        nb += nb_of[i];
    }
    *tpw_out = tpw;
    return nb;
}

// ---- the fused tail (ABI v6; kgnn_tail.hip): project | per-molecule middle | project^T + dW1 | one reduction ----
struct TailWs { size_t z, dz, slab_atoms, slab_tail, total; int slab_atoms_stride; };
static TailWs tail_ws(const ReadoutDims& d, int64_t n_atoms, int64_t n_mols, int slab_floats = TAIL_SLAB) {
    TailWs w;
    auto up = [](size_t v) { return (v + 255) / 256 * 256; };
    w.slab_atoms_stride = d.HP * d.FP + d.HP;
    w.z = 0;
    w.dz = up(w.z + (size_t)n_atoms * 32 * 4);
    w.slab_atoms = up(w.dz + (size_t)n_atoms * 32 * 4);
    w.slab_tail = up(w.slab_atoms + (size_t)2 * RO_ATOM_BLOCKS * w.slab_atoms_stride * 4);
    w.total = up(w.slab_tail + (size_t)(n_mols < TAIL_MAX_BLOCKS ? n_mols : TAIL_MAX_BLOCKS) * slab_floats * 4);   // (an upper bound for any n_loss_mols <= n_mols)
    return w;
}

int mkgnn_tail_supported(int32_t K, int32_t H, int32_t G, const int32_t num_kernels[MKGNN_MAX_DEGREE]) {
    ReadoutDims d;
    if (!num_kernels || !blocks_dims(K, H, G, d) || H > 32 || G > 32) return 0;
    return mkgnn_readout_blocks_supported(K, H, G, num_kernels);
}

size_t mkgnn_tail_workspace_bytes(int32_t K, int32_t H, int32_t G, int64_t n_atoms, int64_t n_mols) {
    ReadoutDims d;
    if (!blocks_dims(K, H, G, d) || n_atoms < 1 || n_mols < 1) return 0;
    return tail_ws(d, n_atoms, n_mols).total;
}

// What every entry point that starts from the z rows ends its front half with (d: blocks_dims' of a shape mkgnn_tail_supported
// takes): the block checks, the workspace (`total`: what the caller needs of it), a pending deferred reduction, the projection.
static int project_into_workspace(const char* who, const mkgnn_readout_params* ro, const int32_t num_kernels[MKGNN_MAX_DEGREE],
                                  const mkgnn_degree_bucket* buckets, const float* sim, int64_t sim_stride, int64_t n_atoms,
                                  size_t total, void* ws, size_t ws_bytes, hipStream_t st, BlockProjArgs& b, const ReadoutDims& d) {
    int64_t n_focal = 0;
    if (int rc = check_blocks(who, ro, num_kernels, buckets, n_atoms, sim_stride, sim, b, d, &n_focal)) return rc;
    if (!ws || ws_bytes < total) return api_fail("%s: workspace too small (%zu < %zu)", who, ws_bytes, total);
    hipError_t e = launch_pending_tail_projection(st, true);       // (it reads the d z rows and fills the slabs the reduction sums)
    if (e == hipSuccess) e = launch_pending_tail_reduce(st);
    if (e == hipSuccess) e = project_blocks(b, d, n_focal, sim, sim_stride, n_atoms, (float*)ws, st);
    return e == hipSuccess ? 0 : api_hip_fail(who, e);
}

// The front half of both tail entry points: the checks they share, with the caller's own (`own`) in their place behind the
// sizes; a reduction an earlier call left pending and nobody took, in front of this call's first launch (its kernels overwrite
// the workspace slabs the pending one still reads, and read the dropout generator state it advances); then
// (1) z = W1[:, block] sim[block] into the head of the workspace.  `need`: the caller's mkgnn_tail*_workspace_bytes.
extern "C++" template <typename Own>
static int tail_project(const char* who, const mkgnn_tail_args* p, Own&& own, size_t (*need)(int32_t, int32_t, int32_t, int64_t, int64_t),
                        void* ws, size_t ws_bytes, hipStream_t st, BlockProjArgs& b, ReadoutDims& d) {
    if (!p) return api_fail("%s: null argument", who);
    const mkgnn_readout_params* ro = &p->readout;
    if (!mkgnn_tail_supported(ro->F, ro->H, ro->G, p->num_kernels) || !blocks_dims(ro->F, ro->H, ro->G, d))
        return api_fail("%s: K=%d H=%d G=%d outside the fused tail (the block-row readout's shapes with H, G <= 32)", who, ro->F, ro->H, ro->G);
    if (p->n_atoms < 1 || p->n_mols < 1 || p->n_loss_mols < 1 || p->n_loss_mols > p->n_mols || p->n_atoms >= (int64_t)1 << 31)
        return api_fail("%s: bad sizes", who);
    if (int rc = own()) return rc;
    if (p->emb && p->emb_stride < ro->G) return api_fail("%s: bad emb stride", who);
    return project_into_workspace(who, ro, p->num_kernels, p->buckets, p->sim, p->sim_stride, p->n_atoms,
                                  need(ro->F, ro->H, ro->G, p->n_atoms, p->n_mols), ws, ws_bytes, st, b, d);
}

// the multi-output tail's workspace: the tail's with slabs for a [32][32] head gradient, then the partial labelled-entry counts
static size_t tail_labels_need(int32_t K, int32_t H, int32_t G, int64_t n_atoms, int64_t n_mols) {
    ReadoutDims d;
    if (!blocks_dims(K, H, G, d) || n_atoms < 1 || n_mols < 1) return 0;
    return tail_ws(d, n_atoms, n_mols, TAILL_SLAB).total + 256;
}
size_t mkgnn_tail_labels_workspace_bytes(int32_t K, int32_t H, int32_t G, int64_t n_atoms, int64_t n_mols, int32_t T) {
    if (T < 1 || T > MKGNN_TASK_HEAD_MAX_TASKS || H > 32 || G > 32) return 0;
    return tail_labels_need(K, H, G, n_atoms, n_mols);   // (the same for every T: a captured step's workspace does not move)
}

// rp: the readout's dropout (mkgnn_tail_fused_readout_dropout), 0 for mkgnn_tail_fused; wt: mkgnn_tail_fused_weighted's weights;
// lb: mkgnn_tail_fused_labels' T-output head and its labels (kgnn_tail_labels.hip in place of the single-task middle kernel)
static int tail_fused(const char* who, const mkgnn_tail_args* p, float rp, void* ws, size_t ws_bytes, void* stream,
                      const mkgnn_loss_weights* wt = nullptr, const mkgnn_tail_labels* lb = nullptr) {
    hipStream_t st = (hipStream_t)stream;
    BlockProjArgs b{};
    ReadoutDims d;
    auto own = [&]() {                                   // what the training tail asks beyond the scoring one
        const mkgnn_readout_params* ro = &p->readout;
        if (!p->in_rowptr || !p->in_col || !p->out_rowptr || !p->out_col || !p->mol_ptr || !p->atom_mol || !ro->lin1_weight ||
            !ro->lin2_weight || !p->head_weight || (!p->target && (!lb || lb->task)) || (lb ? !lb->pred : !p->pred) || !p->loss || !p->grad_sim)
            return api_fail("%s: null pointer", who);
        if (lb) {
            const int32_t T = lb->n_tasks;
            if (T < 1 || T > MKGNN_TASK_HEAD_MAX_TASKS) return api_fail("%s: %d tasks outside [1, %d]", who, (int)T, MKGNN_TASK_HEAD_MAX_TASKS);
            if ((lb->labels == nullptr) == (lb->task == nullptr)) return api_fail("%s: exactly one of labels and task", who);
            if (p->n_loss_mols * T >= (int64_t)1 << 31)
                return api_fail("%s: %lld molecules of %d tasks: the labelled-entry count needs n_loss_mols * T < 2^31", who, (long long)p->n_loss_mols, (int)T);
            if (lb->pred_stride < T || (lb->labels && lb->label_stride < T)) return api_fail("%s: label or pred row stride below T = %d", who, (int)T);
            const int64_t rows = lb->labels ? lb->n_label_rows : lb->n_task;
            if (lb->row_ids ? rows < 1 : rows < p->n_loss_mols) return api_fail("%s: the label source holds %lld rows", who, (long long)rows);
        }
        if (p->dropout_p < 0.f || p->dropout_p >= 1.f) return api_fail("%s: dropout probability %g outside [0, 1)", who, (double)p->dropout_p);
        if (p->dropout_p > 0.f && (!p->rng_state || !p->rng_used)) return api_fail("%s: dropout needs rng_state and rng_used", who);
        if (!(rp >= 0.f && rp < 1.f)) return api_fail("%s: readout dropout probability %g outside [0, 1)", who, (double)rp);
        if (rp > 0.f && (!p->rng_state || !p->rng_used)) return api_fail("%s: readout dropout needs rng_state and rng_used", who);
        if (p->loss_kind < MKGNN_LOSS_BCE_MEAN || p->loss_kind > MKGNN_LOSS_SQERR_SUM) return api_fail("%s: unknown loss kind %d", who, (int)p->loss_kind);
        if (p->grad_sim_stride < ro->F) return api_fail("%s: bad grad_sim stride", who);
        if (wt && wt->pos_weight && p->loss_kind != MKGNN_LOSS_BCE_MEAN) return api_fail("%s: pos_weight needs the BCE loss kind", who);
        if (wt && wt->sample_weight && (wt->weight_ids ? wt->n_sample_weight < 1 : wt->n_sample_weight < p->n_loss_mols))
            return api_fail("%s: sample_weight holds %lld entries", who, (long long)wt->n_sample_weight);
        return 0;
    };
    if (int rc = tail_project(who, p, own, lb ? tail_labels_need : mkgnn_tail_workspace_bytes, ws, ws_bytes, st, b, d)) return rc;
    const mkgnn_readout_params* ro = &p->readout;
    const TailWs w = tail_ws(d, p->n_atoms, p->n_mols, lb ? TAILL_SLAB : TAIL_SLAB);
    float* const z = (float*)((char*)ws + w.z);
    float* const dz = (float*)((char*)ws + w.dz);
    hipError_t e = hipSuccess;
    // (2) the middle: propagate, swish, pool, lin2, head, loss and the way back to d z, per chunk of whole molecules
    TailMidArgs m{};
    m.z = z; m.dz = dz; m.rin = p->in_rowptr; m.cin = p->in_col; m.rout = p->out_rowptr; m.cout = p->out_col;
    m.mol_ptr = p->mol_ptr; m.atom_mol = p->atom_mol; m.n_atoms = p->n_atoms; m.n_mols = p->n_mols; m.n_loss = p->n_loss_mols;
    m.b1 = ro->lin1_bias; m.w2 = ro->lin2_weight; m.b2 = ro->lin2_bias; m.wh = p->head_weight; m.bh = p->head_bias; m.y = p->target;
    m.H = ro->H; m.G = ro->G; m.drop_p = p->dropout_p; m.rng = p->rng_state; m.rdrop_p = rp;
    m.emb = p->emb; m.es = p->emb_stride; m.pred = p->pred;
    m.slab = (float*)((char*)ws + w.slab_tail); m.slab_stride = lb ? TAILL_SLAB : TAIL_SLAB;
    m.mg = tail_group_size(p->n_loss_mols);
    if (wt) {
        m.sw = wt->sample_weight; m.wids = wt->sample_weight ? wt->weight_ids : nullptr; m.n_sw = wt->n_sample_weight;
        m.pw = wt->pos_weight;
    }
    const int nbm = tail_middle_blocks(p->n_loss_mols);
    if (lb) {                                            // (the count launch, then the T-output middle kernel)
        TailLabelArgs la{};
        la.m = m; la.m.pred = nullptr;
        la.T = lb->n_tasks;
        la.labels = lb->labels; la.ls = lb->label_stride; la.n_label_rows = lb->n_label_rows;
        la.task = lb->task; la.n_task = lb->n_task; la.row_ids = lb->row_ids;
        la.pred = lb->pred; la.ps = lb->pred_stride;
        la.counts = (int*)((char*)ws + w.total); la.n_counts = tail_label_count_blocks(p->n_loss_mols, lb->n_tasks);
        e = launch_tail_labels_middle(la, nbm, p->loss_kind, st);
    } else {
        e = launch_tail_middle(m, nbm, p->loss_kind, st);
    }
    if (e != hipSuccess) return api_hip_fail(who, e);
    // (3) d sim[block] = W1[:, block]^T d z,  dW1 partials   (as mkgnn_readout_blocks_backward)
    b.dz = dz; b.dsim = p->grad_sim; b.dss = p->grad_sim_stride;
    int tpw = 1;
    int64_t nb_of[MKGNN_MAX_DEGREE];
    const int64_t nb = project_bwd_blocks(b, &tpw, nb_of);
    if (nb > 2 * RO_ATOM_BLOCKS) return api_fail("%s: internal: %lld blocks for %d slabs", who, (long long)nb, 2 * RO_ATOM_BLOCKS);
    float* const slab_atoms = (float*)((char*)ws + w.slab_atoms);
    b.slab = slab_atoms; b.slab_stride = w.slab_atoms_stride;
    const size_t proj_img = (size_t)4 * (16 * (d.HP + 4) + 16 * 68);
    const size_t proj_lds = ((size_t)d.HP * 68 + (proj_img > 4096 ? proj_img : 4096)) * 4;
    bool defer_proj = false;                             // mkgnn_tail_defer_projection: one-shot, and only beside a deferred reduction
    {
        std::lock_guard<std::mutex> lock(g_pending_reduce_mutex);
        bool& want = g_defer_projection_dev[pending_device()];
        defer_proj = want && p->defer_reduce && nb > 0 && switches().tail_project_in_prepass != 0;
        want = false;
    }
    if (nb > 0 && !defer_proj) {
        g_tail_projection_launches[1].fetch_add(1);
        block_project_bwd_mfma_kernel<2><<<(unsigned)nb, 256, proj_lds, st>>>(b, tpw);
    }
    // (4) every partial slab -> its gradient, the loss; the dropout generator advances (once, for either dropout or both)
    SlabReduceArgs r{};
    int blk = 0;
    auto add = [&](const float* src, int stride, int count, int src_cols, int rows, int cols, float* dst, int dst_stride) {
        if (!dst || count < 1 || rows * cols < 1) return;
        SlabSeg& sg = r.seg[r.nseg++];
        sg.src = src; sg.stride = stride; sg.count = count; sg.src_cols = src_cols; sg.dst_rows = rows; sg.dst_cols = cols;
        sg.dst = dst; sg.blk_start = blk; sg.dst_stride = dst_stride;
        blk += (rows * cols + 31) / 32;
    };
    bool absent = false;
    {
        int64_t b0 = 0;
        for (int i = 0; i < MKGNN_MAX_DEGREE; ++i) {
            if (b.L[i] > 0 && nb_of[i] == 0) absent = true;
            if (nb_of[i] > 0)
                add(slab_atoms + (size_t)b0 * w.slab_atoms_stride + b.off[i], w.slab_atoms_stride, (int)nb_of[i], d.FP, ro->H, b.L[i],
                    p->grad_lin1_weight ? p->grad_lin1_weight + b.off[i] : nullptr, b.K);
            b0 += nb_of[i];
        }
    }
    if (absent && p->grad_lin1_weight) {                 // a degree without atoms: its columns of the gradient are zero
        e = hipMemsetAsync(p->grad_lin1_weight, 0, (size_t)ro->H * b.K * 4, st);
        if (e != hipSuccess) return api_hip_fail(who, e);
    }
    if (lb) {                                            // (the head's segments: [T][32] and [T], reduced in block order as the others)
        add(m.slab + TAILL_B1, TAILL_SLAB, nbm, 32, 1, ro->H, p->grad_lin1_bias, 0);
        add(m.slab + TAILL_W2, TAILL_SLAB, nbm, 32, ro->G, ro->H, p->grad_lin2_weight, 0);
        add(m.slab + TAILL_B2, TAILL_SLAB, nbm, 32, 1, ro->G, p->grad_lin2_bias, 0);
        add(m.slab + TAILL_WH, TAILL_SLAB, nbm, 32, lb->n_tasks, ro->G, p->grad_head_weight, 0);
        add(m.slab + TAILL_BH, TAILL_SLAB, nbm, 32, 1, lb->n_tasks, p->grad_head_bias, 0);
        add(m.slab + TAILL_LOSS, TAILL_SLAB, nbm, 1, 1, 1, p->loss, 0);
    } else {
    add(m.slab + TAIL_B1, TAIL_SLAB, nbm, 32, 1, ro->H, p->grad_lin1_bias, 0);
    add(m.slab + TAIL_W2, TAIL_SLAB, nbm, 32, ro->G, ro->H, p->grad_lin2_weight, 0);
    add(m.slab + TAIL_B2, TAIL_SLAB, nbm, 32, 1, ro->G, p->grad_lin2_bias, 0);
    add(m.slab + TAIL_WH, TAIL_SLAB, nbm, 32, 1, ro->G, p->grad_head_weight, 0);
    add(m.slab + TAIL_BH, TAIL_SLAB, nbm, 1, 1, 1, p->grad_head_bias, 0);
    add(m.slab + TAIL_LOSS, TAIL_SLAB, nbm, 1, 1, 1, p->loss, 0);
    }
    r.drop_p = p->dropout_p > 0.f ? p->dropout_p : rp; r.rng = p->rng_state; r.rng_used = p->rng_used;
    if (p->defer_reduce && blk > 0) {                    // round 6: off the critical chain -- see mkgnn_tail_args.defer_reduce
        e = hipGetLastError();                           // (this call's launches so far: a failed one is reported, not left pending)
        if (e != hipSuccess) return api_hip_fail(who, e);
        std::lock_guard<std::mutex> lock(g_pending_reduce_mutex);
        PendingReduce* slot = pending_reduce_slot();
        slot->r = r; slot->blk = blk;
        if (defer_proj) {
            PendingProject& pp = g_pending_project_dev[pending_device()];
            pp.b = b; pp.tpw = tpw; pp.nb = nb; pp.lds = proj_lds; pp.on = true;
        }
        return 0;
    }
    if (defer_proj) {                                    // (no reduction to ride with after all: blk == 0)
        g_tail_projection_launches[1].fetch_add(1);
        block_project_bwd_mfma_kernel<2><<<(unsigned)nb, 256, proj_lds, st>>>(b, tpw);
    }
    if (blk > 0) slab_reduce_kernel<<<blk, 256, 0, st>>>(r);
    e = hipGetLastError();
    return e == hipSuccess ? 0 : api_hip_fail(who, e);
}

int mkgnn_tail_defer_projection(int32_t on) {
    std::lock_guard<std::mutex> lock(g_pending_reduce_mutex);
    g_defer_projection_dev[pending_device()] = on != 0;
    return 0;
}

int mkgnn_debug_tail_projection_launches(int64_t out[3]) {
    if (!out) return api_fail("mkgnn_debug_tail_projection_launches: null pointer");
    for (int i = 0; i < 3; ++i) out[i] = (int64_t)g_tail_projection_launches[i].load();
    return 0;
}

int mkgnn_tail_fused(const mkgnn_tail_args* p, void* ws, size_t ws_bytes, void* stream) {
    return tail_fused("mkgnn_tail_fused", p, 0.f, ws, ws_bytes, stream);
}

int mkgnn_tail_fused_readout_dropout(const mkgnn_tail_args* p, float readout_dropout_p, void* ws, size_t ws_bytes, void* stream) {
    return tail_fused("mkgnn_tail_fused_readout_dropout", p, readout_dropout_p, ws, ws_bytes, stream);
}

int mkgnn_tail_fused_weighted(const mkgnn_tail_args* p, float readout_dropout_p, const mkgnn_loss_weights* weights, void* ws,
                              size_t ws_bytes, void* stream) {
    return tail_fused("mkgnn_tail_fused_weighted", p, readout_dropout_p, ws, ws_bytes, stream, weights);
}

int mkgnn_tail_fused_labels(const mkgnn_tail_args* p, float readout_dropout_p, const mkgnn_tail_labels* labels,
                            const mkgnn_loss_weights* weights, void* ws, size_t ws_bytes, void* stream) {
    if (!labels) return api_fail("mkgnn_tail_fused_labels: null argument");
    return tail_fused("mkgnn_tail_fused_labels", p, readout_dropout_p, ws, ws_bytes, stream, weights, labels);
}

// ---- the forward-only tail (evaluation mode): project | the middle's forward phases -- two launches, pred and emb only ----
size_t mkgnn_tail_score_workspace_bytes(int32_t K, int32_t H, int32_t G, int64_t n_atoms, int64_t n_mols) {
    ReadoutDims d;
    if (!blocks_dims(K, H, G, d) || n_atoms < 1 || n_mols < 1) return 0;
    return tail_ws(d, n_atoms, n_mols).dz;               // (the z rows: where the training tail's d z rows would begin)
}

int mkgnn_tail_score(const mkgnn_tail_args* p, void* ws, size_t ws_bytes, void* stream) {
    const char* who = "mkgnn_tail_score";
    hipStream_t st = (hipStream_t)stream;
    BlockProjArgs b{};
    ReadoutDims d;
    auto own = [&]() {
        const mkgnn_readout_params* ro = &p->readout;
        if (!p->in_rowptr || !p->in_col || !p->mol_ptr || !p->atom_mol || !ro->lin1_weight || !ro->lin2_weight || !p->head_weight || !p->pred)
            return api_fail("%s: null pointer", who);
        return 0;
    };
    if (int rc = tail_project(who, p, own, mkgnn_tail_score_workspace_bytes, ws, ws_bytes, st, b, d)) return rc;
    const mkgnn_readout_params* ro = &p->readout;
    float* const z = (float*)ws;
    // (2) propagate, swish, pool, lin2, head: the training middle's forward phases, its groups and its grid
    TailMidArgs m{};
    m.z = z; m.rin = p->in_rowptr; m.cin = p->in_col; m.mol_ptr = p->mol_ptr; m.atom_mol = p->atom_mol;
    m.n_atoms = p->n_atoms; m.n_mols = p->n_mols; m.n_loss = p->n_loss_mols;
    m.b1 = ro->lin1_bias; m.w2 = ro->lin2_weight; m.b2 = ro->lin2_bias; m.wh = p->head_weight; m.bh = p->head_bias;
    m.H = ro->H; m.G = ro->G;
    m.emb = p->emb; m.es = p->emb_stride; m.pred = p->pred;
    m.mg = tail_group_size(p->n_loss_mols);
    const hipError_t e = launch_tail_score(m, tail_middle_blocks(p->n_loss_mols), st);      // (hipGetLastError: both launches)
    return e == hipSuccess ? 0 : api_hip_fail(who, e);
}

// ---- Monte Carlo dropout on the forward-only tail: project | the middle's forward phases, the part behind the masks S times
// (kgnn_tail_mc.hip) -- two launches; the generator pair is read, nothing is advanced, no state of the process is involved ----
size_t mkgnn_tail_score_mc_workspace_bytes(int32_t K, int32_t H, int32_t G, int64_t n_atoms, int64_t n_mols) {
    return mkgnn_tail_score_workspace_bytes(K, H, G, n_atoms, n_mols);      // (the z rows)
}

int mkgnn_tail_score_mc(const mkgnn_tail_args* p, float readout_dropout_p, int32_t n_samples, const int64_t* rng_pair,
                        const mkgnn_tail_mc_out* out, void* ws, size_t ws_bytes, void* stream) {
    const char* who = "mkgnn_tail_score_mc";
    hipStream_t st = (hipStream_t)stream;
    BlockProjArgs b{};
    ReadoutDims d;
    const float rp = readout_dropout_p;
    auto own = [&]() {
        const mkgnn_readout_params* ro = &p->readout;
        if (!p->in_rowptr || !p->in_col || !p->mol_ptr || !p->atom_mol || !ro->lin1_weight || !ro->lin2_weight || !p->head_weight ||
            !rng_pair || !out)
            return api_fail("%s: null pointer", who);
        if (n_samples < 1 || n_samples > MKGNN_TAIL_MC_MAX_SAMPLES)
            return api_fail("%s: %d samples outside [1, %d]", who, (int)n_samples, MKGNN_TAIL_MC_MAX_SAMPLES);
        if (!(p->dropout_p >= 0.f && p->dropout_p < 1.f)) return api_fail("%s: dropout probability %g outside [0, 1)", who, (double)p->dropout_p);
        if (!(rp >= 0.f && rp < 1.f)) return api_fail("%s: readout dropout probability %g outside [0, 1)", who, (double)rp);
        if (out->samples && out->samples_stride < n_samples)
            return api_fail("%s: samples stride %lld below %d samples", who, (long long)out->samples_stride, (int)n_samples);
        return 0;
    };
    if (int rc = tail_project(who, p, own, mkgnn_tail_score_mc_workspace_bytes, ws, ws_bytes, st, b, d)) return rc;
    const mkgnn_readout_params* ro = &p->readout;
    TailMcArgs q{};
    TailMidArgs& m = q.m;
    m.z = (float*)ws; m.rin = p->in_rowptr; m.cin = p->in_col; m.mol_ptr = p->mol_ptr; m.atom_mol = p->atom_mol;
    m.n_atoms = p->n_atoms; m.n_mols = p->n_mols; m.n_loss = p->n_loss_mols;
    m.b1 = ro->lin1_bias; m.w2 = ro->lin2_weight; m.b2 = ro->lin2_bias; m.wh = p->head_weight; m.bh = p->head_bias;
    m.H = ro->H; m.G = ro->G; m.drop_p = p->dropout_p; m.rdrop_p = rp; m.rng = rng_pair;
    m.emb = p->emb; m.es = p->emb_stride; m.pred = p->pred;
    m.mg = tail_group_size(p->n_loss_mols);
    q.S = n_samples; q.samples = out->samples; q.ss = out->samples_stride;
    q.mean = out->mean; q.std = out->std; q.acq = out->acq; q.alpha = out->alpha; q.beta = out->beta;
    const hipError_t e = launch_tail_score_mc(q, tail_middle_blocks(p->n_loss_mols), st);      // (hipGetLastError: both launches)
    return e == hipSuccess ? 0 : api_hip_fail(who, e);
}

// ---- every atom's share of every logit (evaluation mode): project | one kernel over atoms (kgnn_atom_contrib.hip) ----
size_t mkgnn_atom_contributions_workspace_bytes(int32_t K, int32_t H, int32_t G, int64_t n_atoms) {
    ReadoutDims d;
    if (!blocks_dims(K, H, G, d) || n_atoms < 1) return 0;
    return tail_ws(d, n_atoms, 1).dz;                    // (the z rows, as mkgnn_tail_score_workspace_bytes)
}

int mkgnn_atom_contributions(const mkgnn_atom_contrib_args* p, void* ws, size_t ws_bytes, void* stream) {
    const char* who = "mkgnn_atom_contributions";
    if (!p) return api_fail("%s: null argument", who);
    const mkgnn_readout_params* ro = &p->readout;
    ReadoutDims d;
    if (!mkgnn_tail_supported(ro->F, ro->H, ro->G, p->num_kernels) || !blocks_dims(ro->F, ro->H, ro->G, d))
        return api_fail("%s: K=%d H=%d G=%d outside the fused tail's shapes (the block-row readout's with H, G <= 32)", who, ro->F, ro->H, ro->G);
    if (p->T < 1 || p->T > MKGNN_ATOM_CONTRIB_MAX_TASKS)
        return api_fail("%s: %d tasks outside [1, %d]", who, (int)p->T, MKGNN_ATOM_CONTRIB_MAX_TASKS);
    if (p->n_atoms < 0 || p->n_atoms >= (int64_t)1 << 31) return api_fail("%s: bad sizes", who);
    if (p->contrib_stride < p->T) return api_fail("%s: contrib stride %lld below T = %d", who, (long long)p->contrib_stride, (int)p->T);
    if (p->head_stride < ro->G) return api_fail("%s: head stride %lld below G = %d", who, (long long)p->head_stride, ro->G);
    if (p->n_atoms == 0) return 0;
    if (!p->in_rowptr || !p->in_col || !ro->lin1_weight || !ro->lin2_weight || !p->head_weight || !p->contrib)
        return api_fail("%s: null pointer", who);
    hipStream_t st = (hipStream_t)stream;
    BlockProjArgs b{};
    if (int rc = project_into_workspace(who, ro, p->num_kernels, p->buckets, p->sim, p->sim_stride, p->n_atoms,
                                        mkgnn_atom_contributions_workspace_bytes(ro->F, ro->H, ro->G, p->n_atoms), ws, ws_bytes, st, b, d))
        return rc;
    AtomContribArgs a{};
    a.z = (const float*)ws; a.rin = p->in_rowptr; a.cin = p->in_col; a.n = p->n_atoms;
    a.b1 = ro->lin1_bias; a.w2 = ro->lin2_weight; a.b2 = ro->lin2_bias; a.wh = p->head_weight; a.wh_stride = p->head_stride;
    a.H = ro->H; a.G = ro->G; a.T = p->T;
    a.out = p->contrib; a.os = p->contrib_stride;
    const hipError_t e = launch_atom_contrib(a, st);
    return e == hipSuccess ? 0 : api_hip_fail(who, e);
}

// keep[r][h] of the readout's dropout: what the fused tail and the molecule-resident step draw for batch atom r (kgnn_philox.h)
struct ReadoutMaskArgs { const int64_t* rng; int64_t n; int H; float p; float* keep; int64_t ks; };
__global__ void __launch_bounds__(256) readout_dropout_mask_kernel(ReadoutMaskArgs a) {
    const int64_t total = a.n * a.H;
    const uint64_t seed = (uint64_t)a.rng[0], offset = (uint64_t)a.rng[1];
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t r = i / a.H;
        const int h = (int)(i - r * a.H);
        a.keep[r * a.ks + h] = keep_scale_of(seed, offset, readout_drop_element(r, a.H, h), a.p);
    }
}

int mkgnn_readout_dropout_mask(const int64_t* rng_pair, int64_t n_rows, int32_t H, float p, float* keep, int64_t keep_stride, void* stream) {
    const char* who = "mkgnn_readout_dropout_mask";
    if (!rng_pair || !keep) return api_fail("%s: null pointer", who);
    if (n_rows < 0 || H < 1 || keep_stride < H) return api_fail("%s: bad sizes", who);
    if (!(p >= 0.f && p < 1.f)) return api_fail("%s: dropout probability %g outside [0, 1)", who, (double)p);
    if (n_rows == 0) return 0;
    ReadoutMaskArgs a{rng_pair, n_rows, H, p, keep, keep_stride};
    const int64_t blocks = (n_rows * H + 255) / 256;
    readout_dropout_mask_kernel<<<(unsigned)(blocks < 4096 ? blocks : 4096), 256, 0, (hipStream_t)stream>>>(a);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : api_hip_fail(who, e);
}

extern "C++" {
namespace mkgnn {
hipError_t launch_pending_tail_reduce(hipStream_t st, bool* launched) {
    if (launched) *launched = false;
    std::lock_guard<std::mutex> lock(g_pending_reduce_mutex);
    PendingReduce* slot = pending_reduce_slot();
    if (slot->blk <= 0) return hipSuccess;
    const int blk = slot->blk;
    slot->blk = 0;
    slab_reduce_kernel<<<blk, 256, 0, st>>>(slot->r);
    if (launched) *launched = true;
    return hipGetLastError();
}

std::atomic<long long> g_tail_projection_launches[3];

bool pending_tail_projection(TailProjection* out) {
    std::lock_guard<std::mutex> lock(g_pending_reduce_mutex);
    const PendingProject& pp = g_pending_project_dev[pending_device()];
    if (!pp.on) return false;
    const BlockProjArgs& b = pp.b;
    out->dsim = b.dsim; out->dss = b.dss; out->dz = b.dz; out->w1 = b.w1; out->H = b.H; out->HP = b.HP; out->K = b.K;
    for (int i = 0; i < MKGNN_MAX_DEGREE; ++i) { out->off[i] = b.off[i]; out->L[i] = b.L[i]; out->sel[i] = b.sel[i]; out->cnt[i] = b.cnt[i]; }
    return true;
}

hipError_t launch_pending_tail_projection(hipStream_t st, bool full) {
    std::lock_guard<std::mutex> lock(g_pending_reduce_mutex);
    PendingProject& pp = g_pending_project_dev[pending_device()];
    if (!pp.on) return hipSuccess;
    pp.on = false;
    BlockProjArgs b = pp.b;
    if (!full) b.dsim = nullptr;
    g_tail_projection_launches[full ? 1 : 2].fetch_add(1);
    block_project_bwd_mfma_kernel<2><<<(unsigned)pp.nb, 256, pp.lds, st>>>(b, pp.tpw);
    return hipGetLastError();
}
}  // namespace mkgnn
}

extern "C" int mkgnn_tail_flush(void* stream) {
    hipError_t e = launch_pending_tail_projection((hipStream_t)stream, true);
    if (e == hipSuccess) e = launch_pending_tail_reduce((hipStream_t)stream);
    return e == hipSuccess ? 0 : api_hip_fail("mkgnn_tail_flush", e);
}

}  // extern "C"
