// Exact per-atom contributions to every logit of the head (mkgnn_atom_contributions).  In evaluation mode
// everything behind the last kernel convolution is
//     pre_n  = b1 + sum_{j -> n} z_j,   z_j = W1[:, block(j)] sim[j, block(j)]      (project, then propagate: kgnn_readout.hip)
//     emb_g  = W2 sum_{n in g} swish(pre_n) + |g| b2                                 (MolKGNNNet.py:144-146)
//     pred_g = Wh emb_g + bh                                                         (model.py:147-150)
// and lin2, the add-pool and the head are linear, so  pred[g, t] = bh[t] + sum_{n in g} c[n, t]  with
//     c[n, t] = sum_h V[t, h] swish(pre_n[h]) + c0[t],    V = Wh W2  ([T, H]),    c0[t] = Wh[t, :] . b2
// -- the share of atom n in task t's logit: exact, additive, complete.  This kernel writes c; bh is not part of it.
//
// One launch over atoms on the 32-float z rows block_project_mfma_kernel leaves (zero rows for atoms in no degree bucket, zero
// lanes beyond H).  A thread is (atom slot of 32, 16-byte lane l of 8: hidden units 4 l .. 4 l + 3), as the tail's gather_rows:
// the first four in-edges of the atom in one batch of loads -- offsets, then columns, then rows -- and a serial loop for the rare
// atom with more (a hub outside the degree buckets).  No molecule chunks, so no limit on a molecule's atoms or edges; neither
// mol_ptr nor atom_mol; no atomics; atom n's T outputs are written by the 8 lanes of its slot alone.
//
// V and c0 are formed by EVERY workgroup in its prologue, from Wh, W2 and b2 through LDS (at most 32 x 32 values of 32
// multiply-adds): a function of the parameters alone, the same bits in every workgroup for any grid.  LDS image of V: [t][32]
// rows at a pitch of 32 floats.  All lanes of a wave read row t at once -- 8 distinct 16-byte slots, 128 contiguous bytes,
// each broadcast to the 8 atom slots of the wave -- so no lane group of a ds_read_b128 sees two addresses on one bank and the rows
// need no padding.  (The staging image of Wh has a pitch of 33: the c0 threads read it one ROW per lane.)
//
// THE EVALUATION ORDER of an output -- one per output; the bits of c[n, t] depend on the parameters (W2, b1, b2), row t of Wh
// and the z rows of n's in-neighbours in CSR order alone: not on n_atoms, the atom's place in block or grid, other atoms, T,
// t's index, contrib_stride or head_stride:
//     V[t][h]   v = +0.0;  for g = 0 .. G - 1 in order:  v = fmaf(Wh[t][g], W2[g][h], v);           +0.0 for h >= H
//     c0[t]     v = +0.0;  for g = 0 .. G - 1 in order:  v = fmaf(Wh[t][g], b2[g], v);              +0.0 for a NULL b2
//     s[h]      +0.0, then  s += z[col[e]][h]  edge by edge in CSR order (plain adds);  an atom without in-edges keeps +0.0
//     pre[h]    s[h] + b1[h]                                                             (+0.0 for a NULL b1 and for h >= H)
//     a[h]      pre[h] * sigmoidf_(pre[h])                                               (kgnn_sigmoid.h: the tail's)
//     lane l    p = V[t][4 l] * a[4 l]  (a plain multiply), then fmaf(V[t][4 l + c], a[4 l + c], p) for c = 1, 2, 3
//     tree      the 8 lanes' p through an xor tree, offsets 4, 2, 1
//     c[n, t]   tree + c0[t]
#include <hip/hip_runtime.h>
#include <cstdint>
#include "kgnn_common.h"

#include "kgnn_launch.h"
#include "kgnn_sigmoid.h"
#include "../../include/molkgnn_hip.h"

namespace mkgnn {
namespace {

typedef mkgnn_f32x4 f32x4;

constexpr int AC_W = 32;                    // the z rows' width, and the most hidden units, embedding columns and tasks
constexpr int AC_SLOTS = 32;                // atoms per pass of a workgroup: 256 threads = 32 slots x 8 lanes
constexpr int AC_WHP = AC_W + 1;            // pitch of the Wh staging image
static_assert(MKGNN_ATOM_CONTRIB_MAX_TASKS == AC_W, "lane l of an atom's 8 keeps tasks l, l + 8, l + 16, l + 24");

__global__ void __launch_bounds__(256) atom_contrib_kernel(AtomContribArgs a) {
    __shared__ __align__(16) float Vs[AC_W * AC_W];          // V[t][h]
    __shared__ float w2s[AC_W * AC_W];                       // W2[g][h], zero beyond G / H
    __shared__ float whs[AC_W * AC_WHP];                     // Wh[t][g], zero beyond G
    __shared__ float b2s[AC_W];
    __shared__ float c0s[AC_W];
    const int tid = threadIdx.x, H = a.H, G = a.G, T = a.T;
    {   // ---- prologue: the parameters into LDS (loads unconditional and clamped, all in flight, masked after), then V and c0
        float w2v[4], whv[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int i = tid + 256 * k, r = i >> 5, c = i & 31;
            w2v[k] = a.w2[(r < G && c < H) ? r * H + c : 0];
            whv[k] = a.wh[(r < T && c < G) ? (int64_t)r * a.wh_stride + c : 0];
        }
        const float b2v = (a.b2 && tid < G) ? a.b2[tid] : 0.f;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int i = tid + 256 * k, r = i >> 5, c = i & 31;
            w2s[i] = (r < G && c < H) ? w2v[k] : 0.f;
            whs[r * AC_WHP + c] = (r < T && c < G) ? whv[k] : 0.f;
        }
        if (tid < AC_W) b2s[tid] = b2v;
        __syncthreads();
        for (int i = tid; i < T * AC_W; i += 256) {
            const int t = i >> 5, h = i & 31;
            float v = 0.f;
            for (int g = 0; g < G; ++g) v = fmaf(whs[t * AC_WHP + g], w2s[g * AC_W + h], v);
            Vs[i] = v;
        }
        if (tid < T) {
            float v = 0.f;
            for (int g = 0; g < G; ++g) v = fmaf(whs[tid * AC_WHP + g], b2s[g], v);
            c0s[tid] = v;
        }
        __syncthreads();
    }
    const int l = tid & 7, slot = tid >> 3;
    f32x4 b1v;
#pragma unroll
    for (int c = 0; c < 4; ++c) b1v[c] = (a.b1 && 4 * l + c < H) ? a.b1[4 * l + c] : 0.f;
    const uint32_t n32 = (uint32_t)a.n;                      // (n_atoms < 2^31)
    // (the trip count is the block's: no divergence round the shuffles; an atom slot beyond n works on atom n - 1 and stores nothing)
    for (int64_t base = (int64_t)blockIdx.x * AC_SLOTS; base < a.n; base += (int64_t)gridDim.x * AC_SLOTS) {
        const int64_t at = base + slot;
        const bool live = at < a.n;
        const int64_t ac = live ? at : a.n - 1;
        const int e0 = a.rin[ac], e1 = a.rin[ac + 1];
        f32x4 s = {0.f, 0.f, 0.f, 0.f};
        if (e0 < e1) {                                       // (nearly every atom; the loads inside are unconditional, clamped)
            int col[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) col[k] = a.cin[e0 + k < e1 ? e0 + k : e1 - 1];
            f32x4 v[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = *(const f32x4*)(a.z + (int64_t)((uint32_t)col[k] < n32 ? col[k] : 0) * AC_W + 4 * l);
#pragma unroll
            for (int k = 0; k < 4; ++k) if (e0 + k < e1 && (uint32_t)col[k] < n32) s += v[k];
            for (int e = e0 + 4; e < e1; ++e) {              // (more than four in-edges)
                const int c = a.cin[e];
                if ((uint32_t)c < n32) s += *(const f32x4*)(a.z + (int64_t)c * AC_W + 4 * l);
            }
        }
        f32x4 act;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const float pre = s[c] + b1v[c];
            act[c] = __fmul_rn(pre, sigmoidf_(pre));
        }
        float mine[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            for (int tt = 0; tt < 8 && 8 * j + tt < T; ++tt) {
                const int t = 8 * j + tt;
                const f32x4 v = *(const f32x4*)&Vs[t * AC_W + 4 * l];
                float p = __fmul_rn(v[0], act[0]);
                p = fmaf(v[1], act[1], p);
                p = fmaf(v[2], act[2], p);
                p = fmaf(v[3], act[3], p);
                p += __shfl_xor(p, 4, 64);
                p += __shfl_xor(p, 2, 64);
                p += __shfl_xor(p, 1, 64);
                const float c = p + c0s[t];
                if (tt == l) mine[j] = c;
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (live && 8 * j + l < T) a.out[at * a.os + 8 * j + l] = mine[j];
    }
}

}  // namespace

hipError_t launch_atom_contrib(const AtomContribArgs& a, hipStream_t st) {
    const int64_t passes = (a.n + AC_SLOTS - 1) / AC_SLOTS;
    const int grid = (int)(passes < ATOM_CONTRIB_MAX_BLOCKS ? passes : ATOM_CONTRIB_MAX_BLOCKS);
    atom_contrib_kernel<<<grid, 256, 0, st>>>(a);
    return hipGetLastError();
}

}  // namespace mkgnn
