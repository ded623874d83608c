// What the single-task head (kgnn_head.hip) and the task-indexed head (kgnn_task_head.hip) share: the block shape, the row
// reduction and the loss kinds' terms -- one copy, so both heads compute a row's pred, loss term and d loss / d pred alike.
// Also the pieces of a cosine's fixed evaluation that several files must compile from ONE text: the sum of squares of a half-wave,
// the clamped inverse norm and the serial dot product (kgnn_embed_cosine.hip, kgnn_max_cosine.hip, kgnn_diverse.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <type_traits>
#include "kgnn_common.h"
#include "../../include/molkgnn_hip.h"

namespace mkgnn {

constexpr int HEAD_ROWS = 16;       // rows per block (two per half-wave: the block's latency is one row's chain, mostly its Philox rounds)

__device__ __forceinline__ float half_wave_sum(float v) {   // xor tree over the 32 lanes of a row
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// the sum of squares of an H-vector (H <= 64) held as v0 = v[h], v1 = v[32 + h] by the 32 lanes of a half-wave, in every lane of it:
// lane h forms v[h] * v[h] (+0.0 at h >= H), applies fmaf(v[32 + h], v[32 + h], .) where 32 + h < H, then the xor tree.  THE one
// definition of a cosine's norm: mkgnn_embed_cosine and mkgnn_embed_max_cosine promise each other's bits through it
__device__ __forceinline__ float half_wave_sumsq(float v0, float v1, int h, int H) {
    float s = h < H ? __fmul_rn(v0, v0) : 0.f;
    if (32 + h < H) s = fmaf(v1, v1, s);
    return half_wave_sum(s);
}

// 1 / max(||v||, eps) from the sum of squares above: correctly rounded square root and division; a NaN sum clamps to eps
__device__ __forceinline__ float inv_clamped_norm(float sumsq) { return 1.f / fmaxf(sqrtf(sumsq), MKGNN_EPS); }

// The dot product of a cosine's definition (kgnn_embed_cosine.hip: products, the optional fmaf, the xor tree, + (+0.0)) evaluated
// SERIALLY by one thread, in the tree's association -- the same bits.  e: a row zero-padded to W = 32 or 64 columns, in registers;
// q: the other vector, padded alike.  Shared by kgnn_max_cosine.hip and kgnn_diverse.hip: one text, one set of bits.
template <int W>
__device__ __forceinline__ float mc_dot(const float (&e)[W], const float* __restrict__ q) {
#pragma clang fp contract(off)
    // (plain operators under the pragma: __fmul_rn / __fadd_rn are header functions compiled under the header's own mode, and a
    // product and the sum it feeds in ONE thread would be fused -- in embed_cosine_kernel a shuffle lies between them)
    float x[32];
#pragma unroll
    for (int j = 0; j < 32; ++j) x[j] = e[j] * q[j];
    if constexpr (W == 64) {
#pragma unroll
        for (int j = 0; j < 32; ++j) x[j] = fmaf(e[32 + j], q[32 + j], x[j]);
    }
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) {
#pragma unroll
        for (int j = 0; j < o; ++j) x[j] = x[j] + x[j + o];
    }
    return x[0] + 0.f;
}

// The loss kind LK (MKGNN_LOSS_*, ABI v8) is a template parameter of every head kernel: the BCE instantiations are the code
// that was there before.  A row's loss term and its d loss / d pred, both before the 1 / B of the mean kinds:
template <int LK>
__device__ __forceinline__ float head_loss_term(float x, float y) {
    if constexpr (LK == MKGNN_LOSS_BCE_MEAN) return fmaxf(x, 0.f) - x * y + log1pf(expf(-fabsf(x)));   // torch's stable form
    else { const float r = x - y; return r * r; }
}
template <int LK>
__device__ __forceinline__ float head_dloss(float x, float y) {
    if constexpr (LK == MKGNN_LOSS_BCE_MEAN) return 1.f / (1.f + expf(-x)) - y;
    else return 2.f * (x - y);
}
// the loss kind (MKGNN_LOSS_*) of a call as a template argument: f(std::integral_constant<int, LK>{}); false: unknown kind
template <typename Fn>
static bool with_loss_kind(int32_t lk, Fn&& f) {
    switch (lk) {
    case MKGNN_LOSS_BCE_MEAN: f(std::integral_constant<int, MKGNN_LOSS_BCE_MEAN>{}); return true;
    case MKGNN_LOSS_SQERR_MEAN: f(std::integral_constant<int, MKGNN_LOSS_SQERR_MEAN>{}); return true;
    case MKGNN_LOSS_SQERR_SUM: f(std::integral_constant<int, MKGNN_LOSS_SQERR_SUM>{}); return true;
    default: return false;
    }
}

}  // namespace mkgnn
