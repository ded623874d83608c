// What the single-task head (kgnn_head.hip) and the task-indexed head (kgnn_task_head.hip) share: the block shape, the row
// reduction and the loss kinds' terms -- one copy, so both heads compute a row's pred, loss term and d loss / d pred alike.
// (half_wave_sum is also the tree of a cosine's fixed evaluation: kgnn_cosine.h.)
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
// BCE with a positive weight p (torch's pos_weight): L = 1 + (p - 1) y;  term = (1 - y) x + L (log1p(e^-|x|) + max(-x, 0)),
// d term / d x = (1 - y) - L sigmoid(-x).  Every product-and-add is an explicit fma, so every instantiation rounds alike;
// expf(x) = inf at a large x gives sigmoid(-x) = 0, and x = -90, y = 1 gives exactly 90 L.
__device__ __forceinline__ float head_loss_term_pos(float x, float y, float p) {
    const float L = fmaf(p - 1.f, y, 1.f);
    return fmaf(L, log1pf(expf(-fabsf(x))) + fmaxf(-x, 0.f), (1.f - y) * x);
}
__device__ __forceinline__ float head_dloss_pos(float x, float y, float p) {
    const float L = fmaf(p - 1.f, y, 1.f);
    return fmaf(-L, 1.f / (1.f + expf(x)), 1.f - y);
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
