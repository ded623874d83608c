// A cosine's fixed evaluation, ONCE.  mkgnn_embed_cosine (kgnn_embed_cosine.hip) defines the float32 value of sim(e, q); the nearest
// reference (kgnn_max_cosine.hip), the diverse picks (kgnn_diverse.hip) and the fused k-NN (kgnn_knn.hip) promise those bits, so all
// four compile every step from this text.  THE BITS of one element depend on the H values of e and of q alone (H <= 64):
//     sumsq(v)  lane h < 32 of a half-wave forms v[h] * v[h] (a plain multiply; +0.0 at lanes >= H), applies fmaf(v[32 + h], v[32 + h], .)
//               where 32 + h < H; the 32 values go through half_wave_sum (the xor tree, offsets 16, 8, 4, 2, 1)      half_wave_sumsq
//     inv(v)    1 / fmaxf(sqrtf(sumsq(v)), eps): correctly rounded root and division; a NaN sum clamps to eps       inv_clamped_norm
//     dot       lane h forms e[h] * q[h], applies fmaf(e[32 + h], q[32 + h], .), the same tree; then + (+0.0), which turns a sum of
//               -0.0 products -- a zero row against negative query values -- into +0.0 and changes nothing else     half_wave_dot
//     sim       (dot * inv(e)) * inv(q), two plain multiplies in that order
// THE SERIAL FORM.  Every step of the xor tree is lane l forming v[l] + v[l ^ o]; float addition is commutative, so all lanes hold the
// same bits and the tree is a fixed binary tree: level 16 adds x[j] + x[j + 16] for j < 16, level 8 those sums j and j + 8, and so on.
// ONE THREAD evaluates it serially in that association (mc_dot) and gets the same bits.  Its vectors are padded with +0.0 to 32
// (H <= 32) or 64 columns: a padded product is (+0.0) * (+0.0) = +0.0, what a lane h >= H contributes; a padded fmaf(+0.0, +0.0, x) is
// x + (+0.0), which differs from the skipped fmaf only where x is -0.0, and the sign of a zero going into a tree of additions can
// change only the sign of a zero coming out, which the + (+0.0) behind the tree removes.  A file that calls mc_dot may contract
// nothing around it: `#pragma clang fp contract(off)` at its top.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "kgnn_common.h"
#include "kgnn_head_terms.h"

namespace mkgnn {

// the two values lane h of a half-wave holds of an H-vector: row[h] and row[32 + h], read from column 0 where they lie behind H
__device__ __forceinline__ void half_wave_load(const float* row, int h, int H, float& v0, float& v1) {
    v0 = row[h < H ? h : 0];
    v1 = row[32 + h < H ? 32 + h : 0];
}

// sumsq of an H-vector held as v0, v1 (above) by the 32 lanes of a half-wave, in every lane of it
__device__ __forceinline__ float half_wave_sumsq(float v0, float v1, int h, int H) {
    float s = h < H ? __fmul_rn(v0, v0) : 0.f;
    if (32 + h < H) s = fmaf(v1, v1, s);
    return half_wave_sum(s);
}

__device__ __forceinline__ float half_wave_row_sumsq(const float* row, int h, int H) {      // ... of the H-vector at `row`
    float v0, v1;
    half_wave_load(row, h, H, v0, v1);
    return half_wave_sumsq(v0, v1, h, H);
}

__device__ __forceinline__ float inv_clamped_norm(float sumsq) { return 1.f / fmaxf(sqrtf(sumsq), MKGNN_EPS); }

// dot of the H-vector held as e0, e1 with the H-vector at q (read only below H), in every lane of the half-wave
__device__ __forceinline__ float half_wave_dot(float e0, float e1, const float* q, int h, int H) {
    float x = h < H ? __fmul_rn(e0, q[h]) : 0.f;              // (never contracted into the tree's first add)
    if (32 + h < H) x = fmaf(e1, q[32 + h], x);
    return half_wave_sum(x) + 0.f;                            // (the xor tree leaves the sum in every lane of the row)
}

// dot, serially by one thread.  e: a row zero-padded to W = 32 or 64 columns, in registers; q: the other vector, padded alike
template <int W>
__device__ __forceinline__ float mc_dot(const float (&e)[W], const float* __restrict__ q) {
#pragma clang fp contract(off)
    // (plain operators under the pragma: __fmul_rn / __fadd_rn are header functions compiled under the header's own mode, and a
    // product and the sum it feeds in ONE thread would be fused -- in half_wave_dot a shuffle lies between them)
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

// The operands of mc_dot for a block of THREADS threads (t: the caller's index), between the caller's barriers: tile slot r < m gets
// row row_of(r) of `src` (rows `stride` floats apart), zero padded from column H to W, and tinv[r] that row's inverse norm from inv[]
template <int W, int THREADS, typename RowOf>
__device__ __forceinline__ void stage_padded_tile(float* tile, float* tinv, int m, RowOf row_of, const float* src, int64_t stride,
                                                  int H, const float* inv, int t) {
    for (int j = t; j < m * W; j += THREADS) {
        const int r = j / W, c = j - r * W;
        const int p = row_of(r);
        tile[j] = c < H ? src[(int64_t)p * stride + c] : 0.f;
    }
    if (t < m) tinv[t] = inv[row_of(t)];
}

}  // namespace mkgnn
