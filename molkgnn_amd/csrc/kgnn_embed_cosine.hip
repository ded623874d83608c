// Cosine similarity of every embedding row with every query (mkgnn_embed_cosine): analogue search over a resident library --
//     sim[i, q] = (emb_i . qry_q) / (max(||emb_i||, eps) * max(||qry_q||, eps)),   eps = MKGNN_EPS = 1e-8f
// each vector clamped on its own (torch's cosine_similarity; the clamp of mkgnn_row_inv_norm).
//
// The layout is task_scores_kernel's (kgnn_task_scores.hip), whose shape this problem has -- an [n, H] matrix against at most 32
// H-wide vectors, H <= 64: HEAD_ROWS rows per 256-thread block, one row per 32-lane half-wave, two passes; the row's (up to) two
// values stay in registers across the loop over q; the queries (at most 32 x 64 floats = 8 KB) are read ONCE per block into LDS,
// RAW: every block normalises them itself (at most 2 048 multiply-adds), so nothing is prepared ahead and one captured launch
// follows the contents of `queries` as well as of `emb`; lane q of the row keeps the result of query q (Q <= 32 = the lanes of a
// row), so a row's Q results leave in one store instruction.  One launch, no workspace, no atomics, no state; element (i, q) is
// written by lane q of row i alone.  The kernel is bound by its launch: plain FP32, no matrix instructions.
//
// THE EVALUATION ORDER of an element -- one per element, whatever n_rows, the row's place in block and grid, Q, q's index, the
// strides or the output layout are (the bits of sim[i, q] depend on the H values of row i and of query q alone) -- is kgnn_cosine.h's:
// this kernel is that text called in order, (half_wave_dot * inv(e)) * inv(q).  inv(q) is computed by a half-wave of the block with
// exactly the lane assignment of a row's, whichever half-wave and whatever Q.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "kgnn_common.h"

#include "kgnn_launch.h"
#include "kgnn_cosine.h"
#include "../../include/molkgnn_hip.h"

namespace mkgnn {
namespace {

constexpr int EC_MAX_H = 64;
constexpr int EC_MAX_Q = MKGNN_EMBED_COSINE_MAX_QUERIES;
static_assert(EC_MAX_Q <= 32, "one lane of a row's half-wave per query");
static_assert(EC_MAX_Q <= MKGNN_TASK_HEAD_MAX_TASKS, "the queries' lists are a TopKTasks");

__global__ void __launch_bounds__(256) embed_cosine_kernel(const float* __restrict__ emb, int64_t es, int64_t n, int H, int Q,
                                                           const float* __restrict__ qry, int64_t qs, float* __restrict__ sim,
                                                           int64_t srs, int64_t sqs) {
    __shared__ float qv[EC_MAX_Q * EC_MAX_H];                   // query q at qv + q * H
    __shared__ float qinv[EC_MAX_Q];
    const int t = threadIdx.x, h = t & 31, g = t >> 5;          // 8 rows x 32 lanes per pass
    constexpr int NP = HEAD_ROWS / 8;
    // the block's rows first (unconditional, clamped), then the queries: all loads in flight together
    float e0[NP], e1[NP];
#pragma unroll
    for (int k = 0; k < NP; ++k) {
        const int64_t i = (int64_t)blockIdx.x * HEAD_ROWS + k * 8 + g;
        const int64_t ic = i < n ? i : n - 1;
        half_wave_load(emb + ic * es, h, H, e0[k], e1[k]);
    }
    for (int j = t; j < Q * H; j += 256) {
        const int q = j / H;
        qv[j] = qry[(int64_t)q * qs + (j - q * H)];
    }
    __syncthreads();
    // 1 / max(||query||, eps): half-wave g takes queries g, g + 8, ... (the trip count is the block's: no divergence round a shuffle)
    for (int q0 = 0; q0 < Q; q0 += 8) {
        const int q = q0 + g < Q ? q0 + g : Q - 1;
        const float s = half_wave_row_sumsq(qv + q * H, h, H);
        if (h == 0 && q0 + g < Q) qinv[q] = inv_clamped_norm(s);
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < NP; ++k) {
        const int64_t i = (int64_t)blockIdx.x * HEAD_ROWS + k * 8 + g;
        const float ie = inv_clamped_norm(half_wave_sumsq(e0[k], e1[k], h, H));
        float mine = 0.f;
        for (int q = 0; q < Q; ++q) {
            const float d = half_wave_dot(e0[k], e1[k], qv + q * H, h, H);
            const float r = __fmul_rn(__fmul_rn(d, ie), qinv[q]);
            if (h == q) mine = r;
        }
        if (i < n && h < Q) sim[i * srs + (int64_t)h * sqs] = mine;
    }
}

}  // namespace
}  // namespace mkgnn

using namespace mkgnn;

extern "C" int mkgnn_embed_cosine(const float* emb, int64_t emb_stride, int64_t n_rows, int32_t H, const float* queries,
                                  int64_t query_stride, int32_t Q, float* sim, int64_t sim_row_stride, int64_t sim_query_stride,
                                  void* stream) {
    const char* who = "mkgnn_embed_cosine";
    if (Q < 1 || Q > EC_MAX_Q) return api_fail("%s: %d queries outside [1, %d]", who, (int)Q, EC_MAX_Q);
    if (H < 1 || H > EC_MAX_H) return api_fail("%s: embedding width %d outside [1, %d]", who, (int)H, EC_MAX_H);
    if (n_rows < 0 || emb_stride < H || query_stride < H) return api_fail("%s: bad shape", who);
    if (n_rows == 0) return 0;
    if (!emb || !queries || !sim) return api_fail("%s: null pointer", who);
    const int64_t blocks = (n_rows + HEAD_ROWS - 1) / HEAD_ROWS;
    if (blocks > 0x7fffff00) return api_fail("%s: bad shape", who);
    // one writer per output: rows of queries, or queries of rows, that do not overlap
    const int64_t rs = sim_row_stride, qs = sim_query_stride;
    const bool rows = rs >= 1 && qs >= 1 && (Q == 1 || rs > (int64_t)(Q - 1) * qs || n_rows == 1);
    const bool cols = rs >= 1 && qs >= 1 && (n_rows == 1 || Q == 1 || qs > (n_rows - 1) * rs);
    if (!rows && !cols)
        return api_fail("%s: sim strides (%lld, %lld) make two outputs share an element", who, (long long)rs, (long long)qs);
    embed_cosine_kernel<<<(unsigned)blocks, 256, 0, (hipStream_t)stream>>>(emb, emb_stride, n_rows, H, Q, queries, query_stride, sim,
                                                                          rs, qs);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : api_hip_fail(who, e);
}
