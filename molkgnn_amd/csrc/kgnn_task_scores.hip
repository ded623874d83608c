// Every task's logit of every row (mkgnn_task_scores): pred[i, t] = emb_i . weight[t] + bias[t] for ALL t < T -- the T-output head of
// a multi-task model in evaluation mode, where a library has no labels and every molecule is ranked in every assay.
//
// The contract is bit equality with the task-indexed head (task_head_kernel, kgnn_task_head.hip) at dropout 0: pred[i, t] is what
// that kernel writes for row i labelled with task t.  So the layout is the head's own -- HEAD_ROWS rows per 256-thread block, one
// row per 32-lane half-wave, two passes -- and so are the products and the tree: lane h forms emb[h] * w[t][h] (a plain multiply),
// applies fmaf(emb[32 + h], w[t][32 + h], .) for H > 32, the 32 values go through half_wave_sum, the bias (or +0.0) is added last.
// What differs is what is held where: the row's (up to) two embedding values stay in registers across the loop over t, the whole
// weight matrix (at most 32 x 64 floats = 8 KB) is read ONCE per block into LDS -- a half-wave reads 32 consecutive floats of a
// row (no bank conflict; the two halves of a wave read different rows' embeddings but the SAME weight row: a broadcast) -- and
// lane t of the row keeps the sum of task t (T <= 32 = the lanes of a row), so a row's T results leave in one store instruction,
// contiguous for the [n, T] layout.  One launch, no workspace, no atomics; element (i, t) is written by lane t of row i alone.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "kgnn_common.h"

#include "kgnn_launch.h"
#include "kgnn_head_terms.h"
#include "../../include/molkgnn_hip.h"

namespace mkgnn {
namespace {

constexpr int TS_MAX_H = 64;        // = TH_MAX_H of the task head
static_assert(MKGNN_TASK_HEAD_MAX_TASKS <= 32, "one lane of a row's half-wave per task");

__global__ void __launch_bounds__(256) task_scores_kernel(const float* __restrict__ emb, int64_t es, int64_t n, int H, int T,
                                                          const float* __restrict__ w, const float* __restrict__ b,
                                                          float* __restrict__ pred, int64_t prs, int64_t pts) {
    __shared__ float ws[MKGNN_TASK_HEAD_MAX_TASKS * TS_MAX_H];
    __shared__ float bs[MKGNN_TASK_HEAD_MAX_TASKS];
    const int t = threadIdx.x, h = t & 31, g = t >> 5;          // 8 rows x 32 lanes per pass
    constexpr int NP = HEAD_ROWS / 8;
    // the block's rows first (unconditional, clamped), then the weights: all loads in flight together
    float e0[NP], e1[NP];
#pragma unroll
    for (int k = 0; k < NP; ++k) {
        const int64_t i = (int64_t)blockIdx.x * HEAD_ROWS + k * 8 + g;
        const int64_t ic = i < n ? i : n - 1;
        e0[k] = emb[ic * es + (h < H ? h : 0)];
        e1[k] = emb[ic * es + (32 + h < H ? 32 + h : 0)];
    }
    for (int q = t; q < T * H; q += 256) ws[q] = w[q];
    if (t < T) bs[t] = b ? b[t] : 0.f;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < NP; ++k) {
        const int64_t i = (int64_t)blockIdx.x * HEAD_ROWS + k * 8 + g;
        float mine = 0.f;
        for (int task = 0; task < T; ++task) {
            const float* wr = ws + task * H;
            float x = h < H ? __fmul_rn(e0[k], wr[h]) : 0.f;       // (never contracted into the tree's first add)
            if (32 + h < H) x = fmaf(e1[k], wr[32 + h], x);
            x = half_wave_sum(x) + bs[task];                       // (the xor tree leaves the sum in every lane of the row)
            if (h == task) mine = x;
        }
        if (i < n && h < T) pred[i * prs + (int64_t)h * pts] = mine;
    }
}

}  // namespace
}  // namespace mkgnn

using namespace mkgnn;

extern "C" int mkgnn_task_scores(const float* emb, int64_t emb_stride, int64_t n_rows, int32_t H, int32_t T, const float* weight,
                                 const float* bias, float* pred, int64_t pred_row_stride, int64_t pred_task_stride, void* stream) {
    const char* who = "mkgnn_task_scores";
    if (T < 1 || T > MKGNN_TASK_HEAD_MAX_TASKS) return api_fail("%s: %d tasks outside [1, %d]", who, (int)T, MKGNN_TASK_HEAD_MAX_TASKS);
    if (H < 1 || H > TS_MAX_H) return api_fail("%s: embedding width %d outside [1, %d]", who, (int)H, TS_MAX_H);
    if (n_rows < 0 || emb_stride < H) return api_fail("%s: bad shape", who);
    if (n_rows == 0) return 0;
    if (!emb || !weight || !pred) return api_fail("%s: null pointer", who);
    const int64_t blocks = (n_rows + HEAD_ROWS - 1) / HEAD_ROWS;
    if (blocks > 0x7fffff00) return api_fail("%s: bad shape", who);
    // one writer per output: rows of tasks, or tasks of rows, that do not overlap
    const int64_t rs = pred_row_stride, ts = pred_task_stride;
    const bool rows = rs >= 1 && ts >= 1 && (T == 1 || rs > (int64_t)(T - 1) * ts || n_rows == 1);
    const bool tasks = rs >= 1 && ts >= 1 && (n_rows == 1 || T == 1 || ts > (n_rows - 1) * rs);
    if (!rows && !tasks)
        return api_fail("%s: pred strides (%lld, %lld) make two outputs share an element", who, (long long)rs, (long long)ts);
    task_scores_kernel<<<(unsigned)blocks, 256, 0, (hipStream_t)stream>>>(emb, emb_stride, n_rows, H, T, weight, bias, pred, rs, ts);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : api_hip_fail(who, e);
}
