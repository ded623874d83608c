// What the task-indexed head (kgnn_task_head.hip) and the label-matrix head (kgnn_label_head.hip) share: the argument struct of
// their kernels, the layout of a block's partial row, and the SECOND launch of both -- task_head_final_kernel, which knows nothing
// of how the first launch formed its partials: per block [T][H + 1] gradient entries (d W | d b per task), then {loss partial,
// labelled count of the block}.  One text, so both heads reduce, divide and advance the generator alike.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "kgnn_common.h"
#include "kgnn_head_terms.h"
#include "../../include/molkgnn_hip.h"

namespace mkgnn {

struct TaskHeadArgs {
    const float* emb; int64_t es; int64_t B; int H; int T;
    const float* w; const float* b; const float* y;      // w [T, H], b [T] or null
    const int32_t* task; const int32_t* row_ids; int64_t n_task;    // row_ids null: task [B]; else task [n_task], row i -> task[row_ids[i]]
    float* pred; float* loss;
    const float* gloss; float* gemb; int64_t ges; float* gw; float* gb;
    float* partial;
    float drop_p;
    int64_t* rng;                  // forward / fused: {seed, offset}, offset advanced by one per call
    int64_t* rng_used;             // forward writes / backward reads the {seed, offset} of this call's mask
    // the weighted entry points (WT) only: mkgnn_loss_weights, all optional
    const float* sw; const int32_t* wids; int64_t n_sw;   // wids null: s_i = sw[i]; else sw[wids[i]], an id outside [0, n_sw): +0.0
    const float* pw;                                      // [T] positive weights (BCE)
};
enum { TH_FORWARD = 0, TH_BACKWARD = 1, TH_FUSED = 2 };
constexpr int TH_MAX_H = 64;        // LDS row of the staged keep * emb: a wave writes two rows, one per 32-lane half (the halves never
                                    // conflict, 32 consecutive floats fill 32 banks), and reads one row at consecutive columns: no padding
constexpr int TH_SCALE_BLOCKS = 64; // blocks of the final kernel that scale grad_emb (at most)

// a block's partial row: [T][H + 1] gradient entries (the gradient passes) | loss | labelled rows
__device__ __host__ __forceinline__ int task_head_entries(int mode, int T, int H) { return mode == TH_FORWARD ? 0 : T * (H + 1); }

// second launch.  grid: 1 (loss, generator) + ceil(Q / 64) (the gradient entries) + the blocks that scale grad_emb
template <int LK, int MODE>
__global__ void __launch_bounds__(256) task_head_final_kernel(TaskHeadArgs a, int nb, int ncol) {
    __shared__ float fin[256];
    __shared__ int cnt[256];
    const int t = threadIdx.x;
    const int Q = task_head_entries(MODE, a.T, a.H), PW = Q + 2;
    const float* part = a.partial;
    // the labelled rows of the call: an integer sum of the blocks' counts
    {
        int n = 0;
        for (int bk = t; bk < nb; bk += 256) n += (int)part[(size_t)bk * PW + Q + 1];
        cnt[t] = n;
        __syncthreads();
        for (int w = 128; w > 0; w >>= 1) {
            if (t < w) cnt[t] += cnt[t + w];
            __syncthreads();
        }
    }
    const int n_lab = cnt[0] > 1 ? cnt[0] : 1;
    const float inv = LK == MKGNN_LOSS_SQERR_SUM ? 1.f : 1.f / (float)n_lab;
    if (blockIdx.x == 0) {
        if (MODE != TH_BACKWARD) {
            float v = 0.f;
            for (int bk = t; bk < nb; bk += 256) v += part[(size_t)bk * PW + Q];
            fin[t] = v;
            __syncthreads();
            for (int w = 128; w > 0; w >>= 1) {
                if (t < w) fin[t] += fin[t + w];
                __syncthreads();
            }
            if (t == 0) {
                a.loss[0] = LK == MKGNN_LOSS_SQERR_SUM ? fin[0] : fin[0] / (float)n_lab;
                if (a.drop_p > 0.f) {
                    const int64_t seed = a.rng[0], offset = a.rng[1];
                    a.rng_used[0] = seed; a.rng_used[1] = offset;
                    a.rng[1] = offset + 1;
                }
            }
        }
        return;
    }
    if ((int)blockIdx.x <= ncol) {
        // entry q of the block partials, four row parts per entry, eight loads in flight per thread; parts combined in a fixed order
        const int q = ((int)blockIdx.x - 1) * 64 + (t & 63), pr = t >> 6;
        float tot = 0.f;
        if (q < Q) {
            for (int bk = pr; bk < nb; bk += 32) {
                float v[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) v[u] = part[(size_t)(bk + 4 * u < nb ? bk + 4 * u : bk) * PW + q];
#pragma unroll
                for (int u = 0; u < 8; ++u) if (bk + 4 * u < nb) tot += v[u];
            }
        }
        fin[t] = tot;
        __syncthreads();
        if (pr == 0 && q < Q) {
            const float r = ((fin[t] + fin[64 + t]) + (fin[128 + t] + fin[192 + t])) * inv;
            const int PC = a.H + 1, task = q / PC, c = q - task * PC;
            if (c < a.H) a.gw[(size_t)task * a.H + c] = r;
            else if (a.gb) a.gb[task] = r;
        }
        return;
    }
    // grad_emb *= 1 / n_lab (launched for the mean kinds only)
    const int64_t nsc = (int64_t)gridDim.x - 1 - ncol, sb = (int64_t)blockIdx.x - 1 - ncol;
    const int64_t total = a.B * a.H;
    for (int64_t e = sb * 256 + t; e < total; e += nsc * 256) {
        const int64_t row = e / a.H;
        const int col = (int)(e - row * a.H);
        a.gemb[row * a.ges + col] *= inv;
    }
}

}  // namespace mkgnn
