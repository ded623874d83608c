// The task-indexed head with masked labels (ABI v8, additive): ffn [T, H] behind the readout, every molecule contributing the
// loss of the ONE task it was measured in (task id per row, or through a resident table: task_table[row_ids[i]]); a task id outside
// [0, T) is "no label".  The single-task head's block shape (kgnn_head_terms.h: HEAD_ROWS rows per block, 32 lanes per row), its
// product and reduction order for a row's pred, its loss terms and its dropout generator protocol.  Two launches per pass:
//   1. task_head_kernel: pred, and per block a partial [T][H + 1] (d W | d b per task) followed by {loss, labelled rows}.  The
//      block's rows (keep * emb, d loss / d pred, task) are staged in LDS; one lane per (task, column) then walks the 16 rows IN
//      ROW ORDER, so the order of every sum is fixed.  grad_emb is written here without the 1 / n_lab of the mean kinds.
//   2. task_head_final_kernel (kgnn_task_head_final.h: the label-matrix head launches it too): block 0 sums the loss partials in a fixed tree and advances the generator; one block per 64
//      (task, column) entries sums the block partials in a fixed order; the remaining blocks scale grad_emb.  Every block counts the
//      labelled rows itself from the integer-valued per-block counts (exact in any order), so nothing waits on another block.
// No float atomics, no "last block done" counter (kgnn_head.hip records why).
// The weighted losses (mkgnn_task_head_weighted_*: a sample weight per row, a positive weight per task, a null task for a
// one-output head) are the template parameter WT of the first kernel; the second one serves both.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "kgnn_common.h"

#include "kgnn_launch.h"
#include "kgnn_philox.h"
#include "kgnn_head_terms.h"
#include "kgnn_task_head_final.h"     // TaskHeadArgs, the partial layout and task_head_final_kernel (shared with kgnn_label_head.hip)
#include "../../include/molkgnn_hip.h"

namespace mkgnn {

// WT: the weighted entry points (mkgnn_task_head_weighted_*) -- a sample weight per row, a positive weight per task, and a null
// task meaning "every row has task 0"; a template parameter so that the instantiations without it stay as they were.  The
// weights only scale a labelled row's loss term and its d loss / d pred, BEFORE grad_loss and the 1 / n_lab of the final kernel
// (which is the unweighted one: it sees nothing of the weights): weights of exactly 1 give the unweighted bits.
template <int LK, int MODE, bool WT = false>
__global__ void __launch_bounds__(256) task_head_kernel(TaskHeadArgs a) {
    __shared__ float ek[HEAD_ROWS][TH_MAX_H];    // keep * emb of the block's rows
    __shared__ float dl[HEAD_ROWS], lt[HEAD_ROWS];   // d loss / d pred (before 1 / n_lab) and loss term: 0 for an unlabelled row
    __shared__ int tk[HEAD_ROWS];                // task of the row, -1: unlabelled or beyond B
    const int t = threadIdx.x, h = t & 31, g = t >> 5;          // 8 rows x 32 lanes per pass
    constexpr int NP = HEAD_ROWS / 8;
    const int Q = task_head_entries(MODE, a.T, a.H), PW = Q + 2;
    const bool drop = a.drop_p > 0.f;
    const int64_t* rs = MODE == TH_BACKWARD ? a.rng_used : a.rng;
    const uint64_t seed = drop ? (uint64_t)rs[0] : 0, offset = drop ? (uint64_t)rs[1] : 0;
    const float gl = MODE == TH_BACKWARD ? a.gloss[0] : 1.f;
    // all loads of the block's rows first (unconditional, clamped): row -> task -> the task's weight row, then the arithmetic
    int tv[NP];
    float xv[NP], yv[NP], pv[NP], w0[NP], bv[NP], ks0[NP], dv[NP];
    float sv[WT ? NP : 1], pwv[WT ? NP : 1];             // (WT) the row's sample weight and its task's positive weight
#pragma unroll
    for (int k = 0; k < NP; ++k) {
        const int64_t i = (int64_t)blockIdx.x * HEAD_ROWS + k * 8 + g;
        const int64_t ic = i < a.B ? i : a.B - 1;
        int32_t tid;
        if (WT && !a.task) {
            tid = 0;                                         // (single-task: T == 1, checked by the host)
        } else if (a.row_ids) {
            const int64_t r = a.row_ids[ic];
            const bool in = r >= 0 && r < a.n_task;          // (an id outside the table: no label)
            tid = a.task[in ? r : 0];
            if (!in) tid = -1;
        } else {
            tid = a.task[ic];
        }
        tv[k] = (i < a.B && tid >= 0 && tid < a.T) ? tid : -1;
        const int tc = tv[k] < 0 ? 0 : tv[k];
        xv[k] = a.emb[ic * a.es + (h < a.H ? h : 0)];
        yv[k] = a.y[ic];
        pv[k] = MODE == TH_BACKWARD ? a.pred[ic] : 0.f;
        w0[k] = h < a.H ? a.w[(size_t)tc * a.H + h] : 0.f;
        bv[k] = (MODE != TH_BACKWARD && a.b) ? a.b[tc] : 0.f;
        if constexpr (WT) {
            float s = 1.f;
            if (a.sw) {
                if (a.wids) {
                    const int64_t r = a.wids[ic];
                    const bool in = r >= 0 && r < a.n_sw;    // (an id outside the table: weight +0.0)
                    s = a.sw[in ? r : 0];
                    if (!in) s = 0.f;
                } else {
                    s = a.sw[ic];
                }
            }
            sv[k] = s;
            pwv[k] = (LK == MKGNN_LOSS_BCE_MEAN && a.pw) ? a.pw[tc] : 1.f;
        }
    }
#pragma unroll
    for (int k = 0; k < NP; ++k) {
        const int64_t i = (int64_t)blockIdx.x * HEAD_ROWS + k * 8 + g;
        const int64_t ic = i < a.B ? i : a.B - 1;
        const bool lab = tv[k] >= 0;
        const int tc = lab ? tv[k] : 0;
        ks0[k] = drop ? keep_scale_of(seed, offset, (uint64_t)ic * a.H + (h < a.H ? h : 0), a.drop_p) : 1.f;
        float x;
        if (MODE == TH_BACKWARD) {
            x = pv[k];
        } else {
            // (the single-task head's product and reduction order: T = 1 with every row labelled gives its pred bit for bit)
            x = h < a.H ? xv[k] * w0[k] : 0.f;
            if (drop) x *= ks0[k];
            for (int h0 = 32; h0 < a.H; h0 += 32)                   // (wider embeddings: the rare path)
                if (h0 + h < a.H) {
                    float e = a.emb[ic * a.es + h0 + h];
                    if (drop) e *= keep_scale_of(seed, offset, (uint64_t)ic * a.H + h0 + h, a.drop_p);
                    x = fmaf(e, a.w[(size_t)tc * a.H + h0 + h], x);
                }
            x = half_wave_sum(x) + bv[k];                           // (the xor tree leaves the sum in every lane of the row)
            if (!lab) x = 0.f;
        }
        // (WT: the weight first, then grad_loss -- s = 1 without a positive weight is the unweighted expression bit for bit)
        const bool pos = WT && LK == MKGNN_LOSS_BCE_MEAN && a.pw;
        if constexpr (WT) dv[k] = lab ? gl * (sv[k] * (pos ? head_dloss_pos(x, yv[k], pwv[k]) : head_dloss<LK>(x, yv[k]))) : 0.f;
        else dv[k] = lab ? gl * head_dloss<LK>(x, yv[k]) : 0.f;
        if (h == 0) {
            const int row = k * 8 + g;
            if (MODE != TH_BACKWARD && i < a.B) a.pred[i] = x;
            dl[row] = dv[k];
            if constexpr (WT) lt[row] = lab ? sv[k] * (pos ? head_loss_term_pos(x, yv[k], pwv[k]) : head_loss_term<LK>(x, yv[k])) : 0.f;
            else lt[row] = lab ? head_loss_term<LK>(x, yv[k]) : 0.f;
            tk[row] = tv[k];
        }
    }
    if (MODE != TH_FORWARD) {
        for (int h0 = 0; h0 < a.H; h0 += 32) {
            const int hh = h0 + h;
            if (hh < a.H) {
#pragma unroll
                for (int k = 0; k < NP; ++k) {
                    const int64_t i = (int64_t)blockIdx.x * HEAD_ROWS + k * 8 + g;
                    const bool lab = tv[k] >= 0;
                    float e = 0.f, ks = 0.f, wv = 0.f;
                    if (lab) {
                        if (h0 == 0) {
                            e = xv[k]; ks = ks0[k]; wv = w0[k];
                        } else {
                            e = a.emb[i * a.es + hh];
                            ks = drop ? keep_scale_of(seed, offset, (uint64_t)i * a.H + hh, a.drop_p) : 1.f;
                            wv = a.w[(size_t)tv[k] * a.H + hh];
                        }
                    }
                    ek[k * 8 + g][hh] = lab ? e * ks : 0.f;
                    if (a.gemb && i < a.B) a.gemb[i * a.ges + hh] = lab ? dv[k] * wv * ks : 0.f;
                }
            }
        }
    }
    __syncthreads();
    float* part = a.partial + (size_t)blockIdx.x * PW;
    const int PC = a.H + 1;                                       // a task's entries: dW[0..H), db
    for (int q = t; q < Q; q += 256) {
        const int task = q / PC, c = q - task * PC;
        float acc = 0.f;
#pragma unroll
        for (int r = 0; r < HEAD_ROWS; ++r)                       // in row order: a fixed sum
            if (tk[r] == task) acc = c < a.H ? fmaf(dl[r], ek[r][c], acc) : acc + dl[r];
        part[q] = acc;
    }
    if (t == 0) {
        float s = 0.f;
        int n = 0;
        for (int r = 0; r < HEAD_ROWS; ++r) { s += lt[r]; n += tk[r] >= 0 ? 1 : 0; }
        part[Q] = s;
        part[Q + 1] = (float)n;                                   // (<= 16: exact)
    }
}

}  // namespace mkgnn

using namespace mkgnn;

// ================================================================== C ABI ==========================
static int64_t task_head_blocks(int64_t n_rows) { return (n_rows + HEAD_ROWS - 1) / HEAD_ROWS; }

// the weighted entry points' extra arguments -> a; returns whether the weighted instantiation is needed (-1: refused).  No
// weight and a task per row: the unweighted instantiation, so the unweighted entry point's bits.
static int task_head_weights(const char* who, int32_t lk, const mkgnn_loss_weights* wt, TaskHeadArgs& a) {
    if (lk != MKGNN_LOSS_BCE_MEAN && lk != MKGNN_LOSS_SQERR_MEAN && lk != MKGNN_LOSS_SQERR_SUM) {
        api_fail("%s: unknown loss kind %d", who, (int)lk);
        return -1;
    }
    if (wt) {
        if (wt->pos_weight && lk != MKGNN_LOSS_BCE_MEAN) { api_fail("%s: pos_weight needs the BCE loss kind", who); return -1; }
        if (wt->sample_weight && (wt->weight_ids ? wt->n_sample_weight < 1 : wt->n_sample_weight < a.B)) {
            api_fail("%s: sample_weight holds %lld entries", who, (long long)wt->n_sample_weight);
            return -1;
        }
        a.sw = wt->sample_weight; a.wids = wt->sample_weight ? wt->weight_ids : nullptr; a.n_sw = wt->n_sample_weight;
        a.pw = wt->pos_weight;
    }
    return (a.sw || a.pw || !a.task) ? 1 : 0;
}

template <int MODE>
static int task_head_launch(const char* who, int32_t lk, const TaskHeadArgs& a, void* stream, bool weighted = false) {
    const int nblk = (int)task_head_blocks(a.B);
    const int Q = task_head_entries(MODE, a.T, a.H);
    const int ncol = (Q + 63) / 64;
    int nscale = 0;
    if (MODE != TH_FORWARD && a.gemb && lk != MKGNN_LOSS_SQERR_SUM) {
        const int64_t want = (a.B * a.H + 1023) / 1024;
        nscale = (int)(want < TH_SCALE_BLOCKS ? want : TH_SCALE_BLOCKS);
    }
    if (!with_loss_kind(lk, [&](auto K) {
            if (weighted) task_head_kernel<decltype(K)::value, MODE, true><<<nblk, 256, 0, (hipStream_t)stream>>>(a);
            else task_head_kernel<decltype(K)::value, MODE><<<nblk, 256, 0, (hipStream_t)stream>>>(a);
            // (the second launch sees nothing of the weights: one instantiation serves both)
            task_head_final_kernel<decltype(K)::value, MODE><<<1 + ncol + nscale, 256, 0, (hipStream_t)stream>>>(a, nblk, ncol);
        }))
        return api_fail("%s: unknown loss kind %d", who, (int)lk);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : api_hip_fail(who, e);
}

// The one argument path of the six entries below: the checks of MODE, the TaskHeadArgs fill, the optional weights and the launch.
// An argument an entry does not have arrives null / 0 and stays so in the kernels' struct.  ``weighted_entry``: the
// mkgnn_task_head_weighted_* entries, which take a null ``task`` (every row has task 0) and ``weights``.
template <int MODE>
static int task_head_run(const char* who, bool weighted_entry, const mkgnn_loss_weights* weights, int32_t lk, const float* emb,
                         int64_t emb_stride, int64_t n_rows, int32_t H, int32_t T, const float* weight, const float* bias,
                         const float* target, const int32_t* task, const int32_t* row_ids, int64_t n_task, float p,
                         int64_t* rng_state, const int64_t* rng_used, const float* pred, float* loss, const float* grad_loss,
                         float* grad_emb, int64_t grad_emb_stride, float* grad_weight, float* grad_bias, void* ws, size_t ws_bytes,
                         void* stream) {
    if (T < 1 || T > MKGNN_TASK_HEAD_MAX_TASKS) return api_fail("%s: %d tasks outside [1, %d]", who, (int)T, MKGNN_TASK_HEAD_MAX_TASKS);
    if (H < 1 || H > TH_MAX_H) return api_fail("%s: embedding width %d outside [1, %d]", who, (int)H, TH_MAX_H);
    if (n_rows < 1 || emb_stride < H || task_head_blocks(n_rows) > 0x7fffff00) return api_fail("%s: bad shape", who);
    if (!task) {                                           // (the weighted entry points: every row has task 0)
        if (!weighted_entry) return api_fail("%s: null task", who);
        if (T != 1 || row_ids) return api_fail("%s: a null task needs T == 1 and no row_ids (T = %d)", who, (int)T);
    } else if (row_ids ? n_task < 1 : n_task < n_rows) return api_fail("%s: task holds %lld entries", who, (long long)n_task);
    if (!(p >= 0.f && p < 1.f)) return api_fail("%s: dropout probability %g outside [0, 1)", who, p);
    if (!ws || ws_bytes < mkgnn_task_head_workspace_bytes(n_rows, H, T) || ((uintptr_t)ws & 3))
        return api_fail("%s: workspace too small or misaligned", who);
    constexpr bool BWD = MODE == TH_BACKWARD;
    if (!emb || !weight || !target || !pred || (BWD ? !grad_loss : !loss) || (MODE != TH_FORWARD && !grad_weight))
        return api_fail("%s: null pointer", who);
    if (grad_emb && grad_emb_stride < H) return api_fail("%s: bad grad_emb stride", who);
    if (p > 0.f && BWD && !rng_used) return api_fail("%s: dropout needs the forward's rng_used", who);
    if (p > 0.f && !BWD && (!rng_state || !rng_used)) return api_fail("%s: dropout needs rng_state and rng_used", who);
    TaskHeadArgs a{};
    a.partial = (float*)((char*)ws + 16);
    a.B = n_rows; a.H = H; a.T = T; a.es = emb_stride; a.task = task; a.row_ids = row_ids; a.n_task = n_task; a.drop_p = p;
    a.emb = emb; a.w = weight; a.b = bias; a.y = target; a.pred = (float*)pred; a.loss = loss; a.gloss = grad_loss;
    a.rng = rng_state; a.rng_used = (int64_t*)rng_used;
    a.gemb = grad_emb; a.ges = grad_emb_stride; a.gw = grad_weight; a.gb = grad_bias;
    const int wt = weighted_entry ? task_head_weights(who, lk, weights, a) : 0;
    if (wt < 0) return 1;
    return task_head_launch<MODE>(who, lk, a, stream, wt == 1);
}

extern "C" {

size_t mkgnn_task_head_workspace_bytes(int64_t n_rows, int32_t H, int32_t T) {
    if (n_rows < 1 || H < 1 || H > TH_MAX_H || T < 1 || T > MKGNN_TASK_HEAD_MAX_TASKS) return 0;
    return 16 + (size_t)task_head_blocks(n_rows) * ((size_t)T * (H + 1) + 2) * 4;
}

int mkgnn_task_head_forward(int32_t loss_kind, const float* emb, int64_t emb_stride, int64_t n_rows, int32_t H, int32_t T,
                            const float* weight, const float* bias, const float* target, const int32_t* task,
                            const int32_t* row_ids, int64_t n_task, float dropout_p, int64_t* rng_state, int64_t* rng_used,
                            float* pred, float* loss, void* ws, size_t ws_bytes, void* stream) {
    return task_head_run<TH_FORWARD>("mkgnn_task_head_forward", false, nullptr, loss_kind, emb, emb_stride, n_rows, H, T, weight,
                                     bias, target, task, row_ids, n_task, dropout_p, rng_state, rng_used, pred, loss, nullptr,
                                     nullptr, 0, nullptr, nullptr, ws, ws_bytes, stream);
}

int mkgnn_task_head_backward(int32_t loss_kind, const float* emb, int64_t emb_stride, int64_t n_rows, int32_t H, int32_t T,
                             const float* weight, const float* target, const int32_t* task, const int32_t* row_ids,
                             int64_t n_task, const float* pred, const float* grad_loss, float dropout_p, const int64_t* rng_used,
                             float* grad_emb, int64_t grad_emb_stride, float* grad_weight, float* grad_bias, void* ws,
                             size_t ws_bytes, void* stream) {
    return task_head_run<TH_BACKWARD>("mkgnn_task_head_backward", false, nullptr, loss_kind, emb, emb_stride, n_rows, H, T, weight,
                                      nullptr, target, task, row_ids, n_task, dropout_p, nullptr, rng_used, pred, nullptr,
                                      grad_loss, grad_emb, grad_emb_stride, grad_weight, grad_bias, ws, ws_bytes, stream);
}

int mkgnn_task_head_fused(int32_t loss_kind, const float* emb, int64_t emb_stride, int64_t n_rows, int32_t H, int32_t T,
                          const float* weight, const float* bias, const float* target, const int32_t* task,
                          const int32_t* row_ids, int64_t n_task, float dropout_p, int64_t* rng_state, int64_t* rng_used,
                          float* pred, float* loss, float* grad_emb, int64_t grad_emb_stride, float* grad_weight,
                          float* grad_bias, void* ws, size_t ws_bytes, void* stream) {
    return task_head_run<TH_FUSED>("mkgnn_task_head_fused", false, nullptr, loss_kind, emb, emb_stride, n_rows, H, T, weight, bias,
                                   target, task, row_ids, n_task, dropout_p, rng_state, rng_used, pred, loss, nullptr, grad_emb,
                                   grad_emb_stride, grad_weight, grad_bias, ws, ws_bytes, stream);
}

int mkgnn_task_head_weighted_forward(int32_t loss_kind, const float* emb, int64_t emb_stride, int64_t n_rows, int32_t H, int32_t T,
                                     const float* weight, const float* bias, const float* target, const int32_t* task,
                                     const int32_t* row_ids, int64_t n_task, float dropout_p, int64_t* rng_state,
                                     int64_t* rng_used, float* pred, float* loss, const mkgnn_loss_weights* weights, void* ws,
                                     size_t ws_bytes, void* stream) {
    return task_head_run<TH_FORWARD>("mkgnn_task_head_weighted_forward", true, weights, loss_kind, emb, emb_stride, n_rows, H, T,
                                     weight, bias, target, task, row_ids, n_task, dropout_p, rng_state, rng_used, pred, loss,
                                     nullptr, nullptr, 0, nullptr, nullptr, ws, ws_bytes, stream);
}

int mkgnn_task_head_weighted_backward(int32_t loss_kind, const float* emb, int64_t emb_stride, int64_t n_rows, int32_t H, int32_t T,
                                      const float* weight, const float* target, const int32_t* task, const int32_t* row_ids,
                                      int64_t n_task, const float* pred, const float* grad_loss, float dropout_p,
                                      const int64_t* rng_used, float* grad_emb, int64_t grad_emb_stride, float* grad_weight,
                                      float* grad_bias, const mkgnn_loss_weights* weights, void* ws, size_t ws_bytes,
                                      void* stream) {
    return task_head_run<TH_BACKWARD>("mkgnn_task_head_weighted_backward", true, weights, loss_kind, emb, emb_stride, n_rows, H, T,
                                      weight, nullptr, target, task, row_ids, n_task, dropout_p, nullptr, rng_used, pred, nullptr,
                                      grad_loss, grad_emb, grad_emb_stride, grad_weight, grad_bias, ws, ws_bytes, stream);
}

int mkgnn_task_head_weighted_fused(int32_t loss_kind, const float* emb, int64_t emb_stride, int64_t n_rows, int32_t H, int32_t T,
                                   const float* weight, const float* bias, const float* target, const int32_t* task,
                                   const int32_t* row_ids, int64_t n_task, float dropout_p, int64_t* rng_state, int64_t* rng_used,
                                   float* pred, float* loss, float* grad_emb, int64_t grad_emb_stride, float* grad_weight,
                                   float* grad_bias, const mkgnn_loss_weights* weights, void* ws, size_t ws_bytes, void* stream) {
    return task_head_run<TH_FUSED>("mkgnn_task_head_weighted_fused", true, weights, loss_kind, emb, emb_stride, n_rows, H, T,
                                   weight, bias, target, task, row_ids, n_task, dropout_p, rng_state, rng_used, pred, loss, nullptr,
                                   grad_emb, grad_emb_stride, grad_weight, grad_bias, ws, ws_bytes, stream);
}

}  // extern "C"
