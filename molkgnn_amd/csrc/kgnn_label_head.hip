// The label-matrix head (mkgnn_label_head_*, additive, ABI v8): ffn [T, H] behind the readout, every molecule carrying a ROW of
// labels -- labels[i, t], NaN for "not measured" (or through a resident table: labels[row_ids[i], t], an id outside the table: no
// label in any task) -- so the network runs once per molecule, not once per (molecule, assay) pair as with the task-indexed head.
//     pred[i, t] = (keep_i * emb_i) . weight[t] + bias[t]                         for EVERY (i, t)
//     loss       = sum over the labelled (i, t) of s_i * term(pred[i, t], labels[i, t]) / max(n_labelled entries, 1)
// The block shape is the heads' own (kgnn_head_terms.h: HEAD_ROWS rows per 256-thread block, one row per 32-lane half) and so are
// the products and the tree of a logit: pred[i, t] is BIT FOR BIT what task_head_kernel writes for row i labelled with task t
// under the same generator state (at dropout 0: mkgnn_task_scores' value).  As in kgnn_task_scores.hip the weight matrix is read
// once per block into LDS and lane t of the row keeps logit t; that lane then forms entry (i, t)'s loss term and d loss / d pred
// (kgnn_head_terms.h), selected on y == y.  Two launches per pass:
//   1. label_head_kernel: pred; grad_emb[i, h] = keep[i, h] * sum over t ASCENDING of d[i, t] * w[t, h], from d and w in LDS (without
//      the 1 / n_lab of the mean kinds); per block a partial [T][H + 1] (d W | d b per task) followed by {loss, labelled entries}:
//      one lane per (task, column) walks the block's 16 rows IN ROW ORDER.  A row's loss is its lanes' xor tree, a block's the 16
//      row sums in row order.  An unlabelled entry is removed by a select everywhere: its label and weight reach nothing.
//   2. task_head_final_kernel (kgnn_task_head_final.h), the task-indexed head's second launch unchanged: the partial layout is
//      that head's on purpose.  The count of a block is at most 512: exact in float32.
// No float atomics, no "last block done" counter (kgnn_head.hip records why).
#include <hip/hip_runtime.h>
#include <cstdint>
#include "kgnn_common.h"

#include "kgnn_launch.h"
#include "kgnn_philox.h"
#include "kgnn_head_terms.h"
#include "kgnn_task_head_final.h"
#include "../../include/molkgnn_hip.h"

namespace mkgnn {
namespace {

static_assert(MKGNN_TASK_HEAD_MAX_TASKS <= 32, "one lane of a row's half-wave per task");

// a: the task head's struct as the final kernel reads it (y, task, n_task unused; row_ids: the ids the LABELS are read through;
// pred [B, T] with row stride ps)
struct LabelHeadArgs {
    TaskHeadArgs a;
    const float* labels; int64_t ls; int64_t n_label_rows;   // row_ids null: labels [>= B, T]; else a table of n_label_rows rows
    int64_t ps;
};

constexpr int LH_D_STRIDE = 33;     // d[row][task]: the two halves of a wave read two rows at one task -- 33 keeps them in two banks

template <int LK, int MODE>
__global__ void __launch_bounds__(256) label_head_kernel(LabelHeadArgs la) {
    const TaskHeadArgs& a = la.a;
    __shared__ float ws[MKGNN_TASK_HEAD_MAX_TASKS * TH_MAX_H];   // weight [T][H]
    __shared__ float bs[MKGNN_TASK_HEAD_MAX_TASKS];
    __shared__ float ek[HEAD_ROWS][TH_MAX_H];                    // keep * emb of the block's rows
    __shared__ float dl[HEAD_ROWS][LH_D_STRIDE];                 // d loss / d pred (before 1 / n_lab): 0 for an unlabelled entry
    __shared__ float lrow[HEAD_ROWS];                            // a row's loss terms, summed
    __shared__ uint32_t lm[HEAD_ROWS];                           // bit t: entry (row, t) is labelled
    const int t = threadIdx.x, h = t & 31, g = t >> 5;          // 8 rows x 32 lanes per pass
    constexpr int NP = HEAD_ROWS / 8;
    const int H = a.H, T = a.T;
    const int Q = task_head_entries(MODE, T, H), PW = Q + 2;
    const bool drop = a.drop_p > 0.f;
    const int64_t* rs = MODE == TH_BACKWARD ? a.rng_used : a.rng;
    const uint64_t seed = drop ? (uint64_t)rs[0] : 0, offset = drop ? (uint64_t)rs[1] : 0;
    const float gl = MODE == TH_BACKWARD ? a.gloss[0] : 1.f;
    const int hc = h < T ? h : 0, c0 = h < H ? h : 0, c1 = 32 + h < H ? 32 + h : 0;
    const bool pos = LK == MKGNN_LOSS_BCE_MEAN && a.pw;
    // all loads of the block's rows first (unconditional, clamped), then the weights: everything in flight together
    float e0[NP], e1[NP], yv[NP], pv[NP], sv[NP], ks0[NP], ks1[NP];
    bool inl[NP];
#pragma unroll
    for (int k = 0; k < NP; ++k) {
        const int64_t i = (int64_t)blockIdx.x * HEAD_ROWS + k * 8 + g;
        const int64_t ic = i < a.B ? i : a.B - 1;
        e0[k] = a.emb[ic * a.es + c0];
        e1[k] = a.emb[ic * a.es + c1];
        int64_t lr = ic;
        bool in = true;
        if (a.row_ids) {
            const int64_t r = a.row_ids[ic];
            in = r >= 0 && r < la.n_label_rows;               // (an id outside the table: no label in any task)
            lr = in ? r : 0;
        }
        inl[k] = in;
        yv[k] = la.labels[lr * la.ls + hc];
        pv[k] = MODE == TH_BACKWARD ? a.pred[ic * la.ps + hc] : 0.f;
        float s = 1.f;
        if (a.sw) {
            if (a.wids) {
                const int64_t r = a.wids[ic];
                const bool win = r >= 0 && r < a.n_sw;         // (an id outside the table: weight +0.0)
                s = a.sw[win ? r : 0];
                if (!win) s = 0.f;
            } else {
                s = a.sw[ic];
            }
        }
        sv[k] = s;
    }
    const float pwl = pos ? a.pw[hc] : 1.f;
    for (int q = t; q < T * H; q += 256) ws[q] = a.w[q];
    if (t < T) bs[t] = (MODE != TH_BACKWARD && a.b) ? a.b[t] : 0.f;
#pragma unroll
    for (int k = 0; k < NP; ++k) {
        const int64_t i = (int64_t)blockIdx.x * HEAD_ROWS + k * 8 + g;
        const int64_t ic = i < a.B ? i : a.B - 1;
        ks0[k] = drop ? keep_scale_of(seed, offset, (uint64_t)ic * H + c0, a.drop_p) : 1.f;
        ks1[k] = (drop && H > 32) ? keep_scale_of(seed, offset, (uint64_t)ic * H + c1, a.drop_p) : 1.f;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < NP; ++k) {
        const int64_t i = (int64_t)blockIdx.x * HEAD_ROWS + k * 8 + g;
        const int row = k * 8 + g;
        const float e1k = drop ? __fmul_rn(e1[k], ks1[k]) : e1[k];
        float x = pv[k];
        if (MODE != TH_BACKWARD) {
            // (task_head_kernel's products and order: (emb * w) * keep at column h, fmaf(emb * keep, w, .) at column 32 + h, the
            // xor tree, the bias last -- never contracted)
            x = 0.f;
            for (int task = 0; task < T; ++task) {
                const float* wr = ws + task * H;
                float v = h < H ? __fmul_rn(e0[k], wr[h]) : 0.f;
                if (drop) v = __fmul_rn(v, ks0[k]);
                if (32 + h < H) v = fmaf(e1k, wr[32 + h], v);
                v = half_wave_sum(v) + bs[task];                  // (the xor tree leaves the sum in every lane of the row)
                if (h == task) x = v;
            }
            if (i < a.B && h < T) a.pred[i * la.ps + h] = x;
        }
        // lane t: entry (i, t).  Only NaN means missing; the sample weight first, then grad_loss (s = 1: the unweighted bits)
        const float y = yv[k];
        const bool lab = i < a.B && h < T && inl[k] && y == y;
        const float d = lab ? gl * (sv[k] * (pos ? head_dloss_pos(x, y, pwl) : head_dloss<LK>(x, y))) : 0.f;
        const float term = lab ? sv[k] * (pos ? head_loss_term_pos(x, y, pwl) : head_loss_term<LK>(x, y)) : 0.f;
        const float rsum = half_wave_sum(term);
        const uint64_t bal = __ballot(lab);
        dl[row][h] = d;
        if (h == 0) {
            lrow[row] = rsum;
            lm[row] = (uint32_t)(bal >> (32 * (g & 1)));
        }
        if (MODE != TH_FORWARD) {
            if (h < H) ek[row][h] = e0[k] * ks0[k];
            if (32 + h < H) ek[row][32 + h] = e1k;
        }
    }
    __syncthreads();
    float* part = a.partial + (size_t)blockIdx.x * PW;
    if (MODE != TH_FORWARD) {
        if (a.gemb) {
#pragma unroll
            for (int k = 0; k < NP; ++k) {
                const int64_t i = (int64_t)blockIdx.x * HEAD_ROWS + k * 8 + g;
                const int row = k * 8 + g;
                const bool any = lm[row] != 0;
                float acc0 = 0.f, acc1 = 0.f;
                for (int task = 0; task < T; ++task) {            // ascending: a fixed sum
                    const float d = dl[row][task];
                    acc0 = fmaf(d, ws[task * H + c0], acc0);
                    if (H > 32) acc1 = fmaf(d, ws[task * H + c1], acc1);
                }
                if (i < a.B) {                                    // (a row without a label: exactly zero)
                    if (h < H) a.gemb[i * a.ges + h] = any ? ks0[k] * acc0 : 0.f;
                    if (32 + h < H) a.gemb[i * a.ges + 32 + h] = any ? ks1[k] * acc1 : 0.f;
                }
            }
        }
        const int PC = H + 1;                                     // a task's entries: dW[0..H), db
        for (int q = t; q < Q; q += 256) {
            const int task = q / PC, c = q - task * PC;
            float acc = 0.f;
#pragma unroll
            for (int r = 0; r < HEAD_ROWS; ++r)                   // in row order: a fixed sum
                if ((lm[r] >> task) & 1u) acc = c < H ? fmaf(dl[r][task], ek[r][c], acc) : acc + dl[r][task];
            part[q] = acc;
        }
    }
    if (t == 0) {
        float s = 0.f;
        int n = 0;
        for (int r = 0; r < HEAD_ROWS; ++r) { s += lrow[r]; n += __popc(lm[r]); }
        part[Q] = s;
        part[Q + 1] = (float)n;                                   // (<= 512: exact)
    }
}

int64_t label_head_blocks(int64_t n_rows) { return (n_rows + HEAD_ROWS - 1) / HEAD_ROWS; }

bool label_head_shape_ok(int64_t n_rows, int32_t H, int32_t T) {
    return n_rows >= 1 && H >= 1 && H <= TH_MAX_H && T >= 1 && T <= MKGNN_TASK_HEAD_MAX_TASKS && n_rows < ((int64_t)1 << 31)
        && n_rows * T < ((int64_t)1 << 31);                       // (the labelled-entry count stays an exact int)
}

template <int MODE>
int label_head_run(const char* who, int32_t lk, const float* emb, int64_t emb_stride, int64_t n_rows, int32_t H, int32_t T,
                   const float* weight, const float* bias, const float* labels, int64_t label_stride, const int32_t* row_ids,
                   int64_t n_label_rows, float p, int64_t* rng_state, const int64_t* rng_used, const float* pred,
                   int64_t pred_stride, float* loss, const float* grad_loss, float* grad_emb, int64_t grad_emb_stride,
                   float* grad_weight, float* grad_bias, const mkgnn_loss_weights* wt, void* wsp, size_t ws_bytes, void* stream) {
    if (lk != MKGNN_LOSS_BCE_MEAN && lk != MKGNN_LOSS_SQERR_MEAN && lk != MKGNN_LOSS_SQERR_SUM)
        return api_fail("%s: unknown loss kind %d", who, (int)lk);
    if (T < 1 || T > MKGNN_TASK_HEAD_MAX_TASKS) return api_fail("%s: %d tasks outside [1, %d]", who, (int)T, MKGNN_TASK_HEAD_MAX_TASKS);
    if (H < 1 || H > TH_MAX_H) return api_fail("%s: embedding width %d outside [1, %d]", who, (int)H, TH_MAX_H);
    if (n_rows < 1 || emb_stride < H) return api_fail("%s: bad shape", who);
    if (!label_head_shape_ok(n_rows, H, T))
        return api_fail("%s: %lld rows of %d tasks: the labelled-entry count needs n_rows * T < 2^31", who, (long long)n_rows, (int)T);
    if (label_stride < T || pred_stride < T) return api_fail("%s: label or pred row stride below T = %d", who, (int)T);
    if (row_ids ? n_label_rows < 1 : n_label_rows < n_rows)
        return api_fail("%s: labels holds %lld rows", who, (long long)n_label_rows);
    if (!(p >= 0.f && p < 1.f)) return api_fail("%s: dropout probability %g outside [0, 1)", who, p);
    if (!wsp || ws_bytes < mkgnn_label_head_workspace_bytes(n_rows, H, T) || ((uintptr_t)wsp & 3))
        return api_fail("%s: workspace too small or misaligned", who);
    constexpr bool BWD = MODE == TH_BACKWARD;
    if (!emb || !weight || !labels || !pred || (BWD ? !grad_loss : !loss) || (MODE != TH_FORWARD && !grad_weight))
        return api_fail("%s: null pointer", who);
    if (grad_emb && grad_emb_stride < H) return api_fail("%s: bad grad_emb stride", who);
    if (p > 0.f && BWD && !rng_used) return api_fail("%s: dropout needs the forward's rng_used", who);
    if (p > 0.f && !BWD && (!rng_state || !rng_used)) return api_fail("%s: dropout needs rng_state and rng_used", who);
    LabelHeadArgs la{};
    TaskHeadArgs& a = la.a;
    a.partial = (float*)((char*)wsp + 16);
    a.B = n_rows; a.H = H; a.T = T; a.es = emb_stride; a.row_ids = row_ids; a.drop_p = p;
    a.emb = emb; a.w = weight; a.b = bias; a.pred = (float*)pred; a.loss = loss; a.gloss = grad_loss;
    a.rng = rng_state; a.rng_used = (int64_t*)rng_used;
    a.gemb = grad_emb; a.ges = grad_emb_stride; a.gw = grad_weight; a.gb = grad_bias;
    la.labels = labels; la.ls = label_stride; la.n_label_rows = n_label_rows; la.ps = pred_stride;
    if (wt) {
        if (wt->pos_weight && lk != MKGNN_LOSS_BCE_MEAN) return api_fail("%s: pos_weight needs the BCE loss kind", who);
        if (wt->sample_weight && (wt->weight_ids ? wt->n_sample_weight < 1 : wt->n_sample_weight < n_rows))
            return api_fail("%s: sample_weight holds %lld entries", who, (long long)wt->n_sample_weight);
        a.sw = wt->sample_weight; a.wids = wt->sample_weight ? wt->weight_ids : nullptr; a.n_sw = wt->n_sample_weight;
        a.pw = wt->pos_weight;
    }
    const int nblk = (int)label_head_blocks(n_rows);
    const int Q = task_head_entries(MODE, T, H);
    const int ncol = (Q + 63) / 64;
    int nscale = 0;
    if (MODE != TH_FORWARD && grad_emb && lk != MKGNN_LOSS_SQERR_SUM) {
        const int64_t want = (n_rows * H + 1023) / 1024;
        nscale = (int)(want < TH_SCALE_BLOCKS ? want : TH_SCALE_BLOCKS);
    }
    with_loss_kind(lk, [&](auto K) {
        label_head_kernel<decltype(K)::value, MODE><<<nblk, 256, 0, (hipStream_t)stream>>>(la);
        // (the task-indexed head's second launch: it sees the partials, not how they were formed)
        task_head_final_kernel<decltype(K)::value, MODE><<<1 + ncol + nscale, 256, 0, (hipStream_t)stream>>>(a, nblk, ncol);
    });
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : api_hip_fail(who, e);
}

}  // namespace
}  // namespace mkgnn

using namespace mkgnn;

extern "C" {

size_t mkgnn_label_head_workspace_bytes(int64_t n_rows, int32_t H, int32_t T) {
    if (!label_head_shape_ok(n_rows, H, T)) return 0;
    return 16 + (size_t)label_head_blocks(n_rows) * ((size_t)T * (H + 1) + 2) * 4;
}

int mkgnn_label_head_forward(int32_t loss_kind, const float* emb, int64_t emb_stride, int64_t n_rows, int32_t H, int32_t T,
                             const float* weight, const float* bias, const float* labels, int64_t label_stride,
                             const int32_t* row_ids, int64_t n_label_rows, float dropout_p, int64_t* rng_state, int64_t* rng_used,
                             float* pred, int64_t pred_stride, float* loss, const mkgnn_loss_weights* weights, void* ws,
                             size_t ws_bytes, void* stream) {
    return label_head_run<TH_FORWARD>("mkgnn_label_head_forward", loss_kind, emb, emb_stride, n_rows, H, T, weight, bias, labels,
                                      label_stride, row_ids, n_label_rows, dropout_p, rng_state, rng_used, pred, pred_stride, loss,
                                      nullptr, nullptr, 0, nullptr, nullptr, weights, ws, ws_bytes, stream);
}

int mkgnn_label_head_backward(int32_t loss_kind, const float* emb, int64_t emb_stride, int64_t n_rows, int32_t H, int32_t T,
                              const float* weight, const float* labels, int64_t label_stride, const int32_t* row_ids,
                              int64_t n_label_rows, const float* pred, int64_t pred_stride, const float* grad_loss,
                              float dropout_p, const int64_t* rng_used, float* grad_emb, int64_t grad_emb_stride,
                              float* grad_weight, float* grad_bias, const mkgnn_loss_weights* weights, void* ws, size_t ws_bytes,
                              void* stream) {
    return label_head_run<TH_BACKWARD>("mkgnn_label_head_backward", loss_kind, emb, emb_stride, n_rows, H, T, weight, nullptr,
                                       labels, label_stride, row_ids, n_label_rows, dropout_p, nullptr, rng_used, pred, pred_stride,
                                       nullptr, grad_loss, grad_emb, grad_emb_stride, grad_weight, grad_bias, weights, ws, ws_bytes,
                                       stream);
}

int mkgnn_label_head_fused(int32_t loss_kind, const float* emb, int64_t emb_stride, int64_t n_rows, int32_t H, int32_t T,
                           const float* weight, const float* bias, const float* labels, int64_t label_stride,
                           const int32_t* row_ids, int64_t n_label_rows, float dropout_p, int64_t* rng_state, int64_t* rng_used,
                           float* pred, int64_t pred_stride, float* loss, float* grad_emb, int64_t grad_emb_stride,
                           float* grad_weight, float* grad_bias, const mkgnn_loss_weights* weights, void* ws, size_t ws_bytes,
                           void* stream) {
    return label_head_run<TH_FUSED>("mkgnn_label_head_fused", loss_kind, emb, emb_stride, n_rows, H, T, weight, bias, labels,
                                    label_stride, row_ids, n_label_rows, dropout_p, rng_state, rng_used, pred, pred_stride, loss,
                                    nullptr, grad_emb, grad_emb_stride, grad_weight, grad_bias, weights, ws, ws_bytes, stream);
}

}  // extern "C"
