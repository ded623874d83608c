// The single-task head and its losses (BCE-with-logits, squared error) behind the readout:
// The tail of the training step (reference model.py: ffn(graph_embedding) -> BCEWithLogitsLoss, mean reduction),
// ~20 tiny PyTorch kernels at B = 4096.  Two launches per pass: 32 lanes per row, 64 rows per block, per-block
// partials; a one-block kernel sums them in a fixed order.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <type_traits>
#include "kgnn_common.h"

#include "kgnn_launch.h"
#include "kgnn_philox.h"
#include "kgnn_head_terms.h"
#include "../../include/molkgnn_hip.h"

namespace mkgnn {

struct HeadArgs {
    const float* emb; int64_t es; int64_t B; int H;
    const float* w; const float* b; const float* y;
    float* pred; float* loss;
    const float* gloss; float* gemb; int64_t ges; float* gw; float* gb;
    float* partial;
    float drop_p;                  // dropout on emb ahead of the product (model.py:150,169), 0 = none
    int64_t* rng;                  // forward: {seed, offset}, offset advanced by one per launch
    int64_t* rng_used;             // forward writes / backward reads the {seed, offset} of this call's mask
};
// HEAD_ROWS, half_wave_sum, head_loss_term / head_dloss and with_loss_kind: kgnn_head_terms.h (shared with kgnn_task_head.hip)
template <int LK>
__device__ __forceinline__ float head_mean(float v, int64_t B) { return LK == MKGNN_LOSS_SQERR_SUM ? v : v / (float)B; }


template <int LK>
__global__ void __launch_bounds__(256) head_forward_kernel(HeadArgs a) {
    __shared__ float red[8];
    const int t = threadIdx.x, h = t & 31, g = t >> 5;          // 8 rows x 32 lanes per pass
    const float bias = a.b ? a.b[0] : 0.f;
    float s = 0.f;
    constexpr int NP = HEAD_ROWS / 8;
    // all loads of the block's 64 rows first (unconditional, clamped), then the arithmetic: one global round trip
    // per block instead of one per pass
    float xv[NP], yv[NP];
    const float w0 = h < a.H ? a.w[h] : 0.f;
    const bool drop = a.drop_p > 0.f;
    const uint64_t seed = drop ? (uint64_t)a.rng[0] : 0, offset = drop ? (uint64_t)a.rng[1] : 0;
#pragma unroll
    for (int k = 0; k < NP; ++k) {
        const int64_t i = (int64_t)blockIdx.x * HEAD_ROWS + k * 8 + g;
        const int64_t ic = i < a.B ? i : a.B - 1;
        xv[k] = a.emb[ic * a.es + (h < a.H ? h : 0)];
        yv[k] = a.y[ic];
    }
#pragma unroll
    for (int k = 0; k < NP; ++k) {
        const int64_t i = (int64_t)blockIdx.x * HEAD_ROWS + k * 8 + g;
        const int64_t ic = i < a.B ? i : a.B - 1;
        float x = h < a.H ? xv[k] * w0 : 0.f;
        if (drop) x *= keep_scale_of(seed, offset, (uint64_t)ic * a.H + (h < a.H ? h : 0), a.drop_p);
        for (int h0 = 32; h0 < a.H; h0 += 32)                   // (wider embeddings: the rare path)
            if (h0 + h < a.H) {
                float e = a.emb[ic * a.es + h0 + h];
                if (drop) e *= keep_scale_of(seed, offset, (uint64_t)ic * a.H + h0 + h, a.drop_p);
                x = fmaf(e, a.w[h0 + h], x);
            }
        x = half_wave_sum(x) + bias;
        if (h == 0 && i < a.B) {
            a.pred[i] = x;
            s += head_loss_term<LK>(x, yv[k]);
        }
    }
    if (h == 0) red[g] = s;
    __syncthreads();
    if (t == 0) {
        float p = 0.f;
        for (int k = 0; k < 8; ++k) p += red[k];
        a.partial[blockIdx.x] = p;
    }
}

// second launch of the forward: the block partials in a fixed tree -> loss; advances the dropout generator.
// (A "last block done" counter inside the first kernel did this in one launch, but the two device-scope fences it
// needs cost 10-15 us on this part -- more than a second, dependent launch: 4.7 us.)
template <int LK>
__global__ void __launch_bounds__(256) head_forward_final_kernel(HeadArgs a, int nblk) {
    __shared__ float fin[256];
    const int t = threadIdx.x;
    float v = 0.f;
    for (int bk = t; bk < nblk; bk += 256) v += a.partial[bk];
    fin[t] = v;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (t < w) fin[t] += fin[t + w];
        __syncthreads();
    }
    if (t == 0) {
        a.loss[0] = head_mean<LK>(fin[0], a.B);
        if (a.drop_p > 0.f) {
            const int64_t seed = a.rng[0], offset = a.rng[1];
            a.rng_used[0] = seed; a.rng_used[1] = offset;
            a.rng[1] = offset + 1;
        }
    }
}

template <int LK>
__global__ void __launch_bounds__(256) head_backward_kernel(HeadArgs a) {
    __shared__ float red[8][33];
    __shared__ float redb[8];
    const int t = threadIdx.x, h = t & 31, g = t >> 5;
    const float gl = head_mean<LK>(a.gloss[0], a.B);
    const int PW = a.H + 1;                                   // partial row: dW[0..H), db
    float db = 0.f;
    constexpr int NP = HEAD_ROWS / 8;
    const bool drop = a.drop_p > 0.f;
    const uint64_t seed = drop ? (uint64_t)a.rng_used[0] : 0, offset = drop ? (uint64_t)a.rng_used[1] : 0;
    // d loss / d pred of the block's rows: loads first (unconditional, clamped), then the arithmetic
    float dv[NP];
    {
        float pv[NP], yv[NP];
#pragma unroll
        for (int k = 0; k < NP; ++k) {
            const int64_t i = (int64_t)blockIdx.x * HEAD_ROWS + k * 8 + g;
            const int64_t ic = i < a.B ? i : a.B - 1;
            pv[k] = a.pred[ic];
            yv[k] = a.y[ic];
        }
#pragma unroll
        for (int k = 0; k < NP; ++k) {
            const int64_t i = (int64_t)blockIdx.x * HEAD_ROWS + k * 8 + g;
            dv[k] = i < a.B ? gl * head_dloss<LK>(pv[k], yv[k]) : 0.f;
            if (h == 0) db += dv[k];
        }
    }
    for (int h0 = 0; h0 < a.H; h0 += 32) {
        const int hh = h0 + h;
        const bool ok = hh < a.H;
        const float wv = ok ? a.w[hh] : 0.f;
        float dw = 0.f;
        float ev[NP];
#pragma unroll
        for (int k = 0; k < NP; ++k) {
            const int64_t i = (int64_t)blockIdx.x * HEAD_ROWS + k * 8 + g;
            const int64_t ic = i < a.B ? i : a.B - 1;
            ev[k] = a.emb[ic * a.es + (ok ? hh : 0)];
        }
#pragma unroll
        for (int k = 0; k < NP; ++k) {
            const int64_t i = (int64_t)blockIdx.x * HEAD_ROWS + k * 8 + g;
            if (i < a.B && ok) {
                const float ks = drop ? keep_scale_of(seed, offset, (uint64_t)i * a.H + hh, a.drop_p) : 1.f;
                dw = fmaf(dv[k], ev[k] * ks, dw);
                if (a.gemb) a.gemb[i * a.ges + hh] = dv[k] * wv * ks;
            }
        }
        red[g][h] = dw;
        __syncthreads();
        if (g == 0 && ok) {
            float p = 0.f;
            for (int k = 0; k < 8; ++k) p += red[k][h];
            a.partial[(size_t)blockIdx.x * PW + hh] = p;
        }
        __syncthreads();
    }
    if (h == 0) redb[g] = db;
    __syncthreads();
    if (t == 0) {
        float p = 0.f;
        for (int k = 0; k < 8; ++k) p += redb[k];
        a.partial[(size_t)blockIdx.x * PW + a.H] = p;
    }
}

// second launch of the backward: column c of the block partials, four row parts per column, eight loads in flight
// per thread; parts combined in a fixed order
__global__ void __launch_bounds__(256) head_backward_final_kernel(HeadArgs a, int nb) {
    __shared__ float fin[4][64];
    const int t = threadIdx.x;
    const int PW = a.H + 1;
    const float* part = a.partial;
    for (int c0 = 0; c0 < PW; c0 += 64) {
        const int c = c0 + (t & 63), pr = t >> 6;
        float tot = 0.f;
        if (c < PW) {
            for (int bk = pr; bk < nb; bk += 32) {
                float v[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) v[u] = part[(size_t)(bk + 4 * u < nb ? bk + 4 * u : bk) * PW + c];
#pragma unroll
                for (int u = 0; u < 8; ++u) if (bk + 4 * u < nb) tot += v[u];
            }
        }
        fin[pr][t & 63] = tot;
        __syncthreads();
        if (pr == 0 && c < PW) {
            const float r = (fin[0][t] + fin[1][t]) + (fin[2][t] + fin[3][t]);
            if (c < a.H) a.gw[c] = r;
            else if (a.gb) a.gb[0] = r;
        }
        __syncthreads();
    }
}

// ---- forward AND the gradients for d loss = 1 in one pass (mkgnn_bce_head_fused): the loss is the end of the graph, its
// own gradient is 1 in every training step, and d loss / d pred = (sigmoid(pred) - y) / B needs nothing but the row's pred --
// so the block that computes a row's pred also writes its row of grad_emb and adds to its partials of grad_weight /
// grad_bias; ONE final kernel sums the loss and the gradient partials.  Two launches where forward + backward took four
// (the four are kept: a caller whose d loss is not 1 scales these, or runs the separate backward).
// partial row of a block: [dW[0..H) | db | loss]
template <int LK>
__global__ void __launch_bounds__(256) head_fused_kernel(HeadArgs a) {
    __shared__ float red[8][33];
    __shared__ float redb[8], redl[8];
    const int t = threadIdx.x, h = t & 31, g = t >> 5;
    const float bias = a.b ? a.b[0] : 0.f;
    const int PW = a.H + 2;
    constexpr int NP = HEAD_ROWS / 8;
    float xv[NP], yv[NP], ks0[NP], dv[NP];
    const float w0 = h < a.H ? a.w[h] : 0.f;
    const bool drop = a.drop_p > 0.f;
    const uint64_t seed = drop ? (uint64_t)a.rng[0] : 0, offset = drop ? (uint64_t)a.rng[1] : 0;
    const float invB = head_mean<LK>(1.f, a.B);
#pragma unroll
    for (int k = 0; k < NP; ++k) {
        const int64_t i = (int64_t)blockIdx.x * HEAD_ROWS + k * 8 + g;
        const int64_t ic = i < a.B ? i : a.B - 1;
        xv[k] = a.emb[ic * a.es + (h < a.H ? h : 0)];
        yv[k] = a.y[ic];
    }
    float ls = 0.f, db = 0.f;
#pragma unroll
    for (int k = 0; k < NP; ++k) {
        const int64_t i = (int64_t)blockIdx.x * HEAD_ROWS + k * 8 + g;
        const int64_t ic = i < a.B ? i : a.B - 1;
        ks0[k] = drop ? keep_scale_of(seed, offset, (uint64_t)ic * a.H + (h < a.H ? h : 0), a.drop_p) : 1.f;
        float x = h < a.H ? xv[k] * w0 : 0.f;
        if (drop) x *= ks0[k];
        for (int h0 = 32; h0 < a.H; h0 += 32)                   // (wider embeddings: the rare path)
            if (h0 + h < a.H) {
                float e = a.emb[ic * a.es + h0 + h];
                if (drop) e *= keep_scale_of(seed, offset, (uint64_t)ic * a.H + h0 + h, a.drop_p);
                x = fmaf(e, a.w[h0 + h], x);
            }
        x = half_wave_sum(x) + bias;                            // (the xor tree leaves the sum in every lane of the row)
        dv[k] = i < a.B ? invB * head_dloss<LK>(x, yv[k]) : 0.f;
        if (h == 0 && i < a.B) {
            a.pred[i] = x;
            ls += head_loss_term<LK>(x, yv[k]);
            db += dv[k];
        }
    }
    for (int h0 = 0; h0 < a.H; h0 += 32) {
        const int hh = h0 + h;
        const bool ok = hh < a.H;
        const float wv = ok ? a.w[hh] : 0.f;
        float dw = 0.f;
#pragma unroll
        for (int k = 0; k < NP; ++k) {
            const int64_t i = (int64_t)blockIdx.x * HEAD_ROWS + k * 8 + g;
            if (i < a.B && ok) {
                float e = xv[k], ks = ks0[k];
                if (h0 > 0) {
                    e = a.emb[i * a.es + hh];
                    ks = drop ? keep_scale_of(seed, offset, (uint64_t)i * a.H + hh, a.drop_p) : 1.f;
                }
                dw = fmaf(dv[k], e * ks, dw);
                if (a.gemb) a.gemb[i * a.ges + hh] = dv[k] * wv * ks;
            }
        }
        red[g][h] = dw;
        __syncthreads();
        if (g == 0 && ok) {
            float p = 0.f;
            for (int k = 0; k < 8; ++k) p += red[k][h];
            a.partial[(size_t)blockIdx.x * PW + hh] = p;
        }
        __syncthreads();
    }
    if (h == 0) { redb[g] = db; redl[g] = ls; }
    __syncthreads();
    if (t == 0) {
        float p = 0.f, q = 0.f;
        for (int k = 0; k < 8; ++k) { p += redb[k]; q += redl[k]; }
        a.partial[(size_t)blockIdx.x * PW + a.H] = p;
        a.partial[(size_t)blockIdx.x * PW + a.H + 1] = q;
    }
}

// columns of the block partials (dW, db, loss), four row parts per column, eight loads in flight; fixed order; advances
// the dropout generator
template <int LK>
__global__ void __launch_bounds__(256) head_fused_final_kernel(HeadArgs a, int nb) {
    __shared__ float fin[4][64];
    const int t = threadIdx.x;
    const int PW = a.H + 2;
    const float* part = a.partial;
    for (int c0 = 0; c0 < PW; c0 += 64) {
        const int c = c0 + (t & 63), pr = t >> 6;
        float tot = 0.f;
        if (c < PW) {
            for (int bk = pr; bk < nb; bk += 32) {
                float v[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) v[u] = part[(size_t)(bk + 4 * u < nb ? bk + 4 * u : bk) * PW + c];
#pragma unroll
                for (int u = 0; u < 8; ++u) if (bk + 4 * u < nb) tot += v[u];
            }
        }
        fin[pr][t & 63] = tot;
        __syncthreads();
        if (pr == 0 && c < PW) {
            const float r = (fin[0][t] + fin[1][t]) + (fin[2][t] + fin[3][t]);
            if (c < a.H) a.gw[c] = r;
            else if (c == a.H) { if (a.gb) a.gb[0] = r; }
            else a.loss[0] = head_mean<LK>(r, a.B);
        }
        __syncthreads();
    }
    if (t == 0 && a.drop_p > 0.f) {
        const int64_t seed = a.rng[0], offset = a.rng[1];
        a.rng_used[0] = seed; a.rng_used[1] = offset;
        a.rng[1] = offset + 1;
    }
}

}  // namespace mkgnn

using namespace mkgnn;

// ================================================================== C ABI ==========================
enum { HEAD_FORWARD = 0, HEAD_BACKWARD = 1, HEAD_FUSED = 2 };

// The one argument path of the ten entries below: the shape, pointer, stride, dropout and workspace checks of MODE, the HeadArgs
// fill and MODE's two launches.  An argument an entry does not have arrives null / 0 and stays so in the kernels' struct.
template <int MODE>
static int head_run(const char* who, int32_t lk, const float* emb, int64_t emb_stride, int64_t n_rows, int32_t H,
                    const float* weight, const float* bias, const float* target, float p, int64_t* rng_state,
                    const int64_t* rng_used, const float* pred, float* loss, const float* grad_loss, float* grad_emb,
                    int64_t grad_emb_stride, float* grad_weight, float* grad_bias, void* ws, size_t ws_bytes, void* stream) {
    if (n_rows < 1 || H < 1 || emb_stride < H) return api_fail("%s: bad shape", who);
    constexpr bool BWD = MODE == HEAD_BACKWARD;
    if (!emb || !weight || !target || !pred || (BWD ? !grad_loss : !loss) || (MODE != HEAD_FORWARD && !grad_weight))
        return api_fail("%s: null pointer", who);
    if (grad_emb && grad_emb_stride < H) return api_fail("%s: bad grad_emb stride", who);
    if (!(p >= 0.f && p < 1.f)) return api_fail("%s: dropout probability %g outside [0, 1)", who, p);
    if (p > 0.f && BWD && !rng_used) return api_fail("%s: dropout needs the forward's rng_used", who);
    if (p > 0.f && !BWD && (!rng_state || !rng_used)) return api_fail("%s: dropout needs rng_state and rng_used", who);
    if (!ws || ws_bytes < mkgnn_bce_head_workspace_bytes(n_rows, H) || ((uintptr_t)ws & 3))
        return api_fail("%s: workspace too small or misaligned", who);
    HeadArgs a{};
    a.partial = (float*)((char*)ws + 16);
    a.emb = emb; a.es = emb_stride; a.B = n_rows; a.H = H; a.w = weight; a.b = bias; a.y = target;
    a.pred = (float*)pred; a.loss = loss; a.gloss = grad_loss; a.gemb = grad_emb; a.ges = grad_emb_stride; a.gw = grad_weight; a.gb = grad_bias;
    a.drop_p = p; a.rng = rng_state; a.rng_used = (int64_t*)rng_used;
    const int nblk = (int)((n_rows + HEAD_ROWS - 1) / HEAD_ROWS);
    hipStream_t s = (hipStream_t)stream;
    if (!with_loss_kind(lk, [&](auto K) {
            constexpr int LK = decltype(K)::value;
            if constexpr (MODE == HEAD_FUSED) {
                head_fused_kernel<LK><<<nblk, 256, 0, s>>>(a);
                head_fused_final_kernel<LK><<<1, 256, 0, s>>>(a, nblk);
            } else if constexpr (MODE == HEAD_FORWARD) {
                head_forward_kernel<LK><<<nblk, 256, 0, s>>>(a);
                head_forward_final_kernel<LK><<<1, 256, 0, s>>>(a, nblk);
            } else {
                head_backward_kernel<LK><<<nblk, 256, 0, s>>>(a);
                head_backward_final_kernel<<<1, 256, 0, s>>>(a, nblk);
            }
        }))
        return api_fail("%s: unknown loss kind %d", who, (int)lk);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : api_hip_fail(who, e);
}

extern "C" {

size_t mkgnn_bce_head_workspace_bytes(int64_t n_rows, int32_t H) {
    if (n_rows < 1 || H < 1) return 0;
    return 16 + (size_t)((n_rows + HEAD_ROWS - 1) / HEAD_ROWS) * (H + 2) * 4;
}

int mkgnn_bce_head_fused(const float* emb, int64_t emb_stride, int64_t n_rows, int32_t H, const float* weight, const float* bias,
                         const float* target, float dropout_p, int64_t* rng_state, int64_t* rng_used, float* pred, float* loss,
                         float* grad_emb, int64_t grad_emb_stride, float* grad_weight, float* grad_bias, void* ws,
                         size_t ws_bytes, void* stream) {
    return head_run<HEAD_FUSED>("mkgnn_bce_head_fused", MKGNN_LOSS_BCE_MEAN, emb, emb_stride, n_rows, H, weight, bias, target,
                                dropout_p, rng_state, rng_used, pred, loss, nullptr, grad_emb, grad_emb_stride, grad_weight,
                                grad_bias, ws, ws_bytes, stream);
}

int mkgnn_head_loss_fused(int32_t loss_kind, const float* emb, int64_t emb_stride, int64_t n_rows, int32_t H, const float* weight,
                          const float* bias, const float* target, float dropout_p, int64_t* rng_state, int64_t* rng_used,
                          float* pred, float* loss, float* grad_emb, int64_t grad_emb_stride, float* grad_weight,
                          float* grad_bias, void* ws, size_t ws_bytes, void* stream) {
    return head_run<HEAD_FUSED>("mkgnn_head_loss_fused", loss_kind, emb, emb_stride, n_rows, H, weight, bias, target, dropout_p,
                                rng_state, rng_used, pred, loss, nullptr, grad_emb, grad_emb_stride, grad_weight, grad_bias, ws,
                                ws_bytes, stream);
}

int mkgnn_bce_head_forward(const float* emb, int64_t emb_stride, int64_t n_rows, int32_t H, const float* weight,
                           const float* bias, const float* target, float* pred, float* loss, void* ws, size_t ws_bytes,
                           void* stream) {
    return head_run<HEAD_FORWARD>("mkgnn_bce_head_forward", MKGNN_LOSS_BCE_MEAN, emb, emb_stride, n_rows, H, weight, bias, target,
                                  0.f, nullptr, nullptr, pred, loss, nullptr, nullptr, 0, nullptr, nullptr, ws, ws_bytes, stream);
}

int mkgnn_bce_head_backward(const float* emb, int64_t emb_stride, int64_t n_rows, int32_t H, const float* weight,
                            const float* target, const float* pred, const float* grad_loss, float* grad_emb,
                            int64_t grad_emb_stride, float* grad_weight, float* grad_bias, void* ws, size_t ws_bytes,
                            void* stream) {
    return head_run<HEAD_BACKWARD>("mkgnn_bce_head_backward", MKGNN_LOSS_BCE_MEAN, emb, emb_stride, n_rows, H, weight, nullptr,
                                   target, 0.f, nullptr, nullptr, pred, nullptr, grad_loss, grad_emb, grad_emb_stride, grad_weight,
                                   grad_bias, ws, ws_bytes, stream);
}

int mkgnn_bce_head_dropout_forward(const float* emb, int64_t emb_stride, int64_t n_rows, int32_t H, const float* weight,
                                   const float* bias, const float* target, float dropout_p, int64_t* rng_state,
                                   int64_t* rng_used, float* pred, float* loss, void* ws, size_t ws_bytes, void* stream) {
    return head_run<HEAD_FORWARD>("mkgnn_bce_head_dropout_forward", MKGNN_LOSS_BCE_MEAN, emb, emb_stride, n_rows, H, weight, bias,
                                  target, dropout_p, rng_state, rng_used, pred, loss, nullptr, nullptr, 0, nullptr, nullptr, ws,
                                  ws_bytes, stream);
}

int mkgnn_bce_head_dropout_backward(const float* emb, int64_t emb_stride, int64_t n_rows, int32_t H, const float* weight,
                                    const float* target, const float* pred, const float* grad_loss, float dropout_p,
                                    const int64_t* rng_used, float* grad_emb, int64_t grad_emb_stride, float* grad_weight,
                                    float* grad_bias, void* ws, size_t ws_bytes, void* stream) {
    return head_run<HEAD_BACKWARD>("mkgnn_bce_head_dropout_backward", MKGNN_LOSS_BCE_MEAN, emb, emb_stride, n_rows, H, weight,
                                   nullptr, target, dropout_p, nullptr, rng_used, pred, nullptr, grad_loss, grad_emb,
                                   grad_emb_stride, grad_weight, grad_bias, ws, ws_bytes, stream);
}

int mkgnn_head_loss_forward(int32_t loss_kind, const float* emb, int64_t emb_stride, int64_t n_rows, int32_t H,
                            const float* weight, const float* bias, const float* target, float* pred, float* loss, void* ws,
                            size_t ws_bytes, void* stream) {
    return head_run<HEAD_FORWARD>("mkgnn_head_loss_forward", loss_kind, emb, emb_stride, n_rows, H, weight, bias, target, 0.f,
                                  nullptr, nullptr, pred, loss, nullptr, nullptr, 0, nullptr, nullptr, ws, ws_bytes, stream);
}

int mkgnn_head_loss_backward(int32_t loss_kind, const float* emb, int64_t emb_stride, int64_t n_rows, int32_t H,
                             const float* weight, const float* target, const float* pred, const float* grad_loss,
                             float* grad_emb, int64_t grad_emb_stride, float* grad_weight, float* grad_bias, void* ws,
                             size_t ws_bytes, void* stream) {
    return head_run<HEAD_BACKWARD>("mkgnn_head_loss_backward", loss_kind, emb, emb_stride, n_rows, H, weight, nullptr, target, 0.f,
                                   nullptr, nullptr, pred, nullptr, grad_loss, grad_emb, grad_emb_stride, grad_weight, grad_bias,
                                   ws, ws_bytes, stream);
}

int mkgnn_head_loss_dropout_forward(int32_t loss_kind, const float* emb, int64_t emb_stride, int64_t n_rows, int32_t H,
                                    const float* weight, const float* bias, const float* target, float dropout_p,
                                    int64_t* rng_state, int64_t* rng_used, float* pred, float* loss, void* ws, size_t ws_bytes,
                                    void* stream) {
    return head_run<HEAD_FORWARD>("mkgnn_head_loss_dropout_forward", loss_kind, emb, emb_stride, n_rows, H, weight, bias, target,
                                  dropout_p, rng_state, rng_used, pred, loss, nullptr, nullptr, 0, nullptr, nullptr, ws, ws_bytes,
                                  stream);
}

int mkgnn_head_loss_dropout_backward(int32_t loss_kind, const float* emb, int64_t emb_stride, int64_t n_rows, int32_t H,
                                     const float* weight, const float* target, const float* pred, const float* grad_loss,
                                     float dropout_p, const int64_t* rng_used, float* grad_emb, int64_t grad_emb_stride,
                                     float* grad_weight, float* grad_bias, void* ws, size_t ws_bytes, void* stream) {
    return head_run<HEAD_BACKWARD>("mkgnn_head_loss_dropout_backward", loss_kind, emb, emb_stride, n_rows, H, weight, nullptr,
                                   target, dropout_p, nullptr, rng_used, pred, nullptr, grad_loss, grad_emb, grad_emb_stride,
                                   grad_weight, grad_bias, ws, ws_bytes, stream);
}

}  // extern "C"
