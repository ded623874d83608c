// AdamW step of the whole model in one launch (gfx950).
//
// The reference trains with torch.optim.AdamW over two parameter groups (model.py:368-385: the kernel banks exempt
// from weight decay).  MolKGNN has ~80 small trainable tensors (132 k floats in all): PyTorch's fused multi-tensor
// path needs two launches per group plus one per group for the step counters -- five launch-bound kernels, ~40 us
// of a 1.3 ms training step, for 2 MB of traffic.  Here the tensor table travels in the kernel arguments (pointers
// are baked into a captured graph exactly like PyTorch's), one block per 1024 elements, each with its own copy of the
// tensor's step counter (round 2: a one-block kernel ahead of it advanced the counters -- 10 us for the pair; a "last block
// done" counter inside the update kernel was measured at 27 us for the two device-scope fences it needs).
//
// Arithmetic: the update of torch's fused kernel (fused_adam_utils.cuh, ADAMW mode), in the same order:
//   p -= lr * wd * p;  m += (1 - b1) (g - m);  v = b2 v + (1 - b2) g g;
//   p -= (lr / (1 - b1^t)) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)
//
// Clipped form (mkgnn_adamw_step_clipped): the global norm of all gradients the step reads, and clip_grad_norm_'s coefficient
// folded into the multiply by grad_scale.  One launch ahead of the update writes a float64 partial of gg^2 per block of the
// table (adamw_sq_partial_kernel); EVERY block of the update adds up all partials in its prologue, in one fixed order, so all
// blocks of all launches of the step hold the same sum bit for bit: the same coefficient everywhere, and a non-finite norm
// skips the step in every block or in none, with no signalling between blocks.  No atomics, no host round trip.
//
// Averaged forms (mkgnn_adamw_step_averaged): an EMA or running mean of every parameter, updated from the p_new the block holds
// in a register -- one more load and store per element, no launch (torch.optim.swa_utils.AveragedModel is two multi-tensor
// launches behind the step), and only for a step that was taken: the decision is the device's.  mkgnn_flat_swap exchanges the
// parameters with their averages for an evaluation, in one launch.
#include <type_traits>
#include "kgnn_launch.h"
#include "../../include/molkgnn_hip.h"

namespace mkgnn {

constexpr int ADAM_MAX_TENSORS = 80;      // per launch: 80 * 40 B of kernel arguments
constexpr int ADAM_MAX_GROUPS = 4;
constexpr int ADAM_CHUNK = 1024;          // elements per block
constexpr int ADAM_CLIP_PROLOGUE_BLOCKS = MKGNN_ADAMW_CLIP_PROLOGUE_BLOCKS;

struct AdamTensor { float* p; const float* g; float* state; const float* active; int32_t n; int32_t group; };
struct AdamGroup { const float* lr_ptr; float lr, beta1, beta2, eps, wd; int32_t maximize; float gscale; };
struct AdamArgs {
    AdamTensor t[ADAM_MAX_TENSORS];
    AdamGroup grp[ADAM_MAX_GROUPS];
    int32_t blk_start[ADAM_MAX_TENSORS + 1];
    int32_t nt;
};
// the clipped update's second argument: `np` partials of sum gg^2 (the whole table's, or the finishing launch's one), the
// threshold, the guard, and -- in the first launch of a step only -- where block 0 writes the stats
struct AdamClip { const double* partial; int32_t np; float max_norm; int32_t skip_nonfinite; float* stats; };
struct AdamClipArgs : AdamArgs { AdamClip c; };
static_assert(sizeof(AdamClipArgs) <= 4096, "kernel arguments of the clipped update");
// the averaged forms: the settings of the weight average behind either argument block.  The average itself needs no pointer: it
// lies behind the tensor's packed state (80 more pointers would not fit the 4096 bytes).
struct AdamAvgArgs : AdamArgs { mkgnn_adamw_average v; };
struct AdamClipAvgArgs : AdamClipArgs { mkgnn_adamw_average v; };
static_assert(sizeof(AdamClipAvgArgs) <= 4096 && sizeof(AdamAvgArgs) <= 4096, "kernel arguments of the averaged update");

// Sum of one double per lane over the 256 lanes of a block, in one fixed order, the same bits in every lane: a butterfly inside
// each wave (both partners of an exchange form the same a + b), then the four wave sums ((w0 + w1) + w2) + w3.
__device__ __forceinline__ double block_sum_256(double x, double* wave_sums /* [4], shared */) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) x += __shfl_xor(x, off, 64);
    if ((threadIdx.x & 63) == 0) wave_sums[threadIdx.x >> 6] = x;
    __syncthreads();
    return ((wave_sums[0] + wave_sums[1]) + wave_sums[2]) + wave_sums[3];
}

// The coefficient multiply of the clipped update, kept out of any fused multiply-add: the update is the unclipped one on
// fl32(gg * coef).
__device__ __forceinline__ float mul_rounded(float a, float b) {
#pragma clang fp contract(off)
    return a * b;
}

// One update of the weight average, avg + fl32(w * fl32(p - avg)): three float32 operations, each rounded, none contracted -- the
// form separate torch operators on the CPU reproduce bit for bit.
__device__ __forceinline__ float lerp_rounded(float avg, float p, float w) {
#pragma clang fp contract(off)
    const float d = p - avg;
    const float wd = w * d;
    return avg + wd;
}

// state of a tensor: [exp_avg | exp_avg_sq | step | 2 reserved | one step counter per block of the tensor].  Every block
// advances ITS OWN copy of the step count and derives the bias corrections from it (two double-precision pow per block), so
// no block reads a counter another block writes: the separate one-block counting kernel of round 2 (a dependent launch,
// 4 us of every step) is gone.  Block 0 also writes the canonical `step` the caller's state_dict reads.
//
// AVG (Args carries `v`): the average of the weights, [avg | canonical n_averaged | one n_averaged per block] directly behind the
// state.  A block that takes the step loads its chunk of avg with the other loads; thread 0 derives the block's weight w from ITS
// copy of the count (in double, rounded once) next to the bias corrections and advances that copy; w == 1 copies p_new, anything
// else is lerp_rounded.  A block that returns early -- idle tensor, skipped step -- has touched neither avg nor a count.
template <class Args, bool AVG = false>
__global__ void __launch_bounds__(256) adamw_step_kernel(Args a) {
    constexpr bool CLIP = std::is_base_of_v<AdamClipArgs, Args>;
    __shared__ float bc[AVG ? 3 : 2];                        // the bias corrections, and the average's weight
    // block -> tensor: the last ti with blk_start[ti] <= blockIdx.x
    int lo = 0, hi = a.nt - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (a.blk_start[mid] <= (int)blockIdx.x) lo = mid; else hi = mid - 1;
    }
    const AdamTensor T = a.t[lo];
    bool idle = false, reports = false;
    if constexpr (!CLIP) {                                   // (its own line: folded into the clipped form's test below, the unclipped
                                                             // instantiation compiles to other instructions than it did)
        if (T.active && *T.active == 0.f) return;            // (block-uniform) no gradient anywhere this step: the step count stands still
    } else {
        idle = T.active && *T.active == 0.f;
        reports = a.c.stats && blockIdx.x == 0;              // the one block that writes the stats stays to do so, idle or not
        if (idle && !reports) return;
    }
    const AdamGroup G = a.grp[T.group];
    const float lr = G.lr_ptr ? *G.lr_ptr : G.lr;
    float* m = T.state;
    float* v = T.state + T.n;
    const int blk = (int)blockIdx.x - a.blk_start[lo];
    const int base = blk * ADAM_CHUNK;
    float g[ADAM_CHUNK / 256], p[ADAM_CHUNK / 256], mi[ADAM_CHUNK / 256], vi[ADAM_CHUNK / 256];
    [[maybe_unused]] float av[ADAM_CHUNK / 256];
    [[maybe_unused]] float* avg = nullptr;
    if constexpr (AVG) avg = T.state + 2 * (size_t)T.n + 3 + (T.n + ADAM_CHUNK - 1) / ADAM_CHUNK;
#pragma unroll
    for (int k = 0; k < ADAM_CHUNK / 256; ++k) {          // all loads first (clamped), then the arithmetic
        const int i = base + 256 * k + (int)threadIdx.x;
        const int ic = i < T.n ? i : T.n - 1;
        g[k] = T.g[ic]; p[k] = T.p[ic]; mi[k] = m[ic]; vi[k] = v[ic];
        if constexpr (AVG) av[k] = avg[ic];
    }
    float coef = 1.f;
    if constexpr (CLIP) {
        // the whole table's sum of gg^2, the same bits in every block of every launch of this step
        __shared__ double wave_sums[4];
        const AdamClip& c = a.c;
        double s = 0.0;
        for (int j = (int)threadIdx.x; j < c.np; j += 256) s += c.partial[j];
        const double S = block_sum_256(s, wave_sums);
        const double norm = sqrt(S);
        const double r = (double)c.max_norm / (norm + 1e-6);
        coef = (float)(r > 1.0 ? 1.0 : r);                   // min(1, r) that keeps a NaN (fmin would drop it)
        const bool skipped = c.skip_nonfinite && !(S < (double)INFINITY);
        if (reports && threadIdx.x == 0) {
            c.stats[0] = (float)norm;
            c.stats[1] = coef;
            if (skipped) c.stats[2] += 1.f;
        }
        if (skipped || idle) return;                         // (block-uniform) before the per-block step count is touched
    }
    if (threadIdx.x == 0) {
        float* tail = T.state + 2 * (size_t)T.n;
        const double t = (double)tail[3 + blk] + 1.0;
        tail[3 + blk] = (float)t;
        if (blk == 0) tail[0] = (float)t;
        bc[0] = (float)(1.0 - pow((double)G.beta1, t));
        bc[1] = sqrtf((float)(1.0 - pow((double)G.beta2, t)));
        if constexpr (AVG) {
            float w = 1.f;                                   // t <= start, or the first update: avg = p_new
            if (t > (double)a.v.start) {
                float* cnt = avg + T.n;                      // [canonical | one per block]
                const double n = (double)cnt[1 + blk];
                if (n >= 1.0) {
                    double d = (double)a.v.decay;
                    if (a.v.warmup) { const double dw = (1.0 + n) / (10.0 + n); d = dw < d ? dw : d; }
                    w = a.v.mode == MKGNN_ADAMW_AVERAGE_MEAN ? (float)(1.0 / (n + 1.0)) : (float)(1.0 - d);
                }
                const float n1 = (float)(n + 1.0);
                cnt[1 + blk] = n1;
                if (blk == 0) cnt[0] = n1;
            }
            bc[2] = w;
        }
    }
    __syncthreads();
    const float bc1 = bc[0], bc2_sqrt = bc[1];
    [[maybe_unused]] float w = 1.f;
    if constexpr (AVG) w = bc[2];
    const float step_size = lr / bc1;
#pragma unroll
    for (int k = 0; k < ADAM_CHUNK / 256; ++k) {
        const int i = base + 256 * k + (int)threadIdx.x;
        if (i < T.n) {
            float gg = (G.maximize ? -g[k] : g[k]) * G.gscale;
            if constexpr (CLIP) gg = mul_rounded(gg, coef);
            float pp = p[k];
            if constexpr (!AVG) {
                pp -= lr * G.wd * pp;
            } else {
                // The averaged instantiations spell out every choice the compiler makes in the two above -- which multiply goes
                // into which multiply-add depends on the code around it, and here it chose otherwise (measured: the unclipped
                // averaged step's exp_avg and exp_avg_sq were not the unclipped step's): the rounded gg, and this multiply-add.
                if constexpr (!CLIP) gg = mul_rounded(G.maximize ? -g[k] : g[k], G.gscale);
                pp = fmaf(-(lr * G.wd), pp, pp);
            }
            const float mm = fmaf(1.f - G.beta1, gg - mi[k], mi[k]);
            float vv;
            if constexpr (!CLIP && !AVG) {
                vv = G.beta2 * vi[k] + (1.f - G.beta2) * gg * gg;
            } else {
                // What the compiler makes of the line above there, spelt out: a multiply-add on the rounded b2 v.  Left to
                // itself it makes two multiplies and an add of it here, and a step with coef = 1 would not be the unclipped step.
                vv = fmaf((1.f - G.beta2) * gg, gg, G.beta2 * vi[k]);
            }
            const float denom = sqrtf(vv) / bc2_sqrt + G.eps;
            pp -= step_size * mm / denom;
            T.p[i] = pp; m[i] = mm; v[i] = vv;
            if constexpr (AVG) avg[i] = w == 1.f ? pp : lerp_rounded(av[k], pp, w);
        }
    }
}

// One float64 partial of gg^2 per block of the table, gg = fl32(+-g * grad_scale) as the update forms it; the block-to-tensor
// search and the blocks are the update's.  Lanes past the tensor's end add nothing (the update's clamped loads are not
// counted); a tensor whose flag reads 0 writes a partial of 0, so every partial is written on every call.
__global__ void __launch_bounds__(256) adamw_sq_partial_kernel(AdamArgs a, double* partial) {
    __shared__ double wave_sums[4];
    int lo = 0, hi = a.nt - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (a.blk_start[mid] <= (int)blockIdx.x) lo = mid; else hi = mid - 1;
    }
    const AdamTensor T = a.t[lo];
    const AdamGroup G = a.grp[T.group];
    const int base = ((int)blockIdx.x - a.blk_start[lo]) * ADAM_CHUNK;
    double s = 0.0;
    if (!(T.active && *T.active == 0.f)) {                   // (block-uniform)
        float g[ADAM_CHUNK / 256];
#pragma unroll
        for (int k = 0; k < ADAM_CHUNK / 256; ++k) {
            const int i = base + 256 * k + (int)threadIdx.x;
            g[k] = T.g[i < T.n ? i : T.n - 1];
        }
#pragma unroll
        for (int k = 0; k < ADAM_CHUNK / 256; ++k) {
            const int i = base + 256 * k + (int)threadIdx.x;
            const double gg = (double)((G.maximize ? -g[k] : g[k]) * G.gscale);
            if (i < T.n) s += gg * gg;
        }
    }
    s = block_sum_256(s, wave_sums);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// Beyond ADAM_CLIP_PROLOGUE_BLOCKS partials the update's blocks do not each read them all: one workgroup sums them first, in a
// fixed order (lane l takes l, l + 256, ...), into the one double the update then reads as its only partial.
__global__ void __launch_bounds__(256) adamw_sq_finish_kernel(const double* partial, int64_t np, double* sum) {
    __shared__ double wave_sums[4];
    double s = 0.0;
    for (int64_t j = threadIdx.x; j < np; j += 256) s += partial[j];
    s = block_sum_256(s, wave_sums);
    if (threadIdx.x == 0) *sum = s;
}

// Many small tensors into their slots of one flat buffer (or back) in ONE launch: the data-parallel step's gradients into the
// buffer RCCL sums (dp.FlatGradAllReduce).  torch._foreach_copy_ over the model's ~50 gradients is two multi-tensor launches of
// 12 us each at the end of every step's backward; this is one of launch-floor length (0.5 MB).
constexpr int COPY_MAX_ITEMS = 120;
struct CopyItem { float* dst; const float* src; int32_t n; int32_t pad; };
struct CopyArgs { CopyItem t[COPY_MAX_ITEMS]; int32_t blk_start[COPY_MAX_ITEMS + 1]; int32_t nt; };
__global__ void __launch_bounds__(256) flat_copy_kernel(CopyArgs a) {
    int lo = 0, hi = a.nt - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (a.blk_start[mid] <= (int)blockIdx.x) lo = mid; else hi = mid - 1;
    }
    const CopyItem T = a.t[lo];
    const int base = ((int)blockIdx.x - a.blk_start[lo]) * ADAM_CHUNK;
    float v[ADAM_CHUNK / 256];
#pragma unroll
    for (int k = 0; k < ADAM_CHUNK / 256; ++k) {
        const int i = base + 256 * k + (int)threadIdx.x;
        v[k] = T.src[i < T.n ? i : T.n - 1];
    }
#pragma unroll
    for (int k = 0; k < ADAM_CHUNK / 256; ++k) {
        const int i = base + 256 * k + (int)threadIdx.x;
        if (i < T.n) T.dst[i] = v[k];
    }
}

// The contents of many small tensor pairs exchanged in ONE launch: the averaged weights into the model and the live ones out of it
// (optim.FusedAdamW.swap_averaged), and back.  flat_copy_kernel's shape: both loads first, then the two stores.
struct SwapItem { float* a; float* b; int32_t n; int32_t pad; };
struct SwapArgs { SwapItem t[COPY_MAX_ITEMS]; int32_t blk_start[COPY_MAX_ITEMS + 1]; int32_t nt; };
static_assert(sizeof(SwapArgs) <= 4096, "kernel arguments of the swap");
__global__ void __launch_bounds__(256) flat_swap_kernel(SwapArgs a) {
    int lo = 0, hi = a.nt - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (a.blk_start[mid] <= (int)blockIdx.x) lo = mid; else hi = mid - 1;
    }
    const SwapItem T = a.t[lo];
    const int base = ((int)blockIdx.x - a.blk_start[lo]) * ADAM_CHUNK;
    float va[ADAM_CHUNK / 256], vb[ADAM_CHUNK / 256];
#pragma unroll
    for (int k = 0; k < ADAM_CHUNK / 256; ++k) {
        const int i = base + 256 * k + (int)threadIdx.x;
        const int ic = i < T.n ? i : T.n - 1;
        va[k] = T.a[ic]; vb[k] = T.b[ic];
    }
#pragma unroll
    for (int k = 0; k < ADAM_CHUNK / 256; ++k) {
        const int i = base + 256 * k + (int)threadIdx.x;
        if (i < T.n) { T.a[i] = vb[k]; T.b[i] = va[k]; }
    }
}

}  // namespace mkgnn

using namespace mkgnn;

extern "C" int mkgnn_flat_swap(const mkgnn_swap_item* items, int32_t n_items, void* stream) {
    if (n_items < 0) return api_fail("mkgnn_flat_swap: %d items", n_items);
    if (n_items == 0) return 0;
    if (!items) return api_fail("mkgnn_flat_swap: null pointer");
    for (int32_t i = 0; i < n_items; ++i)                     // every item is looked at before anything is launched
        if (!items[i].a || !items[i].b || items[i].numel < 1 || items[i].numel > (1 << 30))
            return api_fail("mkgnn_flat_swap: item %d: null pointer or numel %lld out of range", i, (long long)items[i].numel);
    hipStream_t st = (hipStream_t)stream;
    SwapArgs a{};
    for (int32_t first = 0; first < n_items; first += COPY_MAX_ITEMS) {
        const int nt = n_items - first < COPY_MAX_ITEMS ? n_items - first : COPY_MAX_ITEMS;
        int blocks = 0;
        for (int i = 0; i < nt; ++i) {
            const mkgnn_swap_item& s = items[first + i];
            a.t[i] = SwapItem{s.a, s.b, (int32_t)s.numel, 0};
            a.blk_start[i] = blocks;
            blocks += (int)((s.numel + ADAM_CHUNK - 1) / ADAM_CHUNK);
        }
        a.blk_start[nt] = blocks;
        a.nt = nt;
        flat_swap_kernel<<<blocks, 256, 0, st>>>(a);
    }
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : api_hip_fail("mkgnn_flat_swap", e);
}

extern "C" int mkgnn_flat_copy(const mkgnn_copy_item* items, int32_t n_items, void* stream) {
    if (n_items < 0) return api_fail("mkgnn_flat_copy: %d items", n_items);
    if (n_items == 0) return 0;
    if (!items) return api_fail("mkgnn_flat_copy: null pointer");
    hipStream_t st = (hipStream_t)stream;
    CopyArgs a{};
    for (int32_t first = 0; first < n_items; first += COPY_MAX_ITEMS) {
        const int nt = n_items - first < COPY_MAX_ITEMS ? n_items - first : COPY_MAX_ITEMS;
        int blocks = 0;
        for (int i = 0; i < nt; ++i) {
            const mkgnn_copy_item& s = items[first + i];
            if (!s.dst || !s.src || s.numel < 1 || s.numel > (1 << 30))
                return api_fail("mkgnn_flat_copy: item %d: null pointer or numel %lld out of range", first + i, (long long)s.numel);
            a.t[i] = CopyItem{s.dst, s.src, (int32_t)s.numel, 0};
            a.blk_start[i] = blocks;
            blocks += (int)((s.numel + ADAM_CHUNK - 1) / ADAM_CHUNK);
        }
        a.blk_start[nt] = blocks;
        a.nt = nt;
        flat_copy_kernel<<<blocks, 256, 0, st>>>(a);
    }
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : api_hip_fail("mkgnn_flat_copy", e);
}

extern "C" int64_t mkgnn_adamw_state_floats(int64_t numel) {
    return numel < 1 ? 0 : 2 * numel + 3 + (numel + ADAM_CHUNK - 1) / ADAM_CHUNK;
}

// The groups of a call into `a` (0, or the error's return value).
static int adam_fill_groups(AdamArgs& a, const mkgnn_adamw_group* groups, int32_t n_groups, const char* who) {
    for (int g = 0; g < n_groups; ++g) {
        const mkgnn_adamw_group& s = groups[g];
        if (!(s.beta1 >= 0.f && s.beta1 < 1.f && s.beta2 >= 0.f && s.beta2 < 1.f) || s.eps < 0.f || s.weight_decay < 0.f)
            return api_fail("%s: group %d has betas (%g, %g), eps %g, weight_decay %g", who, g, s.beta1, s.beta2, s.eps, s.weight_decay);
        a.grp[g] = AdamGroup{s.lr_device, s.lr, s.beta1, s.beta2, s.eps, s.weight_decay, s.maximize, s.grad_scale};
    }
    return 0;
}

// Tensors [first, first + nt) of the table into `a`: *blocks is the launch's grid (0, or the error's return value).
static int adam_fill_launch(AdamArgs& a, const mkgnn_adamw_tensor* tensors, int32_t first, int nt, int32_t n_groups, const char* who,
                            int* blocks) {
    int b = 0;
    for (int i = 0; i < nt; ++i) {
        const mkgnn_adamw_tensor& s = tensors[first + i];
        if (!s.param || !s.grad || !s.state || s.numel < 1 || s.numel > (1 << 30) || s.group < 0 || s.group >= n_groups)
            return api_fail("%s: tensor %d: null pointer, numel %lld or group %d out of range", who, first + i, (long long)s.numel, s.group);
        a.t[i] = AdamTensor{s.param, s.grad, s.state, s.active, (int32_t)s.numel, s.group};
        a.blk_start[i] = b;
        b += (int)((s.numel + ADAM_CHUNK - 1) / ADAM_CHUNK);
    }
    a.blk_start[nt] = b;
    a.nt = nt;
    *blocks = b;
    return 0;
}

// The unclipped step of `Args` (AdamArgs, or AdamAvgArgs with the average's settings `v`): one launch per 80 tensors.
template <class Args>
static int adam_step(const char* who, const mkgnn_adamw_tensor* tensors, int32_t n_tensors, const mkgnn_adamw_group* groups,
                     int32_t n_groups, const mkgnn_adamw_average* v, void* stream) {
    constexpr bool AVG = std::is_same_v<Args, AdamAvgArgs>;
    if (n_tensors < 0 || n_groups < 1 || n_groups > ADAM_MAX_GROUPS)
        return api_fail("%s: %d tensors, %d groups (1..%d groups)", who, n_tensors, n_groups, ADAM_MAX_GROUPS);
    if (n_tensors == 0) return 0;
    if (!tensors || !groups) return api_fail("%s: null pointer", who);
    hipStream_t st = (hipStream_t)stream;
    Args a{};
    if constexpr (AVG) a.v = *v;
    if (int rc = adam_fill_groups(a, groups, n_groups, who)) return rc;
    if constexpr (AVG) {                                     // the averaged entry looks at every tensor before anything is launched
        for (int32_t first = 0; first < n_tensors; first += ADAM_MAX_TENSORS) {
            const int nt = n_tensors - first < ADAM_MAX_TENSORS ? n_tensors - first : ADAM_MAX_TENSORS;
            int blocks = 0;
            if (int rc = adam_fill_launch(a, tensors, first, nt, n_groups, who, &blocks)) return rc;
        }
    }
    for (int32_t first = 0; first < n_tensors; first += ADAM_MAX_TENSORS) {
        const int nt = n_tensors - first < ADAM_MAX_TENSORS ? n_tensors - first : ADAM_MAX_TENSORS;
        int blocks = 0;
        if (int rc = adam_fill_launch(a, tensors, first, nt, n_groups, who, &blocks)) return rc;
        adamw_step_kernel<Args, AVG><<<blocks, 256, 0, st>>>(a);
    }
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : api_hip_fail(who, e);
}

extern "C" int mkgnn_adamw_step(const mkgnn_adamw_tensor* tensors, int32_t n_tensors, const mkgnn_adamw_group* groups,
                                int32_t n_groups, void* stream) {
    return adam_step<AdamArgs>("mkgnn_adamw_step", tensors, n_tensors, groups, n_groups, nullptr, stream);
}

// blocks of the whole table (a tensor without elements has none)
static int64_t adam_table_blocks(const mkgnn_adamw_tensor* tensors, int32_t n_tensors) {
    int64_t blocks = 0;
    for (int32_t i = 0; tensors && i < n_tensors; ++i)
        if (tensors[i].numel > 0) blocks += (tensors[i].numel + ADAM_CHUNK - 1) / ADAM_CHUNK;
    return blocks;
}

// workspace: one double per block of the table, then the finishing launch's sum
extern "C" size_t mkgnn_adamw_clip_workspace_bytes(const mkgnn_adamw_tensor* tensors, int32_t n_tensors) {
    const int64_t blocks = adam_table_blocks(tensors, n_tensors);
    return blocks ? sizeof(double) * (size_t)(blocks + 1) : 0;
}

// The clipped step of `Args` (AdamClipArgs, or AdamClipAvgArgs with the average's settings `v`).
template <class Args>
static int adam_step_clipped(const char* who, const mkgnn_adamw_tensor* tensors, int32_t n_tensors, const mkgnn_adamw_group* groups,
                             int32_t n_groups, const mkgnn_adamw_average* v, float max_norm, int32_t skip_nonfinite, void* workspace,
                             size_t workspace_bytes, float* stats, void* stream) {
    constexpr bool AVG = std::is_same_v<Args, AdamClipAvgArgs>;
    if (n_tensors < 0 || n_groups < 1 || n_groups > ADAM_MAX_GROUPS)
        return api_fail("%s: %d tensors, %d groups (1..%d groups)", who, n_tensors, n_groups, ADAM_MAX_GROUPS);
    if (!(max_norm > 0.f)) return api_fail("%s: max_norm %g (> 0, or +inf for the norm and the guard alone)", who, max_norm);
    if (!stats || (uintptr_t)stats % alignof(float)) return api_fail("%s: stats is null or misaligned", who);
    if (n_tensors == 0) return 0;
    if (!tensors || !groups) return api_fail("%s: null pointer", who);
    hipStream_t st = (hipStream_t)stream;
    Args a{};
    if constexpr (AVG) a.v = *v;
    if (int rc = adam_fill_groups(a, groups, n_groups, who)) return rc;
    int blocks = 0;
    for (int32_t first = 0; first < n_tensors; first += ADAM_MAX_TENSORS) {   // every tensor is looked at before anything is launched
        const int nt = n_tensors - first < ADAM_MAX_TENSORS ? n_tensors - first : ADAM_MAX_TENSORS;
        if (int rc = adam_fill_launch(a, tensors, first, nt, n_groups, who, &blocks)) return rc;
    }
    const int64_t total = adam_table_blocks(tensors, n_tensors);
    const size_t need = mkgnn_adamw_clip_workspace_bytes(tensors, n_tensors);
    if (!workspace || (uintptr_t)workspace % alignof(double) || workspace_bytes < need)
        return api_fail("%s: workspace is null, not 8-byte aligned, or %zu bytes where mkgnn_adamw_clip_workspace_bytes says %zu", who,
                        workspace_bytes, need);
    double* partial = (double*)workspace;
    int64_t at = 0;
    for (int32_t first = 0; first < n_tensors; first += ADAM_MAX_TENSORS) {
        const int nt = n_tensors - first < ADAM_MAX_TENSORS ? n_tensors - first : ADAM_MAX_TENSORS;
        adam_fill_launch(a, tensors, first, nt, n_groups, who, &blocks);
        adamw_sq_partial_kernel<<<blocks, 256, 0, st>>>(a, partial + at);
        at += blocks;
    }
    AdamClip& c = a.c;
    c = AdamClip{partial, (int32_t)total, max_norm, skip_nonfinite != 0, stats};
    if (total > ADAM_CLIP_PROLOGUE_BLOCKS) {
        adamw_sq_finish_kernel<<<1, 256, 0, st>>>(partial, total, partial + total);
        c.partial = partial + total;
        c.np = 1;
    }
    for (int32_t first = 0; first < n_tensors; first += ADAM_MAX_TENSORS) {
        const int nt = n_tensors - first < ADAM_MAX_TENSORS ? n_tensors - first : ADAM_MAX_TENSORS;
        adam_fill_launch(a, tensors, first, nt, n_groups, who, &blocks);
        adamw_step_kernel<Args, AVG><<<blocks, 256, 0, st>>>(a);
        c.stats = nullptr;                                   // block 0 of the first launch alone writes them
    }
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : api_hip_fail(who, e);
}

extern "C" int mkgnn_adamw_step_clipped(const mkgnn_adamw_tensor* tensors, int32_t n_tensors, const mkgnn_adamw_group* groups,
                                        int32_t n_groups, float max_norm, int32_t skip_nonfinite, void* workspace,
                                        size_t workspace_bytes, float* stats, void* stream) {
    return adam_step_clipped<AdamClipArgs>("mkgnn_adamw_step_clipped", tensors, n_tensors, groups, n_groups, nullptr, max_norm,
                                           skip_nonfinite, workspace, workspace_bytes, stats, stream);
}

extern "C" int64_t mkgnn_adamw_average_floats(int64_t numel) {
    return numel < 1 ? 0 : numel + 1 + (numel + ADAM_CHUNK - 1) / ADAM_CHUNK;
}

extern "C" int mkgnn_adamw_step_averaged(const mkgnn_adamw_tensor* tensors, int32_t n_tensors, const mkgnn_adamw_group* groups,
                                         int32_t n_groups, const mkgnn_adamw_average* avg, float max_norm, int32_t skip_nonfinite,
                                         void* workspace, size_t workspace_bytes, float* stats, void* stream) {
    const char* who = "mkgnn_adamw_step_averaged";
    if (!avg) return api_fail("%s: null average settings", who);
    if (avg->mode != MKGNN_ADAMW_AVERAGE_EMA && avg->mode != MKGNN_ADAMW_AVERAGE_MEAN)
        return api_fail("%s: unknown average mode %d", who, avg->mode);
    if (!(avg->decay >= 0.f && avg->decay < 1.f)) return api_fail("%s: average decay %g (0 <= decay < 1)", who, avg->decay);
    if (avg->start < 0) return api_fail("%s: average start %d (>= 0)", who, avg->start);
    if (max_norm == INFINITY && !skip_nonfinite && !stats)
        return adam_step<AdamAvgArgs>(who, tensors, n_tensors, groups, n_groups, avg, stream);
    return adam_step_clipped<AdamClipAvgArgs>(who, tensors, n_tensors, groups, n_groups, avg, max_norm, skip_nonfinite, workspace,
                                              workspace_bytes, stats, stream);
}
