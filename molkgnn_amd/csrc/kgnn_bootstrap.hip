// Bootstrap replicates of AUC and logAUC (mkgnn_bootstrap_roc): B resamples of a validation fold, none of which is ever sorted.
//
//     The scores are sorted ONCE by the caller.  Replicate b is a vector of integer multiplicities c[r] over the sorted rows --
//     row i of the caller's (or the class-major) order draws row j = lo + ((uint64) philox_word(seed, offset + b, i) * size >> 32)
//     and c[rank[j]] grows by one -- and one ordered walk over the weighted curve.  molkgnn_amd/evaluation.py::bootstrap_reference
//     is the definition; this file computes its integers exactly (two_u, n_pos), its AUC bit for bit (ONE float64 division of two
//     exactly representable integers) and its logAUC within the rounding of a float64 sum.
//
// THE WALK never looks ahead.  A tie group EXISTS in a replicate when one of its ranks was drawn.  The FIRST drawn rank of an
// existing group -- c[r] > 0 and nothing drawn since the group's start -- is its discoverer: the exclusive running sums there are
// the ROC point of the PREVIOUS existing group, (0, 0) for the first.  The discoverers' points, in rank order, and the totals
// (F, T) behind them are the curve S_0 = (0, 0), S_1, .., S_m.  Whoever brings S_g decides S_{g-1}: its term of two_u,
// gf * (2 * tps_before + gt), and whether roc_curve(drop_intermediate=True) keeps it -- S_1 and S_m always, an interior point iff
// its step differs from the next one.  Kept points are compacted once more and every consecutive pair is one clipped trapezoid
// in log10(FPR).
//
// THE LAUNCHES (all on the caller's stream, capturable, no host round trip, no cooperative launch, no flag a workgroup waits on;
// the launch boundary is the only thing that orders workgroups against each other; the only atomics are INTEGER adds):
//   n <= BS_LDS_MAX_N   bootstrap_lds_kernel, one workgroup per replicate: the multiplicities live in LDS (4 n bytes), the workgroup
//                       draws, counts and walks; no global scratch
//   beyond              passes over the replicates, as many at a time as the workspace holds (4 ceil4(n) bytes each): a launch that
//                       clears the pass's multiplicities and n_pos, bootstrap_draw_kernel (grid-wide: BS_DRAW_ROWS rows per block, one
//                       Philox block per thread, atomicAdd on uint32), bootstrap_walk_kernel (one workgroup per replicate)
// One text, walk_replicate, walks both forms in tiles of BS_TILE ranks.  A replicate's outputs are a function of (rank, y_sorted,
// group_last, n, split, seed, offset + b, lower, upper) alone: not of B, of where the call's replicates start, of how many a pass
// holds, of which form ran, or of the run.  The integers and the AUC do not depend on BS_TILE either; the log-area is summed tile
// by tile in rank order, each tile's trapezoids by one fixed tree (four per thread in curve order, a butterfly over the wave, the
// waves in order), so its last bits are a function of BS_TILE, a constant of this file.
//
// mkgnn_bootstrap_early is the same call with the early-recognition functionals of the curve -- the raw sums of average precision,
// of the enrichment factor's hits and of BEDROC's RIE -- taken in the same walk: walk_replicate is ONE text with a compile-time
// policy, the clear and draw kernels and the launch count are shared, and walk_replicate<RocOnly> is the walk described above.
//
// mkgnn_bootstrap_regression bootstraps the regression metrics (RMSE, MAE, R2, Pearson, Spearman, top-fraction recall) of rows with a
// prediction and a truth, BOTH sorted once: the same clear and draw kernels (the unstratified draw, scattered through the
// prediction ranks), then bootstrap_regression_walk_kernel, one workgroup per replicate, which needs prefix counts in two orders
// at once and so is another walk -- see the comment in front of it.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include "kgnn_common.h"

#include "kgnn_launch.h"
#include "kgnn_philox.h"
#include "../../include/molkgnn_hip.h"

#pragma clang fp contract(off)

namespace mkgnn {
namespace {

constexpr int BS_THREADS = 256;                      // threads of every workgroup of this file
constexpr int BS_PER = 4;                            // consecutive ranks (walk) or rows (draw: one Philox block) per thread
constexpr int BS_TILE = BS_THREADS * BS_PER;         // ranks per tile of the walk.  Mirrored by _lib.BOOTSTRAP_TILE
constexpr int BS_DRAW_ROWS = BS_THREADS * BS_PER;    // rows per block of the draw launch.  Mirrored by _lib.BOOTSTRAP_DRAW_ROWS
constexpr int BS_LDS_MAX_N = 8192;                   // the LDS form's largest n (32 KB of multiplicities).  Mirrored by _lib.BOOTSTRAP_LDS_MAX_N
constexpr int BS_NW = BS_THREADS / 64;
static_assert(BS_LDS_MAX_N % BS_PER == 0 && BS_TILE % 4 == 0, "rows of multiplicities are read four at a time");

struct Pt { int32_t f, t; };                         // a ROC point in counts: (false positives, true positives)

// the four words of the Philox block that holds elements e0 .. e0 + 3 (e0 a multiple of 4): philox_word's, one by one
__device__ __forceinline__ void philox_words4(uint64_t seed, uint64_t offset, uint64_t e0, uint32_t (&w)[4]) {
    uint32_t c0 = (uint32_t)(e0 >> 2), c1 = (uint32_t)(e0 >> 34), c2 = (uint32_t)offset, c3 = (uint32_t)(offset >> 32);
    uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    w[0] = c0; w[1] = c1; w[2] = c2; w[3] = c3;
}

// the rank that row i of replicate (seed, off) draws, or -1 for a rank outside [0, n) (a caller's mistake: never an address)
__device__ __forceinline__ int drawn_rank(uint32_t word, int i, int n, int split, const int32_t* __restrict__ rank) {
    const uint32_t lo = i < split ? 0u : (uint32_t)split, size = i < split ? (uint32_t)split : (uint32_t)(n - split);
    const uint32_t j = lo + (uint32_t)(((uint64_t)word * size) >> 32);           // (< lo + size <= n)
    const int r = rank[j];
    return (uint32_t)r < (uint32_t)n ? r : -1;
}

// ---- block-wide integer scans and sums (BS_THREADS threads; `slot` holds BS_NW words; each call begins with a barrier, so a
// caller may reuse the slots -- and anything else in LDS that was read before the call -- right away) ----
__device__ __forceinline__ uint64_t shfl_up64(uint64_t v, int o) {
    const uint32_t lo = (uint32_t)__shfl_up((int)(uint32_t)v, o, 64), hi = (uint32_t)__shfl_up((int)(uint32_t)(v >> 32), o, 64);
    return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ uint64_t shfl_xor64(uint64_t v, int o) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, o, 64), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), o, 64);
    return ((uint64_t)hi << 32) | lo;
}
// exclusive sum of v over the threads before this one; total: the block's sum, in every thread
__device__ __forceinline__ uint64_t block_excl_sum(uint64_t v, unsigned long long* slot, uint64_t& total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint64_t inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint64_t other = shfl_up64(inc, o);
        if (lane >= o) inc += other;
    }
    __syncthreads();
    if (lane == 63) slot[w] = inc;
    __syncthreads();
    uint64_t before = 0, all = 0;
#pragma unroll
    for (int u = 0; u < BS_NW; ++u) {
        const uint64_t s = slot[u];
        if (u < w) before += s;
        all += s;
    }
    total = all;
    return before + inc - v;
}
// exclusive maximum of v (>= -1) over the threads before this one, -1 without one; total: the block's maximum, in every thread
__device__ __forceinline__ int block_excl_max(int v, unsigned long long* slot, int& total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int other = __shfl_up(inc, o, 64);
        if (lane >= o) inc = max(inc, other);
    }
    int excl = __shfl_up(inc, 1, 64);
    if (lane == 0) excl = -1;
    __syncthreads();
    if (lane == 63) slot[w] = (unsigned long long)(long long)inc;
    __syncthreads();
    int all = -1;
#pragma unroll
    for (int u = 0; u < BS_NW; ++u) {
        const int s = (int)(long long)slot[u];
        if (u < w) excl = max(excl, s);
        all = max(all, s);
    }
    total = all;
    return excl;
}
// the block's sum of an integer (any order: exact) and of a double (ONE order: the wave's butterfly, then the waves in order)
__device__ __forceinline__ void block_sum(int64_t& iv, double& dv, unsigned long long* slot, double* dslot) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint64_t a = (uint64_t)iv;
    double d = dv;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        a += shfl_xor64(a, o);
        d += __longlong_as_double((long long)shfl_xor64((uint64_t)__double_as_longlong(d), o));
    }
    __syncthreads();
    if (lane == 0) {
        slot[w] = a;
        dslot[w] = d;
    }
    __syncthreads();
    uint64_t at = 0;
    double dt = 0.0;
#pragma unroll
    for (int u = 0; u < BS_NW; ++u) {
        at += slot[u];
        dt += dslot[u];
    }
    iv = (int64_t)at;
    dv = dt;
}

// ---- the curve ----
__device__ __forceinline__ bool step_differs(Pt a, Pt b, Pt c) { return (b.f - a.f) != (c.f - b.f) || (b.t - a.t) != (c.t - b.t); }
// the term of two_u of the group that leads from a to b: gf * (2 * tps_before + gt)
__device__ __forceinline__ int64_t two_u_term(Pt a, Pt b) { return (int64_t)(b.f - a.f) * (int64_t)(a.t + b.t); }
// the trapezoid in log10(FPR) of the segment a -> b, clipped to [lower, upper] in linear FPR; the TPR at a clip bound by np.interp's
// formula, slope * (x - xa) + ya.  Clip first, logarithm afterwards: log10(0) is never taken
__device__ __forceinline__ double log_trapezoid(Pt a, Pt b, double T, double F, double lower, double upper) {
    const double xa = (double)a.f / F, xb = (double)b.f / F, ya = (double)a.t / T, yb = (double)b.t / T;
    const double ca = fmin(fmax(xa, lower), upper), cb = fmin(fmax(xb, lower), upper);
    if (!(cb > ca)) return 0.0;
    const double slope = (yb - ya) / (xb - xa);                       // (cb > ca: xb > xa)
    const double yca = ca == xa ? ya : slope * (ca - xa) + ya, ycb = cb == xb ? yb : slope * (cb - xa) + ya;
    return (log10(cb) - log10(ca)) * (yca + ycb) / 2.0;
}

struct WalkLds {
    Pt pts[BS_TILE + 2];                 // [0], [1]: the curve's last two points so far; then this tile's discoveries
    Pt kept[BS_TILE + 1];                // [0]: the last kept point so far; then the points this tile decided to keep
    unsigned long long slot[BS_NW];
    double dslot[BS_NW];
};

// ---- the early-recognition functionals of the same curve (mkgnn_bootstrap_early) ----
// The walk's policy.  RocOnly adds nothing: walk_replicate<RocOnly> is mkgnn_bootstrap_roc's walk.  Early also takes every
// consecutive pair S_{g-1}, S_g BEFORE the thinning -- the tie group g with P = f + t of S_{g-1} drawn rows in front, gt = dt
// actives among its sg = dP rows, tps = t of S_g -- and forms from it (evaluation.early_reference is the definition)
//   ap      += (gt / T) * (tps / (P + sg))                                        (gt > 0)
//   rie[a]  += gt * exp(-(alpha (P + 1)) / N) * -expm1(-(alpha sg) / N) / -expm1(-alpha / N) / sg          (gt > 0)
//   hits[j]  = (tps - gt) + gt * (k_j - P) / sg     by the ONE thread whose group holds the cut, P < k_j <= P + sg
// with N = n.  A cut outside [1, n] and an alpha outside (0, 500] (or not finite) match no group and enter no sum: their
// entries are NaN.  ap and rie go through the log-area's tree: four per thread in curve order, the butterfly, the waves in order,
// tile by tile.
struct RocOnly {
    static constexpr bool early = false;
};
struct Early {
    static constexpr bool early = true;
    const int32_t* __restrict__ cuts;    // [J] device
    const double* __restrict__ alphas;   // [A] device
    int J, A;
    double* __restrict__ ap;             // this replicate's: one value, [J], [A]
    double* __restrict__ hits;
    double* __restrict__ rie;
    double (*eslot)[BS_NW];              // LDS: [1 + MKGNN_BOOTSTRAP_MAX_ALPHAS][BS_NW]
};
constexpr int BS_MAX_CUTS = MKGNN_BOOTSTRAP_MAX_CUTS, BS_MAX_ALPHAS = MKGNN_BOOTSTRAP_MAX_ALPHAS;

// what a thread knows of the call's cuts and alphas (the same values in every thread)
struct EarlyConsts {
    int cut[BS_MAX_CUTS];                // 0: no cut (matches no group)
    double alpha[BS_MAX_ALPHAS];         // 0: no alpha
    double den[BS_MAX_ALPHAS];           // -expm1(-alpha / N)
    double dN;
};
__device__ __forceinline__ void early_consts(const Early& P, int n, EarlyConsts& K) {
    K.dN = (double)n;
#pragma unroll
    for (int j = 0; j < BS_MAX_CUTS; ++j) {
        const int k = j < P.J ? P.cuts[j] : 0;
        K.cut[j] = k >= 1 && k <= n ? k : 0;
    }
#pragma unroll
    for (int a = 0; a < BS_MAX_ALPHAS; ++a) {
        const double al = a < P.A ? P.alphas[a] : 0.0;
        K.alpha[a] = al > 0.0 && al <= 500.0 ? al : 0.0;          // (a NaN fails both)
        K.den[a] = -expm1(-K.alpha[a] / K.dN);
    }
}
// the group that leads from a to b: its terms of ap and rie into acc[0], acc[1 + a]; its cuts' hits to memory
__device__ __forceinline__ void early_segment(const Early& P, const EarlyConsts& K, Pt a, Pt b, double dT,
                                              double (&acc)[1 + BS_MAX_ALPHAS]) {
    const int before = a.f + a.t, sg = b.f + b.t - before, gt = b.t - a.t;
#pragma unroll
    for (int j = 0; j < BS_MAX_CUTS; ++j) {
        const int k = K.cut[j];
        if (k > before && k <= before + sg)
            P.hits[j] = (double)a.t + (double)gt * (double)(k - before) / (double)sg;
    }
    if (gt > 0) {
        acc[0] += ((double)gt / dT) * ((double)b.t / (double)(before + sg));
#pragma unroll
        for (int q = 0; q < BS_MAX_ALPHAS; ++q) {
            const double al = K.alpha[q];
            if (al > 0.0)
                acc[1 + q] += (double)gt * exp(-(al * (double)(before + 1)) / K.dN) * (-expm1(-(al * (double)sg) / K.dN)) / K.den[q] /
                              (double)sg;
        }
    }
}
// the wave's butterfly of the 1 + A sums, in block_sum's order; lane 0 leaves them in eslot (read after block_sum's barriers)
__device__ __forceinline__ void early_wave_sums(const Early& P, const double (&acc)[1 + BS_MAX_ALPHAS]) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int q = 0; q < 1 + BS_MAX_ALPHAS; ++q) {
        if (q <= P.A) {                  // (uniform: the whole wave takes the butterfly or none of it does)
            double d = acc[q];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) d += __longlong_as_double((long long)shfl_xor64((uint64_t)__double_as_longlong(d), o));
            if (lane == 0) P.eslot[q][w] = d;
        }
    }
}

// One workgroup walks one replicate: cnt[r] its multiplicities (global memory or LDS), T its drawn actives.  Thread 0 writes the
// four outputs (and, under the Early policy, ap, rie and the NaN entries).
template <class Policy>
__device__ __forceinline__ void walk_replicate(const uint32_t* __restrict__ cnt, const uint8_t* __restrict__ ys,
                                               const uint8_t* __restrict__ glast, int n, int T, double lower, double upper,
                                               WalkLds& L, double* __restrict__ auc, double* __restrict__ logauc,
                                               int64_t* __restrict__ two_u, int32_t* __restrict__ n_pos, const Policy& policy) {
    const int t = threadIdx.x;
    const int F = n - T;
    const double dT = (double)T, dF = (double)F;
    EarlyConsts K;
    double early_sum[1 + BS_MAX_ALPHAS] = {};        // ap, rie[a] so far (every thread carries the same values)
    if constexpr (Policy::early) early_consts(policy, n, K);
    if (t < 2) L.pts[t] = Pt{0, 0};
    if (t == 0) L.kept[0] = Pt{0, 0};
    uint64_t cum = 0;                    // the running sums before this tile: drawn rows in the low word, drawn actives in the high
    int group_start_cum = 0;             // the drawn rows before the start of the group that is open at this tile's first rank
    int emitted = 0;                     // points of the curve so far (S_0 .. S_{emitted - 1})
    int64_t u2 = 0;
    double area = 0.0;                   // (every thread carries the same values)
    for (int base = 0; base < n; base += BS_TILE) {
        const int r0 = base + t * BS_PER;
        uint32_t c[BS_PER];
        bool act[BS_PER], start[BS_PER];
        if (r0 + BS_PER <= n) {          // (rows of multiplicities begin at a multiple of 4 words, r0 is one)
            const uint4 v = *(const uint4*)(cnt + r0);
            c[0] = v.x; c[1] = v.y; c[2] = v.z; c[3] = v.w;
        } else {
#pragma unroll
            for (int k = 0; k < BS_PER; ++k) c[k] = r0 + k < n ? cnt[r0 + k] : 0u;
        }
        bool prev_last = r0 == 0 || (r0 - 1 < n && glast[r0 - 1] != 0);
#pragma unroll
        for (int k = 0; k < BS_PER; ++k) {
            const int r = r0 + k;
            act[k] = r < n && ys[r] != 0;
            start[k] = prev_last;
            prev_last = r < n && glast[r] != 0;
        }
        // running sums in front of every rank
        uint64_t pre[BS_PER], mine = 0;
#pragma unroll
        for (int k = 0; k < BS_PER; ++k) {
            pre[k] = mine;
            mine += (uint64_t)c[k] | ((uint64_t)(act[k] ? c[k] : 0u) << 32);
        }
        uint64_t tile_sum;
        const uint64_t before = cum + block_excl_sum(mine, L.slot, tile_sum);
        // the drawn rows in front of the start of every rank's group: the running maximum of the starts' own sums (they only grow)
        int gs[BS_PER], local = -1;
#pragma unroll
        for (int k = 0; k < BS_PER; ++k) {
            if (start[k]) local = (int)(uint32_t)(before + pre[k]);
            gs[k] = local;
        }
        int tile_max;
        const int open = max(block_excl_max(local, L.slot, tile_max), group_start_cum);
        // discoverers: drawn, and nothing drawn since the group's start
        bool disc[BS_PER];
        uint64_t n_disc = 0;
#pragma unroll
        for (int k = 0; k < BS_PER; ++k) {
            const int g = max(gs[k], open);
            disc[k] = c[k] > 0u && (int)(uint32_t)(before + pre[k]) == g;
            n_disc += disc[k] ? 1u : 0u;
        }
        uint64_t tile_disc;
        int at = 2 + (int)block_excl_sum(n_disc, L.slot, tile_disc);
#pragma unroll
        for (int k = 0; k < BS_PER; ++k) {
            if (disc[k]) {
                const uint64_t s = before + pre[k];
                const int all = (int)(uint32_t)s, tp = (int)(uint32_t)(s >> 32);
                L.pts[at++] = Pt{all - tp, tp};
            }
        }
        __syncthreads();
        // whoever brings S_g decides S_{g-1} (g >= 2): its term of two_u, and whether it is kept
        const int found = (int)tile_disc;
        Pt keep_pt[BS_PER];
        bool keep[BS_PER];
        uint64_t n_keep = 0;
        int64_t term = 0;
        double e4[1 + BS_MAX_ALPHAS] = {};
#pragma unroll
        for (int k = 0; k < BS_PER; ++k) {
            const int i = 2 + t * BS_PER + k, g = emitted + i - 2;
            keep[k] = false;
            if (i < 2 + found && g >= 2) {
                const Pt a = L.pts[i - 2], b = L.pts[i - 1], cpt = L.pts[i];
                term += two_u_term(a, b);
                if constexpr (Policy::early) early_segment(policy, K, a, b, dT, e4);
                keep[k] = g == 2 || step_differs(a, b, cpt);
                keep_pt[k] = b;
            }
            n_keep += keep[k] ? 1u : 0u;
        }
        uint64_t tile_keep;
        int kat = 1 + (int)block_excl_sum(n_keep, L.slot, tile_keep);
#pragma unroll
        for (int k = 0; k < BS_PER; ++k)
            if (keep[k]) L.kept[kat++] = keep_pt[k];
        __syncthreads();
        const int n_kept = (int)tile_keep;
        double a4 = 0.0;
#pragma unroll
        for (int k = 0; k < BS_PER; ++k) {
            const int j = 1 + t * BS_PER + k;
            if (j <= n_kept) a4 += log_trapezoid(L.kept[j - 1], L.kept[j], dT, dF, lower, upper);
        }
        const Pt tail0 = L.pts[found], tail1 = L.pts[found + 1], last_kept = L.kept[n_kept];
        if constexpr (Policy::early) early_wave_sums(policy, e4);   // (eslot was last read before the previous tile's closing barrier)
        block_sum(term, a4, L.slot, L.dslot);        // (its first barrier: every read of pts and kept above is done)
        if constexpr (Policy::early) {
#pragma unroll
            for (int q = 0; q < 1 + BS_MAX_ALPHAS; ++q) {
                if (q <= policy.A) {
                    double dt = 0.0;
#pragma unroll
                    for (int u = 0; u < BS_NW; ++u) dt += policy.eslot[q][u];
                    early_sum[q] += dt;
                }
            }
        }
        if (t == 0) {
            L.pts[0] = tail0;
            L.pts[1] = tail1;
            L.kept[0] = last_kept;
        }
        u2 += term;
        area += a4;
        emitted += found;
        cum += tile_sum;
        group_start_cum = max(group_start_cum, tile_max);
        __syncthreads();
    }
    if (t == 0) {
        // the totals end the curve: S_m = (F, T) decides S_{m-1} as any point does, and is itself kept
        const Pt a = L.pts[0], b = L.pts[1], end = Pt{F, T};
        Pt k = L.kept[0];
        if (emitted >= 2) {
            u2 += two_u_term(a, b);
            if (emitted == 2 || step_differs(a, b, end)) {
                area += log_trapezoid(k, b, dT, dF, lower, upper);
                k = b;
            }
        }
        u2 += two_u_term(b, end);
        area += log_trapezoid(k, end, dT, dF, lower, upper);
        const bool defined = T > 0 && F > 0;
        const double nan = __longlong_as_double(0x7ff8000000000000ll);
        if constexpr (Policy::early) {
            if (emitted >= 2) early_segment(policy, K, a, b, dT, early_sum);
            early_segment(policy, K, b, end, dT, early_sum);
            *policy.ap = early_sum[0];
#pragma unroll
            for (int q = 0; q < BS_MAX_ALPHAS; ++q)
                if (q < policy.A) policy.rie[q] = K.alpha[q] > 0.0 ? early_sum[1 + q] : nan;
#pragma unroll
            for (int j = 0; j < BS_MAX_CUTS; ++j)
                if (j < policy.J && K.cut[j] == 0) policy.hits[j] = nan;
        }
        *auc = defined ? (double)u2 / (double)(2ll * (int64_t)T * (int64_t)F) : nan;
        *logauc = defined ? area / (log10(upper) - log10(lower)) : nan;
        *two_u = u2;
        *n_pos = T;
    }
}

// the block's sum of a small integer, in every thread
__device__ __forceinline__ int block_count(int v, unsigned long long* slot) {
    uint64_t total;
    block_excl_sum((uint64_t)(uint32_t)v, slot, total);
    return (int)total;
}

// the LDS form's draw: replicate (seed, offset + b)'s multiplicities into cnt (LDS); returns its drawn actives, in every thread
__device__ __forceinline__ int draw_into_lds(const int32_t* __restrict__ rank, const uint8_t* __restrict__ ys, int n, int split,
                                             uint64_t seed, uint64_t offset, uint32_t* cnt, unsigned long long* slot) {
    const int t = threadIdx.x, b = blockIdx.x;
    for (int r = t; r < n; r += BS_THREADS) cnt[r] = 0u;
    __syncthreads();
    int actives = 0;
    for (int i0 = t * BS_PER; i0 < n; i0 += BS_THREADS * BS_PER) {
        uint32_t w[4];
        philox_words4(seed, offset + (uint64_t)b, (uint64_t)i0, w);
#pragma unroll
        for (int k = 0; k < BS_PER; ++k) {
            const int i = i0 + k;
            if (i < n) {
                const int r = drawn_rank(w[k], i, n, split, rank);
                if (r >= 0) {
                    atomicAdd(&cnt[r], 1u);
                    actives += ys[r] != 0 ? 1 : 0;
                }
            }
        }
    }
    const int T = block_count(actives, slot);        // (its barriers: every add to cnt is done before the walk reads)
    __syncthreads();
    return T;
}

__global__ void __launch_bounds__(BS_THREADS) bootstrap_lds_kernel(const int32_t* __restrict__ rank, const uint8_t* __restrict__ ys,
                                                                   const uint8_t* __restrict__ glast, int n, int split, uint64_t seed,
                                                                   uint64_t offset, double lower, double upper,
                                                                   double* __restrict__ auc, double* __restrict__ logauc,
                                                                   int64_t* __restrict__ two_u, int32_t* __restrict__ n_pos) {
    __shared__ __attribute__((aligned(16))) uint32_t cnt[BS_LDS_MAX_N];
    __shared__ WalkLds L;
    const int b = blockIdx.x;
    const int T = draw_into_lds(rank, ys, n, split, seed, offset, cnt, L.slot);
    walk_replicate(cnt, ys, glast, n, T, lower, upper, L, auc + b, logauc + b, two_u + b, n_pos + b, RocOnly{});
}

// the replicate's Early policy: block b's rows of the three outputs
__device__ __forceinline__ Early early_of(const int32_t* cuts, int J, const double* alphas, int A, double* ap, double* hits,
                                          double* rie, double (*eslot)[BS_NW], int b) {
    return Early{cuts, alphas, J, A, ap + b, hits + (size_t)b * (size_t)J, rie + (size_t)b * (size_t)A, eslot};
}

__global__ void __launch_bounds__(BS_THREADS) bootstrap_lds_early_kernel(
    const int32_t* __restrict__ rank, const uint8_t* __restrict__ ys, const uint8_t* __restrict__ glast, int n, int split, uint64_t seed,
    uint64_t offset, double lower, double upper, const int32_t* __restrict__ cuts, int J, const double* __restrict__ alphas, int A,
    double* __restrict__ auc, double* __restrict__ logauc, int64_t* __restrict__ two_u, int32_t* __restrict__ n_pos,
    double* __restrict__ ap, double* __restrict__ hits, double* __restrict__ rie) {
    __shared__ __attribute__((aligned(16))) uint32_t cnt[BS_LDS_MAX_N];
    __shared__ WalkLds L;
    __shared__ double eslot[1 + BS_MAX_ALPHAS][BS_NW];
    const int b = blockIdx.x;
    const int T = draw_into_lds(rank, ys, n, split, seed, offset, cnt, L.slot);
    walk_replicate(cnt, ys, glast, n, T, lower, upper, L, auc + b, logauc + b, two_u + b, n_pos + b,
                   early_of(cuts, J, alphas, A, ap, hits, rie, eslot, b));
}

// the pass's multiplicities (words16 chunks of four words) and drawn actives start at zero.  (A launch: a hipMemsetAsync of a few
// bytes was seen to leave its target uncleared when a captured graph is replayed -- see kgnn_components.hip)
__global__ void __launch_bounds__(BS_THREADS) bootstrap_clear_kernel(uint4* __restrict__ cnt, size_t words16, int32_t* __restrict__ n_pos,
                                                                     int nb) {
    const size_t i = (size_t)blockIdx.x * BS_THREADS + threadIdx.x;
    if (i < words16) cnt[i] = make_uint4(0u, 0u, 0u, 0u);
    if (i < (size_t)nb) n_pos[i] = 0;
}

// grid (row blocks, replicates of the pass); cnt and n_pos of the pass are zero at the start
__global__ void __launch_bounds__(BS_THREADS) bootstrap_draw_kernel(const int32_t* __restrict__ rank, const uint8_t* __restrict__ ys,
                                                                    int n, int split, size_t pitch, uint64_t seed, uint64_t offset,
                                                                    uint32_t* __restrict__ cnt, int32_t* __restrict__ n_pos) {
    __shared__ unsigned long long slot[BS_NW];
    const int b = blockIdx.y;
    uint32_t* const mine = cnt + (size_t)b * pitch;
    const int i0 = (int)blockIdx.x * BS_DRAW_ROWS + (int)threadIdx.x * BS_PER;     // (n <= 2^22: every index fits an int)
    int actives = 0;
    if (i0 < n) {
        uint32_t w[4];
        philox_words4(seed, offset + (uint64_t)b, (uint64_t)i0, w);
#pragma unroll
        for (int k = 0; k < BS_PER; ++k) {
            const int i = i0 + k;
            if (i < n) {
                const int r = drawn_rank(w[k], i, n, split, rank);
                if (r >= 0) {
                    atomicAdd(&mine[r], 1u);
                    actives += ys[r] != 0 ? 1 : 0;
                }
            }
        }
    }
    const int total = block_count(actives, slot);
    if (threadIdx.x == 0 && total > 0) atomicAdd(&n_pos[b], total);
}

__global__ void __launch_bounds__(BS_THREADS) bootstrap_walk_kernel(const uint32_t* __restrict__ cnt, size_t pitch,
                                                                    const uint8_t* __restrict__ ys, const uint8_t* __restrict__ glast,
                                                                    int n, double lower, double upper, double* __restrict__ auc,
                                                                    double* __restrict__ logauc, int64_t* __restrict__ two_u,
                                                                    int32_t* __restrict__ n_pos) {
    __shared__ WalkLds L;
    const int b = blockIdx.x;
    const int T = min(max(__builtin_amdgcn_readfirstlane(n_pos[b]), 0), n);
    __syncthreads();                                 // (every thread has read n_pos[b] before thread 0 writes it back)
    walk_replicate(cnt + (size_t)b * pitch, ys, glast, n, T, lower, upper, L, auc + b, logauc + b, two_u + b, n_pos + b, RocOnly{});
}

__global__ void __launch_bounds__(BS_THREADS) bootstrap_walk_early_kernel(
    const uint32_t* __restrict__ cnt, size_t pitch, const uint8_t* __restrict__ ys, const uint8_t* __restrict__ glast, int n,
    double lower, double upper, const int32_t* __restrict__ cuts, int J, const double* __restrict__ alphas, int A,
    double* __restrict__ auc, double* __restrict__ logauc, int64_t* __restrict__ two_u, int32_t* __restrict__ n_pos,
    double* __restrict__ ap, double* __restrict__ hits, double* __restrict__ rie) {
    __shared__ WalkLds L;
    __shared__ double eslot[1 + BS_MAX_ALPHAS][BS_NW];
    const int b = blockIdx.x;
    const int T = min(max(__builtin_amdgcn_readfirstlane(n_pos[b]), 0), n);
    __syncthreads();                                 // (every thread has read n_pos[b] before thread 0 writes it back)
    walk_replicate(cnt + (size_t)b * pitch, ys, glast, n, T, lower, upper, L, auc + b, logauc + b, two_u + b, n_pos + b,
                   early_of(cuts, J, alphas, A, ap, hits, rie, eslot, b));
}

// ---- the regression walk (mkgnn_bootstrap_regression) ----
// One workgroup per replicate, three sweeps over tiles of BS_TILE ranks with a carried prefix.  Cp starts as the replicate's
// multiplicities by PREDICTION rank (the clear and draw launches above) and becomes their inclusive prefix sums in place; Ct gets
// the prefix sums by TRUTH rank.  Both rows are ceil4(n) words, written and read by this workgroup alone: a barrier orders the
// sweeps.  evaluation.regression_reference_sorted is the definition.
//   sweep 1  prediction order: Cp, and the seven moment sums in float64 -- tiles in rank order, a tile's terms four per thread in
//            rank order, the wave's butterfly, the waves in order (the log-area's rule)
//   sweep 2  truth order: c = Cp[x] - Cp[x - 1] with x = cross[r], scanned into Ct
//   sweep 3  truth order: every drawn row gathers a, b and the copies in front of it in both orders; the 3 + J integer sums are
//            exact in any order, so a thread keeps its own until one reduction at the end
// Every index read from cross, first_* and last_* is compared against n before it is an address; a row with one out of range
// enters no sum.
constexpr int BS_REG_MOM = 7, BS_REG_RANK = 3, BS_REG_INT = BS_REG_RANK + BS_MAX_CUTS;

struct RegLds {
    unsigned long long slot[BS_NW];
    double mslot[2][BS_REG_MOM][BS_NW];              // by tile parity: written before a tile's scan, read behind it
    unsigned long long islot[BS_REG_INT][BS_NW];
};

__device__ __forceinline__ bool in_rows(int v, int n) { return (uint32_t)v < (uint32_t)n; }

__global__ void __launch_bounds__(BS_THREADS) bootstrap_regression_walk_kernel(
    uint32_t* cp_all, uint32_t* ct_all, size_t pitch, const int32_t* __restrict__ first_p, const int32_t* __restrict__ last_p,
    const int32_t* __restrict__ cross, const int32_t* __restrict__ first_t, const int32_t* __restrict__ last_t,
    const double* __restrict__ p_sorted, const double* __restrict__ t_by_prank, const double* __restrict__ centre,
    const int32_t* __restrict__ cuts, int J, int n, double* __restrict__ mom, int64_t* __restrict__ rank_sums,
    int64_t* __restrict__ hits, int32_t* __restrict__ n_drawn) {
    __shared__ RegLds L;
    const int t = threadIdx.x, lane = t & 63, w = t >> 6, b = blockIdx.x;
    uint32_t* const Cp = cp_all + (size_t)b * pitch;
    uint32_t* const Ct = ct_all + (size_t)b * pitch;
    const double cen_p = centre[0], cen_t = centre[1];
    // sweep 1
    double msum[BS_REG_MOM] = {};                    // (every thread carries the same values)
    uint32_t carry = 0;
    int parity = 0;
    for (int base = 0; base < n; base += BS_TILE, parity ^= 1) {
        const int r0 = base + t * BS_PER;
        uint32_t c[BS_PER] = {0u, 0u, 0u, 0u};
        if (r0 < n) {                                // (a row is ceil4(n) words, r0 a multiple of 4; the padding was cleared)
            const uint4 v = *(const uint4*)(Cp + r0);
            c[0] = v.x; c[1] = v.y; c[2] = v.z; c[3] = v.w;
        }
        double m4[BS_REG_MOM] = {};
#pragma unroll
        for (int k = 0; k < BS_PER; ++k) {
            // (the loads do not wait for c: a rank without a copy adds an exact 0.0, whatever its products are)
            const int r = min(r0 + k, n - 1);
            const bool live = r0 + k < n && c[k] > 0u;
            const double pv = p_sorted[r], tv = t_by_prank[r], dp = pv - cen_p, dt = tv - cen_t, e = pv - tv, cw = (double)c[k];
            m4[0] += live ? cw * dp : 0.0;
            m4[1] += live ? cw * dt : 0.0;
            m4[2] += live ? cw * (dp * dp) : 0.0;
            m4[3] += live ? cw * (dt * dt) : 0.0;
            m4[4] += live ? cw * (dp * dt) : 0.0;
            m4[5] += live ? cw * fabs(e) : 0.0;
            m4[6] += live ? cw * (e * e) : 0.0;
        }
#pragma unroll
        for (int q = 0; q < BS_REG_MOM; ++q) {
            double d = m4[q];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) d += __longlong_as_double((long long)shfl_xor64((uint64_t)__double_as_longlong(d), o));
            if (lane == 0) L.mslot[parity][q][w] = d;
        }
        uint64_t tile_sum;
        uint32_t run = carry + (uint32_t)block_excl_sum((uint64_t)c[0] + c[1] + c[2] + c[3], L.slot, tile_sum);
        if (r0 < n) {
            uint4 v;
            v.x = run += c[0]; v.y = run += c[1]; v.z = run += c[2]; v.w = run += c[3];
            *(uint4*)(Cp + r0) = v;
        }
#pragma unroll
        for (int q = 0; q < BS_REG_MOM; ++q) {
            double d = 0.0;
#pragma unroll
            for (int u = 0; u < BS_NW; ++u) d += L.mslot[parity][q][u];
            msum[q] += d;
        }
        carry += (uint32_t)tile_sum;
    }
    const int N = (int)carry;
    __syncthreads();                                 // (Cp is whole before anyone gathers from it)
    // sweep 2
    carry = 0;
    for (int base = 0; base < n; base += BS_TILE) {
        const int r0 = base + t * BS_PER;
        uint32_t c[BS_PER] = {0u, 0u, 0u, 0u};
        if (r0 < n) {                                // (no branch between the loads: a thread's four gathers are in flight together)
            int x[BS_PER];
#pragma unroll
            for (int k = 0; k < BS_PER; ++k) x[k] = cross[min(r0 + k, n - 1)];
#pragma unroll
            for (int k = 0; k < BS_PER; ++k) {
                const bool ok = r0 + k < n && in_rows(x[k], n);
                const int xs = ok ? x[k] : 0;
                const uint32_t hi = Cp[xs], lo = Cp[max(xs - 1, 0)];
                c[k] = ok ? hi - (xs > 0 ? lo : 0u) : 0u;
            }
        }
        uint64_t tile_sum;
        uint32_t run = carry + (uint32_t)block_excl_sum((uint64_t)c[0] + c[1] + c[2] + c[3], L.slot, tile_sum);
        if (r0 < n) {
            uint4 v;
            v.x = run += c[0]; v.y = run += c[1]; v.z = run += c[2]; v.w = run += c[3];
            *(uint4*)(Ct + r0) = v;
        }
        carry += (uint32_t)tile_sum;
    }
    __syncthreads();                                 // (Ct is whole)
    // sweep 3
    int cut[BS_MAX_CUTS];
#pragma unroll
    for (int j = 0; j < BS_MAX_CUTS; ++j) {
        const int k = j < J ? cuts[j] : 0;
        cut[j] = k >= 1 && k <= n ? k : 0;           // (0: no copy lies in front of it, the column's sum stays 0)
    }
    uint64_t acc[BS_REG_RANK] = {};
    uint32_t hit[BS_MAX_CUTS] = {};                  // (a column's sum is at most its cut, <= n: 32 bits hold a thread's share)
    for (int base = 0; base < n; base += BS_TILE) {
        const int r0 = base + t * BS_PER;
        if (r0 >= n) continue;
        // no branch between the loads: the gathers of a thread's four rows are in flight together, and a row that is not drawn
        // or has an index out of range reads rank 0 and counts with c = 0
        const uint4 v = *(const uint4*)(Ct + r0);
        const uint32_t incl[BS_PER] = {v.x, v.y, v.z, v.w};
        const uint32_t front = Ct[max(r0 - 1, 0)];
        int x[BS_PER], ft[BS_PER], lt[BS_PER], fp[BS_PER], lp[BS_PER];
        bool ok[BS_PER];
#pragma unroll
        for (int k = 0; k < BS_PER; ++k) {
            const int r = min(r0 + k, n - 1);
            x[k] = cross[r];
            ft[k] = first_t[r];
            lt[k] = last_t[r];
        }
#pragma unroll
        for (int k = 0; k < BS_PER; ++k) {
            ok[k] = r0 + k < n && in_rows(x[k], n) && in_rows(ft[k], n) && in_rows(lt[k], n);
            if (!ok[k]) x[k] = ft[k] = lt[k] = 0;
            fp[k] = first_p[x[k]];
            lp[k] = last_p[x[k]];
        }
        uint32_t cpx[BS_PER], cpf[BS_PER], cpl[BS_PER], ctf[BS_PER], ctl[BS_PER];
#pragma unroll
        for (int k = 0; k < BS_PER; ++k) {
            if (!in_rows(fp[k], n) || !in_rows(lp[k], n)) {
                ok[k] = false;
                fp[k] = lp[k] = 0;
            }
            cpx[k] = Cp[x[k]];
            cpf[k] = Cp[max(fp[k] - 1, 0)];
            cpl[k] = Cp[lp[k]];
            ctf[k] = Ct[max(ft[k] - 1, 0)];
            ctl[k] = Ct[lt[k]];
        }
#pragma unroll
        for (int k = 0; k < BS_PER; ++k) {
            const uint32_t before = k == 0 ? (r0 > 0 ? front : 0u) : incl[k - 1];
            const int c = ok[k] ? (int)(incl[k] - before) : 0;
            const int64_t a = (int64_t)(fp[k] > 0 ? cpf[k] : 0u) + (int64_t)cpl[k] - (int64_t)N;
            const int64_t bb = (int64_t)(ft[k] > 0 ? ctf[k] : 0u) + (int64_t)ctl[k] - (int64_t)N;
            const int64_t ca = (int64_t)c * a, cb = (int64_t)c * bb;
            acc[0] += (uint64_t)(ca * bb);
            acc[1] += (uint64_t)(ca * a);
            acc[2] += (uint64_t)(cb * bb);
            const int ep = (int)cpx[k] - c, et = (int)incl[k] - c;       // (the copies in front of the row's in the two orders)
#pragma unroll
            for (int j = 0; j < BS_MAX_CUTS; ++j)
                hit[j] += (uint32_t)min(min(max(cut[j] - ep, 0), c), min(max(cut[j] - et, 0), c));
        }
    }
    const auto wave_total = [&](uint64_t s, int q) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += shfl_xor64(s, o);
        if (lane == 0) L.islot[q][w] = s;
    };
#pragma unroll
    for (int q = 0; q < BS_REG_RANK; ++q) wave_total(acc[q], q);
#pragma unroll
    for (int j = 0; j < BS_MAX_CUTS; ++j)
        if (j < J) wave_total((uint64_t)hit[j], BS_REG_RANK + j);       // (uniform)
    __syncthreads();
    if (t == 0) {
#pragma unroll
        for (int q = 0; q < BS_REG_MOM; ++q) mom[(size_t)b * BS_REG_MOM + q] = msum[q];
#pragma unroll
        for (int q = 0; q < BS_REG_INT; ++q) {
            if (q < BS_REG_RANK + J) {
                uint64_t s = 0;
#pragma unroll
                for (int u = 0; u < BS_NW; ++u) s += L.islot[q][u];
                if (q < BS_REG_RANK)
                    rank_sums[(size_t)b * BS_REG_RANK + q] = (int64_t)s;
                else
                    hits[(size_t)b * (size_t)J + (q - BS_REG_RANK)] = cut[q - BS_REG_RANK] != 0 ? (int64_t)s : (int64_t)-1;
            }
        }
        n_drawn[b] = N;
    }
}

inline size_t bs_pitch(int64_t n) { return (size_t)((n + 3) / 4 * 4); }      // words of one replicate's multiplicities
inline bool bs_sizes_ok(int64_t n, int64_t reps) { return n >= 1 && n <= MKGNN_BOOTSTRAP_MAX_ROWS && reps >= 1 && reps <= MKGNN_BOOTSTRAP_MAX_REPLICATES; }

}  // namespace
}  // namespace mkgnn

using namespace mkgnn;

extern "C" size_t mkgnn_bootstrap_roc_workspace_bytes(int64_t n, int32_t replicates_per_pass) {
    if (!bs_sizes_ok(n, replicates_per_pass)) return 0;
    if (n <= BS_LDS_MAX_N) return 16;                // (the LDS form uses none; 0 stays the sign of a rejected size)
    return sizeof(uint32_t) * bs_pitch(n) * (size_t)replicates_per_pass;
}

namespace {
// mkgnn_bootstrap_early's additions to mkgnn_bootstrap_roc's arguments; null for the ROC-only call
struct EarlyCall {
    const int32_t* cuts;
    int32_t J;
    const double* alphas;
    int32_t A;
    double *ap, *hits, *rie;
};

// Both entries: every check, then the launches.  Only the walk differs between them.
int bootstrap_run(const char* who, const EarlyCall* e, const int32_t* rank, const uint8_t* y_sorted, const uint8_t* group_last, int64_t n,
                  int64_t split, int32_t B, uint64_t seed, uint64_t offset, double lower, double upper, double* auc, double* logauc,
                  int64_t* two_u, int32_t* n_pos, void* workspace, size_t workspace_bytes, void* stream) {
    static_assert(MKGNN_BOOTSTRAP_MAX_REPLICATES <= 65535, "the draw launch puts a pass's replicates on the grid's y axis");
    if (n < 1 || n > MKGNN_BOOTSTRAP_MAX_ROWS)
        return api_fail("%s: %lld rows outside [1, %d]", who, (long long)n, MKGNN_BOOTSTRAP_MAX_ROWS);
    if (B < 1 || B > MKGNN_BOOTSTRAP_MAX_REPLICATES)
        return api_fail("%s: %d replicates outside [1, %d]", who, (int)B, MKGNN_BOOTSTRAP_MAX_REPLICATES);
    if (split < 0 || split > n) return api_fail("%s: split = %lld outside [0, %lld]", who, (long long)split, (long long)n);
    if (!(lower > 0.0) || !(lower < upper) || !(upper <= 1.0))
        return api_fail("%s: FPR window (%g, %g): 0 < lower < upper <= 1 is required", who, lower, upper);
    if (!rank || !y_sorted || !group_last || !auc || !logauc || !two_u || !n_pos) return api_fail("%s: null pointer", who);
    if ((((uintptr_t)auc | (uintptr_t)logauc | (uintptr_t)two_u) & 7) != 0 || ((uintptr_t)n_pos & 3) != 0 || ((uintptr_t)rank & 3) != 0)
        return api_fail("%s: misaligned rank or output", who);
    if (e) {
        if (e->J < 0 || e->J > MKGNN_BOOTSTRAP_MAX_CUTS)
            return api_fail("%s: %d cuts outside [0, %d]", who, (int)e->J, MKGNN_BOOTSTRAP_MAX_CUTS);
        if (e->A < 0 || e->A > MKGNN_BOOTSTRAP_MAX_ALPHAS)
            return api_fail("%s: %d alphas outside [0, %d]", who, (int)e->A, MKGNN_BOOTSTRAP_MAX_ALPHAS);
        if (!e->ap || (e->J > 0 && (!e->cuts || !e->hits)) || (e->A > 0 && (!e->alphas || !e->rie)))
            return api_fail("%s: null pointer (cuts, alphas, ap, hits or rie)", who);
        if ((((uintptr_t)e->ap | (uintptr_t)e->hits | (uintptr_t)e->rie | (uintptr_t)e->alphas) & 7) != 0 || ((uintptr_t)e->cuts & 3) != 0)
            return api_fail("%s: misaligned cuts, alphas, ap, hits or rie", who);
    }
    const bool lds = n <= BS_LDS_MAX_N;
    const size_t pitch = bs_pitch(n), per = sizeof(uint32_t) * pitch;
    int per_pass = B;
    if (!lds) {
        if (!workspace) return api_fail("%s: null workspace", who);
        if (((uintptr_t)workspace & 15) != 0) return api_fail("%s: workspace not 16-byte aligned", who);
        const size_t fit = workspace_bytes / per;
        if (fit < 1) return api_fail("%s: workspace of %zu bytes, %zu needed for one replicate", who, workspace_bytes, per);
        if (fit < (size_t)B) per_pass = (int)fit;
    }
    const size_t used = lds ? 0 : per * (size_t)per_pass;
    const size_t J = e ? (size_t)e->J : 0, A = e ? (size_t)e->A : 0;
    const Span rd[5] = {{rank, (size_t)n * 4}, {y_sorted, (size_t)n}, {group_last, (size_t)n}, {e ? e->cuts : nullptr, J * 4},
                        {e ? e->alphas : nullptr, A * 8}};
    const Span wr[8] = {{auc, (size_t)B * 8}, {logauc, (size_t)B * 8}, {two_u, (size_t)B * 8}, {n_pos, (size_t)B * 4}, {workspace, used},
                        {e ? e->ap : nullptr, e ? (size_t)B * 8 : 0}, {e ? e->hits : nullptr, (size_t)B * J * 8},
                        {e ? e->rie : nullptr, (size_t)B * A * 8}};
    if (e ? spans_disjoint(who, wr, 8, rd, 5,
                           "an output (auc, logauc, two_u, n_pos, ap, hits, rie) or the workspace aliases rank, y_sorted, group_last, "
                           "cuts or alphas",
                           "the outputs (auc, logauc, two_u, n_pos, ap, hits, rie) and the workspace alias each other")
          : spans_disjoint(who, wr, 5, rd, 3, "an output (auc, logauc, two_u, n_pos) or the workspace aliases rank, y_sorted or group_last",
                           "the outputs (auc, logauc, two_u, n_pos) and the workspace alias each other"))
        return 1;
    const hipStream_t st = (hipStream_t)stream;
    const int ni = (int)n, sp = (int)split;
    if (lds) {
        if (e)
            bootstrap_lds_early_kernel<<<(unsigned)B, BS_THREADS, 0, st>>>(rank, y_sorted, group_last, ni, sp, seed, offset, lower, upper,
                                                                           e->cuts, e->J, e->alphas, e->A, auc, logauc, two_u, n_pos,
                                                                           e->ap, e->hits, e->rie);
        else
            bootstrap_lds_kernel<<<(unsigned)B, BS_THREADS, 0, st>>>(rank, y_sorted, group_last, ni, sp, seed, offset, lower, upper, auc,
                                                                     logauc, two_u, n_pos);
    } else {
        uint32_t* const cnt = (uint32_t*)workspace;
        const unsigned row_blocks = (unsigned)((n + BS_DRAW_ROWS - 1) / BS_DRAW_ROWS);
        for (int b0 = 0; b0 < B; b0 += per_pass) {
            const int nb = B - b0 < per_pass ? B - b0 : per_pass;
            const size_t words16 = pitch / 4 * (size_t)nb;       // (>= nb: the same launch clears n_pos)
            bootstrap_clear_kernel<<<(unsigned)((words16 + BS_THREADS - 1) / BS_THREADS), BS_THREADS, 0, st>>>((uint4*)cnt, words16,
                                                                                                               n_pos + b0, nb);
            bootstrap_draw_kernel<<<dim3(row_blocks, (unsigned)nb), BS_THREADS, 0, st>>>(rank, y_sorted, ni, sp, pitch, seed,
                                                                                         offset + (uint64_t)b0, cnt, n_pos + b0);
            if (e)
                bootstrap_walk_early_kernel<<<(unsigned)nb, BS_THREADS, 0, st>>>(
                    cnt, pitch, y_sorted, group_last, ni, lower, upper, e->cuts, e->J, e->alphas, e->A, auc + b0, logauc + b0, two_u + b0,
                    n_pos + b0, e->ap + b0, e->hits + (size_t)b0 * J, e->rie + (size_t)b0 * A);
            else
                bootstrap_walk_kernel<<<(unsigned)nb, BS_THREADS, 0, st>>>(cnt, pitch, y_sorted, group_last, ni, lower, upper, auc + b0,
                                                                           logauc + b0, two_u + b0, n_pos + b0);
        }
    }
    const hipError_t err = hipGetLastError();
    return err == hipSuccess ? 0 : api_hip_fail(who, err);
}
}  // namespace

extern "C" int mkgnn_bootstrap_roc(const int32_t* rank, const uint8_t* y_sorted, const uint8_t* group_last, int64_t n, int64_t split,
                                   int32_t B, uint64_t seed, uint64_t offset, double lower, double upper, double* auc,
                                   double* logauc, int64_t* two_u, int32_t* n_pos, void* workspace, size_t workspace_bytes,
                                   void* stream) {
    return bootstrap_run("mkgnn_bootstrap_roc", nullptr, rank, y_sorted, group_last, n, split, B, seed, offset, lower, upper, auc, logauc,
                         two_u, n_pos, workspace, workspace_bytes, stream);
}

extern "C" int mkgnn_bootstrap_early(const int32_t* rank, const uint8_t* y_sorted, const uint8_t* group_last, int64_t n, int64_t split,
                                     int32_t B, uint64_t seed, uint64_t offset, double lower, double upper, const int32_t* cuts,
                                     int32_t J, const double* alphas, int32_t A, double* auc, double* logauc, int64_t* two_u,
                                     int32_t* n_pos, double* ap, double* hits, double* rie, void* workspace, size_t workspace_bytes,
                                     void* stream) {
    const EarlyCall e = {cuts, J, alphas, A, ap, hits, rie};
    return bootstrap_run("mkgnn_bootstrap_early", &e, rank, y_sorted, group_last, n, split, B, seed, offset, lower, upper, auc, logauc,
                         two_u, n_pos, workspace, workspace_bytes, stream);
}

extern "C" size_t mkgnn_bootstrap_regression_workspace_bytes(int64_t n, int32_t replicates_per_pass) {
    if (n < 1 || n > MKGNN_BOOTSTRAP_REG_MAX_ROWS || replicates_per_pass < 1 || replicates_per_pass > MKGNN_BOOTSTRAP_MAX_REPLICATES)
        return 0;
    return 2 * sizeof(uint32_t) * bs_pitch(n) * (size_t)replicates_per_pass;
}

extern "C" int mkgnn_bootstrap_regression(const int32_t* rank_p, const int32_t* first_p, const int32_t* last_p, const int32_t* cross,
                                          const int32_t* first_t, const int32_t* last_t, const double* p_sorted,
                                          const double* t_by_prank, const double* centre, const int32_t* cuts, int32_t J, int64_t n,
                                          int32_t B, uint64_t seed, uint64_t offset, double* mom, int64_t* rank_sums, int64_t* hits,
                                          int32_t* n_drawn, void* workspace, size_t workspace_bytes, void* stream) {
    const char* const who = "mkgnn_bootstrap_regression";
    static_assert(MKGNN_BOOTSTRAP_REG_MAX_ROWS <= MKGNN_BOOTSTRAP_MAX_ROWS, "the draw launch is mkgnn_bootstrap_roc's");
    if (n < 1 || n > MKGNN_BOOTSTRAP_REG_MAX_ROWS)
        return api_fail("%s: %lld rows outside [1, %d]", who, (long long)n, MKGNN_BOOTSTRAP_REG_MAX_ROWS);
    if (B < 1 || B > MKGNN_BOOTSTRAP_MAX_REPLICATES)
        return api_fail("%s: %d replicates outside [1, %d]", who, (int)B, MKGNN_BOOTSTRAP_MAX_REPLICATES);
    if (J < 0 || J > MKGNN_BOOTSTRAP_MAX_CUTS) return api_fail("%s: %d cuts outside [0, %d]", who, (int)J, MKGNN_BOOTSTRAP_MAX_CUTS);
    if (!rank_p || !first_p || !last_p || !cross || !first_t || !last_t || !p_sorted || !t_by_prank || !centre || !mom || !rank_sums ||
        !n_drawn || (J > 0 && (!cuts || !hits)))
        return api_fail("%s: null pointer", who);
    if ((((uintptr_t)rank_p | (uintptr_t)first_p | (uintptr_t)last_p | (uintptr_t)cross | (uintptr_t)first_t | (uintptr_t)last_t |
          (uintptr_t)cuts | (uintptr_t)n_drawn) & 3) != 0 ||
        (((uintptr_t)p_sorted | (uintptr_t)t_by_prank | (uintptr_t)centre | (uintptr_t)mom | (uintptr_t)rank_sums | (uintptr_t)hits) & 7) != 0)
        return api_fail("%s: misaligned input or output", who);
    if (!workspace) return api_fail("%s: null workspace", who);
    if (((uintptr_t)workspace & 15) != 0) return api_fail("%s: workspace not 16-byte aligned", who);
    const size_t pitch = bs_pitch(n), per = 2 * sizeof(uint32_t) * pitch;
    const size_t fit = workspace_bytes / per;
    if (fit < 1) return api_fail("%s: workspace of %zu bytes, %zu needed for one replicate", who, workspace_bytes, per);
    const int per_pass = fit < (size_t)B ? (int)fit : (int)B;
    const size_t rows4 = (size_t)n * 4, rows8 = (size_t)n * 8, Jz = (size_t)J;
    const Span rd[10] = {{rank_p, rows4}, {first_p, rows4}, {last_p, rows4},     {cross, rows4}, {first_t, rows4},
                         {last_t, rows4}, {p_sorted, rows8}, {t_by_prank, rows8}, {centre, 16},   {cuts, Jz * 4}};
    const Span wr[5] = {{mom, (size_t)B * BS_REG_MOM * 8}, {rank_sums, (size_t)B * BS_REG_RANK * 8}, {hits, (size_t)B * Jz * 8},
                        {n_drawn, (size_t)B * 4}, {workspace, per * (size_t)per_pass}};
    if (spans_disjoint(who, wr, 5, rd, 10, "an output (mom, rank_sums, hits, n_drawn) or the workspace aliases an input",
                       "the outputs (mom, rank_sums, hits, n_drawn) and the workspace alias each other"))
        return 1;
    const hipStream_t st = (hipStream_t)stream;
    const int ni = (int)n;
    uint32_t* const cp = (uint32_t*)workspace;       // the pass's Cp rows, then its Ct rows
    uint32_t* const ct = cp + pitch * (size_t)per_pass;
    const unsigned row_blocks = (unsigned)((n + BS_DRAW_ROWS - 1) / BS_DRAW_ROWS);
    for (int b0 = 0; b0 < B; b0 += per_pass) {
        const int nb = B - b0 < per_pass ? B - b0 : per_pass;
        const size_t words16 = pitch / 4 * (size_t)nb;
        // the shared clear and draw: the draw's count of "actives" is not used -- the first n bytes of p_sorted stand in for its
        // labels and n_drawn for its counter, which the walk overwrites
        bootstrap_clear_kernel<<<(unsigned)((words16 + BS_THREADS - 1) / BS_THREADS), BS_THREADS, 0, st>>>((uint4*)cp, words16,
                                                                                                           n_drawn + b0, nb);
        bootstrap_draw_kernel<<<dim3(row_blocks, (unsigned)nb), BS_THREADS, 0, st>>>(rank_p, (const uint8_t*)p_sorted, ni, ni, pitch, seed,
                                                                                     offset + (uint64_t)b0, cp, n_drawn + b0);
        bootstrap_regression_walk_kernel<<<(unsigned)nb, BS_THREADS, 0, st>>>(
            cp, ct, pitch, first_p, last_p, cross, first_t, last_t, p_sorted, t_by_prank, centre, cuts, J, ni,
            mom + (size_t)b0 * BS_REG_MOM, rank_sums + (size_t)b0 * BS_REG_RANK, hits + (size_t)b0 * Jz, n_drawn + b0);
    }
    const hipError_t err = hipGetLastError();
    return err == hipSuccess ? 0 : api_hip_fail(who, err);
}
