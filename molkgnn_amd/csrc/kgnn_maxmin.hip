// MaxMin picking: the farthest-first traversal of stored embeddings (mkgnn_maxmin_pick) -- k rows that are as different from each
// other as possible, the similarity at which each was taken, and the pick every other row lies nearest to.
//
//     S[i, p] = the float32 value mkgnn_embed_cosine writes for row i as the ROW and row p as the QUERY, BIT FOR BIT:
//     (dot * inv(e_i)) * inv(e_p).  cur[i] is the largest similarity of row i to the selection so far (its start value, or -inf,
//     before anything nearer turns up).  Per round the candidate with the SMALLEST cur (-0.0 == +0.0, then the lower row) becomes
//     the next pick while cur < stop_sim, and every other valid row meets it: a strictly larger similarity replaces cur and the
//     leader.  molkgnn_amd/screening.py::maxmin_pick_reference is the definition.
//
// THE BITS come from what exists (kgnn_cosine.h): half_wave_row_sumsq and inv_clamped_norm for the norms, S[i, i] formed as
// kgnn_diverse.hip's init_kernel forms it, half_wave_dot (one half-wave per row, the grid-wide pass: coalesced rows) or mc_dot (one
// thread per row, the row in registers: the one-workgroup form) for the products -- the same bits either way.  Nothing in this file
// may be contracted.  THE ARG-MIN compares integers: the ascending key of the float (mm_key) in the high word, the row in the low
// word of one unsigned 64-bit value; a row that is no candidate carries MM_NO_KEY, above every float's key.
//
// THE LAUNCHES (all on the caller's stream, capturable, no atomics, no host round trip, no state between calls; the launch boundary
// is the only thing that orders workgroups against each other):
//   maxmin_init_kernel    MM_ROWS rows per block, one half-wave per row at a time: inv[i], self[i] = S[i, i], the row's flags (valid,
//                         excluded), cur (kept in leader_sim: for a valid row the two are the same value at the end) and leader = -1;
//                         picks = -1, pick_sim = NaN, *n_picks = 0, the "done" word = 0; the block's first partial arg-min
//   n_rows <= MM_TILE     maxmin_tile_kernel: ONE workgroup, one thread per row, the row, cur and leader in registers.  Per round: a
//                         wave reduction on the key, the waves' winners through LDS, the stop rule on the decoded key (uniform); the
//                         winner stages its raw row and inverse norm in LDS and appends itself; behind a barrier every other valid
//                         row evaluates S[j, pick] from broadcast reads and keeps the larger
//   beyond                k_max rounds of two launches.  maxmin_select_kernel (ONE workgroup) reduces the blocks' partial arg-mins,
//                         applies the stop rule, appends the pick and stages its raw row and inverse norm in the workspace -- or
//                         raises "done", after which every remaining launch returns at once.  maxmin_update_kernel (grid-wide,
//                         MM_ROWS rows per block; its threads per block depend on the grid -- the bits do not): every row meets
//                         the staged pick in one pass over emb, and the block writes its new partial arg-min over the rows that
//                         are still candidates
// The result is a function of emb, start_sim, stop_sim and k_max alone: not of MM_ROWS, MM_TILE, the stride or which form ran.
#include <hip/hip_runtime.h>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include "kgnn_common.h"

#include "kgnn_launch.h"
#include "kgnn_cosine.h"
#include "../../include/molkgnn_hip.h"

#pragma clang fp contract(off)

namespace mkgnn {
namespace {

constexpr int MM_MAX_H = 64;
constexpr int MM_TILE = 1024;             // rows (= threads) of the one-workgroup form.  Mirrored by _lib.MAXMIN_TILE
constexpr int MM_ROWS = 256;              // rows per block of the init (= its threads) and update launches.  Mirrored by _lib.MAXMIN_ROWS
// threads per block of the update launch: MM_ROWS (a half-wave walks 32 rows) once that grid fills the chip's wave slots -- 8 such
// blocks on each of 256 compute units --, MM_UPDATE_WIDE (32 half-waves of 8 rows: more waves, shorter chains) below that
constexpr int MM_UPDATE_WIDE = 1024, MM_UPDATE_WIDE_BELOW = 2048;
constexpr int MM_SELECT = 1024;           // threads of the select launch: at most 2^20 / MM_ROWS = 4 096 partials, four per thread
constexpr int MM_STAGE = 68;              // floats of the staged pick: its raw row zero padded to 64 columns, its inverse norm, 3 spare
constexpr int MM_CTL = 4;                 // control words: [0] done, [1] the staged pick's row, 2 spare
constexpr int MM_VALID = 1, MM_EXCLUDED = 2, MM_PICKED = 4;          // a row's flags
constexpr uint32_t MM_NO_KEY = 0xFFFFFFFFu;                          // (above every float's key: +inf's has 23 zero bits)
constexpr uint64_t MM_NONE = 0xFFFFFFFFFFFFFFFFull;

// the float as an unsigned key of the same order, smaller = earlier, -0.0 as +0.0 (never called with a NaN: a candidate's cur is a
// start value that is not NaN or a similarity that is not NaN); and the float a key stands for
__device__ __forceinline__ uint32_t mm_key(float v) {
    const uint32_t bits = __float_as_uint(v);
    const uint32_t b = bits == 0x80000000u ? 0u : bits;
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float mm_unkey(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k); }

__device__ __forceinline__ uint64_t mm_entry(uint32_t key, int row) { return ((uint64_t)key << 32) | (uint32_t)row; }

// the smallest entry of the wave, in every lane
__device__ __forceinline__ uint64_t wave_min_entry(uint64_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, o, 64);
        const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), o, 64);
        const uint64_t other = ((uint64_t)hi << 32) | lo;
        v = other < v ? other : v;
    }
    return v;
}

// the smallest entry of a block of NW waves, in every thread (slot: NW words of LDS; one barrier inside, the caller separates two
// calls by one of its own)
template <int NW>
__device__ __forceinline__ uint64_t block_min_entry(uint64_t v, unsigned long long* slot, int lane, int w) {
    v = wave_min_entry(v);
    if (lane == 0) slot[w] = v;
    __syncthreads();
    uint64_t best = slot[0];
#pragma unroll
    for (int u = 1; u < NW; ++u) {
        const uint64_t other = slot[u];
        best = other < best ? other : best;
    }
    return best;
}

__global__ void __launch_bounds__(MM_ROWS) maxmin_init_kernel(const float* __restrict__ emb, int64_t es, int n, int H, int k_max,
                                                              const float* __restrict__ start_sim, float* __restrict__ inv,
                                                              float* __restrict__ self, int32_t* __restrict__ state,
                                                              uint32_t* __restrict__ pkey, int32_t* __restrict__ prow,
                                                              int32_t* __restrict__ ctl, int32_t* __restrict__ picks,
                                                              float* __restrict__ pick_sim, int32_t* __restrict__ n_picks,
                                                              int32_t* __restrict__ leader, float* __restrict__ leader_sim) {
    __shared__ unsigned long long slot[MM_ROWS / 64];
    const int t = threadIdx.x, h = t & 31, lane = t & 63;
    const int base = blockIdx.x * MM_ROWS + (t >> 5) * 32;        // (n <= 2^20: every index fits an int)
    float mine = 0.f;
#pragma unroll 4
    for (int r = 0; r < 32; ++r) {                                // the half-wave's 32 rows, one at a time; lane r keeps row r's sum
        const int j = base + r, jc = j < n ? j : n - 1;           // (clamped: every lane of a half-wave takes part in the tree)
        const float s = half_wave_row_sumsq(emb + (int64_t)jc * es, h, H);
        if (h == r) mine = s;
    }
    const int j = base + h;
    uint32_t key = MM_NO_KEY;
    if (j < n) {
        const float ie = inv_clamped_norm(mine);
        const float own = __fmul_rn(__fmul_rn(mine + 0.f, ie), ie);      // embed_cosine_kernel's (dot + 0.0) * inv(e) * inv(q), e == q
        const float start = start_sim ? start_sim[j] : -INFINITY;
        const bool valid = own == own, excluded = valid && start != start;
        inv[j] = ie;
        self[j] = own;
        state[j] = (valid ? MM_VALID : 0) | (excluded ? MM_EXCLUDED : 0);
        leader[j] = -1;
        leader_sim[j] = valid ? start : __int_as_float(0x7fc00000);
        if (valid && !excluded) key = mm_key(start);
        if (j < k_max) {
            picks[j] = -1;
            pick_sim[j] = __int_as_float(0x7fc00000);
        }
        if (j == 0) {
            ctl[0] = 0;
            ctl[1] = 0;
            *n_picks = 0;
        }
    }
    const uint64_t best = block_min_entry<MM_ROWS / 64>(mm_entry(key, j), slot, lane, t >> 6);
    if (t == 0) {
        pkey[blockIdx.x] = (uint32_t)(best >> 32);
        prow[blockIdx.x] = (int32_t)(uint32_t)best;
    }
}

template <int W>
__global__ void __launch_bounds__(MM_TILE) maxmin_tile_kernel(const float* __restrict__ emb, int64_t es, int n, int H, float stop_sim,
                                                              int k_max, const float* __restrict__ inv,
                                                              const float* __restrict__ self, const int32_t* __restrict__ state,
                                                              int32_t* __restrict__ picks, float* __restrict__ pick_sim,
                                                              int32_t* __restrict__ n_picks, int32_t* __restrict__ leader,
                                                              float* __restrict__ leader_sim) {
    constexpr int NW = MM_TILE / 64;
    __shared__ __attribute__((aligned(16))) float srow[W];       // the current pick: raw values, zero padded
    __shared__ float sinv;
    __shared__ unsigned long long slot[NW];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int ic = t < n ? t : n - 1;
    float e[W];
#pragma unroll
    for (int j = 0; j < W; ++j) e[j] = j < H ? emb[(int64_t)ic * es + j] : 0.f;
    const float ie = inv[ic], mine = self[ic];
    const int st = t < n ? state[ic] : 0;
    const bool valid = (st & MM_VALID) != 0;
    bool candidate = valid && !(st & MM_EXCLUDED), picked = false;
    float cur = leader_sim[ic];                                  // (the init launch left the start value there)
    int lead = -1;
    int count = 0;
    for (; count < k_max; ++count) {
        const uint64_t best = block_min_entry<NW>(mm_entry(candidate ? mm_key(cur) : MM_NO_KEY, t), slot, lane, w);
        const uint32_t key = (uint32_t)(best >> 32);
        if (key == MM_NO_KEY || !(mm_unkey(key) < stop_sim)) break;      // (uniform: no candidate left, or all within stop_sim)
        const int first = (int)(uint32_t)best;
        if (t == first) {                                        // the next pick: one thread, plain stores
#pragma unroll
            for (int j = 0; j < W; ++j) srow[j] = e[j];
            sinv = ie;
            picks[count] = t;
            pick_sim[count] = cur;
            lead = t;
            cur = mine;
            candidate = false;
            picked = true;
        }
        __syncthreads();                                         // (also: every thread has read this round's slots)
        if (valid && !picked) {                                  // (no barrier inside)
            const float s = (mc_dot<W>(e, srow) * ie) * sinv;
            if (s == s && (cur != cur || s > cur)) {             // (strict: among equally near picks the earlier one leads)
                cur = s;
                lead = first;
            }
        }
        // (the next round's first barrier, inside block_min_entry, lies between these reads of srow and its next writer)
    }
    if (valid) {
        leader[t] = lead;
        leader_sim[t] = cur;
    }
    if (t == 0) *n_picks = count;
}

__global__ void __launch_bounds__(MM_SELECT) maxmin_select_kernel(const float* __restrict__ emb, int64_t es, int n, int H,
                                                                  float stop_sim, int round, int n_blocks,
                                                                  const float* __restrict__ inv, const float* __restrict__ self,
                                                                  int32_t* __restrict__ state, const uint32_t* __restrict__ pkey,
                                                                  const int32_t* __restrict__ prow, float* __restrict__ stage,
                                                                  int32_t* __restrict__ ctl, int32_t* __restrict__ picks,
                                                                  float* __restrict__ pick_sim, int32_t* __restrict__ n_picks,
                                                                  int32_t* __restrict__ leader, float* __restrict__ leader_sim) {
    __shared__ unsigned long long slot[MM_SELECT / 64];
    if (__builtin_amdgcn_readfirstlane(ctl[0]) != 0) return;     // done in an earlier round
    const int t = threadIdx.x;
    uint64_t mine = MM_NONE;
    for (int b = t; b < n_blocks; b += MM_SELECT) {
        const uint64_t other = mm_entry(pkey[b], prow[b]);
        mine = other < mine ? other : mine;
    }
    const uint64_t best = block_min_entry<MM_SELECT / 64>(mine, slot, t & 63, t >> 6);
    const uint32_t key = (uint32_t)(best >> 32);
    const int row = min(max((int)(uint32_t)best, 0), n - 1);
    const float cur = leader_sim[row];                           // (every thread, the same address: the candidate's own bits)
    const bool stop = key == MM_NO_KEY || !(cur < stop_sim);     // no candidate left, or every one already within stop_sim
    __syncthreads();                                             // (cur is read by every thread before one of them replaces it)
    if (stop) {
        if (t == 0) ctl[0] = 1;
        return;
    }
    if (t < 64) stage[t] = t < H ? emb[(int64_t)row * es + t] : 0.f;
    if (t == 0) {
        stage[64] = inv[row];
        ctl[1] = row;
        picks[round] = row;
        pick_sim[round] = cur;
        leader[row] = row;
        leader_sim[row] = self[row];
        state[row] |= MM_PICKED;
        *n_picks = round + 1;
    }
}

template <int THREADS>
__global__ void __launch_bounds__(THREADS) maxmin_update_kernel(const float* __restrict__ emb, int64_t es, int n, int H,
                                                                const float* __restrict__ inv, const int32_t* __restrict__ state,
                                                                const float* __restrict__ stage, const int32_t* __restrict__ ctl,
                                                                uint32_t* __restrict__ pkey, int32_t* __restrict__ prow,
                                                                int32_t* __restrict__ leader, float* __restrict__ leader_sim) {
    constexpr int PER = MM_ROWS / (THREADS / 32);                // rows per half-wave: 8 (all loads in flight together) or 32
    __shared__ float q[64];                                      // the staged pick: raw values, zero padded
    __shared__ float dots[MM_ROWS];
    __shared__ unsigned long long slot[THREADS / 64];
    if (__builtin_amdgcn_readfirstlane(ctl[0]) != 0) return;     // done: nothing was staged
    const int t = threadIdx.x, h = t & 31, g = t >> 5;
    const int pick = min(max(__builtin_amdgcn_readfirstlane(ctl[1]), 0), n - 1);
    if (t < 64) q[t] = stage[t];
    const float sinv = stage[64];
    __syncthreads();
    const int base = blockIdx.x * MM_ROWS + g * PER;
    float mine = 0.f;
#pragma unroll 8
    for (int r = 0; r < PER; ++r) {                               // the half-wave's rows, one at a time; lane r keeps row r's dot
        const int j = base + r, jc = j < n ? j : n - 1;           // (clamped: every lane of a half-wave takes part in the tree)
        float e0, e1;
        half_wave_load(emb + (int64_t)jc * es, h, H, e0, e1);
        const float d = half_wave_dot(e0, e1, q, h, H);
        if (h == r) mine = d;
    }
    if (h < PER) dots[g * PER + h] = mine;
    __syncthreads();
    const int j = blockIdx.x * MM_ROWS + t;                       // thread t < MM_ROWS: the block's row t
    uint32_t key = MM_NO_KEY;
    if (t < MM_ROWS && j < n) {
        const int st = state[j];
        if ((st & MM_VALID) && !(st & MM_PICKED)) {
            const float s = __fmul_rn(__fmul_rn(dots[t], inv[j]), sinv);
            float cur = leader_sim[j];
            if (s == s && (cur != cur || s > cur)) {             // (strict: among equally near picks the earlier one leads)
                cur = s;
                leader_sim[j] = s;
                leader[j] = pick;
            }
            if (!(st & MM_EXCLUDED)) key = mm_key(cur);
        }
    }
    const uint64_t best = block_min_entry<THREADS / 64>(mm_entry(key, j), slot, t & 63, t >> 6);
    if (t == 0) {
        pkey[blockIdx.x] = (uint32_t)(best >> 32);
        prow[blockIdx.x] = (int32_t)(uint32_t)best;
    }
}

// [inverse norms: n floats, padded to 4][self similarities: the same][flags: the same, int32][partial keys: one per MM_ROWS rows,
// padded to 4][partial rows: the same][the staged pick: MM_STAGE floats][control words: MM_CTL]
inline size_t mm_row_words(int64_t n) { return (size_t)((n + 3) / 4 * 4); }
inline size_t mm_blocks(int64_t n) { return (size_t)((n + MM_ROWS - 1) / MM_ROWS); }
inline size_t mm_block_words(int64_t n) { return (mm_blocks(n) + 3) / 4 * 4; }
inline bool mm_sizes_ok(int64_t n) { return n >= 1 && n <= MKGNN_MAXMIN_MAX_ROWS; }

}  // namespace
}  // namespace mkgnn

using namespace mkgnn;

extern "C" size_t mkgnn_maxmin_pick_workspace_bytes(int64_t n_rows) {
    if (!mm_sizes_ok(n_rows)) return 0;
    return sizeof(float) * (3 * mm_row_words(n_rows) + 2 * mm_block_words(n_rows) + MM_STAGE + MM_CTL);
}

extern "C" int mkgnn_maxmin_pick(const float* emb, int64_t emb_stride, int64_t n_rows, int32_t H, const float* start_sim,
                                 float stop_sim, int32_t k_max, int32_t* picks, float* pick_sim, int32_t* n_picks, int32_t* leader,
                                 float* leader_sim, void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "mkgnn_maxmin_pick";
    static_assert(MKGNN_MAXMIN_MAX_ROWS / MM_ROWS <= 4 * MM_SELECT, "the select launch reads four partials per thread at most");
    if (H < 1 || H > MM_MAX_H) return api_fail("%s: embedding width %d outside [1, %d]", who, (int)H, MM_MAX_H);
    if (n_rows < 0 || emb_stride < H) return api_fail("%s: bad shape", who);
    if (stop_sim != stop_sim) return api_fail("%s: stop_sim is NaN", who);
    if (n_rows == 0) return 0;
    if (!mm_sizes_ok(n_rows)) return api_fail("%s: %lld rows: at most %d in one call", who, (long long)n_rows, MKGNN_MAXMIN_MAX_ROWS);
    if (k_max < 1 || k_max > n_rows || k_max > MKGNN_MAXMIN_MAX_PICKS)
        return api_fail("%s: k_max = %d outside [1, %lld]", who, (int)k_max,
                        (long long)(n_rows < MKGNN_MAXMIN_MAX_PICKS ? n_rows : MKGNN_MAXMIN_MAX_PICKS));
    if (!emb || !picks || !pick_sim || !n_picks || !leader || !leader_sim || !workspace) return api_fail("%s: null pointer", who);
    const size_t need = mkgnn_maxmin_pick_workspace_bytes(n_rows);
    if (workspace_bytes < need) return api_fail("%s: workspace of %zu bytes, %zu needed", who, workspace_bytes, need);
    if (((uintptr_t)workspace & 3) != 0) return api_fail("%s: workspace not 4-byte aligned", who);
    // what the launches write -- the five outputs and the workspace -- must not overlap emb or start_sim, nor each other
    const size_t rows = (size_t)n_rows * 4;
    const Span rd[2] = {{emb, ((size_t)(n_rows - 1) * (size_t)emb_stride + (size_t)H) * 4}, {start_sim, start_sim ? rows : 0}};
    const Span wr[6] = {{picks, (size_t)k_max * 4}, {pick_sim, (size_t)k_max * 4}, {n_picks, 4}, {leader, rows}, {leader_sim, rows},
                        {workspace, need}};
    if (spans_disjoint(who, wr, 6, rd, 2,
                       "an output (picks, pick_sim, n_picks, leader, leader_sim) or the workspace aliases emb or start_sim",
                       "the outputs (picks, pick_sim, n_picks, leader, leader_sim) and the workspace alias each other"))
        return 1;
    const hipStream_t st = (hipStream_t)stream;
    const int n = (int)n_rows, nb = (int)mm_blocks(n_rows);
    float* inv = (float*)workspace;
    float* self = inv + mm_row_words(n_rows);
    int32_t* state = (int32_t*)(self + mm_row_words(n_rows));
    uint32_t* pkey = (uint32_t*)(state + mm_row_words(n_rows));
    int32_t* prow = (int32_t*)(pkey + mm_block_words(n_rows));
    float* stage = (float*)(prow + mm_block_words(n_rows));
    int32_t* ctl = (int32_t*)(stage + MM_STAGE);
    maxmin_init_kernel<<<(unsigned)nb, MM_ROWS, 0, st>>>(emb, emb_stride, n, H, k_max, start_sim, inv, self, state, pkey, prow, ctl,
                                                         picks, pick_sim, n_picks, leader, leader_sim);
    if (n <= MM_TILE) {
        if (H <= 32)
            maxmin_tile_kernel<32><<<1, MM_TILE, 0, st>>>(emb, emb_stride, n, H, stop_sim, k_max, inv, self, state, picks, pick_sim,
                                                          n_picks, leader, leader_sim);
        else
            maxmin_tile_kernel<64><<<1, MM_TILE, 0, st>>>(emb, emb_stride, n, H, stop_sim, k_max, inv, self, state, picks, pick_sim,
                                                          n_picks, leader, leader_sim);
    } else {
        for (int round = 0; round < k_max; ++round) {
            maxmin_select_kernel<<<1, MM_SELECT, 0, st>>>(emb, emb_stride, n, H, stop_sim, round, nb, inv, self, state, pkey, prow,
                                                          stage, ctl, picks, pick_sim, n_picks, leader, leader_sim);
            if (nb < MM_UPDATE_WIDE_BELOW)
                maxmin_update_kernel<MM_UPDATE_WIDE><<<(unsigned)nb, MM_UPDATE_WIDE, 0, st>>>(emb, emb_stride, n, H, inv, state, stage,
                                                                                              ctl, pkey, prow, leader, leader_sim);
            else
                maxmin_update_kernel<MM_ROWS><<<(unsigned)nb, MM_ROWS, 0, st>>>(emb, emb_stride, n, H, inv, state, stage, ctl, pkey,
                                                                                prow, leader, leader_sim);
        }
    }
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : api_hip_fail(who, e);
}
