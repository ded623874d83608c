// Diverse hits: leader clustering of a ranked list (mkgnn_diverse_pick) -- the best molecule of every chemical series among the
// top of a screen, and the series every other hit belongs to.
//
//     walk the rows of emb [n, H] in rank order; S[i, p] (p <= i) = the float32 value mkgnn_embed_cosine writes for row i as the
//     ROW and row p as the QUERY, BIT FOR BIT: (dot * inv(e_i)) * inv(e_p).  A row whose S[i, i] is NaN is never picked, never
//     covered and covers nothing.  Otherwise the FIRST pick p so far (in pick order) with S[i, p] > max_sim (strict; a NaN never
//     covers) is its leader; without one the row becomes a pick itself while fewer than k_max exist, and keeps (-1, NaN) after.
//
// THE BITS come from what exists: mc_dot and inv_clamped_norm (kgnn_cosine.h) are the text kgnn_max_cosine.hip compiles, the
// init launch runs half_wave_sumsq -- the function embed_cosine_kernel calls -- and forms S[i, i] from it the way that kernel
// does (for a row against itself the dot product IS the sum of squares: the same products, fmaf and tree).  Nothing in this file
// may be contracted.
//
// THE LAUNCHES (1 + 2 per tile of DV_TILE rows - 1; all on the caller's stream, capturable, no atomics, no host round trip, no
// state between calls).  The selection is sequential by definition; the tiling bounds what ONE workgroup does to DV_TILE rows at a
// time and gives everything behind a tile to the whole chip:
//   init_kernel           one half-wave per row: inv[i] = 1 / max(||e_i||, eps) and self[i] = S[i, i] -> workspace; leader = -1,
//                         leader_sim = NaN, picks = -1, the two counters and *n_picks = 0
//   diverse_tile_kernel   ONE workgroup, one thread per row of the tile, the row in registers.  Rows still undecided (leader ==
//                         -1, self not NaN) are ALIVE; the alive set is one ballot word per wave in LDS, each wave rewrites only its
//                         own word.  Per round every thread finds the first alive row in those words; that row is the next pick:
//                         it stages its raw values and its inverse norm in LDS and appends itself to picks[] (one thread, plain
//                         stores); behind a barrier every alive thread evaluates S[j, pick] from a broadcast read and, above
//                         max_sim, records its leader and dies.  The rounds end when no row is alive or k_max picks exist (the
//                         rest keep -1).  Thread 0 leaves [count before, count after] in the workspace and the count in *n_picks.
//   diverse_cover_kernel  grid-wide over the rows BEHIND the tile, one thread per row as in max_cosine_kernel: walks only the picks
//                         this tile added (the range is read from the two device counters; an empty range returns at once),
//                         gathered through picks[] into LDS tiles of DV_COVER_TILE rows; keeps the FIRST cover (selects, and
//                         the barriers outside them); a row decided earlier loads nothing and computes nothing, and a block
//                         whose rows are all decided leaves the walk.
// A covered row is never revisited and picks arrive in pick order, so "first covering pick" holds globally: a row of a later tile
// has met every earlier tile's picks, tile by tile in order, before its own tile's walk begins.  The result does not depend on
// DV_TILE.  Plain FP32 VALU: the bit contract forbids another summation order.
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

constexpr int DV_MAX_H = 64;
constexpr int DV_COVER_ROWS = 128;        // rows (= threads) per block of the cover launch: max_cosine_kernel's shape
constexpr int DV_COVER_TILE = 32;         // picks per LDS tile of the cover launch: 32 x 64 floats = 8 KB
// rows per tile, by the padded width: one thread per row with the row in registers, so the workgroup's size bounds the registers
// of a thread (1 024 threads: 128; 512: 256).  The compiler's resource report for gfx950 shows 72 registers at 32 columns and 112 at
// 64, without scratch, at 1 024 threads (and the same 112 at 512): both widths take the larger tile -- half the launches.  A width
// that spilled there would take 512.  Mirrored by _lib.diverse_tile(H)
template <int W> struct DvTile;
template <> struct DvTile<32> { static constexpr int value = 1024; };
template <> struct DvTile<64> { static constexpr int value = 1024; };

__global__ void __launch_bounds__(256) init_kernel(const float* __restrict__ emb, int64_t es, int n, int H, int k_max,
                                                   float* __restrict__ inv, float* __restrict__ self, int32_t* __restrict__ cnt,
                                                   int32_t* __restrict__ picks, int32_t* __restrict__ n_picks,
                                                   int32_t* __restrict__ leader, float* __restrict__ leader_sim) {
    const int h = threadIdx.x & 31;
    const int v = blockIdx.x * 8 + (threadIdx.x >> 5);           // (n <= 2^20: every index fits an int)
    const int vc = v < n ? v : n - 1;                             // (clamped: every lane of a half-wave takes part in the tree)
    const float s = half_wave_row_sumsq(emb + (int64_t)vc * es, h, H);
    if (h != 0 || v >= n) return;
    const float ie = inv_clamped_norm(s);
    inv[v] = ie;
    self[v] = __fmul_rn(__fmul_rn(s + 0.f, ie), ie);             // embed_cosine_kernel's (dot + 0.0) * inv(e) * inv(q), e == q
    leader[v] = -1;
    leader_sim[v] = __int_as_float(0x7fc00000);
    if (v < k_max) picks[v] = -1;
    if (v == 0) {
        cnt[0] = 0;
        cnt[1] = 0;
        *n_picks = 0;
    }
}

template <int W>
__global__ void __launch_bounds__(DvTile<W>::value) diverse_tile_kernel(const float* __restrict__ emb, int64_t es, int n, int H,
                                                                        int base, float max_sim, int k_max,
                                                                        const float* __restrict__ inv,
                                                                        const float* __restrict__ self, int32_t* __restrict__ cnt,
                                                                        int32_t* __restrict__ picks, int32_t* __restrict__ n_picks,
                                                                        int32_t* __restrict__ leader,
                                                                        float* __restrict__ leader_sim) {
    constexpr int TILE = DvTile<W>::value, NW = TILE / 64;
    __shared__ __attribute__((aligned(16))) float srow[W];       // the current pick: raw values, zero padded
    __shared__ float sinv;
    __shared__ unsigned long long alive_of[NW];                  // one ballot word per wave, written by that wave alone
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int i = base + t, ic = i < n ? i : n - 1;
    float e[W];
#pragma unroll
    for (int j = 0; j < W; ++j) e[j] = j < H ? emb[(int64_t)ic * es + j] : 0.f;
    const float ie = inv[ic], mine = self[ic];
    int lead = leader[ic];
    float lead_sim = 0.f;
    bool alive = i < n && lead == -1 && mine == mine;
    bool changed = false;
    const int before = min(max(__builtin_amdgcn_readfirstlane(cnt[1]), 0), k_max);
    int count = before;
    {
        const unsigned long long word = __ballot(alive);
        if (lane == 0) alive_of[w] = word;
    }
    int w0 = 0;                                                  // no wave below w0 holds an alive row: a row only ever dies
    for (;;) {
        __syncthreads();                                         // (every wave's word is written; the last pick's walk is over)
        // the first alive row, from the words: every lane reads the same address and the value goes to scalar registers, so the
        // scan is scalar code, the branches are uniform, and it starts at the last pick's wave (the picks arrive in order)
        int first = -1;
        for (int v = w0; v < NW; ++v) {
            const unsigned long long word = alive_of[v];
            const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)word);
            const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)(word >> 32));
            if (lo | hi) {
                first = v * 64 + (lo ? __ffs(lo) - 1 : 31 + __ffs(hi));
                w0 = v;
                break;
            }
        }
        if (first < 0 || count >= k_max) break;
        if (t == first) {                                        // the next pick: one thread, plain stores
#pragma unroll
            for (int j = 0; j < W; ++j) srow[j] = e[j];
            sinv = ie;
            picks[count] = i;
            lead = i;
            lead_sim = mine;
            alive = false;
            changed = true;
        }
        ++count;
        __syncthreads();
        if (alive) {                                             // (no barrier inside: a thread that is not alive just waits)
            const float s = (mc_dot<W>(e, srow) * ie) * sinv;
            if (s > max_sim) {                                   // (strict; false for a NaN)
                lead = base + first;
                lead_sim = s;
                alive = false;
                changed = true;
            }
        }
        const unsigned long long word = __ballot(alive);
        if (lane == 0) alive_of[w] = word;
    }
    if (changed) {
        leader[i] = lead;
        leader_sim[i] = lead_sim;
    }
    if (t == 0) {                                                // (every thread read cnt[1] before the loop's first barrier)
        cnt[0] = before;
        cnt[1] = count;
        *n_picks = count;
    }
}

template <int W>
__global__ void __launch_bounds__(DV_COVER_ROWS) diverse_cover_kernel(const float* __restrict__ emb, int64_t es, int n, int H,
                                                                      int first_row, float max_sim, int k_max,
                                                                      const float* __restrict__ inv,
                                                                      const float* __restrict__ self,
                                                                      const int32_t* __restrict__ cnt,
                                                                      const int32_t* __restrict__ picks,
                                                                      int32_t* __restrict__ leader,
                                                                      float* __restrict__ leader_sim) {
    __shared__ __attribute__((aligned(16))) float tile[DV_COVER_TILE * W];
    __shared__ float tinv[DV_COVER_TILE];
    __shared__ int tidx[DV_COVER_TILE];
    const int c0 = min(max(__builtin_amdgcn_readfirstlane(cnt[0]), 0), k_max);
    const int c1 = min(max(__builtin_amdgcn_readfirstlane(cnt[1]), c0), k_max);
    if (c0 == c1) return;                                        // the tile added no pick
    const int t = threadIdx.x;
    const int i = first_row + blockIdx.x * DV_COVER_ROWS + t, ic = i < n ? i : n - 1;
    const float mine = self[ic];
    bool open = i < n && leader[ic] == -1 && mine == mine;       // undecided, and able to be covered
    const bool was_open = open;
    float e[W];
#pragma unroll
    for (int j = 0; j < W; ++j) e[j] = (open && j < H) ? emb[(int64_t)ic * es + j] : 0.f;
    const float ie = inv[ic];
    int lead = -1;
    float lead_sim = 0.f;
    for (int r0 = c0; r0 < c1; r0 += DV_COVER_TILE) {
        const int m = min(DV_COVER_TILE, c1 - r0);
        if (!__syncthreads_or(open)) break;                      // (also: the previous tile has been walked by every wave)
        const auto pick = [=](int r) { return min(max(picks[r0 + r], 0), n - 1); };      // (slot r: a row of emb, through picks)
        stage_padded_tile<W, DV_COVER_ROWS>(tile, tinv, m, pick, emb, es, H, inv, t);
        if (t < m) tidx[t] = pick(t);
        __syncthreads();
        if (open) {                                              // (no barrier inside; within the walk selects keep the first)
            for (int r = 0; r < m; ++r) {
                const float s = (mc_dot<W>(e, tile + r * W) * ie) * tinv[r];
                const bool hit = open && s > max_sim;
                lead = hit ? tidx[r] : lead;
                lead_sim = hit ? s : lead_sim;
                open = open && !hit;
            }
        }
    }
    if (was_open && !open) {
        leader[i] = lead;
        leader_sim[i] = lead_sim;
    }
}

// [inverse norms: n floats, padded to 4][self similarities: the same][count before the tile, count after it, 2 spare ints]
inline size_t dv_row_floats(int64_t n) { return (size_t)((n + 3) / 4 * 4); }
inline bool dv_sizes_ok(int64_t n) { return n >= 1 && n <= MKGNN_DIVERSE_MAX_ROWS; }

template <int W>
void dv_launch(const float* emb, int64_t es, int n, int H, float max_sim, int k_max, const float* inv, const float* self,
               int32_t* cnt, int32_t* picks, int32_t* n_picks, int32_t* leader, float* leader_sim, hipStream_t st) {
    constexpr int TILE = DvTile<W>::value;
    for (int base = 0; base < n; base += TILE) {
        diverse_tile_kernel<W><<<1, TILE, 0, st>>>(emb, es, n, H, base, max_sim, k_max, inv, self, cnt, picks, n_picks, leader,
                                                   leader_sim);
        const int behind = n - (base + TILE);
        if (behind > 0)
            diverse_cover_kernel<W><<<(unsigned)((behind + DV_COVER_ROWS - 1) / DV_COVER_ROWS), DV_COVER_ROWS, 0, st>>>(
                emb, es, n, H, base + TILE, max_sim, k_max, inv, self, cnt, picks, leader, leader_sim);
    }
}

}  // namespace
}  // namespace mkgnn

using namespace mkgnn;

extern "C" size_t mkgnn_diverse_pick_workspace_bytes(int64_t n_rows) {
    if (!dv_sizes_ok(n_rows)) return 0;
    return sizeof(float) * (2 * dv_row_floats(n_rows) + 4);
}

extern "C" int mkgnn_diverse_pick(const float* emb, int64_t emb_stride, int64_t n_rows, int32_t H, float max_sim, int32_t k_max,
                                  int32_t* picks, int32_t* n_picks, int32_t* leader, float* leader_sim, void* workspace,
                                  size_t workspace_bytes, void* stream) {
    const char* who = "mkgnn_diverse_pick";
    if (H < 1 || H > DV_MAX_H) return api_fail("%s: embedding width %d outside [1, %d]", who, (int)H, DV_MAX_H);
    if (n_rows < 0 || emb_stride < H) return api_fail("%s: bad shape", who);
    if (!(std::fabs(max_sim) <= FLT_MAX)) return api_fail("%s: max_sim must be finite", who);
    if (n_rows == 0) return 0;
    if (!dv_sizes_ok(n_rows)) return api_fail("%s: %lld rows: at most %d in one call", who, (long long)n_rows, MKGNN_DIVERSE_MAX_ROWS);
    if (k_max < 1 || k_max > n_rows) return api_fail("%s: k_max = %d outside [1, %lld]", who, (int)k_max, (long long)n_rows);
    if (!emb || !picks || !n_picks || !leader || !leader_sim || !workspace) return api_fail("%s: null pointer", who);
    const size_t need = mkgnn_diverse_pick_workspace_bytes(n_rows);
    if (workspace_bytes < need) return api_fail("%s: workspace of %zu bytes, %zu needed", who, workspace_bytes, need);
    if (((uintptr_t)workspace & 3) != 0) return api_fail("%s: workspace not 4-byte aligned", who);
    // what the launches write -- the four outputs and the workspace -- must not overlap emb, nor each other: every launch reads
    // emb, and each output has one writer per launch
    const size_t rows = (size_t)n_rows * 4;
    const Span rd = {emb, ((size_t)(n_rows - 1) * (size_t)emb_stride + (size_t)H) * 4};
    const Span wr[5] = {{picks, (size_t)k_max * 4}, {n_picks, 4}, {leader, rows}, {leader_sim, rows}, {workspace, need}};
    if (spans_disjoint(who, wr, 5, &rd, 1, "an output (picks, n_picks, leader, leader_sim) or the workspace aliases emb",
                       "the outputs (picks, n_picks, leader, leader_sim) and the workspace alias each other"))
        return 1;
    const hipStream_t st = (hipStream_t)stream;
    const int n = (int)n_rows;
    float* inv = (float*)workspace;
    float* self = inv + dv_row_floats(n_rows);
    int32_t* cnt = (int32_t*)(self + dv_row_floats(n_rows));
    init_kernel<<<(unsigned)((n + 7) / 8), 256, 0, st>>>(emb, emb_stride, n, H, k_max, inv, self, cnt, picks, n_picks, leader,
                                                         leader_sim);
    if (H <= 32)
        dv_launch<32>(emb, emb_stride, n, H, max_sim, k_max, inv, self, cnt, picks, n_picks, leader, leader_sim, st);
    else
        dv_launch<64>(emb, emb_stride, n, H, max_sim, k_max, inv, self, cnt, picks, n_picks, leader, leader_sim, st);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : api_hip_fail(who, e);
}
