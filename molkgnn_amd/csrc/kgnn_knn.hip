// Analogue search for any number of queries (mkgnn_embed_knn_update): Q running lists of K slots, one per query, updated IN PLACE
// from raw candidate embeddings and raw queries -- fused cosine and top-k, no [n, Q] similarity matrix.
//
//     list q  <-  topk_update_reference(list q, s_q, ids, n_valid, shard_tag),    s_q[i] = the float32 value mkgnn_embed_cosine
//                 writes for row i of emb as the ROW and queries[q] as the QUERY, BIT FOR BIT
//
// THE BITS are kgnn_cosine.h's, as kgnn_max_cosine.hip evaluates them: the inverse norms by half_wave_sumsq / inv_clamped_norm
// (knn_norms_kernel, one half-wave per vector, into the workspace), the dot product serially by ONE lane with mc_dot, then
// (dot * inv(row)) * inv(query) in that orientation.  Nothing in this file may be contracted: the pragma below.
//
// THE ORDER is kgnn_ranked.h's with the id as the only trailing key.  Entries with equal keys keep their order of arrival: a candidate
// enters only where it is STRICTLY before the list's last entry, behind every entry it is not strictly before, in row order.
//
// THE LAUNCHES (two, or three when the candidates are split; all on the caller's stream, capturable, no atomics, no state):
//   knn_norms_kernel   1 / max(||.||, eps) of the Q queries and of the rows below n_valid -> workspace
//   knn_lists_kernel   KNN_WAVES waves per block, ONE WAVE PER (query, part of the candidates); grid = (query blocks, parts).  Per
//                      tile of KNN_TILE = 64 rows the block stages the raw values (zero padded, odd pitch) and their inverse norms
//                      in LDS once for all its waves (the next tile's global loads are in flight under this tile's arithmetic);
//                      lane l takes row l of the tile into registers and forms its similarity with
//                      the wave's query (LDS, one address per wave: a broadcast).  The list lives one slot per lane, sorted.  A
//                      ballot finds the lanes whose candidate is before the last entry under the full order -- after the first
//                      tiles almost none -- and each is inserted at the popcount of the entries that stay ahead of it, the rest
//                      shifted one lane up.  One part: the wave starts from list q and writes it back.  More: it starts from an
//                      empty list and leaves the part's sorted list in the workspace
//   knn_merge_kernel   one wave per query: the old list, then the parts' lists in part order, by the same insertion
// The result is the first K of a total order, so it does not depend on the split (knn_split; mirrored by _lib.knn_split), which
// only has to fill the chip when Q is small.  Plain FP32 VALU: the bit contract forbids the matrix instructions' summation order.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "kgnn_common.h"

#include "kgnn_launch.h"
#include "kgnn_cosine.h"
#include "kgnn_ranked.h"
#include "../../include/molkgnn_hip.h"

#pragma clang fp contract(off)

namespace mkgnn {
namespace {

constexpr int KNN_MAX_H = 64;
constexpr int KNN_WAVES = 4;                // queries (= waves) per block: they share one staged tile (mirrored by _lib.KNN_WAVES)
constexpr int KNN_TILE = 64;                // candidate rows per LDS tile: one per lane (_lib.KNN_TILE)
constexpr int KNN_MIN_PART_TILES = 2;       // a part is at least two tiles: a finer split only grows the merge (_lib.KNN_MIN_PART_TILES)
constexpr int KNN_MAX_PARTS = 32;           // parts of the candidates (grid.y); the workspace holds parts x Q lists (_lib.KNN_MAX_PARTS)
constexpr int KNN_TARGET_BLOCKS = 1024;     // four blocks (sixteen waves) per CU (_lib.KNN_TARGET_BLOCKS)
static_assert(MKGNN_KNN_MAX_K == 64 && KNN_TILE == 64, "one list slot and one candidate per lane of a wave");
static_assert(MKGNN_KNN_MAX_ROWS % KNN_TILE == 0, "whole tiles");

// how a launch splits n rows for Q queries: whole tiles per part, at least KNN_MIN_PART_TILES of them, at most KNN_MAX_PARTS
// parts and no more than bring the grid to KNN_TARGET_BLOCKS blocks
struct KnnSplit { int part_rows, parts; };
inline KnnSplit knn_split(int64_t n, int64_t Q) {
    const int64_t query_blocks = (Q + KNN_WAVES - 1) / KNN_WAVES;
    const int64_t tiles = (n + KNN_TILE - 1) / KNN_TILE;
    int64_t want = (KNN_TARGET_BLOCKS + query_blocks - 1) / query_blocks;
    if (want > KNN_MAX_PARTS) want = KNN_MAX_PARTS;
    int64_t tiles_per_part = (tiles + want - 1) / want;
    if (tiles_per_part < KNN_MIN_PART_TILES) tiles_per_part = KNN_MIN_PART_TILES;
    const int64_t parts = (tiles + tiles_per_part - 1) / tiles_per_part;
    return {(int)(tiles_per_part * KNN_TILE), (int)(parts < 1 ? 1 : parts)};
}

struct Entry { uint32_t bits; int32_t shard, mol; };

__device__ __forceinline__ Entry empty_entry() { return Entry{RANK_EMPTY_BITS, -1, -1}; }
__device__ __forceinline__ bool is_empty(const Entry& e) { return e.bits == RANK_EMPTY_BITS && e.shard == -1 && e.mol == -1; }

// strictly before, under the order of kgnn_ranked.h; this list's trailing key: the id
__device__ __forceinline__ bool before(const Entry& a, const Entry& b) {
    const uint64_t ah = rank_shard_key(score_rank(a.bits, is_empty(a)), a.shard);
    const uint64_t bh = rank_shard_key(score_rank(b.bits, is_empty(b)), b.shard);
    if (ah != bh) return ah < bh;
    return ordered(a.mol) < ordered(b.mol);
}

// One tile of candidates into a wave's list.  mine: slot `lane` of the sorted list (lanes >= K hold what falls off its end); c: this
// lane's candidate, `valid` whether it is one.  The whole wave calls it; every branch is wave-uniform.
__device__ __forceinline__ void knn_insert(Entry& mine, int K, int lane, const Entry& c, bool valid) {
    const Entry last = lane_entry(mine, K - 1);
    unsigned long long mask = __ballot(valid && before(c, last));
    while (mask) {                                           // (the entrants in lane order = row order)
        const int b = __ffsll((long long)mask) - 1;
        mask &= mask - 1;
        const Entry x = lane_entry(c, b);
        if (!before(x, lane_entry(mine, K - 1))) continue;    // (the list has moved on since the ballot)
        // the entries that stay ahead of x -- a prefix of the sorted list, and never slot K - 1 -- give its slot
        const int pos = __popcll(__ballot(lane < K && !before(x, mine)));
        const Entry up{(uint32_t)__shfl_up((int)mine.bits, 1, 64), __shfl_up(mine.shard, 1, 64), __shfl_up(mine.mol, 1, 64)};
        if (lane > pos) mine = up;
        else if (lane == pos) mine = x;
    }
}

__device__ __forceinline__ int knn_valid_rows(const int32_t* n_valid, int64_t n) {
    return n_valid ? (int)min((int64_t)max(*n_valid, 0), n) : (int)n;
}

// vector v of [queries (Q) | rows (n)]: inv[v] = 1 / max(||v||, eps); one half-wave per vector, 8 per block.  A row at or behind
// n_valid is not read: its half-wave walks query 0 in its place and writes nothing
__global__ void __launch_bounds__(256) knn_norms_kernel(const float* __restrict__ qry, int64_t qs, int Q, const float* __restrict__ emb,
                                                        int64_t es, int64_t n, const int32_t* __restrict__ n_valid, int H,
                                                        float* __restrict__ inv) {
    const int h = threadIdx.x & 31;
    const int64_t v = (int64_t)blockIdx.x * 8 + (threadIdx.x >> 5);
    const int nv = knn_valid_rows(n_valid, n);
    const bool real = v < (int64_t)Q + nv;
    const float* row = !real ? qry : v < Q ? qry + v * qs : emb + (v - Q) * es;
    const float s = half_wave_row_sumsq(row, h, H);
    if (h == 0 && real) inv[v] = inv_clamped_norm(s);
}

struct KnnArgs {
    const float* emb; int64_t es, n;
    const int32_t *ids, *n_valid, *shard_tag;
    const float* qry; int64_t qs;
    int32_t H, Q, K, part_rows, parts;
    const float* inv;                                        // [Q | n]
    float* top_sim; int32_t *top_shard, *top_mol;            // [Q, K]
    uint32_t* part_bits; int32_t *part_shard, *part_mol;     // [parts, Q, K] (parts > 1)
};

template <int W>
__global__ void __launch_bounds__(64 * KNN_WAVES) knn_lists_kernel(const KnnArgs a) {
    constexpr int PITCH = W + 1;                             // odd: lane l reads row l, the 64 rows fall into 64 banks
    __shared__ float tile[KNN_TILE * PITCH];
    __shared__ float tinv[KNN_TILE];
    __shared__ __attribute__((aligned(16))) float qv[KNN_WAVES * W];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int64_t q = (int64_t)blockIdx.x * KNN_WAVES + w, qc = q < a.Q ? q : a.Q - 1;   // (clamped: every wave meets every barrier)
    const int H = a.H, K = a.K;
    const int nv = knn_valid_rows(a.n_valid, a.n);
    const int32_t tag = a.shard_tag ? *a.shard_tag : 0;
    const int r_begin = (int)blockIdx.y * a.part_rows, r_end = min(nv, r_begin + a.part_rows);
    for (int c = lane; c < W; c += 64) qv[w * W + c] = c < H ? a.qry[qc * a.qs + c] : 0.f;
    const float iq = a.inv[qc];
    Entry mine = empty_entry();
    const size_t slot = (size_t)qc * K + lane;
    if (a.parts == 1 && q < a.Q && lane < K) mine =Entry{__float_as_uint(a.top_sim[slot]), a.top_shard[slot], a.top_mol[slot]};
    // a tile's values go global -> registers -> LDS: the NEXT tile's loads are issued before this tile's arithmetic, so their
    // latency lies under it instead of between two barriers
    constexpr int PER = KNN_TILE * W / (64 * KNN_WAVES);     // staged values per thread and tile
    float pre[PER], pre_inv = 0.f;
    auto fetch = [&](int r0) {
        const int m = min(KNN_TILE, r_end - r0);
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int j = t + i * 64 * KNN_WAVES, r = j / W, c = j - r * W;
            pre[i] = r < m && c < H ? a.emb[(int64_t)(r0 + r) * a.es + c] : 0.f;
        }
        pre_inv = t < m ? a.inv[(int64_t)a.Q + r0 + t] : 0.f;
    };
    if (r_begin < r_end) fetch(r_begin);
    for (int r0 = r_begin; r0 < r_end; r0 += KNN_TILE) {     // (the block's bounds: every wave makes every pass)
        const int m = min(KNN_TILE, r_end - r0);
        __syncthreads();                                     // (the previous tile has been read by every wave)
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int j = t + i * 64 * KNN_WAVES, r = j / W, c = j - r * W;
            tile[r * PITCH + c] = pre[i];
        }
        if (t < KNN_TILE) tinv[t] = pre_inv;
        __syncthreads();                                     // (the first pass: qv as well)
        if (r0 + KNN_TILE < r_end) fetch(r0 + KNN_TILE);
        const bool valid = lane < m;
        const int lr = valid ? lane : 0;
        float e[W];
#pragma unroll
        for (int j = 0; j < W; ++j) e[j] = tile[lr * PITCH + j];
        const float d = mc_dot<W>(e, qv + w * W);
        const float s = (d * tinv[lr]) * iq;
        const Entry c{__float_as_uint(s), tag, a.ids ? a.ids[r0 + lr] : r0 + lr};
        knn_insert(mine, K, lane, c, valid);
    }
    if (q < a.Q && lane < K) {
        if (a.parts == 1) {
            a.top_sim[slot] = __uint_as_float(mine.bits);
            a.top_shard[slot] = mine.shard;
            a.top_mol[slot] = mine.mol;
        } else {
            const size_t at = ((size_t)blockIdx.y * a.Q + (size_t)q) * K + lane;
            a.part_bits[at] = mine.bits;
            a.part_shard[at] = mine.shard;
            a.part_mol[at] = mine.mol;
        }
    }
}

// one wave per query: the old list, then every part's sorted list in part order -- the order of arrival
__global__ void __launch_bounds__(64 * KNN_WAVES) knn_merge_kernel(const KnnArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t q = (int64_t)blockIdx.x * KNN_WAVES + (threadIdx.x >> 6);
    if (q >= a.Q) return;                                    // (whole waves; the kernel has no barrier)
    const int K = a.K;
    const size_t slot = (size_t)q * K + lane;
    Entry mine = empty_entry();
    if (lane < K) mine = Entry{__float_as_uint(a.top_sim[slot]), a.top_shard[slot], a.top_mol[slot]};
    for (int p = 0; p < a.parts; ++p) {
        const size_t at = ((size_t)p * a.Q + (size_t)q) * K + lane;
        Entry c = empty_entry();
        if (lane < K) c = Entry{a.part_bits[at], a.part_shard[at], a.part_mol[at]};
        knn_insert(mine, K, lane, c, lane < K && !is_empty(c));
    }
    if (lane < K) {
        a.top_sim[slot] = __uint_as_float(mine.bits);
        a.top_shard[slot] = mine.shard;
        a.top_mol[slot] = mine.mol;
    }
}

}  // namespace
}  // namespace mkgnn

using namespace mkgnn;

namespace {
// [inverse norms: Q + n floats, padded to 4][parts x Q x K similarity bits][... shards][... ids]  (the lists: parts > 1 only)
inline size_t knn_norm_floats(int64_t n, int Q) { return (size_t)(((int64_t)Q + n + 3) / 4 * 4); }
inline bool knn_sizes_ok(int64_t n, int Q, int K) {
    return Q >= 1 && Q <= MKGNN_KNN_MAX_QUERIES && K >= 1 && K <= MKGNN_KNN_MAX_K && n >= 0 && n <= MKGNN_KNN_MAX_ROWS;
}
}  // namespace

extern "C" size_t mkgnn_embed_knn_workspace_bytes(int64_t n_rows, int32_t Q, int32_t K) {
    if (!knn_sizes_ok(n_rows, Q, K)) return 0;
    const KnnSplit sp = knn_split(n_rows, Q);
    const size_t lists = sp.parts > 1 ? (size_t)sp.parts * (size_t)Q * (size_t)K : 0;
    return sizeof(float) * (knn_norm_floats(n_rows, Q) + 3 * lists);
}

extern "C" int mkgnn_embed_knn_update(const float* emb, int64_t emb_stride, int64_t n_rows, int32_t H, const int32_t* ids,
                                      const int32_t* n_valid, const int32_t* shard_tag, const float* queries, int64_t query_stride,
                                      int32_t Q, int32_t K, float* top_sim, int32_t* top_shard, int32_t* top_mol, void* workspace,
                                      size_t workspace_bytes, void* stream) {
    const char* who = "mkgnn_embed_knn_update";
    if (Q < 1 || Q > MKGNN_KNN_MAX_QUERIES) return api_fail("%s: %d queries outside [1, %d]", who, (int)Q, MKGNN_KNN_MAX_QUERIES);
    if (K < 1 || K > MKGNN_KNN_MAX_K) return api_fail("%s: K = %d outside [1, %d]", who, (int)K, MKGNN_KNN_MAX_K);
    if (H < 1 || H > KNN_MAX_H) return api_fail("%s: embedding width %d outside [1, %d]", who, (int)H, KNN_MAX_H);
    if (n_rows < 0 || n_rows > MKGNN_KNN_MAX_ROWS)
        return api_fail("%s: %lld rows outside [0, %d]: call per chunk of rows", who, (long long)n_rows, MKGNN_KNN_MAX_ROWS);
    if (emb_stride < H || query_stride < H) return api_fail("%s: a stride below the embedding width %d", who, (int)H);
    if (n_rows == 0) return 0;
    if (!emb || !queries || !top_sim || !top_shard || !top_mol || !workspace) return api_fail("%s: null pointer", who);
    const size_t need = mkgnn_embed_knn_workspace_bytes(n_rows, Q, K);
    if (workspace_bytes < need) return api_fail("%s: workspace of %zu bytes, %zu needed", who, workspace_bytes, need);
    if (((uintptr_t)workspace & 3) != 0) return api_fail("%s: workspace not 4-byte aligned", who);
    // what the launches write -- the three lists and the workspace -- must not overlap what they read, nor each other
    const size_t list = (size_t)Q * (size_t)K * 4;
    const Span wr[4] = {{top_sim, list}, {top_shard, list}, {top_mol, list}, {workspace, need}};
    const Span rd[5] = {{emb, ((size_t)(n_rows - 1) * (size_t)emb_stride + (size_t)H) * 4},
                        {queries, ((size_t)(Q - 1) * (size_t)query_stride + (size_t)H) * 4},
                        {ids, ids ? (size_t)n_rows * 4 : (size_t)0}, {n_valid, n_valid ? (size_t)4 : (size_t)0},
                        {shard_tag, shard_tag ? (size_t)4 : (size_t)0}};
    if (spans_disjoint(who, wr, 4, rd, 5, "an output (a list or the workspace) aliases an input",
                       "the lists and the workspace alias each other"))
        return 1;
    const hipStream_t st = (hipStream_t)stream;
    const KnnSplit sp = knn_split(n_rows, Q);
    KnnArgs a{};
    a.emb = emb; a.es = emb_stride; a.n = n_rows; a.ids = ids; a.n_valid = n_valid; a.shard_tag = shard_tag;
    a.qry = queries; a.qs = query_stride; a.H = H; a.Q = Q; a.K = K; a.part_rows = sp.part_rows; a.parts = sp.parts;
    float* inv = (float*)workspace;
    a.inv = inv;
    a.top_sim = top_sim; a.top_shard = top_shard; a.top_mol = top_mol;
    const size_t lists = (size_t)sp.parts * (size_t)Q * (size_t)K;
    a.part_bits = (uint32_t*)(inv + knn_norm_floats(n_rows, Q));
    a.part_shard = (int32_t*)(a.part_bits + lists);
    a.part_mol = a.part_shard + lists;
    const int64_t vectors = (int64_t)Q + n_rows;
    knn_norms_kernel<<<(unsigned)((vectors + 7) / 8), 256, 0, st>>>(queries, query_stride, Q, emb, emb_stride, n_rows, n_valid, H, inv);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return api_hip_fail(who, e);
    const unsigned query_blocks = (unsigned)((Q + KNN_WAVES - 1) / KNN_WAVES);
    const dim3 grid(query_blocks, (unsigned)sp.parts);
    if (H <= 32)
        knn_lists_kernel<32><<<grid, 64 * KNN_WAVES, 0, st>>>(a);
    else
        knn_lists_kernel<64><<<grid, 64 * KNN_WAVES, 0, st>>>(a);
    e = hipGetLastError();
    if (e != hipSuccess) return api_hip_fail(who, e);
    if (sp.parts > 1) {
        knn_merge_kernel<<<query_blocks, 64 * KNN_WAVES, 0, st>>>(a);
        e = hipGetLastError();
    }
    return e == hipSuccess ? 0 : api_hip_fail(who, e);
}
