// The nearest reference of every embedding row (mkgnn_embed_max_cosine), how many references lie above a threshold of it
// (mkgnn_embed_count_within: the neighbour counts of a Butina clustering), and the stable compaction that hands the rows a filter
// keeps to the running list (mkgnn_select_rows): novelty filter and applicability domain of a screen.
//
//     max_sim[i], arg_ref[i] = the first r, in the order of topk_update_reference (non-NaN before NaN, larger first with
//                              -0.0 == +0.0, then the lower r), of sim(i, r) -- the float32 value mkgnn_embed_cosine writes for row i
//                              and query refs[r], BIT FOR BIT
//
// THE BITS are kgnn_cosine.h's: the inverse norms by half_wave_sumsq / inv_clamped_norm -- the functions embed_cosine_kernel itself
// calls -- for every reference and every row (norms_kernel, into the workspace), the dot product serially by ONE THREAD with mc_dot,
// then (dot * inv(e)) * inv(q).  Nothing in this file may be contracted: the pragma below.
//
// THE LAUNCHES (two, or three when the references are split; all on the caller's stream, capturable, no atomics, no state):
//   norms_kernel       one half-wave per vector: 1 / max(||.||, eps) of the R references and the n rows -> workspace
//   max_cosine_kernel  MC_ROWS rows per block, ONE THREAD PER ROW with the row in registers; grid.y = parts of the reference set;
//                      per MC_TILE references the block stages the raw values (zero padded) and their inverse norms in LDS, every
//                      lane then reads the same address -- a broadcast, conflict-free -- and walks the tile.  One part: it writes
//                      max_sim / arg_ref itself.  More: every part writes its winner to workspace[part][row]
//   combine_kernel     one half-wave per row: the parts' winners under the same rule, equals to the lower index -> max_sim / arg_ref
// The winner is a total order's first element, so it does not depend on how the references are split; the split (mc_split; mirrored
// by _lib.max_cosine_split) only has to fill the chip: a batch of 256 rows is two row blocks, so it is cut into up to MC_MAX_PARTS
// parts of whole tiles, a batch of 4 096 rows against 16 384 references into 64 parts of 8 tiles (MC_TARGET_BLOCKS blocks in all).
// Plain FP32 VALU: the bit contract forbids another summation order, and with it the matrix instructions.
//
// THE COUNT is a second reduction over the SAME walk: max_cosine_kernel takes what it does with every sim(i, r) as a policy --
// McFirstMax keeps the first maximum, McCountAbove counts the r with sim(i, r) > min_sim (strict; a NaN fails it) -- so norms_kernel,
// the split, the staging and the tile loop exist once.  counts[i] is a sum of integers: one part writes it itself, more parts write
// workspace[part][row] and count_combine_kernel adds them, in any order the same number.
//
// THE LISTS (mkgnn_embed_neighbours_within) are a third reduction over the same walk: McFillAbove writes every (r, sim(i, r)) the
// count counts, in ascending r, into the row's segment of a CSR whose row pointers the caller made from the counts.  A part of a
// split launch has to know how many pairs the parts before it hold, so a split call runs the COUNT walk into workspace[part][row]
// first, fill_offsets_kernel turns every row's partials into exclusive offsets (and writes found[i], their sum), and the FILL walk
// starts each part at its offset: one writer per slot, no atomics.  THE GUARD: a row writes only slots s with
// 0 <= row_ptr[i] <= s < min(row_ptr[i + 1], capacity) -- whatever row_ptr holds; what does not fit is counted and dropped.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "kgnn_common.h"

#include "kgnn_launch.h"
#include "kgnn_cosine.h"
#include "../../include/molkgnn_hip.h"

#pragma clang fp contract(off)

namespace mkgnn {
namespace {

constexpr int MC_MAX_H = 64;
constexpr int MC_ROWS = 128;              // rows (= threads) per block: two waves share one staged tile
constexpr int MC_TILE = 32;               // references per LDS tile: 32 x 64 floats = 8 KB, twenty blocks' worth per CU
constexpr int MC_MAX_PARTS = 256;         // parts of the reference set (grid.y); the workspace holds parts x rows winners
constexpr int MC_TARGET_BLOCKS = 2048;    // eight blocks (sixteen waves) per CU
constexpr int SEL_THREADS = 1024;         // mkgnn_select_rows: one workgroup, 1 024 slots per pass

// how a launch splits R references for n rows: whole tiles per part, at most MC_MAX_PARTS parts, no more than fill the chip
struct McSplit { int part_refs, parts; };
inline McSplit mc_split(int64_t n, int R) {
    const int64_t row_blocks = (n + MC_ROWS - 1) / MC_ROWS;
    const int tiles = (R + MC_TILE - 1) / MC_TILE;
    int64_t want = (MC_TARGET_BLOCKS + row_blocks - 1) / row_blocks;
    if (want > tiles) want = tiles;
    if (want > MC_MAX_PARTS) want = MC_MAX_PARTS;
    const int tiles_per_part = (tiles + (int)want - 1) / (int)want;
    return {tiles_per_part * MC_TILE, (tiles + tiles_per_part - 1) / tiles_per_part};
}

// vector v of [refs (R) | rows (n)]: inv[v] = 1 / max(||v||, eps); one half-wave per vector, 8 per block
__global__ void __launch_bounds__(256) norms_kernel(const float* __restrict__ refs, int64_t rs, int R, const float* __restrict__ emb,
                                                    int64_t es, int64_t n, int H, float* __restrict__ inv) {
    const int h = threadIdx.x & 31;
    const int64_t v = (int64_t)blockIdx.x * 8 + (threadIdx.x >> 5), total = (int64_t)R + n;
    const int64_t vc = v < total ? v : total - 1;                 // (clamped: every lane of a half-wave takes part in the tree)
    const float* row = vc < R ? refs + vc * rs : emb + (vc - R) * es;
    const float s = half_wave_row_sumsq(row, h, H);
    if (h == 0 && v < total) inv[v] = inv_clamped_norm(s);
}

// the order: a non-NaN beats a NaN, a larger value beats a smaller one (-0.0 == +0.0: no strict >), the earlier one stays otherwise
__device__ __forceinline__ bool mc_better(float s, float best) { return s == s && (best != best || s > best); }

// What a walk does with the similarities of one row: Out is what a launch writes to (and any scalar it compares with); take() sees
// sim(i, r) of every reference of the part in order -- `live` is false where the walk hands the last reference of an odd tile in a
// second time -- and store() writes the part's result to slot `at`.
struct McFirstMax {                                              // the first maximum of the order above and its reference
    struct Out { float* sim; int32_t* arg; };
    float best;
    int arg;
    __device__ __forceinline__ McFirstMax(const Out&, int r_begin, int64_t, int64_t, bool)
        : best(__int_as_float(0x7fc00000)), arg(r_begin) {}      // "nothing yet": any first value replaces it, a NaN leaves it
    __device__ __forceinline__ void take(float s, int r, bool) { // (a second look at the same reference: the strict order ignores it)
        const bool b = mc_better(s, best);
        best = b ? s : best;
        arg = b ? r : arg;
    }
    __device__ __forceinline__ void store(const Out& o, int64_t at) const {
        o.sim[at] = best;
        o.arg[at] = arg;
    }
};

struct McCountAbove {                                            // how many references lie above min_sim: strict, a NaN never counts
    struct Out { int32_t* count; float min_sim; };
    float bound;
    int count;
    __device__ __forceinline__ McCountAbove(const Out& o, int, int64_t, int64_t, bool) : bound(o.min_sim), count(0) {}
    // The empty asm emits nothing; it makes each similarity opaque where it arrives.  Without it the two comparisons of a pair of
    // references are one two-wide operation to the compiler, which then packs EVERY step above them across the two references:
    // v_pk_mul_f32 / v_pk_add_f32 on operands that are not neighbours in registers -- 232 registers at 32 columns, 256 and spills
    // into the accumulation registers at 64, more moves than arithmetic, 1.4 / 1.8 times the first maximum's time.  With it each
    // reference's products and tree levels are packed along the columns, whose operands are neighbours as they come from LDS: 77
    // / 112 registers, the same bits (a packed operation rounds each element once).  -DMKGNN_COUNT_PLAIN: without
    __device__ __forceinline__ void take(float s, int, bool live) {
#ifndef MKGNN_COUNT_PLAIN
        asm volatile("" : "+v"(s));
#endif
        count += (live && s > bound) ? 1 : 0;
    }
    __device__ __forceinline__ void store(const Out& o, int64_t at) const { o.count[at] = count; }
};

// The references above min_sim themselves, in the order the walk meets them (ascending r), into the row's segment of a CSR.
// `room` is THE GUARD: the slots the row may write, counted from its first one -- row_ptr[row] plus what the earlier parts of a
// split launch found -- up to min(row_ptr[row + 1], capacity); 0 where row_ptr[row] lies outside [0, capacity), where the segment
// is empty or runs backwards, where the earlier parts have filled it, and for the lanes behind the last row.  A pair found behind
// `room` is counted and not stored, so nothing row_ptr holds can make a store leave [row_ptr[row], min(row_ptr[row + 1], capacity)).
// One part: store() writes found[row] (every pair, stored or not).  More: fill_offsets_kernel has written it.
struct McFillAbove {
    struct Out {
        int32_t* ref; float* sim; int32_t* found;                // (found: null in a split launch)
        const int64_t* row_ptr; const int32_t* offset;           // (offset [parts][n]: null in a launch of one part)
        int64_t capacity; float min_sim;
    };
    float bound;
    int count, room;
    int32_t* ref;
    float* sim;
    __device__ __forceinline__ McFillAbove(const Out& o, int, int64_t row, int64_t at, bool row_live)
        : bound(o.min_sim), count(0), room(0), ref(o.ref), sim(o.sim) {
        if (!row_live) return;
        const int64_t lo = o.row_ptr[row], hi = min(o.row_ptr[row + 1], o.capacity);
        if (lo < 0 || lo >= hi) return;                          // (so 0 <= lo < hi <= capacity from here on)
        const int64_t left = hi - lo - (o.offset ? (int64_t)max(o.offset[at], 0) : 0);
        if (left <= 0) return;
        room = (int)min(left, (int64_t)0x7fffffff);
        ref += hi - left;                                        // the part's first slot: lo + offset
        sim += hi - left;
    }
    // (no empty asm as in McCountAbove::take: the conditional stores already keep the two references of a pair apart -- 86 / 150
    // registers at 32 / 64 columns with it and without, no spills, the same bits: DESIGN.md 4.5l)
    __device__ __forceinline__ void take(float s, int r, bool live) {
        const bool hit = live && s > bound;
        if (hit && count < room) {
            ref[count] = r;
            sim[count] = s;
        }
        count += hit ? 1 : 0;
    }
    __device__ __forceinline__ void store(const Out& o, int64_t at) const {
        if (o.found) o.found[at] = count;
    }
};

template <int W, typename Red>
__global__ void __launch_bounds__(MC_ROWS) max_cosine_kernel(const float* __restrict__ emb, int64_t es, int64_t n, int H,
                                                             const float* __restrict__ refs, int64_t rs, int R, int part_refs,
                                                             const float* __restrict__ inv, const typename Red::Out out) {
    __shared__ __attribute__((aligned(16))) float tile[MC_TILE * W];
    __shared__ float tinv[MC_TILE];
    const int t = threadIdx.x;
    const int64_t i = (int64_t)blockIdx.x * MC_ROWS + t, ic = i < n ? i : n - 1;
    float e[W];
#pragma unroll
    for (int j = 0; j < W; ++j) e[j] = j < H ? emb[ic * es + j] : 0.f;
    const float ie = inv[R + ic];
    const int r_begin = blockIdx.y * part_refs, r_end = min(R, r_begin + part_refs);
    Red red(out, r_begin, ic, (int64_t)blockIdx.y * n + ic, i < n);       // (the row, its slot of a part's results, a real row)
    for (int r0 = r_begin; r0 < r_end; r0 += MC_TILE) {
        const int m = min(MC_TILE, r_end - r0);
        __syncthreads();                                         // (the previous tile has been walked by every wave)
        stage_padded_tile<W, MC_ROWS>(tile, tinv, m, [r0](int r) { return r0 + r; }, refs, rs, H, inv, t);
        __syncthreads();
        // two references in flight -- one's LDS reads under the other's adds -- and selects, not branches, between them; an odd
        // tile's last reference is taken twice, the second time not `live`
        for (int r = 0; r < m; r += 2) {
            const bool pair = r + 1 < m;
            const int r1 = pair ? r + 1 : r;
            const float d0 = mc_dot<W>(e, tile + r * W), d1 = mc_dot<W>(e, tile + r1 * W);
            const float s0 = (d0 * ie) * tinv[r], s1 = (d1 * ie) * tinv[r1];
            red.take(s0, r0 + r, true);
            red.take(s1, r0 + r1, pair);
        }
    }
    if (i < n) red.store(out, (int64_t)blockIdx.y * n + i);      // (one part: out is the outputs themselves, slot i)
}

// the order between two candidates of DIFFERENT references: mc_better, and among equals (two NaNs, a == b) the lower index --
// symmetric, so both lanes of an exchange keep the same one, and what a sequential walk in reference order keeps
__device__ __forceinline__ bool mc_first(float s, int a, float t, int b) {
    const bool tie = (s != s && t != t) || s == t;
    return tie ? a < b : mc_better(s, t);
}

// one half-wave per row: lane l takes parts l, l + 32, ... (independent loads), then an xor tree under mc_first
__global__ void __launch_bounds__(256) combine_kernel(const float* __restrict__ part_sim, const int32_t* __restrict__ part_arg,
                                                      int64_t n, int parts, float* __restrict__ max_sim,
                                                      int32_t* __restrict__ arg_ref) {
    const int l = threadIdx.x & 31;
    const int64_t i = (int64_t)blockIdx.x * 8 + (threadIdx.x >> 5), ic = i < n ? i : n - 1;
    float best = __int_as_float(0x7fc00000);
    int arg = 0x7fffffff;                                        // (no part: loses to every candidate, a NaN one included)
    for (int p = l; p < parts; p += 32) {
        const float s = part_sim[(int64_t)p * n + ic];
        const int a = part_arg[(int64_t)p * n + ic];
        if (mc_first(s, a, best, arg)) { best = s; arg = a; }
    }
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) {
        const float s = __shfl_xor(best, o, 64);
        const int a = __shfl_xor(arg, o, 64);
        if (mc_first(s, a, best, arg)) { best = s; arg = a; }
    }
    if (l == 0 && i < n) {
        max_sim[i] = best;
        arg_ref[i] = arg;
    }
}

// one half-wave per row: lane l adds the partial counts of parts l, l + 32, ..., then an xor tree of integer additions
__global__ void __launch_bounds__(256) count_combine_kernel(const int32_t* __restrict__ part_count, int64_t n, int parts,
                                                            int32_t* __restrict__ counts) {
    const int l = threadIdx.x & 31;
    const int64_t i = (int64_t)blockIdx.x * 8 + (threadIdx.x >> 5), ic = i < n ? i : n - 1;
    int c = 0;
    for (int p = l; p < parts; p += 32) c += part_count[(int64_t)p * n + ic];
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    if (l == 0 && i < n) counts[i] = c;
}

// one thread per row: the parts' partial counts become exclusive offsets over the parts, in place; found[i] is their sum
__global__ void __launch_bounds__(256) fill_offsets_kernel(int32_t* __restrict__ part_count, int64_t n, int parts,
                                                           int32_t* __restrict__ found) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    int before = 0;
    for (int p = 0; p < parts; ++p) {
        const int c = part_count[(int64_t)p * n + i];
        part_count[(int64_t)p * n + i] = before;
        before += c;
    }
    found[i] = before;
}

// mkgnn_select_rows: one workgroup; per pass of SEL_THREADS slots a ballot per wave, the waves' counts through LDS, the kept
// slots written behind the passes before -- in slot order, so the compaction is stable
__global__ void __launch_bounds__(SEL_THREADS) select_rows_kernel(const float* __restrict__ scores, const int32_t* __restrict__ ids,
                                                                  const float* __restrict__ key, int B,
                                                                  const int32_t* __restrict__ n_valid,
                                                                  const float* __restrict__ bounds, float* __restrict__ out_scores,
                                                                  int32_t* __restrict__ out_ids, int32_t* __restrict__ n_kept) {
    constexpr int NW = SEL_THREADS / 64;
    __shared__ int wave_count[NW];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int nv = min(max(*n_valid, 0), B);
    const float lo = bounds[0], hi = bounds[1];
    int base = 0;
    for (int b0 = 0; b0 < nv; b0 += SEL_THREADS) {               // (nv is the block's: every thread makes every pass)
        const int i = b0 + t;
        bool keep = false;
        if (i < nv) {
            const float k = key[i];
            keep = lo <= k && k <= hi;                           // (a NaN key fails both)
        }
        const unsigned long long mask = __ballot(keep);
        if (lane == 0) wave_count[w] = __popcll(mask);
        __syncthreads();
        int before = 0, all = 0;
#pragma unroll
        for (int v = 0; v < NW; ++v) {
            const int c = wave_count[v];
            before += v < w ? c : 0;
            all += c;
        }
        if (keep) {
            const int o = base + before + __popcll(mask & ((1ull << lane) - 1ull));
            out_scores[o] = scores[i];
            out_ids[o] = ids[i];
        }
        base += all;
        __syncthreads();                                         // (wave_count is rewritten by the next pass)
    }
    if (t == 0) *n_kept = base;
}

}  // namespace
}  // namespace mkgnn

using namespace mkgnn;

static_assert(MKGNN_MAX_COSINE_MAX_REFS % MC_TILE == 0, "whole tiles");

namespace {
// [inverse norms: R + n floats, padded to 4][parts x n winners' values][parts x n winners' indices]
inline size_t mc_norm_floats(int64_t n, int R) { return (size_t)(((int64_t)R + n + 3) / 4 * 4); }
inline bool mc_sizes_ok(int64_t n, int R) {
    return R >= 1 && R <= MKGNN_MAX_COSINE_MAX_REFS && n >= 1 && n <= 0x7fffffff;      // (every grid dimension fits)
}
}  // namespace

extern "C" size_t mkgnn_embed_max_cosine_workspace_bytes(int64_t n_rows, int32_t R) {
    if (!mc_sizes_ok(n_rows, R)) return 0;
    const McSplit sp = mc_split(n_rows, R);
    const size_t winners = sp.parts > 1 ? (size_t)sp.parts * (size_t)n_rows : 0;
    return sizeof(float) * (mc_norm_floats(n_rows, R) + 2 * winners);
}

extern "C" int mkgnn_embed_max_cosine(const float* emb, int64_t emb_stride, int64_t n_rows, int32_t H, const float* refs,
                                      int64_t ref_stride, int32_t R, float* max_sim, int32_t* arg_ref, void* workspace,
                                      size_t workspace_bytes, void* stream) {
    const char* who = "mkgnn_embed_max_cosine";
    if (R < 1 || R > MKGNN_MAX_COSINE_MAX_REFS)
        return api_fail("%s: %d references outside [1, %d]", who, (int)R, MKGNN_MAX_COSINE_MAX_REFS);
    if (H < 1 || H > MC_MAX_H) return api_fail("%s: embedding width %d outside [1, %d]", who, (int)H, MC_MAX_H);
    if (n_rows < 0 || emb_stride < H || ref_stride < H) return api_fail("%s: bad shape", who);
    if (n_rows == 0) return 0;
    if (!emb || !refs || !max_sim || !arg_ref || !workspace) return api_fail("%s: null pointer", who);
    if (!mc_sizes_ok(n_rows, R)) return api_fail("%s: %lld rows: at most 2^31 - 1 in one call", who, (long long)n_rows);
    const size_t need = mkgnn_embed_max_cosine_workspace_bytes(n_rows, R);
    if (workspace_bytes < need)
        return api_fail("%s: workspace of %zu bytes, %zu needed", who, workspace_bytes, need);
    if (((uintptr_t)workspace & 3) != 0) return api_fail("%s: workspace not 4-byte aligned", who);
    const hipStream_t st = (hipStream_t)stream;
    const McSplit sp = mc_split(n_rows, R);
    float* inv = (float*)workspace;
    float* part_sim = inv + mc_norm_floats(n_rows, R);
    int32_t* part_arg = (int32_t*)(part_sim + (size_t)sp.parts * (size_t)n_rows);
    const int64_t vectors = (int64_t)R + n_rows;
    norms_kernel<<<(unsigned)((vectors + 7) / 8), 256, 0, st>>>(refs, ref_stride, R, emb, emb_stride, n_rows, H, inv);
    const dim3 grid((unsigned)((n_rows + MC_ROWS - 1) / MC_ROWS), (unsigned)sp.parts);
    const McFirstMax::Out out = {sp.parts > 1 ? part_sim : max_sim, sp.parts > 1 ? part_arg : arg_ref};
    if (H <= 32)
        max_cosine_kernel<32, McFirstMax><<<grid, MC_ROWS, 0, st>>>(emb, emb_stride, n_rows, H, refs, ref_stride, R, sp.part_refs, inv, out);
    else
        max_cosine_kernel<64, McFirstMax><<<grid, MC_ROWS, 0, st>>>(emb, emb_stride, n_rows, H, refs, ref_stride, R, sp.part_refs, inv, out);
    if (sp.parts > 1)
        combine_kernel<<<(unsigned)((n_rows + 7) / 8), 256, 0, st>>>(part_sim, part_arg, n_rows, sp.parts, max_sim, arg_ref);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : api_hip_fail(who, e);
}

// [inverse norms: R + n floats, padded to 4][parts x n partial counts, when the references are split]
extern "C" size_t mkgnn_embed_count_within_workspace_bytes(int64_t n_rows, int32_t R) {
    if (!mc_sizes_ok(n_rows, R)) return 0;
    const McSplit sp = mc_split(n_rows, R);
    const size_t partials = sp.parts > 1 ? (size_t)sp.parts * (size_t)n_rows : 0;
    return sizeof(float) * (mc_norm_floats(n_rows, R) + partials);
}

extern "C" int mkgnn_embed_count_within(const float* emb, int64_t emb_stride, int64_t n_rows, int32_t H, const float* refs,
                                        int64_t ref_stride, int32_t R, float min_sim, int32_t* counts, void* workspace,
                                        size_t workspace_bytes, void* stream) {
    const char* who = "mkgnn_embed_count_within";
    if (R < 1 || R > MKGNN_MAX_COSINE_MAX_REFS)
        return api_fail("%s: %d references outside [1, %d]", who, (int)R, MKGNN_MAX_COSINE_MAX_REFS);
    if (H < 1 || H > MC_MAX_H) return api_fail("%s: embedding width %d outside [1, %d]", who, (int)H, MC_MAX_H);
    if (n_rows < 0 || emb_stride < H || ref_stride < H) return api_fail("%s: bad shape", who);
    if (!(min_sim - min_sim == 0.f)) return api_fail("%s: min_sim is not a finite threshold", who);
    if (n_rows == 0) return 0;
    if (!emb || !refs || !counts || !workspace) return api_fail("%s: null pointer", who);
    if (!mc_sizes_ok(n_rows, R)) return api_fail("%s: %lld rows: at most 2^31 - 1 in one call", who, (long long)n_rows);
    const size_t need = mkgnn_embed_count_within_workspace_bytes(n_rows, R);
    if (workspace_bytes < need)
        return api_fail("%s: workspace of %zu bytes, %zu needed", who, workspace_bytes, need);
    if (((uintptr_t)workspace & 3) != 0) return api_fail("%s: workspace not 4-byte aligned", who);
    // what the launches write -- counts, the workspace -- must not overlap what they read, nor each other (refs may be emb)
    const Span wr[2] = {{counts, (size_t)n_rows * 4}, {workspace, need}};
    const Span rd[2] = {{emb, ((size_t)(n_rows - 1) * (size_t)emb_stride + (size_t)H) * 4},
                        {refs, ((size_t)(R - 1) * (size_t)ref_stride + (size_t)H) * 4}};
    if (spans_disjoint(who, wr, 2, rd, 2, "an output (counts, workspace) aliases an input", "counts and the workspace alias each other"))
        return 1;
    const hipStream_t st = (hipStream_t)stream;
    const McSplit sp = mc_split(n_rows, R);
    float* inv = (float*)workspace;
    int32_t* part_count = (int32_t*)(inv + mc_norm_floats(n_rows, R));
    const int64_t vectors = (int64_t)R + n_rows;
    norms_kernel<<<(unsigned)((vectors + 7) / 8), 256, 0, st>>>(refs, ref_stride, R, emb, emb_stride, n_rows, H, inv);
    const dim3 grid((unsigned)((n_rows + MC_ROWS - 1) / MC_ROWS), (unsigned)sp.parts);
    const McCountAbove::Out out = {sp.parts > 1 ? part_count : counts, min_sim};
    if (H <= 32)
        max_cosine_kernel<32, McCountAbove><<<grid, MC_ROWS, 0, st>>>(emb, emb_stride, n_rows, H, refs, ref_stride, R, sp.part_refs, inv, out);
    else
        max_cosine_kernel<64, McCountAbove><<<grid, MC_ROWS, 0, st>>>(emb, emb_stride, n_rows, H, refs, ref_stride, R, sp.part_refs, inv, out);
    if (sp.parts > 1)
        count_combine_kernel<<<(unsigned)((n_rows + 7) / 8), 256, 0, st>>>(part_count, n_rows, sp.parts, counts);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : api_hip_fail(who, e);
}

// the count's workspace: [inverse norms][parts x n partial counts, then offsets, when the references are split]
extern "C" size_t mkgnn_embed_neighbours_within_workspace_bytes(int64_t n_rows, int32_t R) {
    return mkgnn_embed_count_within_workspace_bytes(n_rows, R);
}

extern "C" int mkgnn_embed_neighbours_within(const float* emb, int64_t emb_stride, int64_t n_rows, int32_t H, const float* refs,
                                             int64_t ref_stride, int32_t R, float min_sim, const int64_t* row_ptr, int64_t capacity,
                                             int32_t* nbr_ref, float* nbr_sim, int32_t* found, void* workspace,
                                             size_t workspace_bytes, void* stream) {
    const char* who = "mkgnn_embed_neighbours_within";
    if (R < 1 || R > MKGNN_MAX_COSINE_MAX_REFS)
        return api_fail("%s: %d references outside [1, %d]", who, (int)R, MKGNN_MAX_COSINE_MAX_REFS);
    if (H < 1 || H > MC_MAX_H) return api_fail("%s: embedding width %d outside [1, %d]", who, (int)H, MC_MAX_H);
    if (n_rows < 0 || emb_stride < H || ref_stride < H) return api_fail("%s: bad shape", who);
    if (capacity < 0 || capacity > ((int64_t)1 << 60)) return api_fail("%s: bad shape: a capacity of %lld slots", who, (long long)capacity);
    if (!(min_sim - min_sim == 0.f)) return api_fail("%s: min_sim is not a finite threshold", who);
    if (n_rows == 0) return 0;
    if (!emb || !refs || !row_ptr || !found || !workspace || (capacity > 0 && (!nbr_ref || !nbr_sim)))
        return api_fail("%s: null pointer", who);
    if (!mc_sizes_ok(n_rows, R)) return api_fail("%s: %lld rows: at most 2^31 - 1 in one call", who, (long long)n_rows);
    const size_t need = mkgnn_embed_neighbours_within_workspace_bytes(n_rows, R);
    if (workspace_bytes < need)
        return api_fail("%s: workspace of %zu bytes, %zu needed", who, workspace_bytes, need);
    if (((uintptr_t)workspace & 3) != 0) return api_fail("%s: workspace not 4-byte aligned", who);
    // what the launches write -- the lists, found, the workspace -- must not overlap what they read, nor each other (refs may be emb)
    const Span wr[4] = {{nbr_ref, (size_t)capacity * 4}, {nbr_sim, (size_t)capacity * 4}, {found, (size_t)n_rows * 4}, {workspace, need}};
    const Span rd[3] = {{emb, ((size_t)(n_rows - 1) * (size_t)emb_stride + (size_t)H) * 4},
                        {refs, ((size_t)(R - 1) * (size_t)ref_stride + (size_t)H) * 4},
                        {row_ptr, ((size_t)n_rows + 1) * 8}};
    if (spans_disjoint(who, wr, 4, rd, 3, "an output (nbr_ref, nbr_sim, found, workspace) aliases an input",
                       "the outputs (nbr_ref, nbr_sim, found, workspace) alias each other"))
        return 1;
    const hipStream_t st = (hipStream_t)stream;
    const McSplit sp = mc_split(n_rows, R);
    const bool split = sp.parts > 1;
    float* inv = (float*)workspace;
    int32_t* part_count = (int32_t*)(inv + mc_norm_floats(n_rows, R));
    const int64_t vectors = (int64_t)R + n_rows;
    norms_kernel<<<(unsigned)((vectors + 7) / 8), 256, 0, st>>>(refs, ref_stride, R, emb, emb_stride, n_rows, H, inv);
    const dim3 grid((unsigned)((n_rows + MC_ROWS - 1) / MC_ROWS), (unsigned)sp.parts);
    if (split) {                                                 // the parts' counts, then every part's first slot, and found
        const McCountAbove::Out cnt = {part_count, min_sim};
        if (H <= 32)
            max_cosine_kernel<32, McCountAbove><<<grid, MC_ROWS, 0, st>>>(emb, emb_stride, n_rows, H, refs, ref_stride, R, sp.part_refs, inv, cnt);
        else
            max_cosine_kernel<64, McCountAbove><<<grid, MC_ROWS, 0, st>>>(emb, emb_stride, n_rows, H, refs, ref_stride, R, sp.part_refs, inv, cnt);
        fill_offsets_kernel<<<(unsigned)((n_rows + 255) / 256), 256, 0, st>>>(part_count, n_rows, sp.parts, found);
    }
    const McFillAbove::Out out = {nbr_ref, nbr_sim, split ? nullptr : found, row_ptr, split ? part_count : nullptr, capacity, min_sim};
    if (H <= 32)
        max_cosine_kernel<32, McFillAbove><<<grid, MC_ROWS, 0, st>>>(emb, emb_stride, n_rows, H, refs, ref_stride, R, sp.part_refs, inv, out);
    else
        max_cosine_kernel<64, McFillAbove><<<grid, MC_ROWS, 0, st>>>(emb, emb_stride, n_rows, H, refs, ref_stride, R, sp.part_refs, inv, out);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : api_hip_fail(who, e);
}

extern "C" int mkgnn_select_rows(const float* scores, const int32_t* ids, const float* key, int32_t B, const int32_t* n_valid,
                                 const float* bounds, float* out_scores, int32_t* out_ids, int32_t* n_kept, void* stream) {
    const char* who = "mkgnn_select_rows";
    if (B < 1) return api_fail("%s: %d slots: at least one is needed", who, (int)B);
    if (!scores || !ids || !key || !n_valid || !bounds || !out_scores || !out_ids || !n_kept) return api_fail("%s: null pointer", who);
    // what the launch writes -- out_scores, out_ids, *n_kept -- must not overlap what it reads, nor each other: thread 0 writes
    // *n_kept after other threads have read the scalars and written the outputs
    const size_t bytes = (size_t)B * 4;
    const Span wr[3] = {{out_scores, bytes}, {out_ids, bytes}, {n_kept, 4}};
    const Span rd[5] = {{scores, bytes}, {ids, bytes}, {key, bytes}, {n_valid, 4}, {bounds, 8}};
    if (spans_disjoint(who, wr, 3, rd, 5, "an output (out_scores, out_ids, n_kept) aliases an input",
                       "the outputs (out_scores, out_ids, n_kept) alias each other"))
        return 1;
    select_rows_kernel<<<1, SEL_THREADS, 0, (hipStream_t)stream>>>(scores, ids, key, B, n_valid, bounds, out_scores, out_ids, n_kept);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : api_hip_fail(who, e);
}
