// What each kernel learned (mkgnn_kernel_exemplars_update): C running lists, one per kernel column of a convolution layer's output
// sim [N, C], each the K atoms of a library that column matches best.  List c -- slots [c K, (c + 1) K) of (top_score, top_shard,
// top_mol, top_atom) -- becomes the first K entries, sorted, of  old list c  U  the candidates of c  under the total order of
// include/molkgnn_hip.h: mkgnn_topk_update's, extended by the atom.  molkgnn_amd/screening.py::kernel_exemplars_reference is the
// definition this is tested against, bit for bit.
//
// A candidate is an atom of the batch: slot s < count_d of degree d names atom n = selected_index_d[s], which competes in the L_d
// columns of its own degree and in no other -- if it is a real atom (n < *n_valid_atoms) of a live molecule (atom_mol[n] <
// clamp(*n_live, 0, B)).  Its entry is (bits of sim[n, c], *shard_tag, mol_ids[atom_mol[n]], n - mol_ptr[atom_mol[n]]) and, as the
// last key, its position K + s behind the old list: the order is total, so a sorting network gives the stable result.
//
//   exemplar_runs_kernel   one workgroup per (tile of EX_TILE slots of ONE degree, chunk of EX_CHUNK columns of that degree).  The
//                          atoms' scores are read once, each atom's columns contiguously, and laid down in LDS; on the way every
//                          score meets the last entry of its column's old list (all K-th slots of the chunk lie in LDS) under the
//                          FULL order.  A column none of the tile's candidates displaces writes flag 0 and does no more -- after
//                          the first batches of a screen that is nearly every (tile, column).  Any other column is taken by one
//                          wave: bitonic sort of the tile's entries 64 at a time in registers (wave shuffles), halves merged, the
//                          best Kp (K rounded up to a power of two) written as a sorted run, flag 1.
//   exemplar_merge_kernel  one wave per column: the old list one slot per lane, the flagged runs in tile order, each by
//                          m[t] = min(list[t], run[Kp - 1 - t]) and log2(Kp) merge stages (topk_merge_kernel's step).
// Integers only (scores are compared through their bit patterns), no atomics, no process-wide state; n_live, shard_tag and
// n_valid_atoms are read on the device; every flag, run entry and list slot has one writer.  Nothing outside an atom's own column
// block is read from sim, and nothing of an atom that is no candidate.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "kgnn_launch.h"
#include "kgnn_ranked.h"
#include "../../include/molkgnn_hip.h"

namespace mkgnn {
namespace {

constexpr int EX_TILE = 128;              // slots per tile (mirrored by _lib.EXEMPLARS_TILE)
constexpr int EX_CHUNK = 64;              // columns per workgroup of the runs launch
constexpr int EX_THREADS = 256;
constexpr int EX_MERGE_COLUMNS = 4;       // columns (= waves) per workgroup of the merge launch
static_assert(MKGNN_EXEMPLARS_MAX_K == 64, "one list slot per lane of a wave");
static_assert(EX_TILE % 64 == 0 && EX_TILE <= EX_THREADS, "whole waves of slots, one thread per slot for the slot's facts");

struct Entry { uint32_t bits; int32_t shard, mol, atom; uint32_t pos; };

__device__ __forceinline__ Entry empty_entry(uint32_t pos) { return Entry{RANK_EMPTY_BITS, -1, -1, -1, pos}; }
__device__ __forceinline__ bool is_empty(const Entry& e) { return e.bits == RANK_EMPTY_BITS && e.shard == -1 && e.mol == -1 && e.atom == -1; }

// the order of kgnn_ranked.h; this list's trailing keys: the molecule, the atom, then the position
__device__ __forceinline__ bool before(const Entry& a, const Entry& b) {
    const uint64_t ah = rank_shard_key(score_rank(a.bits, is_empty(a)), a.shard);
    const uint64_t bh = rank_shard_key(score_rank(b.bits, is_empty(b)), b.shard);
    if (ah != bh) return ah < bh;
    const uint64_t am = ((uint64_t)ordered(a.mol) << 32) | ordered(a.atom);
    const uint64_t bm = ((uint64_t)ordered(b.mol) << 32) | ordered(b.atom);
    if (am != bm) return am < bm;
    return a.pos < b.pos;
}

// the layout of one call, by value: per degree its slots, its column block and where its flags and runs begin (in (tile, column)
// pairs: pair p owns flag p and the run entries [p Kp, (p + 1) Kp))
struct ExArgs {
    const int64_t* sel[MKGNN_MAX_DEGREE];
    int32_t count[MKGNN_MAX_DEGREE], col_begin[MKGNN_MAX_DEGREE], L[MKGNN_MAX_DEGREE], tiles[MKGNN_MAX_DEGREE];
    int32_t block_begin[MKGNN_MAX_DEGREE + 1];          // the runs launch: the blocks of degree d are [block_begin[d], block_begin[d + 1])
    int32_t pair_begin[MKGNN_MAX_DEGREE];
    const float* sim; int64_t sim_stride, n_atoms;
    const int32_t *atom_mol, *mol_ptr, *mol_ids, *n_live, *shard_tag;
    const int64_t* n_valid_atoms;
    int32_t B, K, Kp, C, pitch;
    float* top_score; int32_t *top_shard, *top_mol, *top_atom;
    int32_t* flags; uint4* runs; uint32_t* run_pos;
};

__global__ void __launch_bounds__(EX_THREADS) exemplar_runs_kernel(const ExArgs a) {
    extern __shared__ uint32_t tile[];                   // [EX_TILE][pitch] score bits, pitch odd: a column is read without conflicts
    __shared__ int32_t s_atom_row[EX_TILE], s_mol[EX_TILE], s_atom[EX_TILE];      // atom row n (-1: no candidate), its id pair
    __shared__ uint32_t t_bits[EX_CHUNK];                // the chunk's thresholds: slot K - 1 of every column's old list
    __shared__ int32_t t_shard[EX_CHUNK], t_mol[EX_CHUNK], t_atom[EX_CHUNK];
    __shared__ int32_t s_any[EX_CHUNK];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    int d = 0;
    while (d < MKGNN_MAX_DEGREE - 1 && (int)blockIdx.x >= a.block_begin[d + 1]) ++d;
    const int L = a.L[d], chunks = (L + EX_CHUNK - 1) / EX_CHUNK;
    const int local = (int)blockIdx.x - a.block_begin[d];
    const int tl = local / chunks, j0 = (local - tl * chunks) * EX_CHUNK;        // the tile, the chunk's first column in the block
    const int Lc = min(EX_CHUNK, L - j0), c0 = a.col_begin[d] + j0;
    const int64_t s0 = (int64_t)tl * EX_TILE;
    const int K = a.K, Kp = a.Kp, pitch = a.pitch;
    const int32_t tag = *a.shard_tag;
    if (t < EX_TILE) {
        const int64_t s = s0 + t;
        int32_t row = -1, mol = -1, atom = -1;
        if (s < a.count[d]) {
            const int64_t n = a.sel[d][s];
            const int64_t nva = a.n_valid_atoms ? *a.n_valid_atoms : a.n_atoms;
            if (n >= 0 && n < a.n_atoms && n < nva) {
                const int32_t live = min(max(*a.n_live, 0), a.B);
                const int32_t g = a.atom_mol[n];
                if (g >= 0 && g < live) {
                    row = (int32_t)n;
                    mol = a.mol_ids[g];
                    atom = (int32_t)(n - (int64_t)a.mol_ptr[g]);
                }
            }
        }
        s_atom_row[t] = row; s_mol[t] = mol; s_atom[t] = atom;
    }
    if (t < Lc) {
        const size_t at = (size_t)(c0 + t) * K + (K - 1);
        t_bits[t] = __float_as_uint(a.top_score[at]);
        t_shard[t] = a.top_shard[at]; t_mol[t] = a.top_mol[at]; t_atom[t] = a.top_atom[at];
        s_any[t] = 0;
    }
    __syncthreads();
    // every candidate's scores: an atom's Lc columns are contiguous in sim and consecutive threads take consecutive columns
    for (int i = t; i < EX_TILE * Lc; i += EX_THREADS) {
        const int r = i / Lc, j = i - r * Lc;
        const int32_t row = s_atom_row[r];
        if (row < 0) continue;
        const uint32_t bits = __float_as_uint(a.sim[(int64_t)row * a.sim_stride + c0 + j]);
        tile[r * pitch + j] = bits;
        const Entry e{bits, tag, s_mol[r], s_atom[r], (uint32_t)K + (uint32_t)(s0 + r)};
        const Entry last{t_bits[j], t_shard[j], t_mol[j], t_atom[j], (uint32_t)(K - 1)};
        if (before(e, last)) s_any[j] = 1;               // (plain store of the one value any writer stores)
    }
    __syncthreads();
    // no barrier from here on: a wave takes the columns w, w + 4, ... on its own
    const size_t pair0 = (size_t)a.pair_begin[d] + (size_t)tl * L + j0;
    for (int j = w; j < Lc; j += EX_THREADS / 64) {
        const bool any = s_any[j] != 0;                  // (one address: uniform in the wave)
        if (lane == 0) a.flags[pair0 + j] = any ? 1 : 0;
        if (!any) continue;
        Entry best = empty_entry(0xFFFFFFFFu);
        for (int h = 0; h < EX_TILE / 64; ++h) {
            const int r = h * 64 + lane;
            const int32_t row = s_atom_row[r];
            const uint32_t pos = (uint32_t)K + (uint32_t)(s0 + r);
            Entry e = row < 0 ? empty_entry(pos) : Entry{tile[r * pitch + j], tag, s_mol[r], s_atom[r], pos};
            for (int k = 2; k <= 64; k <<= 1)
                for (int jj = k >> 1; jj > 0; jj >>= 1) wave_exchange(e, lane, jj, (lane & k) == 0);
            if (h == 0) {
                best = e;
            } else {                                     // the best 64 of both sorted halves, as a bitonic sequence; then sorted
                const Entry o = lane_entry(e, 63 - lane);
                if (before(o, best)) best = o;
                wave_merge_stages(best, lane, 64);
            }
        }
        if (lane < Kp) {
            const size_t at = (pair0 + j) * Kp + lane;
            a.runs[at] = make_uint4(best.bits, (uint32_t)best.shard, (uint32_t)best.mol, (uint32_t)best.atom);
            a.run_pos[at] = best.pos;
        }
    }
}

__global__ void __launch_bounds__(64 * EX_MERGE_COLUMNS) exemplar_merge_kernel(const ExArgs a) {
    const int lane = threadIdx.x & 63;
    const int c = blockIdx.x * EX_MERGE_COLUMNS + (threadIdx.x >> 6);
    if (c >= a.C) return;                                // (whole waves; the kernel has no barrier)
    int d = -1;
    for (int k = 0; k < MKGNN_MAX_DEGREE; ++k)
        if (c >= a.col_begin[k] && c < a.col_begin[k] + a.L[k]) d = k;
    if (d < 0 || a.tiles[d] == 0) return;                // a column no degree owns, or one without slots: its list stays
    const int K = a.K, Kp = a.Kp, L = a.L[d], tiles = a.tiles[d];
    const size_t pair0 = (size_t)a.pair_begin[d] + (size_t)(c - a.col_begin[d]);
    Entry cur = empty_entry(0xFFFFFFFFu);
    const size_t mine = (size_t)c * K + lane;
    if (lane < K) cur = Entry{__float_as_uint(a.top_score[mine]), a.top_shard[mine], a.top_mol[mine], a.top_atom[mine], (uint32_t)lane};
    bool changed = false;
    for (int t0 = 0; t0 < tiles; t0 += 64) {
        const int32_t f = t0 + lane < tiles ? a.flags[pair0 + (size_t)(t0 + lane) * L] : 0;
        unsigned long long mask = __ballot(f != 0);
        while (mask) {                                   // (uniform: the flagged tiles in tile order)
            const int b = __ffsll((long long)mask) - 1;
            mask &= mask - 1;
            const size_t at = (pair0 + (size_t)(t0 + b) * L) * Kp + (lane < Kp ? Kp - 1 - lane : 0);
            const uint4 v = a.runs[at];
            const Entry run{v.x, (int32_t)v.y, (int32_t)v.z, (int32_t)v.w, a.run_pos[at]};
            if (lane < Kp && before(run, cur)) cur = run;
            wave_merge_stages(cur, lane, Kp);
            changed = true;
        }
    }
    if (changed && lane < K) {
        a.top_score[mine] = __uint_as_float(cur.bits);
        a.top_shard[mine] = cur.shard;
        a.top_mol[mine] = cur.mol;
        a.top_atom[mine] = cur.atom;
    }
}

constexpr int64_t EX_MAX_COUNT = (int64_t)1 << 30;       // slots of one degree: positions K + s stay below 2^31

// the column blocks: inside [0, C), disjoint; false otherwise
inline bool blocks_ok(const int32_t* col_begin, const int32_t* L, int32_t C) {
    for (int d = 0; d < MKGNN_MAX_DEGREE; ++d) {
        if (L[d] < 0 || col_begin[d] < 0 || col_begin[d] > C || L[d] > C - col_begin[d]) return false;
        for (int e = 0; e < d; ++e)
            if (L[d] > 0 && L[e] > 0 && col_begin[d] < col_begin[e] + L[e] && col_begin[e] < col_begin[d] + L[d]) return false;
    }
    return true;
}

// (tile, column) pairs of the call and the blocks of its runs launch; false for refused sizes
inline bool layout(const int64_t* count, const int32_t* L, int32_t K, int32_t C, ExArgs* out, size_t* pairs) {
    if (!count || !L || K < 1 || K > MKGNN_EXEMPLARS_MAX_K || C < 1 || C > MKGNN_EXEMPLARS_MAX_COLUMNS) return false;
    size_t p = 0;
    int64_t blocks = 0;
    for (int d = 0; d < MKGNN_MAX_DEGREE; ++d) {
        if (count[d] < 0 || count[d] > EX_MAX_COUNT || L[d] < 0 || L[d] > C) return false;
        const int64_t tiles = L[d] > 0 ? (count[d] + EX_TILE - 1) / EX_TILE : 0;
        if (out) {
            out->count[d] = (int32_t)count[d]; out->L[d] = L[d]; out->tiles[d] = (int32_t)tiles;
            out->block_begin[d] = (int32_t)blocks; out->pair_begin[d] = (int32_t)p;
        }
        p += (size_t)tiles * (size_t)L[d];
        blocks += tiles * ((L[d] + EX_CHUNK - 1) / EX_CHUNK);
    }
    if (p > ((size_t)1 << 31) - 1 || blocks > ((int64_t)1 << 31) - 1) return false;
    if (out) out->block_begin[MKGNN_MAX_DEGREE] = (int32_t)blocks;
    *pairs = p;
    return true;
}

// [flags: one int32 per pair, padded to 16 bytes][runs: Kp uint4 per pair][their positions: Kp uint32 per pair]
inline size_t flag_bytes(size_t pairs) { return (pairs * 4 + 15) / 16 * 16; }

}  // namespace
}  // namespace mkgnn

using namespace mkgnn;

extern "C" size_t mkgnn_kernel_exemplars_workspace_bytes(const int64_t count[MKGNN_MAX_DEGREE],
                                                         const int32_t num_kernels[MKGNN_MAX_DEGREE], int32_t K, int32_t C) {
    size_t pairs = 0;
    if (!layout(count, num_kernels, K, C, nullptr, &pairs)) return 0;
    return 256 + flag_bytes(pairs) + pairs * (size_t)pow2_at_least(K) * (sizeof(uint4) + sizeof(uint32_t));
}

extern "C" int mkgnn_kernel_exemplars_update(const float* sim, int64_t sim_stride, int64_t n_atoms,
                                             const mkgnn_degree_bucket buckets[MKGNN_MAX_DEGREE],
                                             const int32_t col_begin[MKGNN_MAX_DEGREE], const int32_t num_kernels[MKGNN_MAX_DEGREE],
                                             const int32_t* atom_mol, const int32_t* mol_ptr, const int32_t* mol_ids, int32_t B,
                                             const int32_t* n_live, const int64_t* n_valid_atoms, const int32_t* shard_tag,
                                             int32_t K, int32_t C, float* top_score, int32_t* top_shard, int32_t* top_mol,
                                             int32_t* top_atom, void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "mkgnn_kernel_exemplars_update";
    if (!sim || !buckets || !col_begin || !num_kernels || !atom_mol || !mol_ptr || !mol_ids || !n_live || !shard_tag || !top_score ||
        !top_shard || !top_mol || !top_atom || !workspace)
        return api_fail("%s: null pointer", who);
    if (K < 1 || K > MKGNN_EXEMPLARS_MAX_K) return api_fail("%s: K = %d outside [1, %d]", who, (int)K, MKGNN_EXEMPLARS_MAX_K);
    if (C < 1 || C > MKGNN_EXEMPLARS_MAX_COLUMNS)
        return api_fail("%s: C = %d outside [1, %d]", who, (int)C, MKGNN_EXEMPLARS_MAX_COLUMNS);
    if (B < 1) return api_fail("%s: B = %d", who, (int)B);
    if (n_atoms < 1 || n_atoms > EX_MAX_COUNT) return api_fail("%s: %lld atoms outside [1, 2^30]", who, (long long)n_atoms);
    if (sim_stride < C) return api_fail("%s: sim_stride = %lld below C = %d", who, (long long)sim_stride, (int)C);
    if (!blocks_ok(col_begin, num_kernels, C))
        return api_fail("%s: the column blocks must lie inside [0, %d) and must not overlap", who, (int)C);
    int64_t count[MKGNN_MAX_DEGREE];
    for (int d = 0; d < MKGNN_MAX_DEGREE; ++d) {
        count[d] = buckets[d].count;
        if (count[d] < 0) return api_fail("%s: negative count of degree %d", who, d + 1);
        if (count[d] > n_atoms) return api_fail("%s: %lld slots of degree %d for %lld atoms", who, (long long)count[d], d + 1, (long long)n_atoms);
        if (count[d] > 0 && num_kernels[d] > 0 && !buckets[d].selected_index) return api_fail("%s: null selected_index of degree %d", who, d + 1);
    }
    ExArgs a{};
    size_t pairs = 0;
    if (!layout(count, num_kernels, K, C, &a, &pairs)) return api_fail("%s: the sizes cannot be laid out", who);
    const size_t need = mkgnn_kernel_exemplars_workspace_bytes(count, num_kernels, K, C);
    if (workspace_bytes < need) return api_fail("%s: workspace of %zu bytes, %zu needed", who, workspace_bytes, need);
    if ((uintptr_t)workspace % 16) return api_fail("%s: workspace must be 16-byte aligned", who);
    // what the launches write -- the four lists and the workspace -- must not overlap what they read, nor each other
    const size_t list = (size_t)C * (size_t)K * 4;
    const Span wr[5] = {{top_score, list}, {top_shard, list}, {top_mol, list}, {top_atom, list}, {workspace, need}};
    Span rd[7 + MKGNN_MAX_DEGREE] = {{sim, ((size_t)(n_atoms - 1) * (size_t)sim_stride + (size_t)C) * 4},
                                     {atom_mol, (size_t)n_atoms * 4}, {mol_ptr, ((size_t)B + 1) * 4}, {mol_ids, (size_t)B * 4},
                                     {n_live, 4}, {shard_tag, 4}, {n_valid_atoms, n_valid_atoms ? (size_t)8 : (size_t)0}};
    for (int d = 0; d < MKGNN_MAX_DEGREE; ++d)
        rd[7 + d] = {buckets[d].selected_index, buckets[d].selected_index ? (size_t)count[d] * 8 : (size_t)0};
    if (spans_disjoint(who, wr, 5, rd, 7 + MKGNN_MAX_DEGREE, "an output (a list or the workspace) aliases an input",
                       "the lists and the workspace alias each other"))
        return 1;
    const int32_t Kp = pow2_at_least(K);
    int maxL = 1;
    for (int d = 0; d < MKGNN_MAX_DEGREE; ++d) {
        a.sel[d] = buckets[d].selected_index;
        a.col_begin[d] = col_begin[d];
        if (num_kernels[d] > maxL) maxL = num_kernels[d];
    }
    a.sim = sim; a.sim_stride = sim_stride; a.n_atoms = n_atoms;
    a.atom_mol = atom_mol; a.mol_ptr = mol_ptr; a.mol_ids = mol_ids; a.n_live = n_live; a.shard_tag = shard_tag;
    a.n_valid_atoms = n_valid_atoms;
    a.B = B; a.K = K; a.Kp = Kp; a.C = C;
    a.pitch = (maxL < EX_CHUNK ? maxL : EX_CHUNK) | 1;
    a.top_score = top_score; a.top_shard = top_shard; a.top_mol = top_mol; a.top_atom = top_atom;
    char* const ws = (char*)workspace + 256;
    a.flags = (int32_t*)ws;
    a.runs = (uint4*)(ws + flag_bytes(pairs));
    a.run_pos = (uint32_t*)(ws + flag_bytes(pairs) + pairs * (size_t)Kp * sizeof(uint4));
    const int blocks = a.block_begin[MKGNN_MAX_DEGREE];
    if (blocks == 0) return 0;                           // no degree has both slots and columns: every list stays
    hipStream_t st = (hipStream_t)stream;
    exemplar_runs_kernel<<<blocks, EX_THREADS, (size_t)EX_TILE * a.pitch * sizeof(uint32_t), st>>>(a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return api_hip_fail(who, e);
    exemplar_merge_kernel<<<(C + EX_MERGE_COLUMNS - 1) / EX_MERGE_COLUMNS, 64 * EX_MERGE_COLUMNS, 0, st>>>(a);
    e = hipGetLastError();
    return e == hipSuccess ? 0 : api_hip_fail(who, e);
}
