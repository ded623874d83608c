// Running top-k on the device (mkgnn_topk_update): the sorted list (top_score, top_shard, top_mol)[K] becomes the best K entries
// of  old list  U  {(scores[i], *shard_tag, ids[i]) : i < min(*n_valid, B)}  under the total order of include/molkgnn_hip.h.
// molkgnn_amd/screening.py::topk_update_reference is the definition this is tested against, bit for bit.
//
// An entry travels as four dwords: the score's bits (copied, never recomputed), shard, molecule and its position in the
// concatenation [old list | batch] -- the last key of the order, which makes it total, so that a sorting network (not stable by
// itself) gives the stable result.  One entry per thread in registers; a compare-exchange with a partner less than 64 lanes away
// is four wave shuffles, one further away goes through LDS (two buffers in turn: one barrier per stage).
//
//   topk_runs_kernel    (only when B > 1024) one workgroup per 1024 batch slots: bitonic sort of the tile, its best Kp entries
//                       (Kp = K rounded up to a power of two) into the workspace as a sorted run; tiles past n_valid write nothing
//   topk_merge_kernel   ONE workgroup: the old list in registers, then run after run: m[t] = min(list[t], run[Kp - 1 - t]) holds
//                       the best Kp of both as a bitonic sequence, log2(Kp) merge stages sort it; a run whose best entry ranks
//                       after the list's last one is passed over (the steady state of a screen).  With B <= 1024 it sorts the
//                       only tile itself: one launch.
// Integers only (scores are compared through their bit patterns), no atomics, no process-wide state; n_valid and shard_tag are
// read on the device.  Slot t of the list is written by thread t alone.
//
// mkgnn_topk_update_tasks: T lists in one update (a library ranked per assay of a multi-task model).  The same two kernels with the
// task on blockIdx.y -- topk_runs_kernel on a (tiles, T) grid, topk_merge_kernel on a (1, T) grid: block (., y) reads the scores
// scores[i * row_stride + y * task_stride], list y ([T, K] arrays) and the runs of task y (their own n_tiles * Kp entries of the
// workspace).  Blocks of different tasks share nothing; the pass-over verdict is uniform inside a block, as before.
// mkgnn_topk_update is the T = 1 call of the same launcher (strides 1 and 0).
#include <cstdint>
#include "kgnn_launch.h"
#include "kgnn_ranked.h"
#include "../../include/molkgnn_hip.h"

namespace mkgnn {
namespace {

constexpr int TOPK_THREADS = 1024, TOPK_TILE = TOPK_THREADS;
static_assert(MKGNN_TOPK_MAX_K == TOPK_TILE, "one list entry per thread");

struct Entry { uint32_t bits; int32_t shard, mol; uint32_t pos; };

__device__ __forceinline__ Entry empty_entry(uint32_t pos) { return Entry{RANK_EMPTY_BITS, -1, -1, pos}; }
__device__ __forceinline__ bool is_empty(const Entry& e) { return e.bits == RANK_EMPTY_BITS && e.shard == -1 && e.mol == -1; }

// the order of kgnn_ranked.h; this list's trailing keys: the molecule, then the position
__device__ __forceinline__ bool before(const Entry& a, const Entry& b) {
    const uint64_t ah = rank_shard_key(score_rank(a.bits, is_empty(a)), a.shard);
    const uint64_t bh = rank_shard_key(score_rank(b.bits, is_empty(b)), b.shard);
    if (ah != bh) return ah < bh;
    const uint64_t al = ((uint64_t)ordered(a.mol) << 32) | a.pos;
    const uint64_t bl = ((uint64_t)ordered(b.mol) << 32) | b.pos;
    return al < bl;
}

__device__ __forceinline__ uint4 pack(const Entry& e) { return make_uint4(e.bits, (uint32_t)e.shard, (uint32_t)e.mol, e.pos); }
__device__ __forceinline__ Entry unpack(const uint4 v) { return Entry{v.x, (int32_t)v.y, (int32_t)v.z, v.w}; }

// one compare-exchange stage of the network: thread t and thread t ^ j; the thread whose bit j is clear keeps the earlier
// entry when `up`.  Every thread of the workgroup calls it (barrier inside when j >= 64); `flip` picks the LDS buffer.
__device__ __forceinline__ void exchange(Entry& e, int j, bool up, uint4 (*buf)[TOPK_TILE], int& flip) {
    const int t = threadIdx.x;
    Entry o;
    if (j < 64) {
        o = lane_entry(e, t ^ j);                        // (kgnn_ranked.h: the wave's own stage; the LDS stage shares the compare)
    } else {
        buf[flip][t] = pack(e);
        __syncthreads();
        o = unpack(buf[flip][t ^ j]);
        flip ^= 1;                                       // (the next stage writes the other buffer: no second barrier)
    }
    const bool keep_first = ((t & j) == 0) == up;
    if (before(o, e) == keep_first) e = o;
}

// ascending bitonic sort of the workgroup's TOPK_TILE entries
__device__ __forceinline__ void sort_tile(Entry& e, uint4 (*buf)[TOPK_TILE], int& flip) {
    const int t = threadIdx.x;
    for (int k = 2; k <= TOPK_TILE; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) exchange(e, j, (t & k) == 0, buf, flip);
}

__device__ __forceinline__ int clamp_valid(const int32_t* n_valid, int32_t B) {
    const int32_t v = *n_valid;
    return v < 0 ? 0 : (v > B ? B : v);
}

// batch slot i as an entry (position Kpos + i); slots at or past nv rank as empty slots behind everything
__device__ __forceinline__ Entry batch_entry(const float* scores, int64_t row_stride, const int32_t* ids, int32_t tag, int64_t i,
                                             int32_t nv, int32_t K) {
    const uint32_t pos = (uint32_t)K + (uint32_t)i;
    if (i >= nv) return empty_entry(pos);
    return Entry{__float_as_uint(scores[i * row_stride]), tag, ids[i], pos};
}

__global__ void __launch_bounds__(TOPK_THREADS) topk_runs_kernel(const float* __restrict__ scores, int64_t row_stride,
                                                                 int64_t task_stride, const int32_t* __restrict__ ids,
                                                                 int32_t B, const int32_t* __restrict__ n_valid,
                                                                 const int32_t* __restrict__ shard_tag, int32_t K, int32_t Kp,
                                                                 uint4* __restrict__ runs) {
    __shared__ uint4 buf[2][TOPK_TILE];
    const int nv = clamp_valid(n_valid, B);
    const int64_t i0 = (int64_t)blockIdx.x * TOPK_TILE;
    if (i0 >= nv) return;                                // (uniform: the merge passes this tile over as well)
    int flip = 0;
    scores += (int64_t)blockIdx.y * task_stride;         // (the task's scores and its own runs)
    runs += (size_t)blockIdx.y * gridDim.x * Kp;
    Entry e = batch_entry(scores, row_stride, ids, *shard_tag, i0 + threadIdx.x, nv, K);
    sort_tile(e, buf, flip);
    if ((int)threadIdx.x < Kp) runs[(size_t)blockIdx.x * Kp + threadIdx.x] = pack(e);
}

__global__ void __launch_bounds__(TOPK_THREADS) topk_merge_kernel(const float* __restrict__ scores, int64_t row_stride,
                                                                  int64_t task_stride, const int32_t* __restrict__ ids,
                                                                  int32_t B, const int32_t* __restrict__ n_valid,
                                                                  const int32_t* __restrict__ shard_tag, int32_t K, int32_t Kp,
                                                                  float* top_score, int32_t* top_shard, int32_t* top_mol,
                                                                  const uint4* __restrict__ runs, int n_tiles) {
    __shared__ uint4 buf[2][TOPK_TILE];
    __shared__ uint4 last;                               // the list's entry K - 1, for the pass-over test
    const int t = threadIdx.x;
    const int nv = clamp_valid(n_valid, B);
    int flip = 0;
    scores += (int64_t)blockIdx.y * task_stride;         // (the task's scores, its list and its own runs)
    top_score += (size_t)blockIdx.y * K; top_shard += (size_t)blockIdx.y * K; top_mol += (size_t)blockIdx.y * K;
    runs += (size_t)blockIdx.y * n_tiles * Kp;
    // the old list: slot t in thread t; the slots from K to the tile's end rank behind every real slot
    Entry cur = empty_entry(0xFFFFFFFFu);
    if (t < K) cur = Entry{__float_as_uint(top_score[t]), top_shard[t], top_mol[t], (uint32_t)t};
    for (int tile = 0; tile < n_tiles; ++tile) {
        const int64_t i0 = (int64_t)tile * TOPK_TILE;
        if (i0 >= nv) break;
        Entry run;                                       // thread t: entry Kp - 1 - t of the tile's sorted run (t < Kp)
        if (n_tiles == 1) {
            Entry e = batch_entry(scores, row_stride, ids, *shard_tag, i0 + t, nv, K);
            sort_tile(e, buf, flip);
            buf[flip][t] = pack(e);
            if (t == K - 1) last = pack(cur);
            __syncthreads();
            run = unpack(buf[flip][t < Kp ? Kp - 1 - t : t]);
            flip ^= 1;
        } else {
            if (t == K - 1) last = pack(cur);
            __syncthreads();
            run = unpack(runs[(size_t)tile * Kp + (t < Kp ? Kp - 1 - t : 0)]);
        }
        // nothing of a run whose best entry ranks after the list's entry K - 1 can enter the first K: every thread reads the two
        // entries from where they already lie and reaches the same verdict
        const Entry best = n_tiles == 1 ? unpack(buf[flip ^ 1][0]) : unpack(runs[(size_t)tile * Kp]);
        const bool skip = before(unpack(last), best);
        __syncthreads();                                 // (`last` and the buffers are free again)
        if (skip) continue;
        if (t < Kp && before(run, cur)) cur = run;
        for (int j = Kp >> 1; j > 0; j >>= 1) exchange(cur, j, true, buf, flip);
    }
    if (t < K) {
        top_score[t] = __uint_as_float(cur.bits);
        top_shard[t] = cur.shard;
        top_mol[t] = cur.mol;
    }
}

inline size_t n_tiles_of(int32_t B) { return ((size_t)B + TOPK_TILE - 1) / TOPK_TILE; }

}  // namespace
}  // namespace mkgnn

using namespace mkgnn;

extern "C" size_t mkgnn_topk_tasks_workspace_bytes(int32_t B, int32_t K, int32_t T) {
    if (B < 1 || K < 1 || K > MKGNN_TOPK_MAX_K || T < 1 || T > MKGNN_TASK_HEAD_MAX_TASKS) return 0;
    const size_t tiles = n_tiles_of(B);
    return 256 + (tiles > 1 ? (size_t)T * tiles * (size_t)pow2_at_least(K) * sizeof(uint4) : 0);
}

extern "C" size_t mkgnn_topk_workspace_bytes(int32_t B, int32_t K) { return mkgnn_topk_tasks_workspace_bytes(B, K, 1); }

// the one launcher: T lists, the task on the grid's second dimension
static int topk_launch(const char* who, const float* scores, int64_t row_stride, int64_t task_stride, const int32_t* ids, int32_t B,
                       int32_t T, const int32_t* n_valid, const int32_t* shard_tag, int32_t K, float* top_score, int32_t* top_shard,
                       int32_t* top_mol, void* workspace, size_t workspace_bytes, void* stream) {
    if (!scores || !ids || !n_valid || !shard_tag || !top_score || !top_shard || !top_mol || !workspace)
        return api_fail("%s: null pointer", who);
    if (B < 1) return api_fail("%s: B = %d", who, (int)B);
    if (K < 1 || K > MKGNN_TOPK_MAX_K) return api_fail("%s: K = %d outside [1, %d]", who, (int)K, MKGNN_TOPK_MAX_K);
    if (T < 1 || T > MKGNN_TASK_HEAD_MAX_TASKS) return api_fail("%s: T = %d outside [1, %d]", who, (int)T, MKGNN_TASK_HEAD_MAX_TASKS);
    if (row_stride < 0 || task_stride < 0) return api_fail("%s: negative score stride", who);
    if ((uintptr_t)workspace % 16) return api_fail("%s: workspace must be 16-byte aligned", who);
    if (workspace_bytes < mkgnn_topk_tasks_workspace_bytes(B, K, T)) return api_fail("%s: workspace too small", who);
    const int32_t Kp = pow2_at_least(K);
    const int tiles = (int)n_tiles_of(B);
    uint4* const runs = (uint4*)((char*)workspace + 256);
    hipStream_t st = (hipStream_t)stream;
    if (tiles > 1) {
        topk_runs_kernel<<<dim3(tiles, T), TOPK_THREADS, 0, st>>>(scores, row_stride, task_stride, ids, B, n_valid, shard_tag, K, Kp, runs);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return api_hip_fail(who, e);
    }
    topk_merge_kernel<<<dim3(1, T), TOPK_THREADS, 0, st>>>(scores, row_stride, task_stride, ids, B, n_valid, shard_tag, K, Kp, top_score,
                                                           top_shard, top_mol, runs, tiles);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : api_hip_fail(who, e);
}

extern "C" int mkgnn_topk_update(const float* scores, const int32_t* ids, int32_t B, const int32_t* n_valid, const int32_t* shard_tag,
                                 int32_t K, float* top_score, int32_t* top_shard, int32_t* top_mol, void* workspace,
                                 size_t workspace_bytes, void* stream) {
    return topk_launch("mkgnn_topk_update", scores, 1, 0, ids, B, 1, n_valid, shard_tag, K, top_score, top_shard, top_mol, workspace,
                       workspace_bytes, stream);
}

extern "C" int mkgnn_topk_update_tasks(const float* scores, int64_t score_row_stride, int64_t score_task_stride, const int32_t* ids,
                                       int32_t B, int32_t T, const int32_t* n_valid, const int32_t* shard_tag, int32_t K,
                                       float* top_score, int32_t* top_shard, int32_t* top_mol, void* workspace,
                                       size_t workspace_bytes, void* stream) {
    return topk_launch("mkgnn_topk_update_tasks", scores, score_row_stride, score_task_stride, ids, B, T, n_valid, shard_tag, K,
                       top_score, top_shard, top_mol, workspace, workspace_bytes, stream);
}
