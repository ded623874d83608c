// The connected components of a graph given as CSR neighbour lists (mkgnn_graph_components): the single-linkage clusters of a
// similarity threshold, when the lists are mkgnn_embed_neighbours_within's self-join.
//
//     labels[v] = the smallest vertex of v's component; u and v are linked if col holds v in u's segment OR u in v's
//
// HOOK AND COMPRESS, in rounds of two launches over three arrays -- A (= labels) and two copies in the workspace, B and C:
//   hook      every stored edge (u, v): the parents A[u], A[v] of the PREVIOUS round -- roots, after its compression -- and an
//             atomicMin of the larger root's entry of the copy T down to the smaller root.  A is only read: a snapshot.  T == A
//             when the round begins; the atomics' order does not matter, every entry ends at the minimum of what was offered
//   compress  every vertex follows T from its entry to a root (parents only decrease: no cycles; T is only read) and writes that
//             root to A and to the OTHER copy, which is the next round's T
// The fixpoint is unique -- every vertex at its component's minimum -- so the result is deterministic.  A call enqueues a FIXED
// number of rounds, 2 ceil(log2 max(n, 2)) + 1 (DESIGN.md 4.5l has the argument), without a host round trip: changed[k] is set by
// round k's hook when an atomicMin lowered an entry; the compress of a round that changed nothing and every launch behind it
// return at once.  Correctness does not rest on the number: state[1] says whether the last round changed nothing, and a call with
// resume = 1 goes on from the labels that are there.
//
// NOTHING IS INDEXED WITH WHAT THE INPUT HOLDS UNCHECKED: a segment is walked only if 0 <= row_ptr[u] <= row_ptr[u + 1] <= row_ptr[n],
// an edge is used only if 0 <= col[e] < n, a label taken over by resume = 1 only if 0 <= labels[v] <= v (else v); anything else is
// skipped and reported in state[2].
#include <hip/hip_runtime.h>
#include <cstdint>
#include "kgnn_common.h"
#include "kgnn_launch.h"
#include "../../include/molkgnn_hip.h"

namespace mkgnn {
namespace {

constexpr int CC_BLOCK = 256;
constexpr int CC_LANES = 16;                   // lanes per vertex of the hook: a quarter wave strides over the segment
constexpr int CC_MAX_ROUNDS = 63;              // 2 * 31 + 1
constexpr int CC_FLAGS = 72;                   // changed[CC_MAX_ROUNDS], then the bad-input flag; padded

inline int cc_rounds(int n) {
    int lg = 0;
    while (((int64_t)1 << lg) < (n < 2 ? 2 : n)) ++lg;
    return 2 * lg + 1;
}

__global__ void cc_clear_kernel(int32_t* __restrict__ flags) {
    if (threadIdx.x < CC_FLAGS) flags[threadIdx.x] = 0;
}

// B[v] = v, or on resume the label that is there if it can be one (a vertex no larger than v)
__global__ void __launch_bounds__(CC_BLOCK) cc_init_kernel(const int32_t* __restrict__ labels, int n, int resume,
                                                           int32_t* __restrict__ B, int32_t* __restrict__ bad) {
    const int64_t v = (int64_t)blockIdx.x * CC_BLOCK + threadIdx.x;
    if (v >= n) return;
    int l = (int)v;
    if (resume) {
        const int had = labels[v];
        if (had >= 0 && had <= l) l = had; else *bad = 1;
    }
    B[v] = l;
}

// gate: the flag of this round's hook (null: run); T is only read, A and the other copy N are written
__global__ void __launch_bounds__(CC_BLOCK) cc_compress_kernel(const int32_t* __restrict__ gate, const int32_t* __restrict__ T, int n,
                                                               int32_t* __restrict__ A, int32_t* __restrict__ N) {
    if (gate && *gate == 0) return;
    const int64_t v = (int64_t)blockIdx.x * CC_BLOCK + threadIdx.x;
    if (v >= n) return;
    int p = T[v];
    for (int q = T[p]; q != p; q = T[p]) p = q;                  // (every entry of T is a vertex no larger than its index)
    A[v] = p;
    N[v] = p;
}

// gate: the flag of the round before (null: the first round); A is only read, T takes the atomics
__global__ void __launch_bounds__(CC_BLOCK) cc_hook_kernel(const int32_t* __restrict__ gate, const int64_t* __restrict__ row_ptr,
                                                           const int32_t* __restrict__ col, int n, const int32_t* __restrict__ A,
                                                           int32_t* __restrict__ T, int32_t* __restrict__ changed,
                                                           int32_t* __restrict__ bad) {
    if (gate && *gate == 0) return;
    const int64_t t = (int64_t)blockIdx.x * CC_BLOCK + threadIdx.x;
    const int64_t u = t / CC_LANES;
    const int lane = (int)(t % CC_LANES);
    if (u >= n) return;
    const int64_t beg = row_ptr[u], end = row_ptr[u + 1], nnz = row_ptr[n];
    if (beg < 0 || end < beg || end > nnz) {
        if (lane == 0) *bad = 1;
        return;
    }
    const int ru = A[u];
    for (int64_t e = beg + lane; e < end; e += CC_LANES) {
        const int v = col[e];
        if (v < 0 || v >= n) { *bad = 1; continue; }
        const int rv = A[v];
        if (rv == ru) continue;
        const int hi = max(ru, rv), lo = min(ru, rv);
        if (atomicMin(&T[hi], lo) > lo) *changed = 1;
    }
}

__global__ void cc_finish_kernel(const int32_t* __restrict__ flags, int rounds, int32_t* __restrict__ state) {
    if (threadIdx.x != 0) return;
    int changing = 0;
    for (int k = 0; k < rounds; ++k) changing += flags[k] != 0 ? 1 : 0;
    state[0] = changing;
    state[1] = (rounds == 0 || flags[rounds - 1] == 0) ? 1 : 0;
    state[2] = flags[CC_MAX_ROUNDS] != 0 ? 1 : 0;
    state[3] = 0;
}

}  // namespace
}  // namespace mkgnn

using namespace mkgnn;

// [B: n int32][C: n int32][changed: one int32 per round, the bad-input flag: 72 int32]
extern "C" size_t mkgnn_graph_components_workspace_bytes(int32_t n) {
    if (n < 0 || n > MKGNN_COMPONENTS_MAX_VERTICES) return 0;
    return sizeof(int32_t) * (2 * (size_t)n + CC_FLAGS);
}

extern "C" int mkgnn_graph_components(const int64_t* row_ptr, const int32_t* col, int32_t n, int32_t* labels, int32_t* state,
                                      int32_t resume, int32_t* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "mkgnn_graph_components";
    if (n < 0 || n > MKGNN_COMPONENTS_MAX_VERTICES)
        return api_fail("%s: %d vertices outside [0, %d]", who, (int)n, MKGNN_COMPONENTS_MAX_VERTICES);
    const int cap = (int)(resume >> 8);                          // (diagnostics: fewer rounds than the bound, for the tests of resume)
    if (resume < 0 || (resume & 0xff) > 1 || cap > CC_MAX_ROUNDS) return api_fail("%s: resume = %d is neither 0 nor 1", who, (int)resume);
    if (!state || !workspace || !row_ptr || (n > 0 && !labels)) return api_fail("%s: null pointer", who);
    const size_t need = mkgnn_graph_components_workspace_bytes(n);
    if (workspace_bytes < need) return api_fail("%s: workspace of %zu bytes, %zu needed", who, workspace_bytes, need);
    if (((uintptr_t)workspace & 3) != 0) return api_fail("%s: workspace not 4-byte aligned", who);
    const Span wr[3] = {{labels, (size_t)n * 4}, {state, 16}, {workspace, need}};
    const Span rd = {row_ptr, ((size_t)n + 1) * 8};
    if (spans_disjoint(who, wr, 3, &rd, 1, "an output (labels, state, workspace) aliases row_ptr",
                       "labels, state and the workspace alias each other"))
        return 1;
    const hipStream_t st = (hipStream_t)stream;
    int32_t *B = workspace, *C = workspace + n, *flags = workspace + 2 * (size_t)n;
    const int full = cc_rounds(n), rounds = n == 0 ? 0 : (cap > 0 && cap < full ? cap : full);
    const unsigned vertex_blocks = (unsigned)(((int64_t)n + CC_BLOCK - 1) / CC_BLOCK);
    const unsigned edge_blocks = (unsigned)(((int64_t)n * CC_LANES + CC_BLOCK - 1) / CC_BLOCK);
    cc_clear_kernel<<<1, 128, 0, st>>>(flags);                   // (a launch: a hipMemsetAsync here left the flags uncleared when a captured graph was replayed)
    if (n > 0) {
        cc_init_kernel<<<vertex_blocks, CC_BLOCK, 0, st>>>(labels, n, resume & 1, B, flags + CC_MAX_ROUNDS);
        cc_compress_kernel<<<vertex_blocks, CC_BLOCK, 0, st>>>(nullptr, B, n, labels, C);
    }
    int32_t *T = C, *other = B;
    for (int k = 0; k < rounds; ++k) {
        cc_hook_kernel<<<edge_blocks, CC_BLOCK, 0, st>>>(k ? flags + k - 1 : nullptr, row_ptr, col, n, labels, T, flags + k,
                                                         flags + CC_MAX_ROUNDS);
        cc_compress_kernel<<<vertex_blocks, CC_BLOCK, 0, st>>>(flags + k, T, n, labels, other);
        int32_t* swap = T; T = other; other = swap;
    }
    cc_finish_kernel<<<1, 64, 0, st>>>(flags, rounds, state);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : api_hip_fail(who, e);
}
