// What the fused tail's middle kernels share (kgnn_tail.hip: training and forward-only forms; kgnn_tail_mc.hip: the Monte Carlo
// dropout form): the chunk capacities, the LDS pitches and the device helpers of the per-atom and per-molecule phases.  Moved
// here unchanged from kgnn_tail.hip, so that every instantiation there keeps its statements.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "kgnn_common.h"
#include "kgnn_philox.h"
#include "../../include/molkgnn_hip.h"

namespace mkgnn {
namespace tail {

constexpr int NT = 256;                 // threads per workgroup: 8 row slots x 32 hidden lanes
constexpr int AC = MKGNN_TAIL_MAX_ATOMS, EC = MKGNN_TAIL_MAX_EDGES, MC = 12;      // chunk capacity: atoms, edges (each way), molecules
constexpr int MG_MIN = 1, MG_MAX = 8;   // molecules per group (the unit of work distribution): tail_group_size below
constexpr int HP = 36;                  // LDS pitch of the 32-wide rows: 16-byte aligned rows, 4 banks apart
constexpr int WP = 33;                  // ... of W2's rows (read one float per lane: odd, conflict-free)
typedef mkgnn_f32x4 f32x4;

// (sigmoidf_, the sigmoid on the transcendental unit: kgnn_sigmoid.h -- shared with kgnn_atom_contrib.hip)
__device__ __forceinline__ float half_sum(float v) {       // xor tree over the 32 lanes of a row slot
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float lane_of(float v, int k) { return __shfl(v, (int)(threadIdx.x & 32) | k, 64); }    // lane k of my row slot

// out[u] = sum over the edges of atom at0 + 32 u of rows[col][4 l .. 4 l + 3]  (rp: local edge offsets, ec: local atom of every
// edge, -1 = none; a thread is (atom slot, lane l of 8): 16 bytes of a 32-wide row).  The first four edges of all NA atoms in
// one batch of reads -- offsets, then columns, then rows -- and a serial tail for the rare atom with more (atoms outside the
// degree buckets); an atom beyond A contributes nothing.  Fixed order: edge by edge.
template <int NA>
__device__ __forceinline__ void gather_rows(const int* rp, const int* ec, const float* rows, int at0, int A, int l, f32x4 (&out)[NA]) {
    int lo[NA], hi[NA], col[NA][4];
#pragma unroll
    for (int u = 0; u < NA; ++u) {
        const int at = at0 + 32 * u, ac = at < A ? at : max(A - 1, 0);
        lo[u] = rp[ac]; hi[u] = at < A ? rp[ac + 1] : lo[u];
    }
#pragma unroll
    for (int u = 0; u < NA; ++u)
#pragma unroll
        for (int k = 0; k < 4; ++k) col[u][k] = ec[lo[u] + k < hi[u] ? lo[u] + k : (hi[u] > lo[u] ? lo[u] : 0)];
    f32x4 v[NA][4];
#pragma unroll
    for (int u = 0; u < NA; ++u)
#pragma unroll
        for (int k = 0; k < 4; ++k) v[u][k] = *(const f32x4*)(rows + ((unsigned)col[u][k] < (unsigned)A ? col[u][k] : 0) * HP + 4 * l);
#pragma unroll
    for (int u = 0; u < NA; ++u) {
        f32x4 s = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < 4; ++k) if (lo[u] + k < hi[u] && col[u][k] >= 0) s += v[u][k];
        for (int e = lo[u] + 4; e < hi[u]; ++e) { const int c = ec[e]; if (c >= 0) s += *(const f32x4*)(rows + c * HP + 4 * l); }
        out[u] = s;
    }
}

// the readout's keep multipliers of hidden units 4 l .. 4 l + 3 of batch atom `atom` (kgnn_philox.h; 1 at and beyond H)
__device__ __forceinline__ void readout_keep4(uint64_t seed, uint64_t offset, int64_t atom, int H, int l, float p, float (&ks)[4]) {
    if ((H & 3) == 0 && 4 * l < H) {                     // (H = 32: always -- a 4-aligned element, one Philox block)
        keep_scale4_of(seed, offset, readout_drop_element(atom, H, 4 * l), p, ks);
        return;
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) ks[c] = 4 * l + c < H ? keep_scale_of(seed, offset, readout_drop_element(atom, H, 4 * l + c), p) : 1.f;
}

// LDS of the forward-only forms: no pre / d pre rows, no per-molecule gradient rows, nothing by source (26 236 bytes against the
// training form's 52 468)
constexpr int LDS_FLOATS_FWD = 32 * WP + AC * HP + 96;
constexpr int LDS_INTS_FWD = AC + (AC + 1) + EC + 2 * (MC + 1) + 4;

}  // namespace tail
}  // namespace mkgnn
