// The order of include/molkgnn_hip.h's ranked lists, ONCE: kgnn_topk.hip, kgnn_exemplars.hip and kgnn_knn.hip promise their results --
// and each other's -- bit for bit against molkgnn_amd/screening.py::topk_update_reference, so they compile the order from this text.
//
// An entry is (score bits, shard, trailing keys); entries compare lexicographically on unsigned words, smaller = earlier: the score's
// rank (score_rank), the shard (signed, ascending), then the file's own trailing keys (mol, pos / mol, atom, pos / mol) -- integer
// comparisons only.  An EMPTY slot holds RANK_EMPTY_BITS (-inf) and -1 in every id field; which fields those are is the file's own,
// so the emptiness test is passed in (a true -inf score with real ids ranks as the number it is).  Each file keeps its own Entry
// struct (dwords only) and `before`; the wave-level pieces are templated on that struct and cost one shuffle per dword, in field order.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace mkgnn {

constexpr uint32_t RANK_EMPTY_BITS = 0xFF800000u;            // the score bits of an empty slot

// the score's rank as an unsigned key, smaller = earlier: non-NaN scores descending (-0.0 as +0.0), then NaN, then an empty slot
// (bits by reference, as the entries themselves are passed: by value the compiler spells the last line as an xor with 0x7FFFFFFF --
// the same value, but the kernels' code stays what it was only with the reference)
__device__ __forceinline__ uint32_t score_rank(const uint32_t& bits, bool is_empty) {
    if (is_empty) return 0xFFFFFFFFu;
    if ((bits & 0x7FFFFFFFu) > 0x7F800000u) return 0xFFFFFFFEu;
    const uint32_t b = bits == 0x80000000u ? 0u : bits;
    return (b & 0x80000000u) ? b : ~(b | 0x80000000u);            // = ~(the ascending key): +inf -> 0x007FFFFF, -inf -> RANK_EMPTY_BITS
}

// a signed id as an unsigned word of the same order; the high key of every list's order: (rank of the score, shard)
__device__ __forceinline__ uint32_t ordered(int32_t x) { return (uint32_t)x ^ 0x80000000u; }
__device__ __forceinline__ uint64_t rank_shard_key(uint32_t rank, int32_t shard) { return ((uint64_t)rank << 32) | ordered(shard); }

// a list of K slots travels through the networks as Kp = the next power of two
inline int32_t pow2_at_least(int32_t k) { int32_t p = 1; while (p < k) p <<= 1; return p; }

// the entry of lane `from` (its low six bits), in every lane of the wave
template <typename Entry>
__device__ __forceinline__ Entry lane_entry(const Entry& e, int from) {
    static_assert(sizeof(Entry) % 4 == 0, "an entry is whole dwords");
    constexpr int N = sizeof(Entry) / 4;
    int w[N];
    __builtin_memcpy(w, &e, sizeof(Entry));
#pragma unroll
    for (int i = 0; i < N; ++i) w[i] = __shfl(w[i], from, 64);
    Entry o;
    __builtin_memcpy(&o, w, sizeof(Entry));
    return o;
}

// one compare-exchange stage inside a wave: lane l and lane l ^ j (0 < j < 64); the lane whose bit j is clear keeps the earlier entry
// when `up`.  The file's `before(const Entry&, const Entry&)` is found at the call
template <typename Entry>
__device__ __forceinline__ void wave_exchange(Entry& e, int lane, int j, bool up) {
    const Entry o = lane_entry(e, lane ^ j);
    const bool keep_first = ((lane & j) == 0) == up;
    if (before(o, e) == keep_first) e = o;
}

// a bitonic sequence of n entries (n a power of two <= 64, in every aligned group of n lanes) -> ascending
template <typename Entry>
__device__ __forceinline__ void wave_merge_stages(Entry& e, int lane, int n) {
    for (int j = n >> 1; j > 0; j >>= 1) wave_exchange(e, lane, j, true);
}

}  // namespace mkgnn
