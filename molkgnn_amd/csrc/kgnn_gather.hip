// Gather-collate from a device-resident shard (mkgnn_gather_compact): an arbitrary list of molecules -- repeats allowed, order
// kept -- into the fixed-shape compact wire form, on the GPU.  molkgnn_amd/shards.py::gather_compact is the definition this is
// tested against, byte for byte.
//
// Two launches on the caller's stream, integers only, no atomics, no process-wide state:
//   gather_scan_kernel  ONE workgroup: per slot the molecule's atom / bond / per-degree counts (read through ids), exclusive
//                       prefix offsets and the slot's first source atom / bond into the workspace, the batch totals, and the
//                       small wire fields (y, mol_ptr, n_valid_atoms)
//   gather_fill_kernel  the grid: a wave owns 64 consecutive output rows (atoms, then bonds); every lane finds its row's slot
//                       by bisection of the offsets ONCE, then the wave copies the 64 rows together, lane after lane along the
//                       output, so the stores are contiguous and a molecule's rows are read in one run
// What the device finds wrong goes into the status word (workspace[0]); ids and extents are clamped, so nothing is read
// outside the shard or written outside the wire fields whatever the ids hold.
//
// mkgnn_gather_compact_packed is the same gather from a shard whose atom features are held as packed records
// (mkgnn_resident_shard_packed; molkgnn_amd/shards.py::pack_x / unpack_x define the form).  The scan kernel is the same kernel;
// the fill kernel differs in the x field of the atom half only, which it decodes column by column through the column table.
#include <cstdint>
#include "kgnn_launch.h"
#include "../../include/molkgnn_hip.h"

namespace mkgnn {
namespace {

// workspace (int32): header | atom_off [n + 1] | bond_off [n + 1] | src_atom [n] | src_bond [n]
constexpr int GWS_STATUS = 0, GWS_NA = 1, GWS_NB = 2, GWS_NPAD = 3, GWS_NEED = 4, GWS_HEAD = 16;
constexpr int SCAN_THREADS = 1024, SCAN_WAVES = SCAN_THREADS / 64;
constexpr int FILL_THREADS = 256, FILL_ROWS = FILL_THREADS;      // 4 waves x 64 rows

inline size_t up256(size_t v) { return (v + 255) / 256 * 256; }

struct GatherArgs {
    mkgnn_resident_shard s;
    const int32_t* ids;
    int32_t n;                      // slots
    int32_t A, B2;                  // atoms / bonds of the shape
    int32_t target[4];              // N_1 .. N_4 of the shape
    int32_t pad_molecules;
    int32_t vec_x, vec_p;           // rows of x / p copied in 16-byte pieces
    float* wx; float* wp; int32_t* wij; uint8_t* wattr; float* wy; int32_t* wmp; int64_t* wnva;
    int32_t* ws;
};

// the packed form of x: the table travels with the launch (the entry point has checked it), the kernel keeps it in LDS
struct PackedX {
    const uint32_t* rec;            // records, read in dwords
    int32_t rec_dwords;
    int32_t col[MKGNN_PACKED_MAX_X_DIM];
};

__device__ __forceinline__ int64_t min64(int64_t a, int64_t b) { return a < b ? a : b; }

__device__ __forceinline__ int64_t scan_up(int64_t v, int width) {       // inclusive scan over the first `width` lanes
    const int lane = threadIdx.x & 63;
    for (int d = 1; d < width; d <<= 1) {
        const int64_t up = __shfl_up(v, d, 64);
        if (lane >= d) v += up;
    }
    return v;
}

// inclusive scan of six counters over the workgroup's threads (thread order): the waves scan their lanes, then every wave scans
// the sixteen wave totals in its first lanes; `tot` receives the workgroup totals
__device__ __forceinline__ void block_scan6(int64_t v[6], int64_t tot[6], int64_t (*wave_sum)[6]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < 6; ++k) v[k] = scan_up(v[k], 64);
    if (lane == 63) {
#pragma unroll
        for (int k = 0; k < 6; ++k) wave_sum[wave][k] = v[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const int64_t w = scan_up(lane < SCAN_WAVES ? wave_sum[lane][k] : 0, SCAN_WAVES);
        const int64_t before = __shfl(w, wave > 0 ? wave - 1 : 0, 64);
        tot[k] = __shfl(w, SCAN_WAVES - 1, 64);
        if (wave > 0) v[k] += before;
    }
}

__global__ void __launch_bounds__(SCAN_THREADS) gather_scan_kernel(const GatherArgs a) {
    __shared__ int64_t wave_sum[SCAN_WAVES][6];
    const int t = threadIdx.x;
    const int64_t n = a.n, M = a.s.n_molecules;
    const int64_t chunk = (n + SCAN_THREADS - 1) / SCAN_THREADS;
    const int64_t s0 = min64(t * chunk, n), s1 = min64(s0 + chunk, n);
    int bad = 0;
    int64_t v[6] = {0, 0, 0, 0, 0, 0};                 // atoms, bonds, atoms of degree 1..4 of this thread's slots
    for (int64_t s = s0; s < s1; ++s) {
        int64_t id = a.ids[s];
        if (id < 0 || id >= M) { bad = 1; id = id < 0 ? 0 : M - 1; }
        v[0] += a.s.mol_atom_ptr[id + 1] - a.s.mol_atom_ptr[id];
        v[1] += a.s.mol_bond_ptr[id + 1] - a.s.mol_bond_ptr[id];
        const int4 d = *(const int4*)(a.s.mol_deg + 4 * id);
        v[2] += d.x; v[3] += d.y; v[4] += d.z; v[5] += d.w;
    }
    const int64_t mine[2] = {v[0], v[1]};
    int64_t tot[6];
    block_scan6(v, tot, wave_sum);
    bad = __syncthreads_or(bad);
    // second pass over the same slots: exclusive offsets (saturated at the shape's extents: what lies past them is not copied)
    int32_t* const atom_off = a.ws + GWS_HEAD;
    int32_t* const bond_off = atom_off + n + 1;
    int32_t* const src_atom = bond_off + n + 1;
    int32_t* const src_bond = src_atom + n;
    int64_t ao = v[0] - mine[0], bo = v[1] - mine[1];
    for (int64_t s = s0; s < s1; ++s) {
        int64_t id = a.ids[s];
        id = id < 0 ? 0 : (id >= M ? M - 1 : id);
        const int32_t a0 = a.s.mol_atom_ptr[id], b0 = a.s.mol_bond_ptr[id];
        atom_off[s] = (int32_t)min64(ao, a.A);
        bond_off[s] = (int32_t)min64(bo, a.B2);
        src_atom[s] = a0;
        src_bond[s] = b0;
        ao += a.s.mol_atom_ptr[id + 1] - a0;
        bo += a.s.mol_bond_ptr[id + 1] - b0;
        a.wy[s] = a.s.y[id];
        a.wmp[s + 1] = (int32_t)min64(ao, a.A);
    }
    // totals, the padding's closed forms and the fit of the shape
    const int64_t na = tot[0], nb = tot[1];
    int64_t need[4], n_pad = 0, stubs = 0;
    int misfit = 0;
    for (int d = 0; d < 4; ++d) {
        need[d] = (int64_t)a.target[d] - tot[2 + d];
        if (need[d] < 0) { misfit = 1; need[d] = 0; }
        n_pad += need[d];
        stubs += need[d] * (d + 1);
    }
    if (na + n_pad != a.A || (stubs & 1) || 2 * nb + stubs != 2 * (int64_t)a.B2) misfit = 1;
    const int64_t na_c = min64(na, a.A);
    // padding atom k belongs to padding molecule (k * pad_molecules) / n_pad: molecule q ends after ceil((q + 1) n_pad / pad) atoms
    for (int64_t q = t; q < a.pad_molecules; q += SCAN_THREADS) {
        const int64_t upto = ((q + 1) * n_pad + a.pad_molecules - 1) / a.pad_molecules;
        a.wmp[n + 1 + q] = (int32_t)min64(na_c + min64(upto, n_pad), a.A);
    }
    if (t == 0) {
        a.wmp[0] = 0;
        a.wnva[0] = na_c;
        atom_off[n] = (int32_t)na_c;
        bond_off[n] = (int32_t)min64(nb, a.B2);
        a.ws[GWS_STATUS] = (bad ? MKGNN_GATHER_BAD_ID : 0) | (misfit ? MKGNN_GATHER_MISFIT : 0);
        a.ws[GWS_NA] = (int32_t)na_c;
        a.ws[GWS_NB] = (int32_t)min64(nb, a.B2);
        for (int d = 0; d < 4; ++d) a.ws[GWS_NEED + d] = (int32_t)min64(need[d], a.A);
        a.ws[GWS_NPAD] = (int32_t)min64(n_pad, 4 * (int64_t)a.A);
    }
}

// the slot s in [0, n) with off[s] <= r < off[s + 1] (r < off[n]; empty slots are passed over)
__device__ __forceinline__ int find_slot(const int32_t* __restrict__ off, int n, int32_t r) {
    int lo = 0, hi = n;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (off[mid] <= r) lo = mid; else hi = mid;
    }
    return lo;
}

// 64 output rows [r0, r0 + 64) of `units` T each, copied by the wave: lane L holds the source row of output row r0 + L (-1: a
// zero row); piece j of the tile belongs to row j / units.  Every lane runs every trip (the shuffles need the whole wave).
template <typename T>
__device__ __forceinline__ void copy_rows(T* __restrict__ dst, const T* __restrict__ src, int units, int32_t r0, int32_t n_rows,
                                          int32_t src_row) {
    const int lane = threadIdx.x & 63;
    T* const out = dst + (size_t)r0 * units;
    for (int i = 0; i < units; ++i) {
        const int j = lane + 64 * i;
        const int row = j / units, c = j - row * units;
        const int32_t sr = __shfl(src_row, row, 64);
        T v{};
        if (sr >= 0) v = src[(size_t)sr * units + c];
        if (r0 + row < n_rows) out[j] = v;
    }
}

// the padding atom (0-based among the padding atoms) that owns bond stub s: the atoms come in degree order and an atom of
// degree d owns d consecutive stubs
__device__ __forceinline__ int64_t stub_atom(int64_t s, const int4 need) {
    const int64_t c1 = need.x, c2 = 2 * (int64_t)need.y, c3 = 3 * (int64_t)need.z, c4 = 4 * (int64_t)need.w;
    if (s < c1) return s;
    s -= c1;
    if (s < c2) return need.x + s / 2;
    s -= c2;
    if (s < c3) return (int64_t)need.x + need.y + s / 3;
    s -= c3;
    const int64_t n_pad = (int64_t)need.x + need.y + need.z + need.w;
    if (s < c4) return n_pad - need.w + s / 4;
    return n_pad > 0 ? n_pad - 1 : 0;
}

// column c of one record: an fp32 at byte offset e (e >= 0), or the int8 at byte offset -e - 1 (out of its dword by two shifts)
__device__ __forceinline__ float decode_column(const uint32_t* __restrict__ rec, int32_t e) {
    if (e >= 0) return __uint_as_float(rec[e >> 2]);
    const int off = -e - 1;
    const int32_t b = (int32_t)(rec[off >> 2] << (24 - 8 * (off & 3))) >> 24;
    return (float)b;
}

// copy_rows for x out of packed records: the same pieces in the same places (16-byte pieces when VEC), every element decoded
// through the column table `col` (LDS)
template <bool VEC>
__device__ __forceinline__ void decode_rows(float* __restrict__ dst, const PackedX& px, const int32_t* col, int x_dim, int32_t r0,
                                            int32_t n_rows, int32_t src_row) {
    const int lane = threadIdx.x & 63;
    const int units = VEC ? x_dim / 4 : x_dim;
    for (int i = 0; i < units; ++i) {
        const int j = lane + 64 * i;
        const int row = j / units, c = j - row * units;
        const int32_t sr = __shfl(src_row, row, 64);
        const uint32_t* const rec = px.rec + (size_t)(sr >= 0 ? sr : 0) * px.rec_dwords;
        if constexpr (VEC) {
            float4 v = {0.0f, 0.0f, 0.0f, 0.0f};
            if (sr >= 0) {
                v.x = decode_column(rec, col[4 * c]);
                v.y = decode_column(rec, col[4 * c + 1]);
                v.z = decode_column(rec, col[4 * c + 2]);
                v.w = decode_column(rec, col[4 * c + 3]);
            }
            if (r0 + row < n_rows) ((float4*)(dst + (size_t)r0 * x_dim))[j] = v;
        } else {
            float v = 0.0f;
            if (sr >= 0) v = decode_column(rec, col[c]);
            if (r0 + row < n_rows) dst[(size_t)r0 * x_dim + j] = v;
        }
    }
}

// the source atom of this lane's output row r0 + lane (-1: a padding row)
__device__ __forceinline__ int32_t source_atom(const GatherArgs& a, int32_t r0) {
    const int lane = threadIdx.x & 63;
    const int n = a.n;
    const int32_t* const atom_off = a.ws + GWS_HEAD;
    const int32_t* const src_atom = atom_off + 2 * (n + 1);
    const int32_t r = r0 + lane;
    int32_t sr = -1;
    if (r < a.ws[GWS_NA]) {
        const int s = find_slot(atom_off, n, r);
        sr = src_atom[s] + (r - atom_off[s]);
    }
    return sr;
}

__device__ __forceinline__ void copy_p_rows(const GatherArgs& a, int32_t r0, int32_t sr) {
    if (a.vec_p) copy_rows<float4>((float4*)a.wp, (const float4*)a.s.p, a.s.p_dim / 4, r0, a.A, sr);
    else copy_rows<float>(a.wp, a.s.p, a.s.p_dim, r0, a.A, sr);
}

__device__ __forceinline__ void fill_bond_tile(const GatherArgs& a, int atom_blocks) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n = a.n;
    const int32_t* const atom_off = a.ws + GWS_HEAD;
    const int32_t* const bond_off = atom_off + n + 1;
    const int32_t* const src_atom = bond_off + n + 1;
    const int32_t* const src_bond = src_atom + n;
    const int32_t na = a.ws[GWS_NA], nb = a.ws[GWS_NB];
    const int32_t b0 = (((int32_t)blockIdx.x - atom_blocks) * 4 + wave) * 64;
    if (b0 >= a.B2) return;
    const int32_t b = b0 + lane;
    int32_t sb = -1;                                     // source bond of this lane's output bond (-1: a padding bond)
    if (b < a.B2) {
        int2 ij;
        if (b < nb) {
            const int s = find_slot(bond_off, n, b);
            sb = src_bond[s] + (b - bond_off[s]);
            const int32_t shift = atom_off[s] - src_atom[s];
            ij = *(const int2*)(a.s.bond_ij + 2 * (size_t)sb);
            ij.x += shift; ij.y += shift;
        } else {
            const int4 need = *(const int4*)(a.ws + GWS_NEED);
            const int64_t s = 2 * (int64_t)(b - nb);
            ij.x = (int32_t)min64(na + stub_atom(s, need), a.A - 1);
            ij.y = (int32_t)min64(na + stub_atom(s + 1, need), a.A - 1);
        }
        ij.x = ij.x < a.A ? ij.x : a.A - 1;
        ij.y = ij.y < a.A ? ij.y : a.A - 1;
        *(int2*)(a.wij + 2 * (size_t)b) = ij;
    }
    // attribute bytes of the tile's 64 bonds: 16 * e_dim dwords, one per lane and trip, each put together from four bytes (of up
    // to four bonds); the last dword of the field may be a partial one
    const int E = a.s.e_dim;
    const size_t field = (size_t)a.B2 * E;
    uint8_t* const out = a.wattr + (size_t)b0 * E;
    const size_t left = field - (size_t)b0 * E;          // bytes of the field from this tile's first on
    for (int i = 0; i * 64 < 16 * E; ++i) {
        const int q = lane + 64 * i;
        uint32_t word = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int byte = (4 * q + k) < 64 * E ? 4 * q + k : 64 * E - 1;
            const int bond = byte / E, col = byte - bond * E;
            const int32_t src = __shfl(sb, bond, 64);
            uint32_t v = col == 0 ? 1u : 0u;
            if (src >= 0) v = a.s.bond_attr[(size_t)src * E + col];
            word |= v << (8 * k);
        }
        if (q < 16 * E) {
            const size_t at = 4 * (size_t)q;
            if (at + 4 <= left) *(uint32_t*)(out + at) = word;
            else
                for (int k = 0; k < 4; ++k)
                    if (at + k < left) out[at + k] = (uint8_t)(word >> (8 * k));
        }
    }
}

__global__ void __launch_bounds__(FILL_THREADS) gather_fill_kernel(const GatherArgs a, int atom_blocks) {
    if ((int)blockIdx.x >= atom_blocks) { fill_bond_tile(a, atom_blocks); return; }
    const int32_t r0 = ((int32_t)blockIdx.x * 4 + (int32_t)(threadIdx.x >> 6)) * 64;
    if (r0 >= a.A) return;
    const int32_t sr = source_atom(a, r0);
    if (a.vec_x) copy_rows<float4>((float4*)a.wx, (const float4*)a.s.x, a.s.x_dim / 4, r0, a.A, sr);
    else copy_rows<float>(a.wx, a.s.x, a.s.x_dim, r0, a.A, sr);
    copy_p_rows(a, r0, sr);
}

// the same grid for a packed shard: a.s.x is null, x comes out of px
__global__ void __launch_bounds__(FILL_THREADS) gather_fill_packed_kernel(const GatherArgs a, int atom_blocks, const PackedX px) {
    if ((int)blockIdx.x >= atom_blocks) { fill_bond_tile(a, atom_blocks); return; }
    __shared__ int32_t col[MKGNN_PACKED_MAX_X_DIM];
    if ((int)threadIdx.x < a.s.x_dim) col[threadIdx.x] = px.col[threadIdx.x];
    __syncthreads();
    const int32_t r0 = ((int32_t)blockIdx.x * 4 + (int32_t)(threadIdx.x >> 6)) * 64;
    if (r0 >= a.A) return;
    const int32_t sr = source_atom(a, r0);
    if (a.vec_x) decode_rows<true>(a.wx, px, col, a.s.x_dim, r0, a.A, sr);
    else decode_rows<false>(a.wx, px, col, a.s.x_dim, r0, a.A, sr);
    copy_p_rows(a, r0, sr);
}

}  // namespace
}  // namespace mkgnn

using namespace mkgnn;

extern "C" size_t mkgnn_gather_compact_workspace_bytes(int64_t n_ids) {
    if (n_ids < 0) return 0;
    return up256(((size_t)GWS_HEAD + 4 * (size_t)n_ids + 2) * sizeof(int32_t));
}

// the checks, the wire fields and the two launches of both entry points; px: the packed form of x (s->x is not used), or null
static int gather_launch(const char* who, const mkgnn_resident_shard* s, const PackedX* px, const int32_t* ids, int64_t n_ids,
                         const int64_t shape[6], int32_t pad_molecules, void* wire, size_t wire_bytes, void* workspace, void* stream) {
    if (!ids || !shape || !wire || !workspace) return api_fail("%s: null pointer", who);
    if ((!px && !s->x) || !s->p || !s->bond_ij || !s->y || !s->mol_atom_ptr || !s->mol_bond_ptr || !s->mol_deg)
        return api_fail("%s: a shard array is null", who);
    if (s->n_molecules < 1 || s->x_dim < 1 || s->p_dim < 1 || s->e_dim < 0 || (s->e_dim && !s->bond_attr))
        return api_fail("%s: empty shard or bad feature widths", who);
    if (n_ids < 1 || n_ids >= (1ll << 30)) return api_fail("%s: %lld ids", who, (long long)n_ids);
    if (pad_molecules < 0) return api_fail("%s: negative pad_molecules", who);
    for (int k = 0; k < 6; ++k)
        if (shape[k] < 0 || shape[k] >= (1ll << 31)) return api_fail("%s: shape[%d] = %lld", who, k, (long long)shape[k]);
    if (shape[0] < 1 || shape[1] % 2) return api_fail("%s: the shape holds no atom or an odd number of directed edges", who);
    if ((uintptr_t)wire % 256 || (uintptr_t)workspace % 16 || (uintptr_t)s->mol_deg % 16 || (uintptr_t)s->bond_ij % 8)
        return api_fail("%s: wire must be 256-byte aligned, workspace and mol_deg 16-byte, bond_ij 8-byte", who);
    if (wire_bytes < mkgnn_collate_compact_bytes(shape, n_ids, pad_molecules, s->x_dim, s->p_dim, s->e_dim))
        return api_fail("%s: wire buffer too small", who);
    GatherArgs a;
    a.s = *s; a.ids = ids; a.n = (int32_t)n_ids;
    a.A = (int32_t)shape[0]; a.B2 = (int32_t)(shape[1] / 2);
    for (int d = 0; d < 4; ++d) a.target[d] = (int32_t)shape[2 + d];
    a.pad_molecules = pad_molecules;
    a.vec_x = s->x_dim % 4 == 0 && (px || (uintptr_t)s->x % 16 == 0);
    a.vec_p = s->p_dim % 4 == 0 && (uintptr_t)s->p % 16 == 0;
    const size_t A = (size_t)a.A, B2 = (size_t)a.B2, G = (size_t)n_ids + (size_t)pad_molecules;
    char* o = (char*)wire;
    a.wx = (float*)o;        o += up256(A * s->x_dim * 4);
    a.wp = (float*)o;        o += up256(A * s->p_dim * 4);
    a.wij = (int32_t*)o;     o += up256(B2 * 2 * 4);
    a.wattr = (uint8_t*)o;   o += up256(B2 * s->e_dim);
    a.wy = (float*)o;        o += up256((size_t)n_ids * 4);
    a.wmp = (int32_t*)o;     o += up256((G + 1) * 4);
    a.wnva = (int64_t*)o;
    a.ws = (int32_t*)workspace;
    hipStream_t st = (hipStream_t)stream;
    gather_scan_kernel<<<1, SCAN_THREADS, 0, st>>>(a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return api_hip_fail(px ? "mkgnn_gather_compact_packed: scan launch" : "mkgnn_gather_compact: scan launch", e);
    const int atom_blocks = (int)((A + FILL_ROWS - 1) / FILL_ROWS), bond_blocks = (int)((B2 + FILL_ROWS - 1) / FILL_ROWS);
    if (px) gather_fill_packed_kernel<<<atom_blocks + bond_blocks, FILL_THREADS, 0, st>>>(a, atom_blocks, *px);
    else gather_fill_kernel<<<atom_blocks + bond_blocks, FILL_THREADS, 0, st>>>(a, atom_blocks);
    e = hipGetLastError();
    return e == hipSuccess ? 0 : api_hip_fail(px ? "mkgnn_gather_compact_packed: fill launch" : "mkgnn_gather_compact: fill launch", e);
}

extern "C" int mkgnn_gather_compact(const mkgnn_resident_shard* s, const int32_t* ids, int64_t n_ids, const int64_t shape[6],
                                    int32_t pad_molecules, void* wire, size_t wire_bytes, void* workspace, void* stream) {
    const char* who = "mkgnn_gather_compact";
    if (!s) return api_fail("%s: null pointer", who);
    return gather_launch(who, s, nullptr, ids, n_ids, shape, pad_molecules, wire, wire_bytes, workspace, stream);
}

extern "C" int mkgnn_gather_compact_packed(const mkgnn_resident_shard_packed* s, const int32_t* ids, int64_t n_ids,
                                           const int64_t shape[6], int32_t pad_molecules, void* wire, size_t wire_bytes,
                                           void* workspace, void* stream) {
    const char* who = "mkgnn_gather_compact_packed";
    if (!s) return api_fail("%s: null pointer", who);
    if (!s->x_rec || !s->x_col) return api_fail("%s: a shard array is null", who);
    if (s->x_dim < 1 || s->x_dim > MKGNN_PACKED_MAX_X_DIM)
        return api_fail("%s: x_dim = %d, a packed shard holds 1 .. %d columns", who, (int)s->x_dim, MKGNN_PACKED_MAX_X_DIM);
    if ((uintptr_t)s->x_rec % 4) return api_fail("%s: x_rec must be 4-byte aligned (the records are read in dwords)", who);
    // the table against the record: every entry inside it, floats on dword boundaries, and the record exactly as long as the
    // layout makes it (nf floats, nq bytes, padded to a dword)
    PackedX px;
    int nf = 0, nq = 0;
    for (int c = 0; c < s->x_dim; ++c) {
        const int32_t e = s->x_col[c];
        if (e >= 0) {
            if (e % 4 || (int64_t)e + 4 > s->rec_bytes) return api_fail("%s: x_col[%d] = %d: no fp32 of the record", who, c, (int)e);
            ++nf;
        } else {
            if (-(int64_t)e - 1 >= s->rec_bytes) return api_fail("%s: x_col[%d] = %d: no byte of the record", who, c, (int)e);
            ++nq;
        }
        px.col[c] = e;
    }
    for (int c = s->x_dim; c < MKGNN_PACKED_MAX_X_DIM; ++c) px.col[c] = 0;
    if (s->rec_bytes != 4 * nf + 4 * ((nq + 3) / 4))
        return api_fail("%s: rec_bytes = %d, the table's %d fp32 and %d int8 columns make %d", who, (int)s->rec_bytes, nf, nq,
                        4 * nf + 4 * ((nq + 3) / 4));
    px.rec = (const uint32_t*)s->x_rec;
    px.rec_dwords = s->rec_bytes / 4;
    mkgnn_resident_shard u;
    u.x = nullptr; u.p = s->p; u.bond_ij = s->bond_ij; u.bond_attr = s->bond_attr; u.y = s->y;
    u.mol_atom_ptr = s->mol_atom_ptr; u.mol_bond_ptr = s->mol_bond_ptr; u.mol_deg = s->mol_deg;
    u.n_molecules = s->n_molecules; u.x_dim = s->x_dim; u.p_dim = s->p_dim; u.e_dim = s->e_dim; u.reserved = 0;
    return gather_launch(who, &u, &px, ids, n_ids, shape, pad_molecules, wire, wire_bytes, workspace, stream);
}
