// C ABI of libmolkgnn_hip.so (include/molkgnn_hip.h): argument checks, workspace
// carving and kernel launches.  No allocation, no synchronisation.
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <mutex>

#include "kgnn_launch.h"
#include "kgnn_split.h"

using namespace mkgnn;

static thread_local char g_err[512] = "";

namespace mkgnn {
int api_fail(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return 1;
}
int api_hip_fail(const char* what, hipError_t e) { return api_fail("%s: %s", what, hipGetErrorString(e)); }
int spans_disjoint(const char* who, const Span* writes, int n_writes, const Span* reads, int n_reads, const char* reads_text,
                   const char* writes_text) {
    // Every pair is looked at and the conflict that begins at the LOWEST address is the one reported (among equals the first in the
    // order: write i against the reads, then against the writes behind it).  A buffer that starts inside another one and runs on past
    // its end is then reported against the one it starts in, whatever the allocator happened to place behind that.
    auto overlap_start = [](const Span& x, const Span& y) -> const char* {
        const char *xp = (const char*)x.p, *yp = (const char*)y.p;
        return x.n && y.n && xp < yp + y.n && yp < xp + x.n ? (xp > yp ? xp : yp) : nullptr;
    };
    const char *first = nullptr, *text = nullptr;
    for (int i = 0; i < n_writes; ++i) {
        for (int j = 0; j < n_reads; ++j) {
            const char* at = overlap_start(writes[i], reads[j]);
            if (at && (!first || at < first)) { first = at; text = reads_text; }
        }
        for (int j = i + 1; j < n_writes; ++j) {
            const char* at = overlap_start(writes[i], writes[j]);
            if (at && (!first || at < first)) { first = at; text = writes_text; }
        }
    }
    return first ? api_fail("%s: %s", who, text) : 0;
}
}  // namespace mkgnn

// The four degree buckets are independent.  At the batch sizes a molecule model sees, one bucket
// does not fill 256 CUs for long (a few atom tiles per SIMD, and prologue/tail dominate), so the
// per-degree kernels of one call run concurrently on three helper streams forked from and joined
// back into the caller's stream with events (a fork/join that hipGraph capture records as is).
// Streams and events are created once per device on first use.
struct DegreeStreams {
    hipStream_t aux[3];
    hipEvent_t fork;
    hipEvent_t join[3];
    bool ready;
    bool deferred;      // aux[0] carries bank-gradient chains nobody has joined yet (MKGNN_BACKWARD_DEFER_BANK)
    std::once_flag once;
};
static DegreeStreams g_streams[16];

// Created once per device under std::call_once (two host threads making their first call on one device do not race on
// the table).  The fork / join events are per device: the header's threading rule -- one host thread per device inside
// the backward call at a time -- is what keeps two callers from recording the same event.
static DegreeStreams* degree_streams() {
    if (switches().serial) return nullptr;               // diagnostics: keep everything on one stream
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) return nullptr;
    DegreeStreams& p = g_streams[dev];
    std::call_once(p.once, [&p]() {
        bool ok = true;
        // MKGNN_HELPER_PRIORITY (diagnostics): "low" / "high" = the helpers at the least / greatest stream priority
        int least = 0, greatest = 0;
        const char env_prio = switches().helper_priority;
        const bool ranged = env_prio && hipDeviceGetStreamPriorityRange(&least, &greatest) == hipSuccess;
        const int prio = (ranged && env_prio == 'l') ? least : ((ranged && env_prio == 'h') ? greatest : 0);
        for (int i = 0; i < 3 && ok; ++i) {
            ok = ((ranged && prio != 0) ? hipStreamCreateWithPriority(&p.aux[i], hipStreamNonBlocking, prio)
                                        : hipStreamCreateWithFlags(&p.aux[i], hipStreamNonBlocking)) == hipSuccess &&
                 hipEventCreateWithFlags(&p.join[i], hipEventDisableTiming) == hipSuccess;
        }
        ok = ok && hipEventCreateWithFlags(&p.fork, hipEventDisableTiming) == hipSuccess;
        p.ready = ok;
    });
    return p.ready ? &p : nullptr;
}

// Stream on which degree slot `i` (0 = most work) runs; slot 0 stays on the caller's stream.
struct ForkJoin {
    DegreeStreams* p;
    hipStream_t main;
    bool used[3];
    // Inside a hipGraph capture: ONE helper stream.  The x-gradient chain (rows kernels of the four degrees, then
    // the gather) stays on the caller's stream, the bank-gradient chain (bank kernels, then the reduce) runs on the
    // helper; they share nothing until the join.  Replayed graphs pay ~25 us per extra branch: one branch gains
    // (1.575 -> 1.518 ms per step), two more lose (1.634 ms), one per degree lost more.  MKGNN_FORK_MODE=0 disables it.
    bool two_way = false;
    hipError_t begin(hipStream_t st, bool enable) {
        // inside a hipGraph capture the buckets stay on the one captured stream: replayed graphs ran the
        // forked branches slower than the plain chain (measured 1.41 M vs 1.59 M molecules/s)
        hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
        const bool fork_in_graph = switches().fork_in_graph;                            // diagnostics: re-measure that choice
        const bool capturing = hipStreamIsCapturing(st, &cap) == hipSuccess && cap != hipStreamCaptureStatusNone;
        if (enable && capturing && switches().fork_mode && !fork_in_graph) two_way = true;
        else if (enable && !fork_in_graph && capturing) enable = false;
        main = st; p = enable ? degree_streams() : nullptr;
        used[0] = used[1] = used[2] = false;
        if (!p) return hipSuccess;
        // (inside a capture the fork point is recorded where the helper is first needed: a fork here, ahead of the pre-pass,
        // would give the kernel before it a second child in the graph -- a cross-stream edge costs the caller's chain ~5 us --
        // and the helper's kernels all follow the re-fork behind the pre-pass anyway)
        return two_way ? hipSuccess : hipEventRecord(p->fork, main);
    }
    hipStream_t stream(int slot, hipError_t* e) {
        *e = hipSuccess;
        if (!p || slot == 0) return main;
        const int i = slot - 1;
        if (!used[i]) {
            if (two_way) *e = hipEventRecord(p->fork, main);
            if (*e == hipSuccess) *e = hipStreamWaitEvent(p->aux[i], p->fork, 0);
            used[i] = true;
        }
        return p->aux[i];
    }
    // move the fork point behind everything enqueued on the caller's stream so far, for helpers that have not been taken yet
    // (begin() recorded it; inside a capture it is recorded where a helper is first needed anyway)
    hipError_t fork_here() {
        if (!p || two_way) return hipSuccess;
        return hipEventRecord(p->fork, main);
    }
    // order the helper after everything enqueued on the caller's stream so far (a second fork point)
    hipError_t refork(int slot) {
        if (!p || slot == 0) return hipSuccess;
        hipError_t e = hipEventRecord(p->fork, main);
        if (e != hipSuccess) return e;
        used[slot - 1] = true;
        return hipStreamWaitEvent(p->aux[slot - 1], p->fork, 0);
    }
    hipError_t end() {
        if (!p) return hipSuccess;
        for (int i = 0; i < 3; ++i) {
            if (!used[i]) continue;
            hipError_t e = hipEventRecord(p->join[i], p->aux[i]);
            if (e != hipSuccess) return e;
            e = hipStreamWaitEvent(main, p->join[i], 0);
            if (e != hipSuccess) return e;
        }
        return hipSuccess;
    }
};

// ---- dispatch: which kernel family every degree of a call takes.  Decided once per call by pure host functions (no HIP call; they
// read the switch table and the products overrides) before anything is enqueued; the entry points and the two queries read the same plan.
struct ConvShape {                       // what the dispatch looks at: shapes, presence and alignment, never contents
    int L[4]; int64_t count[4]; const float* e_unit[4];
    int F, E; int64_t n_atoms, x_stride, out_stride;
    bool x_aligned;                      // x starts on a 16-byte boundary (a query without x: true)
    bool grad_x, grad_x_aligned;         // backward: the input gradient is wanted; its rows are 16-byte aligned
    bool active(int i) const { return count[i] > 0 && L[i] > 0; }
    bool small(int i) const { return (uint64_t)count[i] * (uint64_t)L[i] < (1ull << 32); }      // 32-bit offsets into [N_d, L] planes
    int stream_groups() const { const bool use[4] = {active(0), active(1), active(2), active(3)}; return stream_forward_groups(L, use); }
};
static ConvShape conv_shape(const mkgnn_kernel_bank banks[4], const mkgnn_degree_bucket buckets[4], int F, int E, int64_t n_atoms,
                            const float* x, int64_t x_stride, int64_t out_stride, const float* grad_x = nullptr, int64_t grad_x_stride = 0) {
    ConvShape s{};
    for (int i = 0; i < 4; ++i) { s.L[i] = banks[i].num_kernels; s.count[i] = buckets[i].count; s.e_unit[i] = buckets[i].nei_edge_unit; }
    s.F = F; s.E = E; s.n_atoms = n_atoms; s.x_stride = x_stride; s.out_stride = out_stride;
    s.x_aligned = (((uintptr_t)x) & 15) == 0;
    s.grad_x = grad_x != nullptr; s.grad_x_aligned = grad_x_stride % 4 == 0 && (((uintptr_t)grad_x) & 15) == 0;
    return s;
}

enum FwdFamily : uint8_t { FWD_SKIP, FWD_GENERIC, FWD_LDS_BANK, FWD_STREAMED };
struct FwdDispatch {
    FwdFamily deg[4];
    bool rows_split_ok;                  // every degree with atoms and kernels fits the streamed kernel with split-fp16 products
    int refused_degree;                  // variants 2, 3: the first degree (1..4) the MFMA kernels do not cover; 0 = none
    int overflow_groups;                 // variants 2, 3: column groups the banks need where a launch's table overflows; 0 = none
    const char* overflow_launch;         //   ... which launch: "streamed" / "fused"
};
// variant: 0 automatic, 1 generic, 2 MFMA, 3 MFMA with bf16 products (flags masked off)
static FwdDispatch plan_conv_forward(const ConvShape& s, int variant) {
    const Switches& sw = switches();
    FwdDispatch p{};
    const bool aligned = (s.x_stride % 4 == 0) && s.x_aligned && ((uint64_t)s.n_atoms * (uint64_t)s.x_stride < (1ull << 32));
    // the streamed kernel (kgnn_fwd_stream.hip) takes the reference's bank shapes, and the bf16 variant at the model's row widths; round 1's
    // LDS-bank kernel every other covered shape; rows wider than it takes (F > 112) only the streamed kernel, so only the exact-fp32 variants
    const bool stream_on = sw.fwd_stream && (variant != 3 || (sw.bf16_stream && stream_forward_bf16_supported(s.F)));
    bool fuse[4], old_ok[4], stream_ok[4], use_stream[4], any = false, all_stream = true;
    int groups[4], total_groups = 0, only_groups[4], total_only = 0;
    for (int i = 0; i < 4; ++i) {
        old_ok[i] = mfma_forward_supported(i + 1, s.F, s.E, s.L[i]);
        stream_ok[i] = stream_forward_supported(i + 1, s.F, s.E, s.L[i], s.n_atoms, s.x_stride, s.out_stride, s.e_unit[i]);
        const bool stream_only = !old_ok[i] && variant != 3 && sw.fwd_stream && stream_ok[i];
        fuse[i] = s.active(i) && variant != 1 && aligned && s.small(i) && (old_ok[i] || stream_only);
        groups[i] = (fuse[i] && old_ok[i]) ? fused_group_count(i + 1, s.F, s.L[i]) : 0;
        only_groups[i] = (fuse[i] && !old_ok[i]) ? stream_column_parts(i + 1, s.L[i]) : 0;
        total_groups += groups[i]; total_only += only_groups[i];
        if (s.active(i)) { any = true; all_stream = all_stream && s.small(i) && stream_ok[i]; }
    }
    p.rows_split_ok = sw.rows_split && !sw.fwd_pp_env && sw.fwd_stream && stream_rows_split_supported(s.F) && aligned && any &&
                      all_stream && s.stream_groups() <= FUSED_MAX_GROUPS;
    // Both launches hold FUSED_MAX_GROUPS (degree, column part) groups; very wide banks are demoted, largest first.  (1) degrees only the
    // streamed kernel covers cannot move to the LDS-bank kernel: past the table, to the generic kernels.  (2) the covered degrees, counted as the
    // LDS-bank kernel splits them: likewise.  (3) what still overflows the streamed launch: to the LDS-bank kernel, widest first.
    auto demote = [&](int* g, int& total, const char* launch) {
        while (total > FUSED_MAX_GROUPS) {
            int big = 0;
            for (int i = 1; i < 4; ++i) if (g[i] > g[big]) big = i;
            if (variant >= 2) { p.overflow_groups = total; p.overflow_launch = launch; return false; }
            total -= g[big]; g[big] = 0; fuse[big] = false;
        }
        return true;
    };
    if (!demote(only_groups, total_only, "streamed") || !demote(groups, total_groups, "fused")) return p;
    for (int i = 0; i < 4; ++i) use_stream[i] = fuse[i] && stream_on && stream_ok[i];
    while (stream_forward_groups(s.L, use_stream) > FUSED_MAX_GROUPS) {
        int big = -1;
        for (int i = 0; i < 4; ++i)
            if (use_stream[i] && old_ok[i] && (big < 0 || stream_column_parts(i + 1, s.L[i]) > stream_column_parts(big + 1, s.L[big]))) big = i;
        if (big < 0) break;                              // (cannot happen: (1) keeps the degrees that cannot move within the table)
        use_stream[big] = false;
    }
    for (int i = 0; i < 4; ++i) {
        p.deg[i] = !s.active(i) ? FWD_SKIP : (use_stream[i] ? FWD_STREAMED : (fuse[i] ? FWD_LDS_BANK : FWD_GENERIC));
        if (variant >= 2 && p.deg[i] == FWD_GENERIC && !p.refused_degree) p.refused_degree = i + 1;
    }
    return p;
}

enum BwdFamily : uint8_t { BWD_SKIP, BWD_ZERO_FILL, BWD_GENERIC, BWD_LDS_PAIR, BWD_MFMA_LDS, BWD_STREAMED };
struct BwdDispatch {
    BwdFamily deg[4];                    // (BWD_MFMA_LDS: MFMA rows + LDS bank kernel; the facts below say which all-degree launches carry its halves)
    bool bank_fused;                     // the bank gradients of all degrees in one launch
    bool rows_streamed;                  // the x-gradient rows of all degrees in the streamed rows launch
    bool bank_streamed;                  // that one bank launch is the streamed MFMA kernel behind the coefficient pre-pass
    bool covers;                         // the streamed pair covers every degree with atoms and kernels, whatever the variant says
    bool through_nei_ok, rows_split_ok;  // MKGNN_BACKWARD_THROUGH_NEIGHBOURS / MKGNN_BACKWARD_ROWS_SPLIT can be honoured
    int refused_degree;                  // variant 2: the first degree (1..4) the fast kernels do not cover; 0 = none
};
// variant: 0 automatic, 1 generic kernels, 2 fast kernels (flags masked off)
static BwdDispatch plan_conv_backward(const ConvShape& s, int variant) {
    const Switches& sw = switches();
    const bool force_generic = variant == 1, force_fast = variant == 2;
    BwdDispatch p{};
    // the streamed pair (rows + bank kernels on the pre-pass's records; 16-byte rows: LDS-DMA pieces) runs whatever round 1's kernels say
    bool lds_ok[4] = {}, mfma_ok[4] = {}, any = false, rows_ok = true, bank_ok = true;
    p.covers = !sw.no_mfma_bwd && sw.bank_fused && sw.rows_stream && sw.bank_stream && (s.x_stride % 4) == 0 && s.x_aligned;
    for (int i = 0; i < 4; ++i) {
        if (!s.active(i)) continue;
        any = true;
        lds_ok[i] = lds_backward_supported(i + 1, s.F, s.E, s.L[i], s.x_stride, s.x_aligned);
        mfma_ok[i] = mfma_backward_supported(i + 1, s.F, s.E, s.L[i], s.x_stride, s.x_aligned, s.n_atoms);
        rows_ok = rows_ok && rows_stream_supported(i + 1, s.F, s.E, s.L[i]);
        bank_ok = bank_ok && bank_stream_supported(i + 1, s.F, s.E, s.L[i], s.n_atoms, s.x_stride, s.e_unit[i]);
        p.covers = p.covers && s.small(i);
    }
    p.covers = p.covers && any && rows_ok && bank_ok && s.stream_groups() <= FUSED_MAX_GROUPS;
    const bool stream_all = p.covers && !force_generic;
    // The bank gradients of all four degrees in one launch when every degree runs the MFMA rows + LDS bank pair: neutral at batch
    // 4096, 4-10 % of a step at batches <= 2048, where four launches of a few latency-bound blocks each ran one after the other.
    p.bank_fused = sw.bank_fused && !sw.no_mfma_bwd && !force_generic;
    for (int i = 0; i < 4; ++i)
        if (s.active(i) && !stream_all && !(lds_ok[i] && mfma_ok[i])) p.bank_fused = false;
    // the x-gradient rows of all degrees in one streamed launch when every degree's shape is covered (kgnn_bwd_rows_stream.hip)
    p.rows_streamed = p.bank_fused && sw.rows_stream && rows_ok;
    // the reference's bank shapes: the streamed MFMA kernel (kgnn_bwd_stream.hip); anything else: the LDS / VALU one
    p.bank_streamed = p.bank_fused && any && sw.bank_stream && bank_ok && s.stream_groups() <= FUSED_MAX_GROUPS;
    for (int i = 0; i < 4; ++i) {
        if (s.count[i] <= 0) continue;
        // atoms but no kernels for them in this set (a fixed / trainable split, kernels.py:699-720): the CSR still points at their rows
        if (s.L[i] <= 0) { p.deg[i] = s.grad_x ? BWD_ZERO_FILL : BWD_SKIP; continue; }
        const bool fast_ok = stream_all || lds_ok[i];
        if (force_fast && !stream_all && !(fast_ok && mfma_ok[i]) && !p.refused_degree) p.refused_degree = i + 1;
        if (!fast_ok || force_generic) p.deg[i] = BWD_GENERIC;
        else if (!(stream_all || (!sw.no_mfma_bwd && mfma_ok[i]))) p.deg[i] = BWD_LDS_PAIR;
        else p.deg[i] = (p.rows_streamed && p.bank_streamed) ? BWD_STREAMED : BWD_MFMA_LDS;
    }
    // grad_out as the gradient of h = propagate(out): only the streamed pair folds that step in (its pre-pass sums the neighbours' rows);
    // pre-split rows: only the streamed bank kernel and the pipelined gather read them.  (bank_fused: every degree is on the all-degree launches.)
    p.through_nei_ok = p.bank_streamed && p.rows_streamed;
    p.rows_split_ok = p.through_nei_ok && bank_stream_rows_split_supported(s.F) && (!s.grad_x || s.grad_x_aligned);
    return p;
}

// degree index (0..3) -> concurrency slot, most expensive bucket first (N_d * L_d * (d*d + 1))
static void degree_slots(const mkgnn_kernel_bank banks[4], const mkgnn_degree_bucket buckets[4], int slot_of[4]) {
    double cost[4];
    int order[4] = {0, 1, 2, 3};
    for (int i = 0; i < 4; ++i) cost[i] = (double)buckets[i].count * banks[i].num_kernels * ((i + 1) * (i + 1) + 1);
    for (int a = 0; a < 4; ++a)
        for (int b = a + 1; b < 4; ++b)
            if (cost[order[b]] > cost[order[a]]) { int t = order[a]; order[a] = order[b]; order[b] = t; }
    for (int r = 0; r < 4; ++r) slot_of[order[r]] = r;
}

namespace mkgnn {
GridCaps g_grid_caps;
PlanInfo g_last_plan[3];
}  // namespace mkgnn

// Measurement hook for bench.py (mkgnn_debug_time_backward): when enabled, a backward call keeps all its kernels on the
// caller's stream, one after the other (no helper streams: every kernel alone on the GPU), and brackets each with HIP
// events recorded on that stream: 0 coefficient pre-pass, 1 rows gradient, 2 bank gradient, 3 bank reduce, 4 gather.
// One benchmarking thread; the flag is atomic, the events are not per caller.
static std::atomic<bool> g_time_bwd{false};
static hipEvent_t g_bwd_ev[5][2];
static bool g_bwd_ev_made = false, g_bwd_ev_used[5];
struct BwdTimer {
    hipStream_t st; int k; bool on;
    BwdTimer(hipStream_t s, int which) : st(s), k(which), on(g_time_bwd.load()) {
        if (on) { (void)hipEventRecord(g_bwd_ev[k][0], st); g_bwd_ev_used[k] = true; }
    }
    ~BwdTimer() { if (on) (void)hipEventRecord(g_bwd_ev[k][1], st); }
};

extern "C" {

// Diagnostics (not part of the drop-in ABI; used by tests/ and tools/): grid caps of the streamed forward / rows-gradient /
// bank-gradient kernels, 0 = default, otherwise 8..512, effective from the next launch; and the block split of the last
// launch of each: out[3 k ..] = {blocks, fewest, most atom tiles per stream over the (degree, column part) groups}; out[9 + k] =
// how many times streamed kernel k has been launched (forward, rows gradient, bank gradient).
int mkgnn_debug_set_grid_caps(int32_t forward_blocks, int32_t rows_blocks, int32_t bank_blocks) {
    for (int32_t v : {forward_blocks, rows_blocks, bank_blocks})
        if (v != 0 && (v < 8 || v > FUSED_MAX_BLOCKS)) return api_fail("mkgnn_debug_set_grid_caps: %d outside 8..%d (0 = default)", v, FUSED_MAX_BLOCKS);
    g_grid_caps.fwd.store(forward_blocks); g_grid_caps.rows.store(rows_blocks); g_grid_caps.bank.store(bank_blocks);
    return 0;
}
// reads the runtime's sticky last-error away (after a failed hipGraph capture the next launch check would report it)
int mkgnn_debug_clear_error(void) { (void)hipGetLastError(); return 0; }
int mkgnn_debug_time_backward(int32_t enable) {
    if (enable && !g_bwd_ev_made) {
        for (int k = 0; k < 5; ++k)
            for (int j = 0; j < 2; ++j)
                if (hipEventCreate(&g_bwd_ev[k][j]) != hipSuccess) return api_fail("mkgnn_debug_time_backward: hipEventCreate failed");
        g_bwd_ev_made = true;
    }
    for (int k = 0; k < 5; ++k) g_bwd_ev_used[k] = false;
    g_time_bwd.store(enable != 0);
    return 0;
}
// out[k] = duration (ms) of kernel k of the last timed backward call (see BwdTimer), -1 where it did not run
int mkgnn_debug_last_backward_ms(float out[5]) {
    if (!out || !g_bwd_ev_made) return api_fail("mkgnn_debug_last_backward_ms: timing was never enabled");
    for (int k = 0; k < 5; ++k) {
        out[k] = -1.f;
        if (!g_bwd_ev_used[k]) continue;
        if (hipEventSynchronize(g_bwd_ev[k][1]) != hipSuccess) continue;
        float ms = -1.f;
        if (hipEventElapsedTime(&ms, g_bwd_ev[k][0], g_bwd_ev[k][1]) == hipSuccess) out[k] = ms;
    }
    return 0;
}
int mkgnn_debug_last_plans(int32_t out[12]) {
    if (!out) return api_fail("mkgnn_debug_last_plans: null pointer");
    for (int k = 0; k < 3; ++k) {
        out[3 * k] = g_last_plan[k].blocks.load(); out[3 * k + 1] = g_last_plan[k].min_iters.load(); out[3 * k + 2] = g_last_plan[k].max_iters.load();
        out[9 + k] = g_last_plan[k].launches.load();        // launches of the streamed kernel since the library was loaded
    }
    return 0;
}

// The power-of-two scales of the split-fp16 products (kgnn_split.h), evaluated on the HOST -- the same inline functions the kernels
// compile, plain exponent-field arithmetic -- for the exhaustive property test of tests/test_host_cpu.py (no GPU needed):
// out = bits of { split_scale_for<10>(amax), split_unscale_of<12>(that)   [the rows kernel's pair],
//                 split_scale_for_exponent<18>(exponent of amax), split_unscale_of<0>(that)   [the bank kernel's],
//                 split_row_scale_of(amax), split_row_inv(amax)   [pre-split rows / the forward's row scale, amax read as 1 / |x|] }
int mkgnn_debug_split_scales(uint32_t amax_bits, uint32_t out[6]) {
    if (!out) return api_fail("mkgnn_debug_split_scales: null pointer");
    const float amax = split_bits_to_float(amax_bits);
    const float s_rows = split_scale_for<10>(amax), u_rows = split_unscale_of<12>(s_rows);
    const float s_bank = split_scale_for_exponent<18>((int)((amax_bits >> 23) & 0xffu)), u_bank = split_unscale_of<0>(s_bank);
    out[0] = split_float_to_bits(s_rows); out[1] = split_float_to_bits(u_rows);
    out[2] = split_float_to_bits(s_bank); out[3] = split_float_to_bits(u_bank);
    out[4] = split_float_to_bits(split_row_scale_of(amax)); out[5] = split_float_to_bits(split_row_inv(amax));
    return 0;
}

int mkgnn_abi_version(void) { return MKGNN_ABI_VERSION; }

const char* mkgnn_last_error(void) { return g_err; }

int mkgnn_row_inv_norm(const float* x, int64_t x_stride, int64_t n_rows, int32_t F, float* inv_norm, void* stream) {
    if (n_rows < 0 || F <= 0 || x_stride < F) return api_fail("mkgnn_row_inv_norm: bad shape n=%lld F=%d stride=%lld",
                                                         (long long)n_rows, F, (long long)x_stride);
    if (n_rows && (!x || !inv_norm)) return api_fail("mkgnn_row_inv_norm: null pointer");
    hipError_t e = launch_row_inv_norm(x, x_stride, n_rows, F, inv_norm, (hipStream_t)stream);
    return e == hipSuccess ? 0 : api_hip_fail("mkgnn_row_inv_norm", e);
}

int mkgnn_rows_presplit(const float* x, int64_t x_stride, int64_t n_rows, int32_t F, float* inv_norm, float* out, int64_t out_stride,
                        void* stream) {
    if (n_rows < 0 || F <= 0 || x_stride < F || out_stride < F) return api_fail("mkgnn_rows_presplit: bad shape");
    if (n_rows == 0) return 0;
    if (!x || !inv_norm || !out) return api_fail("mkgnn_rows_presplit: null pointer");
    hipError_t e = hipSuccess;
    if (!try_rows_presplit(x, x_stride, n_rows, F, inv_norm, out, out_stride, (hipStream_t)stream, &e))
        return api_fail("mkgnn_rows_presplit: rows of at most 256 floats, 16-byte aligned (strides multiples of 4 floats)");
    return e == hipSuccess ? 0 : api_hip_fail("mkgnn_rows_presplit", e);
}

int mkgnn_unit_rows8(const float* in, int64_t n_rows, int32_t E, float* out, void* stream) {
    if (n_rows < 0 || E < 1 || E > 8) return api_fail("mkgnn_unit_rows8: %lld rows of width %d (1..8)", (long long)n_rows, E);
    if (n_rows && (!in || !out)) return api_fail("mkgnn_unit_rows8: null pointer");
    hipError_t e = launch_unit_rows8(in, n_rows, E, out, (hipStream_t)stream);
    return e == hipSuccess ? 0 : api_hip_fail("mkgnn_unit_rows8", e);
}

size_t mkgnn_workspace_bytes(const int32_t num_kernels[MKGNN_MAX_DEGREE], int32_t F, int32_t E, int64_t n_atoms,
                             int64_t n_edges) {
    return make_layout(num_kernels, F, E, n_atoms, n_edges).total;
}

static int check_common(const char* who, const mkgnn_kernel_bank banks[4], const mkgnn_degree_bucket buckets[4],
                        const float* x, int64_t x_stride, const float* inv_norm, int64_t n_atoms, int32_t F, int32_t E,
                        int32_t need_coordinates, int64_t* n_edges_out) {
    if (!banks || !buckets) return api_fail("%s: banks/buckets is null", who);
    if (F <= 0 || F > 256) return api_fail("%s: node attribute width F=%d outside 1..256", who, F);
    if (E <= 0 || E > 64) return api_fail("%s: edge attribute width E=%d outside 1..64", who, E);
    if (n_atoms < 0 || x_stride < F) return api_fail("%s: bad x shape", who);
    if (n_atoms && (!x || !inv_norm)) return api_fail("%s: x/inv_norm is null", who);
    int64_t n_edges = 0, n_focal = 0;
    for (int i = 0; i < 4; ++i) {
        const mkgnn_kernel_bank& b = banks[i];
        const mkgnn_degree_bucket& k = buckets[i];
        if (b.num_kernels < 0 || b.num_kernels > 4096) return api_fail("%s: degree %d has %d kernels", who, i + 1, b.num_kernels);
        if (k.count < 0) return api_fail("%s: degree %d bucket count %lld", who, i + 1, (long long)k.count);
        if (k.count > 0) {
            // num_kernels == 0 with atoms present: the degree is skipped here (its rows are left
            // untouched); the host raises the reference's exception (kernels.py:717-721) when
            // neither a fixed nor a trainable bank exists for such a degree.
            if (!k.selected_index || !k.nei_index || !k.nei_edge_attr)
                return api_fail("%s: degree %d bucket has null index/edge tensors", who, i + 1);
            if (i == 3 && need_coordinates && (!k.p_focal || !k.nei_p || !b.p_support))
                return api_fail("%s: degree-4 coordinates are required in the last layer (chirality)", who);
        }
        if (b.num_kernels > 0 && (!b.x_center || !b.x_support || !b.edge_attr_support || !b.support_attr_sc_weight ||
                                  !b.center_attr_sc_weight || !b.edge_attr_support_sc_weight))
            return api_fail("%s: degree %d bank has null parameters", who, i + 1);
        n_edges += k.count * (i + 1);
        n_focal += k.count;
    }
    if (n_focal > n_atoms) return api_fail("%s: buckets hold %lld atoms, batch has %lld", who, (long long)n_focal, (long long)n_atoms);
    *n_edges_out = n_edges;
    return 0;
}

static thread_local TouchArgs g_touch_hint;           // (count == 0: none pending)
extern "C++" {
namespace mkgnn {
bool take_touch_hint(TouchArgs& out) {
    if (g_touch_hint.count <= 0) return false;
    out = g_touch_hint;
    g_touch_hint.count = 0;
    return true;
}
}  // namespace mkgnn
}

// Present blocks of d loss / d x (kgnn_launch.h GradBlocks): a thread-local hint, like the touch hint, that the NEXT
// mkgnn_kernelsetconv_backward of this thread takes (and clears, whatever it does with it)
static thread_local GradBlocks g_grad_blocks_hint;     // (present8 == null: none pending)
static std::atomic<int> g_poison_bwd{0};
extern "C++" {
namespace mkgnn {
std::atomic<long long> g_grad_blocks_launches;
bool take_grad_blocks_hint(GradBlocks& out) {
    out = g_grad_blocks_hint;
    g_grad_blocks_hint = GradBlocks{};
    return out.present8 != nullptr;
}
}  // namespace mkgnn
}

int mkgnn_backward_grad_blocks(const int8_t* present8, const int32_t num_kernels[MKGNN_MAX_DEGREE]) {
    g_grad_blocks_hint = GradBlocks{};
    if (!present8) return 0;                                       // withdrawn
    if (!num_kernels) return api_fail("mkgnn_backward_grad_blocks: null pointer");
    GradBlocks gb{present8, 0, 0};
    int off = 0;
    for (int d = 1; d <= 4; ++d) {
        const int L = num_kernels[d - 1];
        // (blocks of one byte per entry, every degree with columns: what the masked kernels take; anything else: no hint, whole rows)
        if (L < 1 || off + L > 255) return 0;
        gb.blk_off |= (uint64_t)off << (8 * d);
        gb.blk_len |= (uint64_t)L << (8 * d);
        off += L;
    }
    g_grad_blocks_hint = gb;
    return 0;
}

// tests: backward calls since the library was loaded whose gather read and wrote present chunks only
int64_t mkgnn_debug_grad_blocks_launches(void) { return g_grad_blocks_launches.load(); }
// tests: a backward call fills its contribution rows and grad_x with NaN before anything is launched (what no kernel writes stays NaN)
int mkgnn_debug_poison_backward(int32_t enable) { g_poison_bwd.store(enable ? 1 : 0); return 0; }

int mkgnn_touch_hint(const void* const* arrays, const size_t* bytes, int32_t count) {
    if (count <= 0 || !arrays || !bytes) {
        const int had = g_touch_hint.count > 0 ? 1 : 0;
        g_touch_hint.count = 0;
        return had;
    }
    TouchArgs ta{};
    for (int k = 0; k < count && ta.count < TOUCH_MAX; ++k) {      // the 16-byte aligned interior of every array (at most 4 GiB - 16 of it)
        if (!arrays[k] || bytes[k] < 32) continue;
        const uintptr_t lo = ((uintptr_t)arrays[k] + 15) & ~(uintptr_t)15, hi = ((uintptr_t)arrays[k] + bytes[k]) & ~(uintptr_t)15;
        if (hi <= lo) continue;
        const size_t n = hi - lo;
        ta.ptr[ta.count] = (const char*)lo;
        ta.bytes[ta.count] = (uint32_t)(n > 0xfffffff0u ? 0xfffffff0u : n);
        ++ta.count;
    }
    g_touch_hint = ta;
    return 0;
}

// a preparation left pending by mkgnn_bank_prepare_deferred: per device (armed and taken by the forward's thread; the mutex keeps
// the slot whole)
struct PendingPrepare { PrepManyArgs m; bool armed; };
static PendingPrepare g_pending_prepare[16];
static std::mutex g_pending_prepare_mutex;
static PendingPrepare* pending_prepare_slot() {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) dev = 0;
    return &g_pending_prepare[dev];
}
extern "C++" {
namespace mkgnn {
bool take_pending_prepare(PrepManyArgs& out) {
    std::lock_guard<std::mutex> lock(g_pending_prepare_mutex);
    PendingPrepare* p = pending_prepare_slot();
    if (!p->armed) return false;
    out = p->m;
    p->armed = false;
    return true;
}
}  // namespace mkgnn
}

static int bank_prepare_impl(const char* who, int32_t count, const mkgnn_kernel_bank* banks, const int32_t* F, int32_t E,
                             void* const* workspaces, const size_t* workspace_bytes, bool defer, void* stream);

int mkgnn_bank_prepare_deferred(int32_t count, const mkgnn_kernel_bank* banks, const int32_t* F, int32_t E, void* const* workspaces,
                                const size_t* workspace_bytes) {
    return bank_prepare_impl("mkgnn_bank_prepare_deferred", count, banks, F, E, workspaces, workspace_bytes, true, nullptr);
}

int mkgnn_bank_prepare_flush(void* stream) {
    PrepManyArgs m;
    if (!take_pending_prepare(m)) return 0;
    (void)take_touch_hint(m.touch);
    hipError_t e = launch_bank_prepare_args(m, (hipStream_t)stream);
    return e == hipSuccess ? 0 : api_hip_fail("mkgnn_bank_prepare_flush", e);
}

int mkgnn_bank_prepare_withdraw(void) {
    PrepManyArgs m;
    return take_pending_prepare(m) ? 1 : 0;
}

int mkgnn_bank_prepare(int32_t count, const mkgnn_kernel_bank* banks, const int32_t* F, int32_t E, void* const* workspaces,
                       const size_t* workspace_bytes, void* stream) {
    if (int rc = mkgnn_bank_prepare_flush(stream)) return rc;        // (one left pending and never taken: first, in order)
    return bank_prepare_impl("mkgnn_bank_prepare", count, banks, F, E, workspaces, workspace_bytes, false, stream);
}

static int bank_prepare_impl(const char* who, int32_t count, const mkgnn_kernel_bank* banks, const int32_t* F, int32_t E,
                             void* const* workspaces, const size_t* workspace_bytes, bool defer, void* stream) {
    if (count < 0 || count > PREP_MANY_MAX) return api_fail("%s: %d calls (0..%d per launch)", who, count, PREP_MANY_MAX);
    TouchArgs ta{};
    if (!defer) (void)take_touch_hint(ta);
    if (count == 0 && ta.count == 0) return 0;
    if (count > 0 && (!banks || !F || !workspaces || !workspace_bytes || E <= 0)) return api_fail("%s: bad arguments", who);
    WorkspaceLayout w[PREP_MANY_MAX];
    char* ws[PREP_MANY_MAX];
    int Fs[PREP_MANY_MAX];
    for (int k = 0; k < count; ++k) {
        int32_t L[4];
        for (int i = 0; i < 4; ++i) {
            const mkgnn_kernel_bank& b = banks[4 * k + i];
            L[i] = b.num_kernels;
            if (L[i] < 0) return api_fail("%s: call %d degree %d has %d kernels", who, k, i + 1, L[i]);
            if (L[i] > 0 && (!b.x_center || !b.x_support || !b.edge_attr_support || !b.support_attr_sc_weight ||
                             !b.center_attr_sc_weight || !b.edge_attr_support_sc_weight))
                return api_fail("%s: call %d degree %d bank has null parameters", who, k, i + 1);
        }
        if (F[k] <= 0) return api_fail("%s: call %d has F=%d", who, k, F[k]);
        w[k] = make_layout(L, F[k], E, 0, 0);
        if (!workspaces[k] || workspace_bytes[k] < w[k].bank[3].end)
            return api_fail("%s: call %d: workspace of %zu bytes, the banks need %zu", who, k, workspace_bytes[k], w[k].bank[3].end);
        ws[k] = (char*)workspaces[k];
        Fs[k] = F[k];
    }
    if (defer) {
        if (count > PREP_MANY_MAX) return api_fail("%s: at most %d calls", who, PREP_MANY_MAX);
        std::lock_guard<std::mutex> lock(g_pending_prepare_mutex);
        PendingPrepare* p = pending_prepare_slot();
        if (p->armed) return api_fail("%s: a deferred preparation is already pending on this device (mkgnn_bank_prepare_flush)", who);
        build_bank_prepare_many(count, banks, w, ws, Fs, E, &p->m);
        p->armed = p->m.prep_blocks > 0;
        return 0;
    }
    hipError_t e = launch_bank_prepare_many(count, banks, w, ws, Fs, E, (hipStream_t)stream, ta.count ? &ta : nullptr);
    return e == hipSuccess ? 0 : api_hip_fail(who, e);
}

// pre-split rows (MKGNN_VARIANT_ROWS_SPLIT / MKGNN_BACKWARD_ROWS_SPLIT): the forward puts every degree with atoms and kernels on the
// streamed kernel with split-fp16 products, and the backward on the streamed pair
static bool rows_split_covered(const ConvShape& s, const FwdDispatch& fwd) {
    return fwd.rows_split_ok && bank_stream_rows_split_supported(s.F) && plan_conv_backward(s, 0).covers;
}

int mkgnn_kernelsetconv_forward(const mkgnn_kernel_bank banks[MKGNN_MAX_DEGREE],
                                const mkgnn_degree_bucket buckets[MKGNN_MAX_DEGREE], const float* x, int64_t x_stride,
                                const float* inv_norm, int64_t n_atoms, int32_t F, int32_t E, int32_t is_last_layer,
                                float* out, int64_t out_stride, const mkgnn_saved saved[MKGNN_MAX_DEGREE],
                                void* workspace, size_t workspace_bytes, int32_t variant, void* stream) {
    const char* who = "mkgnn_kernelsetconv_forward";                            // ---- check
    int64_t n_edges = 0;
    if (int rc = check_common(who, banks, buckets, x, x_stride, inv_norm, n_atoms, F, E, is_last_layer, &n_edges)) return rc;
    int32_t L[4], K = 0;
    for (int i = 0; i < 4; ++i) { L[i] = banks[i].num_kernels; K += L[i]; }
    if (out_stride < K || (n_atoms && !out)) return api_fail("%s: bad out (stride %lld, K %d)", who, (long long)out_stride, K);
    WorkspaceLayout w = make_layout(L, F, E, n_atoms, n_edges);
    if (workspace_bytes < w.fwd_end || !workspace)
        return api_fail("%s: workspace of %zu bytes, need %zu", who, workspace_bytes, w.fwd_end);
    const bool block_rows_only = (variant & MKGNN_VARIANT_BLOCK_ROWS) != 0;     // the caller reads only each atom's own block
    const bool bank_prepared = (variant & MKGNN_VARIANT_BANK_PREPARED) != 0;    // mkgnn_bank_prepare has filled the workspace's head
    const bool rows_split = (variant & MKGNN_VARIANT_ROWS_SPLIT) != 0;          // x is pre-split (kgnn_split.h)
    variant &= ~(MKGNN_VARIANT_BLOCK_ROWS | MKGNN_VARIANT_BANK_PREPARED | MKGNN_VARIANT_ROWS_SPLIT);
    if (variant < 0 || variant > 3) return api_fail("%s: variant %d", who, variant);
    // ---- plan: the fused MFMA launch takes every degree whose shape it covers, the rest run on the generic kernels
    const ConvShape shape = conv_shape(banks, buckets, F, E, n_atoms, x, x_stride, out_stride);
    const FwdDispatch plan = plan_conv_forward(shape, variant);
    if (rows_split && (variant == 1 || variant == 3 || !rows_split_covered(shape, plan)))
        return api_fail("%s: MKGNN_VARIANT_ROWS_SPLIT needs the streamed kernels with split-fp16 products for every degree "
                        "(mkgnn_rows_split_supported(..) tells)", who);
    if (const int g = plan.overflow_groups)
        return api_fail("%s: the banks need %d column groups, the %s launch holds %d", who, g, plan.overflow_launch, FUSED_MAX_GROUPS);
    if (const int d = plan.refused_degree)
        return api_fail("%s: MFMA variant does not cover degree %d with F=%d E=%d L=%d stride=%lld", who, d, F, E, L[d - 1], (long long)x_stride);
    // ---- launch
    hipStream_t st = (hipStream_t)stream; char* ws = (char*)workspace;
    hipError_t e = bank_prepared ? hipSuccess : launch_bank_prepare(banks, w, ws, F, E, st);
    if (e != hipSuccess) return api_hip_fail("bank_prepare", e);
    // every atom's row is zero outside its own degree block (kernels.py:674-675, 725-727): one
    // streaming memset, the degree kernels then write only their column blocks
    // (alignment padding up to the next multiple of four columns is zeroed with it when the stride holds it)
    if (n_atoms > 0 && K > 0 && !block_rows_only) {
        const int64_t K4 = (K + 3) / 4 * 4;
        if (K4 == out_stride) e = hipMemsetAsync(out, 0, (size_t)n_atoms * out_stride * 4, st);   // contiguous: one fill kernel, not two
        else e = hipMemset2DAsync(out, (size_t)out_stride * 4, 0, (size_t)(K4 <= out_stride ? K4 : K) * 4, (size_t)n_atoms, st);
        if (e != hipSuccess) return api_hip_fail("output memset", e);
    }
    FusedFwdArgs fa; memset(&fa, 0, sizeof(fa));
    fa.x = x; fa.xs = x_stride; fa.inv = inv_norm; fa.out = out; fa.os = out_stride;
    fa.K = K; fa.F = F; fa.E = E; fa.last = is_last_layer ? 1 : 0; fa.n_atoms = n_atoms;
    fa.bf16 = variant == 3 ? 1 : 0;
    fa.x_split = rows_split ? 1 : 0;
    bool use_stream[4], use_bank[4], any_fused = false;
    int off = 0;
    for (int i = 0; i < 4; ++i) {
        const int d = i + 1; FwdArgs a;
        a.x = x; a.xs = x_stride; a.inv = inv_norm;
        a.sel = buckets[i].selected_index; a.nei = buckets[i].nei_index; a.e_nei = buckets[i].nei_edge_attr;
        a.p_focal = buckets[i].p_focal; a.p_nei = buckets[i].nei_p;
        a.n = buckets[i].count; a.F = F; a.E = E; a.L = L[i]; a.last = is_last_layer ? 1 : 0;
        a.cen = (const float*)(ws + w.bank[i].cen); a.sup = (const float*)(ws + w.bank[i].sup);
        a.edg = (const float*)(ws + w.bank[i].edg); a.chir = (const int8_t*)(ws + w.bank[i].chir);
        a.mix = (const float*)(ws + w.bank[i].mix);
        a.padded = (const float*)(ws + w.bank[i].padded); a.edge_padded = (const float*)(ws + w.bank[i].edge_padded);
        a.n_atoms = n_atoms;
        a.out = out; a.os = out_stride; a.off = off; a.K = K;
        a.pair = saved ? saved[i].pair_state : nullptr;
        a.chir_out = (saved && d == 4 && is_last_layer) ? saved[i].chirality : nullptr;
        off += L[i];
        use_stream[i] = plan.deg[i] == FWD_STREAMED; use_bank[i] = plan.deg[i] == FWD_LDS_BANK;
        if (use_stream[i] || use_bank[i]) {
            FusedDeg& g = fa.deg[i];
            g.sel = a.sel; g.nei = a.nei; g.e_nei = a.e_nei; g.e_unit = buckets[i].nei_edge_unit; g.p_focal = a.p_focal; g.p_nei = a.p_nei;
            g.padded = a.padded; g.edge_padded = a.edge_padded; g.chir = a.chir; g.mix = a.mix;
            g.eqflag = (const int8_t*)(ws + w.eqflag);
            g.signflag = (const int8_t*)(ws + w.signflag);
            g.pair = a.pair; g.chir_out = a.chir_out;
            g.n = a.n; g.L = a.L; g.off = a.off;
            any_fused = true;
        } else if (plan.deg[i] == FWD_GENERIC) {
            e = launch_forward_generic(d, a, st);
            if (e != hipSuccess) return api_hip_fail("kernelconv forward launch", e);
        }
    }
    if (any_fused) {
        e = launch_forward_fused(fa, use_stream, use_bank, st);
        if (e != hipSuccess) return api_hip_fail("fused kernelconv forward launch", e);
    }
    return 0;
}

int mkgnn_kernelsetconv_backward(const mkgnn_kernel_bank banks[MKGNN_MAX_DEGREE],
                                 const mkgnn_degree_bucket buckets[MKGNN_MAX_DEGREE], const float* x, int64_t x_stride,
                                 const float* inv_norm, int64_t n_atoms, int32_t F, int32_t E, int32_t is_last_layer,
                                 const float* grad_out, int64_t grad_out_stride,
                                 const mkgnn_saved saved[MKGNN_MAX_DEGREE], const int32_t* scatter_rowptr,
                                 const int32_t* scatter_rows, float* grad_x, int64_t grad_x_stride,
                                 const mkgnn_kernel_bank_grad grads[MKGNN_MAX_DEGREE], void* workspace,
                                 size_t workspace_bytes, int32_t workspace_from_forward, int32_t variant, void* stream) {
    const char* who = "mkgnn_kernelsetconv_backward";                           // ---- check
    GradBlocks gb;
    const bool gb_hint = take_grad_blocks_hint(gb);                             // (taken before any return: it is this call's alone)
    const bool defer_bank = (variant & MKGNN_BACKWARD_DEFER_BANK) != 0;
    const bool through_nei = (variant & MKGNN_BACKWARD_THROUGH_NEIGHBOURS) != 0;
    const bool rows_split = (variant & MKGNN_BACKWARD_ROWS_SPLIT) != 0;         // x is pre-split (kgnn_split.h)
    variant &= ~(MKGNN_BACKWARD_DEFER_BANK | MKGNN_BACKWARD_THROUGH_NEIGHBOURS | MKGNN_BACKWARD_ROWS_SPLIT);
    if (variant < 0 || variant > 2) return api_fail("%s: variant %d (0 = automatic, 1 = generic kernels, 2 = fast kernels)", who, variant);
    int64_t n_edges = 0;
    if (int rc = check_common(who, banks, buckets, x, x_stride, inv_norm, n_atoms, F, E, 0, &n_edges)) return rc;
    if (!saved || !grads) return api_fail("%s: saved/grads is null", who);
    int32_t L[4], K = 0;
    for (int i = 0; i < 4; ++i) { L[i] = banks[i].num_kernels; K += L[i]; }
    if (grad_out_stride < K || (n_atoms && !grad_out)) return api_fail("%s: bad grad_out", who);
    if (grad_x && grad_x_stride < F) return api_fail("%s: bad grad_x stride", who);
    // (no atom of degree 1..4 -- a batch without bonds: nothing reaches x, the gradient is zero and no CSR is read)
    if (grad_x && n_atoms && n_edges > 0 && (!scatter_rowptr || !scatter_rows)) return api_fail("%s: scatter CSR is null", who);
    WorkspaceLayout w = make_layout(L, F, E, n_atoms, n_edges);
    if (workspace_bytes < w.total || !workspace) return api_fail("%s: workspace of %zu bytes, need %zu", who, workspace_bytes, w.total);
    for (int i = 0; i < 4; ++i) {
        if (buckets[i].count > 0 && L[i] > 0 && !saved[i].pair_state) return api_fail("%s: degree %d has no saved forward state", who, i + 1);
        if (i == 3 && is_last_layer && buckets[i].count > 0 && !saved[i].chirality)
            return api_fail("%s: degree-4 chirality signs were not saved", who);
    }
    // ---- plan
    const BwdDispatch plan = plan_conv_backward(conv_shape(banks, buckets, F, E, n_atoms, x, x_stride, 0, grad_x, grad_x_stride), variant);
    if (const int d = plan.refused_degree)
        return api_fail("%s: the fast kernels do not cover degree %d with F=%d E=%d L=%d stride=%lld", who, d, F, E, L[d - 1], (long long)x_stride);
    if (through_nei && !plan.through_nei_ok)
        return api_fail("%s: MKGNN_BACKWARD_THROUGH_NEIGHBOURS needs the streamed kernels for every degree "
                        "(mkgnn_backward_streams(..) tells)", who);
    if (rows_split && !plan.rows_split_ok)
        return api_fail("%s: MKGNN_BACKWARD_ROWS_SPLIT needs the streamed kernels with split-fp16 products for every degree "
                        "(mkgnn_rows_split_supported(..) tells)", who);
    const bool fuse_bank = plan.bank_fused, rows_streamed = plan.rows_streamed, streamed = plan.bank_streamed;
    // present blocks: the gather where the pipelined one applies and the blocks are this call's columns (whatever kernels wrote the
    // contribution rows wrote whole rows: the masked gather reads a part of them)
    // (the conditions under which launch_backward_gather takes the pipelined kernel: contribution rows exist -- n_edges counts their
    // neighbour slots -- and the shapes fit; F <= 255: one byte per block table entry)
    bool gb_gather = gb_hint && switches().grad_blocks && variant != 1 && grad_x && n_edges > 0 && F <= 255 &&
                     backward_gather_aligned_supported((const float*)((char*)workspace + w.contrib), (F + 3) / 4 * 4, scatter_rows, x, x_stride,
                                                       n_atoms, F, grad_x, grad_x_stride);
    if (gb_gather) {
        int width = 0;
        for (int d = 1; d <= 4; ++d) width += (int)((gb.blk_len >> (8 * d)) & 0xFF);
        gb_gather = width == F;
    }
    // ---- fill the argument blocks
    hipStream_t st = (hipStream_t)stream; char* ws = (char*)workspace;
    BwdArgs bank_a[4];
    BankReduceArgs reduce[4];
    bool bank_use[4];                                // the degrees of the all-degree launches
    const float* e_unit4[4]; float* coefq4[4];
    int off = 0; int64_t base = 0;
    size_t coef_off = w.coefq_off[0];
    for (int i = 0; i < 4; ++i) {
        BwdArgs& a = bank_a[i];
        a.x = x; a.xs = x_stride; a.inv = inv_norm;
        a.sel = buckets[i].selected_index; a.nei = buckets[i].nei_index; a.e_nei = buckets[i].nei_edge_attr;
        a.n = buckets[i].count; a.F = F; a.E = E; a.L = L[i];
        a.cen = (const float*)(ws + w.bank[i].cen); a.sup = (const float*)(ws + w.bank[i].sup);
        a.edg = (const float*)(ws + w.bank[i].edg); a.mix = (const float*)(ws + w.bank[i].mix);
        a.gout = grad_out; a.gs = grad_out_stride; a.off = off;
        a.pair = saved[i].pair_state;
        a.chir = (i == 3 && is_last_layer) ? saved[i].chirality : nullptr;
        a.contrib = (float*)(ws + w.contrib); a.contrib_base = base; a.CS = (F + 3) / 4 * 4;
        a.slab = (float*)(ws + w.slab_off[i]);
        a.padded = (const float*)(ws + w.bank[i].padded);
        a.nchunk = (int)(a.n < BWD_BANK_BLOCKS ? (a.n > 0 ? a.n : 1) : BWD_BANK_BLOCKS);
        a.theta_slab = (float*)(ws + w.theta_off[i]);
        BankReduceArgs& r = reduce[i];               // (its partials: set where the degree's kernels are launched)
        r.slab = a.slab; r.F = F; r.E = E; r.L = L[i];
        r.cen = a.cen; r.sup = a.sup; r.edg = a.edg;
        r.icen = (const float*)(ws + w.bank[i].icen); r.isup = (const float*)(ws + w.bank[i].isup);
        r.iedg = (const float*)(ws + w.bank[i].iedg);
        r.g = grads[i];
        off += L[i]; base += buckets[i].count * (i + 2);
        bank_use[i] = fuse_bank && plan.deg[i] >= BWD_MFMA_LDS;
        e_unit4[i] = buckets[i].nei_edge_unit; coefq4[i] = nullptr;
        if (!bank_use[i]) continue;
        coefq4[i] = (float*)(ws + coef_off);
        coef_off += (size_t)((buckets[i].count + 15) / 16) * ((L[i] + 15) / 16) * 512 * 4;
    }
    const bool any_bank = bank_use[0] || bank_use[1] || bank_use[2] || bank_use[3];
    // ---- launch: the x-gradient chain (rows kernels, then the gather) and the bank chain (bank kernels, then the reduce)
    hipError_t e = hipSuccess;
    if (g_poison_bwd.load() && grad_x && n_atoms) {
        int64_t rows_all = 0;
        for (int i = 0; i < 4; ++i) rows_all += buckets[i].count * (i + 2);
        e = hipMemsetAsync(ws + w.contrib, 0xFF, (size_t)rows_all * ((F + 3) / 4 * 4) * sizeof(float), st);
        if (e == hipSuccess)
            e = hipMemset2DAsync(grad_x, (size_t)grad_x_stride * sizeof(float), 0xFF, (size_t)F * sizeof(float), (size_t)n_atoms, st);
        if (e != hipSuccess) return api_hip_fail("poison", e);
    }
    if (!workspace_from_forward) {                   // else the normalised bank of the forward call is still there
        e = launch_bank_prepare(banks, w, ws, F, E, st);
        if (e != hipSuccess) return api_hip_fail("bank_prepare", e);
    }
    int slot_of[4];
    degree_slots(banks, buckets, slot_of);
    ForkJoin fj;
    e = fj.begin(st, !g_time_bwd.load());            // (timed for bench.py: everything on the caller's stream)
    if (e != hipSuccess) return api_hip_fail("stream fork", e);
    // a projection the fused tail left pending (mkgnn_tail_defer_projection): taken over when this call is the reader of its
    // d sim and runs the streamed kernels beside a forked helper; anything else gets the launch that was left out, here and now
    TailProjection tp;
    bool project = false;
    if (pending_tail_projection(&tp)) {
        project = grad_out == tp.dsim && grad_out_stride == tp.dss && streamed && rows_streamed && !through_nei && defer_bank && fj.p != nullptr &&
                  any_bank && K == tp.K;
        for (int i = 0; i < 4 && project; ++i) {
            const bool same = L[i] == tp.L[i] && bank_a[i].off == tp.off[i] && buckets[i].count == tp.cnt[i] &&
                              (tp.cnt[i] == 0 || buckets[i].selected_index == tp.sel[i]);
            const bool wanted = tp.cnt[i] > 0 && tp.L[i] > 0;        // (the projection kernel writes these rows of d sim)
            project = same && (!wanted || bank_use[i]) && bank_stream_projection_supported(tp.H, tp.HP, L[i]);
        }
        if (!project) {
            e = launch_pending_tail_projection(st, true);
            if (e != hipSuccess) return api_hip_fail("deferred tail projection launch", e);
            // it writes the d sim every degree's kernels read, and the helpers' fork point was recorded in front of it: a degree
            // on a helper stream (generic or LDS kernels) would read grad_out before it is written
            e = fj.fork_here();
            if (e != hipSuccess) return api_hip_fail("stream fork", e);
        }
    }
    bool bank_on_main = false;                       // some bank gradient was computed on the caller's stream
    for (int i = 0; i < 4; ++i) {                    // (the launch order of the degrees makes no measurable difference)
        const int d = i + 1;
        const BwdArgs& a = bank_a[i];
        hipStream_t dst = fj.stream(fj.two_way ? 0 : slot_of[i], &e);
        if (e != hipSuccess) return api_hip_fail("stream fork", e);
        int nchunk = a.n > 0 ? a.nchunk : 0;
        int ntheta = -1;
        if (plan.deg[i] == BWD_ZERO_FILL) {
            e = hipMemsetAsync(a.contrib + (size_t)a.contrib_base * a.CS, 0, (size_t)a.n * (d + 1) * a.CS * sizeof(float), dst);
            if (e != hipSuccess) return api_hip_fail("contribution rows memset", e);
        } else if (plan.deg[i] == BWD_GENERIC) {
            e = launch_backward_generic(d, a, dst);
            bank_on_main = true;
        } else if (plan.deg[i] >= BWD_LDS_PAIR) {
            const bool rows_mfma = plan.deg[i] != BWD_LDS_PAIR;
            hipStream_t st_rows = dst, st_bank = dst;
            if (fj.two_way && !rows_mfma) bank_on_main = true;
            if (fj.two_way && rows_mfma) {
                st_rows = st;
                if (!fuse_bank) {                        // (fused: the bank kernels are launched below, behind the pre-pass's re-fork)
                    st_bank = fj.stream(1, &e);
                    if (e != hipSuccess) return api_hip_fail("stream fork", e);
                }
            }
            // (without grad_x nobody reads contribution rows: the fused bank gradients sum the score-weight partials themselves)
            if (rows_mfma && !rows_streamed && (grad_x || !fuse_bank)) {
                e = launch_backward_rows_mfma(d, a, &ntheta, st_rows);
                if (e != hipSuccess) return api_hip_fail("kernelconv backward launch", e);
            }
            if (!fuse_bank) e = launch_backward_lds(d, a, &nchunk, &ntheta, !rows_mfma, st_bank);     // (fused: below, all degrees together)
        }
        if (e != hipSuccess) return api_hip_fail("kernelconv backward launch", e);
        BankReduceArgs& r = reduce[i];
        r.nchunk = nchunk;
        if (ntheta >= 0) { r.theta_src = a.theta_slab; r.theta_stride = 4; r.theta_count = ntheta; }
        else {
            r.theta_src = a.slab + (size_t)L[i] * F + (size_t)L[i] * d * F + (size_t)L[i] * d * E;
            r.theta_stride = bank_floats(d, L[i], F, E); r.theta_count = nchunk;
        }
    }
    BankStreamLaunch bsl;
    int nchunk4[4] = {0, 0, 0, 0}, ntheta4[4] = {0, 0, 0, 0};
    if (streamed) {
        // the pre-pass first, on the caller's stream: its records (dL/dsc and permutation ids in tile order) feed both
        // the rows kernel here and the bank kernel on the helper
        plan_backward_bank_stream(bank_a, bank_use, e_unit4, coefq4, nchunk4, ntheta4, through_nei, &bsl);
        bsl.x_split = rows_split ? 1 : 0;
        if (project) { bsl.a.proj_dz = tp.dz; bsl.a.proj_w1 = tp.w1; bsl.a.proj_H = tp.H; bsl.a.proj_HP = tp.HP; bsl.a.proj_K = tp.K; }
        if (project && switches().tail_project_in_prepass >= 2) {
            // the dW1 half of the projection (its slabs are what the deferred reduction sums) needs d z and sim only: the helper
            // is forked in FRONT of the pre-pass for it, so that it runs beside the pre-pass and not beside the rows kernel, in
            // front of the reduction and the bank kernel, which it held up there (47 us; measured)
            e = fj.refork(1);
            if (e != hipSuccess) return api_hip_fail("stream fork", e);
            e = launch_pending_tail_projection(fj.p->aux[0], false);
            if (e != hipSuccess) return api_hip_fail("deferred tail projection launch", e);
        }
        { BwdTimer t(st, 0); e = launch_coef_prepare(bsl, st); }
        if (e != hipSuccess) return api_hip_fail("coefficient pre-pass launch", e);
        e = fj.refork(1);
        if (e != hipSuccess) return api_hip_fail("stream fork", e);
    }
    if (rows_streamed && any_bank && grad_x) {
        BwdTimer t(st, 1);
        e = launch_backward_rows_stream(bank_a, bank_use, streamed ? coefq4 : nullptr, st);
        if (e != hipSuccess) return api_hip_fail("streamed rows launch", e);
    }
    if (any_bank) {
        hipStream_t st_bank = fj.stream(1, &e);      // the helper (the caller's stream when nothing is forked)
        if (e != hipSuccess) return api_hip_fail("stream fork", e);
        if (project) {                               // (no-op where the early fork in front of the pre-pass has launched it)
            e = launch_pending_tail_projection(st_bank, false);
            if (e != hipSuccess) return api_hip_fail("deferred tail projection launch", e);
        }
        if (st_bank != st) {                         // a fused tail's deferred reduction rides in front of the bank kernel
            e = launch_pending_tail_reduce(st_bank);
            if (e != hipSuccess) return api_hip_fail("deferred tail reduction launch", e);
        }
        {
            BwdTimer t(st_bank, 2);
            if (streamed) e = launch_backward_bank_stream(bsl, st_bank);
            else e = launch_backward_bank_fused(bank_a, bank_use, nchunk4, ntheta4, st_bank);
        }
        if (e != hipSuccess) return api_hip_fail("fused bank gradient launch", e);
        for (int i = 0; i < 4; ++i)
            if (bank_use[i]) {
                reduce[i].nchunk = nchunk4[i];
                reduce[i].theta_src = bank_a[i].theta_slab; reduce[i].theta_stride = 4; reduce[i].theta_count = ntheta4[i];
            }
    }
    // two chains: the reduce follows the bank kernels on the helper, the gather follows the rows kernels here
    const bool split = fj.two_way && !bank_on_main && fj.used[0];
    if (!split) {
        e = fj.end();
        if (e != hipSuccess) return api_hip_fail("stream join", e);
    }
    hipStream_t st_reduce = st;
    if (split) {
        st_reduce = fj.stream(1, &e);
        if (e != hipSuccess) return api_hip_fail("stream fork", e);
    }
    { BwdTimer t(st_reduce, 3); e = launch_bank_reduce_all(reduce, st_reduce); }   // one launch for the four banks
    if (e != hipSuccess) return api_hip_fail("bank gradient reduce launch", e);
    if (grad_x && n_edges == 0) {
        if (n_atoms) e = hipMemset2DAsync(grad_x, (size_t)grad_x_stride * sizeof(float), 0, (size_t)F * sizeof(float), (size_t)n_atoms, st);
        if (e != hipSuccess) return api_hip_fail("zero input gradient", e);
    } else if (grad_x) {
        BwdTimer t(st, 4);
        if (gb_gather) {
            e = launch_backward_gather_grad_blocks((const float*)(ws + w.contrib), (F + 3) / 4 * 4, scatter_rowptr, scatter_rows, x, x_stride,
                                                   inv_norm, n_atoms, F, grad_x, grad_x_stride, st, rows_split, gb);
            if (e == hipSuccess) g_grad_blocks_launches.fetch_add(1);
        } else
        e = launch_backward_gather((const float*)(ws + w.contrib), (F + 3) / 4 * 4, base, scatter_rowptr, scatter_rows, x,
                                   x_stride, inv_norm, n_atoms, F, grad_x, grad_x_stride, variant != 1, st, rows_split);
        if (e != hipSuccess) return api_hip_fail("backward gather launch", e);
    }
    if (split && defer_bank && fj.used[0] && !fj.used[1] && !fj.used[2]) {
        fj.p->deferred = true;                       // the caller joins (mkgnn_backward_join), after the last layer's backward
    } else if (split) {
        e = fj.end();
        if (e != hipSuccess) return api_hip_fail("stream join", e);
    }
    return 0;
}

int mkgnn_backward_streams(const mkgnn_kernel_bank banks[MKGNN_MAX_DEGREE], const mkgnn_degree_bucket buckets[MKGNN_MAX_DEGREE],
                           const float* x, int64_t x_stride, int64_t n_atoms, int32_t F, int32_t E) {
    if (!banks || !buckets) return 0;
    return plan_conv_backward(conv_shape(banks, buckets, F, E, n_atoms, x, x_stride, 0), 0).covers ? 1 : 0;
}

int mkgnn_rows_split_supported(const mkgnn_kernel_bank banks[MKGNN_MAX_DEGREE], const mkgnn_degree_bucket buckets[MKGNN_MAX_DEGREE],
                               int64_t x_stride, int64_t out_stride, int64_t n_atoms, int32_t F, int32_t E) {
    if (!banks || !buckets || F < 1 || E < 1) return 0;
    const ConvShape s = conv_shape(banks, buckets, F, E, n_atoms, nullptr, x_stride, out_stride);
    return rows_split_covered(s, plan_conv_forward(s, 0)) ? 1 : 0;
}

// Diagnostics: the family every degree of a forward / backward call with these arguments would take -- the same ConvShape and the
// same two plan functions as the entry points, nothing enqueued.  out[0..3] FwdFamily, out[4..7] BwdFamily, out[8..10] = bank_fused,
// rows_streamed, bank_streamed.  (variants as the entry points take them, flags masked off; want_grad_x == 0: as grad_x == NULL)
int mkgnn_debug_conv_dispatch(const mkgnn_kernel_bank banks[MKGNN_MAX_DEGREE], const mkgnn_degree_bucket buckets[MKGNN_MAX_DEGREE],
                              const float* x, int64_t x_stride, int64_t out_stride, int64_t n_atoms, int32_t F, int32_t E,
                              int32_t fwd_variant, int32_t bwd_variant, int32_t want_grad_x, const float* grad_x, int64_t grad_x_stride,
                              int32_t out[11]) {
    const char* who = "mkgnn_debug_conv_dispatch";
    if (!banks || !buckets || !out) return api_fail("%s: null pointer", who);
    fwd_variant &= ~(MKGNN_VARIANT_BLOCK_ROWS | MKGNN_VARIANT_BANK_PREPARED | MKGNN_VARIANT_ROWS_SPLIT);
    bwd_variant &= ~(MKGNN_BACKWARD_DEFER_BANK | MKGNN_BACKWARD_THROUGH_NEIGHBOURS | MKGNN_BACKWARD_ROWS_SPLIT);
    if (fwd_variant < 0 || fwd_variant > 3 || bwd_variant < 0 || bwd_variant > 2)
        return api_fail("%s: variants %d / %d", who, fwd_variant, bwd_variant);
    const FwdDispatch fwd = plan_conv_forward(conv_shape(banks, buckets, F, E, n_atoms, x, x_stride, out_stride), fwd_variant);
    const BwdDispatch bwd = plan_conv_backward(conv_shape(banks, buckets, F, E, n_atoms, x, x_stride, 0, want_grad_x ? grad_x : nullptr,
                                                          grad_x_stride), bwd_variant);
    for (int i = 0; i < 4; ++i) { out[i] = fwd.deg[i]; out[4 + i] = bwd.deg[i]; }
    out[8] = bwd.bank_fused; out[9] = bwd.rows_streamed; out[10] = bwd.bank_streamed;
    return 0;
}

int mkgnn_backward_join(void* stream) {
    DegreeStreams* p = degree_streams();
    if (!p || !p->deferred) return 0;
    p->deferred = false;
    hipError_t e = hipEventRecord(p->join[0], p->aux[0]);
    if (e == hipSuccess) e = hipStreamWaitEvent((hipStream_t)stream, p->join[0], 0);
    return e == hipSuccess ? 0 : api_hip_fail("mkgnn_backward_join", e);
}

int mkgnn_segment_sum_rows(const float* in, int64_t in_stride, const int32_t* rowptr, const int32_t* col, int64_t n_rows,
                           int32_t width, float* out, int64_t out_stride, float* inv_norm, void* stream) {
    if (n_rows < 0 || width <= 0 || width > 16384 || in_stride < width || out_stride < width)
        return api_fail("mkgnn_segment_sum_rows: bad shape");
    if (n_rows && (!in || !rowptr || !out)) return api_fail("mkgnn_segment_sum_rows: null pointer");
    hipError_t e = launch_segment_sum(in, in_stride, rowptr, col, n_rows, width, out, out_stride, inv_norm, (hipStream_t)stream);
    return e == hipSuccess ? 0 : api_hip_fail("mkgnn_segment_sum_rows", e);
}

int mkgnn_segment_sum_block_rows(const float* in, int64_t in_stride, const int32_t* rowptr, const int32_t* col,
                                 const int8_t* degree, int64_t n_rows, const int32_t num_kernels[MKGNN_MAX_DEGREE],
                                 int32_t mode, float* out, int64_t out_stride, float* inv_norm, void* stream) {
    const char* who = "mkgnn_segment_sum_block_rows";
    if (mode < 1 || mode > 3) return api_fail("%s: mode %d (1 = block-row sources, 2 = block-row destinations, 3 = 1 with pre-split output)", who, mode);
    if (mode == 3 && !inv_norm) return api_fail("%s: mode 3 (pre-split rows) needs inv_norm", who);
    if (!num_kernels) return api_fail("%s: num_kernels is null", who);
    int width = 0;
    for (int i = 0; i < MKGNN_MAX_DEGREE; ++i) {
        if (num_kernels[i] < 0 || num_kernels[i] > 255) return api_fail("%s: num_kernels[%d] = %d outside 0..255", who, i, num_kernels[i]);
        width += num_kernels[i];
    }
    if (n_rows < 0 || width <= 0 || in_stride < width || out_stride < width) return api_fail("%s: bad shape", who);
    if (n_rows == 0) return 0;
    if (!in || !rowptr || !col || !out || (mode == 2 && !degree)) return api_fail("%s: null pointer", who);
    if (!segment_sum_blocks_supported(in, in_stride, n_rows, width, out, out_stride))
        return api_fail("%s: needs 16-byte aligned rows (strides multiples of 4 floats), at most 255 columns and fewer than 2^28 rows", who);
    hipError_t e = launch_segment_sum_blocks(in, in_stride, rowptr, col, degree, n_rows, width, num_kernels, mode, out, out_stride,
                                             inv_norm, (hipStream_t)stream);
    return e == hipSuccess ? 0 : api_hip_fail(who, e);
}

}  // extern "C"
