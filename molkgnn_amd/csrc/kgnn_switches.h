// Every MKGNN_* environment switch the library reads, parsed once per process at the first use of any of them (not at library
// load: tools set os.environ before their first call).  The only getenv of csrc/; INTEGRATION.md has the table.  Run-time
// overrides (mkgnn_debug_set_*_products, mkgnn_debug_set_grid_caps) stay with their kernels and win over the values here.
#pragma once
#include <stdio.h>
#include <stdlib.h>

// compile-time defaults of the switches below (make EXTRA=-DMKGNN_FWD_PP_DEFAULT=1 ...)
#ifndef MKGNN_FWD_PP_DEFAULT
#define MKGNN_FWD_PP_DEFAULT 0
#endif
#ifndef MKGNN_FWD_PAIR_DEFAULT
#define MKGNN_FWD_PAIR_DEFAULT 0
#endif
#ifndef MKGNN_FWD_SPLIT_DEFAULT
#define MKGNN_FWD_SPLIT_DEFAULT 1
#endif
#ifndef MKGNN_BWD_SPLIT_DEFAULT
#define MKGNN_BWD_SPLIT_DEFAULT 1
#endif

namespace mkgnn {

struct Switches {        // (bool: is set, or on unless the value starts with '0' where the comment says "=0"; int: atoi)
    bool serial;              // MKGNN_SERIAL (is set): every kernel of a call on the caller's stream, no helper streams
    bool fork_in_graph;       // MKGNN_FORK_IN_GRAPH (is set): one helper stream per degree inside a hipGraph capture too
    bool no_mfma_bwd;         // MKGNN_NO_MFMA_BWD (is set): backward on the LDS rows kernel, per degree (A/B against the MFMA rows kernels)
    bool fork_mode;           // MKGNN_FORK_MODE=0: no helper stream inside a hipGraph capture (default: one, the bank chain's)
    bool bank_fused;          // MKGNN_BANK_FUSED=0: one bank-gradient launch per degree
    bool rows_stream;         // MKGNN_ROWS_STREAM=0: one kc_backward_rows_mfma launch per degree, not the streamed rows kernel
    bool bank_stream;         // MKGNN_BANK_STREAM=0: the LDS / VALU bank-gradient kernel, not the streamed MFMA one
    bool fwd_stream;          // MKGNN_FWD_STREAM=0: round 1's LDS-bank forward kernel, not the streamed one
    bool bf16_stream;         // MKGNN_BF16_STREAM=0: the bf16 forward variant stays on the LDS-bank kernel
    bool rows_split;          // MKGNN_ROWS_SPLIT=0: mkgnn_rows_split_supported answers 0 (no pre-split rows)
    bool grad_blocks;         // MKGNN_GRAD_BLOCKS=0: mkgnn_backward_grad_blocks is ignored (the backward writes whole rows of d loss / d h)
    int tail_project_in_prepass;    // MKGNN_TAIL_PROJECT_IN_PREPASS: 0 = the fused tail's d sim projection stays a launch of its own (A/B);
                                    //   1 = its dW1 half on the helper stream behind the pre-pass's fork, in front of the deferred reduction;
                                    //   2 (unset) = the helper forked in front of the pre-pass for it: it runs beside the pre-pass
    bool bn_one_launch;       // MKGNN_BN_ONE_LAUNCH=1 (starts with '1'): batch norm statistics | grid barrier | apply in one launch (it lost)
    bool bn_merge;            // MKGNN_BN_MERGE=0: the batch norm merges its block partials in the loop form at every width (A/B; the same bits)
    char helper_priority;     // MKGNN_HELPER_PRIORITY=low / high (first character): the helper streams at the least / greatest priority (0: default)
    int fwd_pp;               // MKGNN_FWD_PP: 1 = ping-pong forward blocks where they apply (unset: MKGNN_FWD_PP_DEFAULT)
    bool fwd_pp_env;          //   ... set to a non-zero value in the environment: no pre-split rows
    int fwd_split;            // MKGNN_FWD_SPLIT: 0 = the streamed forward's products in fp32 (unset: MKGNN_FWD_SPLIT_DEFAULT)
    int bwd_split;            // MKGNN_BWD_SPLIT: 0 = the streamed backward kernels' products in fp32 (unset: MKGNN_BWD_SPLIT_DEFAULT)
    int fwd_pair;             // MKGNN_FWD_PAIR: distance of the streamed forward's block pairs (unset: MKGNN_FWD_PAIR_DEFAULT)
    int rows_stream_blocks;   // MKGNN_ROWS_STREAM_BLOCKS: grid cap of the streamed rows kernel (0: unset; the launch checks the range)
    int bank_stream_blocks;   // MKGNN_BANK_STREAM_BLOCKS: grid cap of the streamed bank kernel (0: unset; the launch checks the range)
    int bank_blocks;          // MKGNN_BANK_BLOCKS: blocks of the per-degree LDS bank kernel (0: unset; the launch checks the range)
    int csr_blocks;           // MKGNN_CSR_BLOCKS: grid cap of the segment-sum / gather kernels (unset: 4096)
    int csr_fixed4;           // MKGNN_CSR_FIXED4: fixed-degree variant of the pipelined gather (unset: 0)
    int csr_cpl;              // MKGNN_CSR_CPL: 1 / 2 = every segment-sum / gather launch with one / two row chunks per lane (unset: per kind)
    bool stream_cost_set;     // MKGNN_STREAM_COST: cost per tile and degree for the streamed forward's block split (all four parsed)
    double stream_cost[4];
};

inline const Switches& switches() {
    static const Switches table = [] {
        auto is_set = [](const char* name) { return getenv(name) != nullptr; };
        auto not_0 = [](const char* name) { const char* e = getenv(name); return !(e && e[0] == '0'); };
        auto number = [](const char* name, int unset) { const char* e = getenv(name); return e ? atoi(e) : unset; };
        Switches s{};
        s.serial = is_set("MKGNN_SERIAL"); s.fork_in_graph = is_set("MKGNN_FORK_IN_GRAPH"); s.no_mfma_bwd = is_set("MKGNN_NO_MFMA_BWD");
        s.fork_mode = not_0("MKGNN_FORK_MODE"); s.bank_fused = not_0("MKGNN_BANK_FUSED"); s.rows_stream = not_0("MKGNN_ROWS_STREAM");
        s.bank_stream = not_0("MKGNN_BANK_STREAM"); s.fwd_stream = not_0("MKGNN_FWD_STREAM"); s.bf16_stream = not_0("MKGNN_BF16_STREAM");
        s.rows_split = not_0("MKGNN_ROWS_SPLIT"); s.grad_blocks = not_0("MKGNN_GRAD_BLOCKS"); s.tail_project_in_prepass = number("MKGNN_TAIL_PROJECT_IN_PREPASS", 2);
        if (const char* e = getenv("MKGNN_BN_ONE_LAUNCH")) s.bn_one_launch = e[0] == '1';
        s.bn_merge = not_0("MKGNN_BN_MERGE");
        if (const char* e = getenv("MKGNN_HELPER_PRIORITY")) s.helper_priority = e[0];
        s.fwd_pp = number("MKGNN_FWD_PP", MKGNN_FWD_PP_DEFAULT); s.fwd_pp_env = number("MKGNN_FWD_PP", 0) != 0;
        s.fwd_split = number("MKGNN_FWD_SPLIT", MKGNN_FWD_SPLIT_DEFAULT); s.bwd_split = number("MKGNN_BWD_SPLIT", MKGNN_BWD_SPLIT_DEFAULT);
        s.fwd_pair = number("MKGNN_FWD_PAIR", MKGNN_FWD_PAIR_DEFAULT); s.bank_blocks = number("MKGNN_BANK_BLOCKS", 0);
        s.rows_stream_blocks = number("MKGNN_ROWS_STREAM_BLOCKS", 0); s.bank_stream_blocks = number("MKGNN_BANK_STREAM_BLOCKS", 0);
        s.csr_blocks = number("MKGNN_CSR_BLOCKS", 256 * 16); s.csr_fixed4 = number("MKGNN_CSR_FIXED4", 0);
        s.csr_cpl = number("MKGNN_CSR_CPL", 0);
        if (const char* e = getenv("MKGNN_STREAM_COST"))
            s.stream_cost_set = sscanf(e, "%lf,%lf,%lf,%lf", &s.stream_cost[0], &s.stream_cost[1], &s.stream_cost[2], &s.stream_cost[3]) == 4;
        return s;
    }();
    return table;
}

}  // namespace mkgnn
