/*
 * molkgnn_hip.h -- C ABI of the MI355X (gfx950) molecular-kernel convolution.
 *
 * This is the drop-in boundary for ONE path of LanceKnight/MolKGNN: the
 * degree-bucketed atom-neighbourhood x learnable-kernel similarity
 * (reference models/MolKGNN/kernels.py, KernelConv / KernelSetConv) and its
 * immediate caller's neighbour sum (models/MolKGNN/KernelLayer.py, MolGCN).
 * The reference has no FFI of its own (it is pure Python over ATen); the entry
 * points below are what a binding for this path would bind, one per reference
 * function, and INTEGRATION.md shows the ctypes stub.
 *
 * Conventions
 *   - plain C, no torch types; every pointer is a DEVICE pointer unless it says host;
 *   - floats are fp32, indices int64 exactly as the reference's tensors hold them;
 *   - the caller owns every buffer (inputs, outputs, workspace); nothing is
 *     allocated or freed inside, no call synchronises, every kernel is launched
 *     on `stream` (a hipStream_t passed as void*), so calls are graph-capturable;
 *   - return 0 on success, non-zero on a rejected argument or a launch error;
 *     mkgnn_last_error() then describes it (thread-local, host pointer);
 *   - no state is kept between calls except lazily created helper streams / events (one set per device,
 *     created under std::call_once); calls on DIFFERENT devices or different streams of one device may run from
 *     different host threads, but mkgnn_kernelsetconv_backward forks onto the device's helper streams, so at
 *     most one host thread per device may be inside it at a time (PyTorch's autograd engine guarantees that:
 *     one backward thread per device).
 *
 * Shapes use the reference's names: N atoms in the batch, F node-attribute
 * width, E edge-attribute width, D = 3 coordinates, d = degree (1..4),
 * N_d atoms of degree d, L_d kernels of degree d, K = L_1+L_2+L_3+L_4.
 */
#ifndef MOLKGNN_HIP_H
#define MOLKGNN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MKGNN_MAX_DEGREE 4
#define MKGNN_ABI_VERSION 8

/* Loss kinds of the single-task head (ABI v8): the loss over the n counted molecules and its d loss / d pred_g.
 *   BCE_MEAN    mean of BCEWithLogits (data.py:37)          (sigmoid(p) - y) / n
 *   SQERR_MEAN  sum (p - y)^2 / n     (MSELoss())           2 (p - y) / n
 *   SQERR_SUM   sum (p - y)^2         (MSELoss(reduction='sum'): the docking-score task, data.py:49-53)   2 (p - y) */
#define MKGNN_LOSS_BCE_MEAN 0
#define MKGNN_LOSS_SQERR_MEAN 1
#define MKGNN_LOSS_SQERR_SUM 2

/* One KernelConv's parameters (reference kernels.py:50-84).  The three score
 * weights are the 0-d parameters support_attr_sc_weight, center_attr_sc_weight
 * and edge_attr_support_sc_weight; length_sc_weight / angle_sc_weight are never
 * read by the reference's forward (kernels.py:402-422) and are not passed. */
typedef struct mkgnn_kernel_bank {
    int32_t num_kernels;              /* L_d; 0 = this degree has no kernels       */
    int32_t reserved;
    const float* x_center;            /* [L_d, F]                                   */
    const float* x_support;           /* [L_d, d, F]                                */
    const float* edge_attr_support;   /* [L_d, d, E]                                */
    const float* p_support;           /* [L_d, d, 3]  (read only for d = 4, last layer) */
    const float* support_attr_sc_weight;      /* [1] */
    const float* center_attr_sc_weight;       /* [1] */
    const float* edge_attr_support_sc_weight; /* [1] */
} mkgnn_kernel_bank;

/* Gradients of one bank; same shapes.  p_support has no gradient in the
 * reference (kernels.py:279-350 is not differentiable) and has no slot. */
typedef struct mkgnn_kernel_bank_grad {
    float* x_center;
    float* x_support;
    float* edge_attr_support;
    float* support_attr_sc_weight;
    float* center_attr_sc_weight;
    float* edge_attr_support_sc_weight;
} mkgnn_kernel_bank_grad;

/* One degree's receptive fields, the tensors ToXAndPAndEdgeAttrForDeg produces
 * (reference wrapper.py:596-635) after PyG collation. */
typedef struct mkgnn_degree_bucket {
    int64_t count;                    /* N_d                                         */
    const int64_t* selected_index;    /* [N_d]      focal atom ids                   */
    const int64_t* nei_index;         /* [N_d * d]  neighbour atom ids, edge-list order */
    const float* nei_edge_attr;       /* [N_d, d, E] raw bond attributes             */
    const float* p_focal;             /* [N_d, 3]   (d = 4, last layer only; else may be NULL) */
    const float* nei_p;               /* [N_d, d, 3] (same)                          */
    const float* nei_edge_unit;       /* [N_d, d, 8] nei_edge_attr / max(|.|, 1e-8), zero padded (mkgnn_unit_rows8; E <= 8);
                                         may be NULL.  The bond attributes of a batch are the same in every layer and every
                                         step: a caller that keeps them (molkgnn_amd.plan does) saves the forward kernel the
                                         per-tile normalisation, and lets it take the streamed kernel */
} mkgnn_degree_bucket;

/* What forward keeps for backward, per degree (caller-allocated). */
typedef struct mkgnn_saved {
    float* pair_state;                /* [N_d, L_d, 4] per (atom, kernel) pair, one 16-byte record: the support score of
                                         the chosen permutation, the centre score, the edge score (kernels.py:357-373,
                                         386-395) and the chosen permutation's index (the bits of an int32).  One record
                                         is one 16-byte store in the forward and one 16-byte load in the backward;
                                         may be NULL (nothing is kept) */
    int8_t* chirality;                /* [N_d, L_d] +1/-1 (d = 4, last layer); may be NULL           */
} mkgnn_saved;

/* ABI history.  v3: pair records (mkgnn_saved.pair_state).  v4: the AdamW state buffer of a tensor is
 * mkgnn_adamw_state_floats(numel) = 2 numel + 3 + ceil(numel / 1024) floats (v3: 2 numel + 3) -- a caller built against
 * v3 would hand mkgnn_adamw_step a buffer its blocks write past, so the version check must refuse it; the
 * molecule-resident small-batch entry points (mkgnn_molecule_*) were added with the same version.  v5: the statistics-only
 * batch-norm companion (mkgnn_bn_stats, mkgnn_batchnorm_update_stats, mkgnn_batchnorm_forward_with_stats).  v6: pre-split rows
 * (MKGNN_VARIANT_ROWS_SPLIT / MKGNN_BACKWARD_ROWS_SPLIT / MKGNN_BN_SPLIT_ROWS, mkgnn_rows_presplit, mode 3 of
 * mkgnn_segment_sum_block_rows) and the fused tail (mkgnn_tail_*).  v7: mkgnn_touch_hint. */
int mkgnn_abi_version(void);
const char* mkgnn_last_error(void);

/* 1 / max(||x_n||, 1e-8) for every row (the cosine normalisation of
 * torch.nn.CosineSimilarity as used at kernels.py:189).  inv_norm: [N]. */
int mkgnn_row_inv_norm(const float* x, int64_t x_stride, int64_t n_rows, int32_t F,
                       float* inv_norm, void* stream);

/* out[r, 0..7] = in[r, 0..E-1] / max(||in[r]||, 1e-8), zero beyond E (E <= 8): the unit bond-attribute rows
 * mkgnn_degree_bucket.nei_edge_unit holds.  in: [n_rows, E] contiguous, out: [n_rows, 8]. */
int mkgnn_unit_rows8(const float* in, int64_t n_rows, int32_t E, float* out, void* stream);

/* Bytes of scratch the two calls below need for these sizes. */
size_t mkgnn_workspace_bytes(const int32_t num_kernels[MKGNN_MAX_DEGREE], int32_t F, int32_t E,
                             int64_t n_atoms, int64_t n_edges);

/* BaseKernelSetConv.forward (kernels.py:610-751) with the per-degree gather
 * (:519-548), KernelConv.calculate_total_score (:353-425) and the reorder to
 * node order (:743-747) fused: out[n, :] for atom n holds the L_d scores of its
 * own degree in columns [off_d, off_d + L_d) and zeros elsewhere.
 *   x        [N, F] with row stride x_stride (floats)
 *   inv_norm [N] from mkgnn_row_inv_norm
 *   out      [N, K] with row stride out_stride, fully overwritten (rows of atoms in no bucket
 *            are zero).  If out_stride holds K rounded up to a multiple of 4, that alignment
 *            padding is zeroed too, so the next layer can read 16-byte rows.
 * variant: 0 = automatic, 1 = generic VALU kernels, 2 = MFMA kernels (exact fp32),
 *          3 = MFMA kernels with bf16 operands for the node-feature dot products (fp32 accumulate; the
 *              "bf16 similarity path": scores within ~1e-3 of the fp32 ones, the chosen order may differ
 *              between near-tied permutations).  2 and 3 fail if a degree's shape is not covered.
 *          | MKGNN_VARIANT_BLOCK_ROWS: the caller will read only each atom's own column block (as
 *              mkgnn_segment_sum_block_rows does): nothing outside the blocks is written, not even zeros. */
#define MKGNN_VARIANT_BLOCK_ROWS 0x100
/*          | MKGNN_VARIANT_BANK_PREPARED: `workspace` already holds this call's normalised kernel bank, written by
 *              mkgnn_bank_prepare for these banks, F and E since the parameters last changed. */
#define MKGNN_VARIANT_BANK_PREPARED 0x200
/*          | MKGNN_VARIANT_ROWS_SPLIT (ABI v6): the rows of `x` are PRE-SPLIT -- written by mkgnn_segment_sum_block_rows mode 3 (or
 *              mkgnn_batchnorm_forward* with MKGNN_BN_SPLIT_ROWS): every four consecutive floats x[4 g .. 4 g + 3] of a row are stored
 *              as the sixteen bytes  fp16 hi(0..3) | fp16 lo(0..3)  of x * 2^(exponent(inv_norm[n]) + 8), hi = fp16(.), lo =
 *              fp16(. - hi) -- the operand the streamed kernels' matrix instructions take, so that no wave converts a row again
 *              (same bytes per row, same strides; the forward's scores are bit for bit those of the fp32 rows).  Such rows
 *              exist only between two calls of this library (the reference's h = propagate(sim_sc), KernelLayer.py:119-123,
 *              kernels.py:527,543).  Needs mkgnn_rows_split_supported(..) == 1; fails otherwise. */
#define MKGNN_VARIANT_ROWS_SPLIT 0x400
/* Rows from OUTSIDE the library in that form (benchmarks, tests; a training step's rows come pre-split from their producers):
 * inv_norm[n] = 1 / max(|x[n]|, 1e-8) exactly as mkgnn_row_inv_norm, out[n] = the pre-split row.  16-byte aligned rows, F <= 256. */
int mkgnn_rows_presplit(const float* x, int64_t x_stride, int64_t n_rows, int32_t F, float* inv_norm, float* out,
                        int64_t out_stride, void* stream);
/* The parameter-only part of `count` (<= 4 per call) forward calls -- unit-normalised kernel rows in the layouts the
 * kernels read, their norms, the chirality sign tables, the mixing weights: reference kernels.py:189, 279-350,
 * 386-395 -- in ONE launch: call k has banks[4 k .. 4 k + 3], feature width F[k], and gets the head of workspaces[k]
 * (a buffer of at least mkgnn_workspace_bytes(..) for that call) filled.  The banks depend on the parameters only, so
 * a model prepares all its layers at the start of a step instead of one small dependent launch per layer. */
int mkgnn_bank_prepare(int32_t count, const mkgnn_kernel_bank* banks, const int32_t* F, int32_t E,
                       void* const* workspaces, const size_t* workspace_bytes, void* stream);
/* The same preparation left PENDING on the current device (ABI v7): nothing is launched; the next mkgnn_batchnorm_forward*
 * (training mode) on this device carries its tasks in blocks behind its own statistics launch -- a launch bound by latency, where
 * they cost nothing, instead of 5 us of launch floor on the chain in front of the first convolution -- or
 * mkgnn_bank_prepare_flush(stream) launches it on its own, whichever comes first (mkgnn_bank_prepare flushes a pending one
 * too).  banks, F and the workspaces are read at the LAUNCH: they must stay as they are until then.  The caller MUST flush (or
 * mkgnn_bank_prepare_withdraw, which returns 1 if one was pending) before the first mkgnn_kernelsetconv_forward with
 * MKGNN_VARIANT_BANK_PREPARED, and before the workspaces go.  One pending preparation per device. */
int mkgnn_bank_prepare_deferred(int32_t count, const mkgnn_kernel_bank* banks, const int32_t* F, int32_t E,
                                void* const* workspaces, const size_t* workspace_bytes);
int mkgnn_bank_prepare_flush(void* stream);
int mkgnn_bank_prepare_withdraw(void);
/* A hint (ABI v7): `count` (<= 16) device arrays that the NEXT call of this host thread to mkgnn_bank_prepare or to
 * mkgnn_batchnorm_forward* (training mode) READS once and discards, with spare blocks of a launch it makes anyway -- the index
 * arrays of the batch the convolutions that follow will gather through (mkgnn_degree_bucket.selected_index / nei_index /
 * nei_edge_unit, the CSR of propagate).  Nothing is computed from them and no result depends on it: after a backward pass has
 * moved a gigabyte through the caches they are cold, and the first convolution of a step -- the one with the least matrix work
 * per fetched row to hide a miss behind -- pays 8-9 us of its 30 for them at the benchmark batch; read beside the batch norm's
 * statistics (a launch bound by latency, not by bandwidth) they cost nothing.  The arrays must stay allocated until that next
 * call's launch has run.  mkgnn_touch_hint(NULL, NULL, 0) withdraws a hint nobody took; returns 1 if there was one, else 0. */
int mkgnn_touch_hint(const void* const* arrays, const size_t* bytes, int32_t count);

int mkgnn_kernelsetconv_forward(const mkgnn_kernel_bank banks[MKGNN_MAX_DEGREE],
                                const mkgnn_degree_bucket buckets[MKGNN_MAX_DEGREE],
                                const float* x, int64_t x_stride, const float* inv_norm,
                                int64_t n_atoms, int32_t F, int32_t E, int32_t is_last_layer,
                                float* out, int64_t out_stride,
                                const mkgnn_saved saved[MKGNN_MAX_DEGREE],
                                void* workspace, size_t workspace_bytes, int32_t variant, void* stream);

/* Gradient of the call above (what autograd derives for the reference).
 *   grad_out  [N, K] (stride grad_out_stride)
 *   scatter   CSR over atoms of the contribution rows that belong to each atom:
 *             contribution rows are numbered bucket by bucket, atom by atom,
 *             (focal, neighbour 0, .., neighbour d-1); scatter_rowptr [N+1],
 *             scatter_rows [sum_d N_d (d+1)] (int32).  Built once per batch by
 *             the host (molkgnn_amd.plan).
 *   grad_x    [N, F] (stride grad_x_stride), fully overwritten
 *   grads     per-degree parameter gradients, fully overwritten.
 *   workspace_from_forward  non-zero: `workspace` is the buffer the forward call of this layer used,
 *             untouched since, with the same banks / shapes: the normalised kernel bank in it is reused
 *             instead of being recomputed.
 *   variant   0 = automatic (the MFMA rows / LDS bank / pipelined gather kernels wherever a degree's shape is
 *             covered, the generic kernels elsewhere), 1 = the generic one-wave-per-atom kernels and the plain
 *             gather for every degree (the A/B reference of the parity tests), 2 = the fast kernels, failing if a
 *             degree with atoms and kernels is not covered by them.
 *             | MKGNN_BACKWARD_DEFER_BANK: `grad_x` is complete in stream order as always, but the kernel-bank
 *             gradients (`grads`) are left running on the device's helper stream when the call returns: they -- and the
 *             buffers their kernels read: x, inv_norm, grad_out, saved, the buckets, the workspace -- must not be
 *             touched until mkgnn_backward_join(stream) has been called.  The next layer's backward (which needs only
 *             grad_x) then overlaps this layer's bank gradients instead of waiting for them: nothing but the optimiser
 *             reads a weight gradient.  Honoured where the call forks at all (inside a hipGraph capture with the fast
 *             kernels); elsewhere the call is complete on return as without the flag and the join is a no-op. */
#define MKGNN_BACKWARD_DEFER_BANK 0x100
/*             | MKGNN_BACKWARD_THROUGH_NEIGHBOURS: `grad_out` is not the gradient of this call's `out` but of
 *             h = propagate(out) (KernelLayer.py:119-123: h[i] = sum over edges j -> i of out[j]), [N, K] like it.  The
 *             gradient of out[n, l] is then the sum of grad_out[m, l] over the targets m of n's edges, which are exactly
 *             the bucket's nei_index entries of n: the kernels' pre-pass sums those d rows itself and the caller skips
 *             the propagate step's own gradient pass.  Needs the streamed kernels for every degree
 *             (mkgnn_backward_streams); fails otherwise. */
#define MKGNN_BACKWARD_THROUGH_NEIGHBOURS 0x200
/*             | MKGNN_BACKWARD_ROWS_SPLIT (ABI v6): `x` is pre-split as in the forward call (MKGNN_VARIANT_ROWS_SPLIT): the bank
 *             kernel takes the halves as they are, the gather that undoes the row normalisation reads x / |x| as (hi + lo)
 *             mantissa(inv_norm) 2^-8.  grad_x is ordinary fp32.  Needs mkgnn_rows_split_supported(..) == 1. */
#define MKGNN_BACKWARD_ROWS_SPLIT 0x400
int mkgnn_kernelsetconv_backward(const mkgnn_kernel_bank banks[MKGNN_MAX_DEGREE],
                                 const mkgnn_degree_bucket buckets[MKGNN_MAX_DEGREE],
                                 const float* x, int64_t x_stride, const float* inv_norm,
                                 int64_t n_atoms, int32_t F, int32_t E, int32_t is_last_layer,
                                 const float* grad_out, int64_t grad_out_stride,
                                 const mkgnn_saved saved[MKGNN_MAX_DEGREE],
                                 const int32_t* scatter_rowptr, const int32_t* scatter_rows,
                                 float* grad_x, int64_t grad_x_stride,
                                 const mkgnn_kernel_bank_grad grads[MKGNN_MAX_DEGREE],
                                 void* workspace, size_t workspace_bytes, int32_t workspace_from_forward,
                                 int32_t variant, void* stream);

/* 1 when a backward call with these banks, buckets and x would run every degree that has atoms and kernels on the
 * streamed kernels (the condition of MKGNN_BACKWARD_THROUGH_NEIGHBOURS), else 0.  Launches nothing. */
int mkgnn_backward_streams(const mkgnn_kernel_bank banks[MKGNN_MAX_DEGREE],
                           const mkgnn_degree_bucket buckets[MKGNN_MAX_DEGREE],
                           const float* x, int64_t x_stride, int64_t n_atoms, int32_t F, int32_t E);

/* 1 when both the forward and the backward call with these banks, buckets and strides take pre-split rows
 * (MKGNN_VARIANT_ROWS_SPLIT / MKGNN_BACKWARD_ROWS_SPLIT): every degree with atoms and kernels on the streamed kernels with the
 * split-fp16 products (rows of at most 112 floats, 16-byte aligned, unit bond rows present).  Launches nothing. */
int mkgnn_rows_split_supported(const mkgnn_kernel_bank banks[MKGNN_MAX_DEGREE],
                               const mkgnn_degree_bucket buckets[MKGNN_MAX_DEGREE],
                               int64_t x_stride, int64_t out_stride, int64_t n_atoms, int32_t F, int32_t E);

/* Makes `stream` wait for every bank-gradient chain that calls with MKGNN_BACKWARD_DEFER_BANK left on this device's
 * helper stream (no-op when there is none).  Graph-capturable: captured, it is the edge that joins the helper branch. */
int mkgnn_backward_join(void* stream);

/* MolGCN.propagate with aggr='add' (KernelLayer.py:14,119-123) as a CSR segment
 * sum: out[i, :] = sum_{k in [rowptr[i], rowptr[i+1])} in[col[k], :].
 * Forward uses the edges grouped by target (col = sources); the gradient is the
 * same call on the edges grouped by source (col = targets).  width <= strides.
 * 16-byte aligned rows (bases, strides % 4 == 0 and >= width rounded up to 4, width <= 256) take the
 * pipelined kernel, which also writes the alignment padding of `out` as zero.
 * inv_norm (may be NULL): also write 1 / max(||out[i]||, 1e-8) -- the next layer's cosine needs it,
 * so the producer of h hands it over instead of a separate pass over h. */
int mkgnn_segment_sum_rows(const float* in, int64_t in_stride, const int32_t* rowptr,
                           const int32_t* col, int64_t n_rows, int32_t width,
                           float* out, int64_t out_stride, float* inv_norm, void* stream);

/* The same sum where one side is the [N, K] output of a kernel convolution, whose row n is non-zero only in the
 * column block of atom n's degree (K = sum of num_kernels, block d = columns [off_d, off_d + num_kernels[d-1])):
 *   mode 1  the gathered rows `in` are block rows (MolGCN.propagate's forward: h = sum of neighbours' sim_sc).  col
 *           entries carry the source atom's degree (0 = in no bucket, contributes nothing) in bits 28..30; only the
 *           source's block is read -- ~K / L_d times fewer bytes per edge -- and memory outside the blocks is never
 *           looked at (the producer may leave it unwritten: MKGNN_VARIANT_BLOCK_ROWS).  out: dense [n_rows, K],
 *           inv_norm as above.  Bit-identical to mkgnn_segment_sum_rows on the zero-filled input.
 *   mode 2  the written rows `out` are block rows (its backward: d sim_sc = sum of the targets' dense d h rows, of
 *           which the convolution's backward reads only atom n's own block).  degree: [n_rows] int8, 0..4; only
 *           that block of out[n] is summed and written, the rest of the row is left untouched.  inv_norm unused.
 *   mode 3  (ABI v6) mode 1 with `out` written PRE-SPLIT (MKGNN_VARIANT_ROWS_SPLIT above; inv_norm required): for a caller whose
 *           only reader of out is the next mkgnn_kernelsetconv_forward / _backward.
 * Rows must be 16-byte aligned (strides multiples of 4 floats); K <= 255; n_rows < 2^28. */
int mkgnn_segment_sum_block_rows(const float* in, int64_t in_stride, const int32_t* rowptr, const int32_t* col,
                                 const int8_t* degree, int64_t n_rows, const int32_t num_kernels[MKGNN_MAX_DEGREE],
                                 int32_t mode, float* out, int64_t out_stride, float* inv_norm, void* stream);

/* ---- the consumers either side of the convolution stack -------------------
 *
 * Readout, reference MolKGNNNet.py:144-146:
 *     out[g] = sum_{n in molecule g} lin2( keep[n] * swish( lin1(h[n]) ) )
 * evaluated as  W2 (sum_n keep[n] * swish(W1 h[n] + b1)) + |g| b2  (lin2 and the add-pool commute).
 * Atoms of one molecule are contiguous (PyG batches): mol_ptr[g] .. mol_ptr[g+1].
 * Limits: F <= 128, H <= 64, G <= 64; h rows 16-byte aligned, h_stride a multiple of 4 and
 * >= F rounded up to 4. */
typedef struct mkgnn_readout_params {
    const float* lin1_weight;   /* [H, F] graph_embedding_lin1.weight */
    const float* lin1_bias;     /* [H] or NULL */
    const float* lin2_weight;   /* [G, H] graph_embedding_lin2.weight */
    const float* lin2_bias;     /* [G] or NULL */
    int32_t F, H, G;
} mkgnn_readout_params;

/* Row stride (floats) of the `pre` and `pooled` buffers below: H rounded up to 32 or 64. */
int32_t mkgnn_readout_hidden_stride(int32_t H);
size_t mkgnn_readout_workspace_bytes(int32_t F, int32_t H, int32_t G, int64_t n_atoms, int64_t n_mols);

/* keep_scale: [n_atoms, H] dropout multipliers (0 or 1/(1-p)), NULL = no dropout.
 * Writes pre [n_atoms, HS] (lin1 output, kept for backward), pooled [n_mols, HS], out [n_mols, G]. */
int mkgnn_readout_forward(const mkgnn_readout_params* params, const float* h, int64_t h_stride,
                          int64_t n_atoms, const int32_t* mol_ptr, int64_t n_mols,
                          const float* keep_scale, float* pre, float* pooled,
                          float* out, int64_t out_stride, void* stream);

/* atom_mol: [n_atoms] molecule id of every atom.  grad_h (may be NULL) is fully overwritten; the four
 * parameter gradients (each may be NULL) are fully overwritten, summed in a fixed order. */
int mkgnn_readout_backward(const mkgnn_readout_params* params, const float* h, int64_t h_stride,
                           int64_t n_atoms, const int32_t* mol_ptr, const int32_t* atom_mol, int64_t n_mols,
                           const float* keep_scale, const float* pre, const float* pooled,
                           const float* grad_out, int64_t grad_out_stride,
                           float* grad_h, int64_t grad_h_stride,
                           float* grad_lin1_weight, float* grad_lin1_bias,
                           float* grad_lin2_weight, float* grad_lin2_bias,
                           void* workspace, size_t workspace_bytes, void* stream);

/* The same readout fed by the BLOCK ROWS of the last kernel convolution instead of by h = propagate(sim)
 * (KernelLayer.py:119-123 followed by MolKGNNNet.py:144-146): both steps are linear and row n of sim is non-zero only in
 * the column block of atom n's degree, so  z[n] = W1[:, block(n)] sim[n, block(n)]  is taken first and the H-wide rows are
 * propagated,  pre = propagate(z) + b1.  Same sums, re-associated; no dense [N, K] h and no gradient of it.
 *   sim [n_atoms, K] block rows (as MKGNN_VARIANT_BLOCK_ROWS leaves them), K = sum num_kernels = params->F, num_kernels <= 64
 *   buckets: only count and selected_index are read (the projection works on 16-atom tiles of one degree bucket, on the
 *   matrix cores); in_* / out_*: mkgnn_plan_build's CSRs of edge_index by target / by source
 *   z, pre (forward), dz (backward): [n_atoms, HS], HS = mkgnn_readout_hidden_stride(H); pooled, gate_sum [n_mols, HS].
 *   gate_sum NULL (inference): pre holds propagate(z), WITHOUT b1.  gate_sum non-NULL (a backward will follow): the forward
 *   leaves  gate = keep_scale * swish'(pre + b1)  IN PLACE of pre and its per-molecule sums in gate_sum; the backward takes
 *   that buffer as `gate` (d loss / d pre = dA[molecule] * gate is formed on the fly inside the propagate^T pass; db1 comes
 *   from gate_sum) and needs neither keep_scale nor pre.  grad_sim: [n_atoms, K] block rows (every atom's own block is
 *   written), may be NULL.
 * Limits: K <= 255, every block <= 64 kernels, H <= 64, G <= 64.  Workspace of the backward:
 * mkgnn_readout_blocks_workspace_bytes. */
size_t mkgnn_readout_blocks_workspace_bytes(int32_t K, int32_t H, int32_t G, int64_t n_mols);
int mkgnn_readout_blocks_supported(int32_t F, int32_t H, int32_t G, const int32_t num_kernels[MKGNN_MAX_DEGREE]);
int mkgnn_readout_blocks_forward(const mkgnn_readout_params* params, const float* sim, int64_t sim_stride,
                                 const int32_t num_kernels[MKGNN_MAX_DEGREE],
                                 const mkgnn_degree_bucket buckets[MKGNN_MAX_DEGREE], int64_t n_atoms,
                                 const int32_t* in_rowptr, const int32_t* in_col, const int32_t* mol_ptr, int64_t n_mols,
                                 const float* keep_scale, float* z, float* pre, float* pooled, float* gate_sum,
                                 float* out, int64_t out_stride, void* stream);
int mkgnn_readout_blocks_backward(const mkgnn_readout_params* params, const float* sim, int64_t sim_stride,
                                  const int32_t num_kernels[MKGNN_MAX_DEGREE],
                                  const mkgnn_degree_bucket buckets[MKGNN_MAX_DEGREE], int64_t n_atoms,
                                  const int32_t* out_rowptr, const int32_t* out_col, const int32_t* mol_ptr,
                                  const int32_t* atom_mol, int64_t n_mols, const float* gate, const float* gate_sum,
                                  const float* pooled, const float* grad_out, int64_t grad_out_stride,
                                  float* dz, float* grad_sim, int64_t grad_sim_stride,
                                  float* grad_lin1_weight, float* grad_lin1_bias, float* grad_lin2_weight,
                                  float* grad_lin2_bias, void* workspace, size_t workspace_bytes, void* stream);

/* ---- the tail of a training step, fused (ABI v6) ----------------------------------------------------------------------
 * Everything behind the last kernel convolution, forward AND backward:
 *     h = propagate(sim)                                  KernelLayer.py:119-123
 *     emb_g = pool_g( lin2( swish( lin1(h) ) ) )          MolKGNNNet.py:144-146   (its dropout: the _readout_dropout entry)
 *     loss = mean_g BCEWithLogits( ffn( dropout(emb_g) ), target_g )     model.py:147-150, 169, 190-198; data.py:37
 * and, for d loss = 1, d loss / d sim (block rows: only every atom's own column block is written -- what the last
 * convolution's backward reads) and the six parameter gradients.  The loss is a mean over molecules, so a molecule's chain
 * back to d loss / d z is taken while it sits in LDS: FOUR launches -- z = W1 sim on the matrix cores; one kernel over chunks
 * of whole molecules for propagate, swish, pool, lin2, head, loss, their gradients and propagate^T; d sim = W1^T d z with the
 * dW1 partials on the matrix cores; one fixed-order reduction of all partial slabs -- in place of the nine of
 * mkgnn_readout_blocks_forward + mkgnn_bce_head_fused + mkgnn_readout_blocks_backward.  Same formulas, same re-associations
 * (project before propagate, pool before lin2), the same dropout mask as mkgnn_bce_head_fused for the same rng_state.
 *   sim         [n_atoms, K] block rows of the last mkgnn_kernelsetconv_forward (MKGNN_VARIANT_BLOCK_ROWS), K = readout.F,
 *               16-byte aligned rows; buckets [MKGNN_MAX_DEGREE]: count and selected_index are read (as the block-row readout)
 *   in_* / out_*  the edges grouped by target (columns = sources) / by source (columns = targets), int32, as for
 *               mkgnn_segment_sum_rows; mol_ptr [n_mols + 1], atom_mol [n_atoms]: atoms of a molecule contiguous, edges inside
 *   n_loss_mols the leading molecules that enter the loss (the rest -- padding molecules -- get zero gradients)
 *   rng_state   {seed, offset} int64, read and advanced by one when dropout_p > 0; rng_used receives what was read
 *   emb         [n_mols, G] or NULL;  pred [n_loss_mols];  loss [1];  grad_sim [n_atoms, K] block rows; grad_* may be NULL
 * Limits: mkgnn_tail_supported (the block-row readout's shapes with H <= 32 and G <= 32); and NO MOLECULE with more than
 * MKGNN_TAIL_MAX_ATOMS atoms or MKGNN_TAIL_MAX_EDGES edges (each way) -- the caller, who knows the molecule sizes, checks;
 * a molecule that breaks the promise is skipped and the loss comes back NaN.  workspace: mkgnn_tail_workspace_bytes. */
#define MKGNN_TAIL_MAX_ATOMS 128
#define MKGNN_TAIL_MAX_EDGES 512
typedef struct mkgnn_tail_args {
    const float* sim; int64_t sim_stride;
    int32_t num_kernels[MKGNN_MAX_DEGREE];
    const mkgnn_degree_bucket* buckets;      /* [MKGNN_MAX_DEGREE] */
    const int32_t* in_rowptr; const int32_t* in_col;
    const int32_t* out_rowptr; const int32_t* out_col;
    const int32_t* mol_ptr; const int32_t* atom_mol;
    int64_t n_atoms, n_mols, n_loss_mols;
    mkgnn_readout_params readout;
    const float* head_weight;   /* [G] ffn.weight */
    const float* head_bias;     /* [1] or NULL */
    const float* target;        /* [n_loss_mols] */
    float dropout_p;
    int64_t* rng_state; int64_t* rng_used;
    float* emb; int64_t emb_stride;
    float* pred; float* loss;
    float* grad_sim; int64_t grad_sim_stride;
    float *grad_lin1_weight, *grad_lin1_bias, *grad_lin2_weight, *grad_lin2_bias, *grad_head_weight, *grad_head_bias;
    /* (ABI v7) != 0: the last launch -- the fixed-order reduction that writes loss, the six parameter gradients and advances the
     * dropout generator; nothing before the optimiser reads any of them -- is NOT made by this call but by the calling thread's next
     * mkgnn_kernelsetconv_backward that forks a helper stream (on that stream, in front of its bank kernel: off the chain the next
     * layer's gradient waits for), or by mkgnn_tail_flush, whichever comes first.  grad_sim is complete when this call's launches
     * are.  The caller MUST call mkgnn_tail_flush(stream) before anything reads those outputs on `stream`. */
    int32_t defer_reduce;
    /* (ABI v8) MKGNN_LOSS_*: the loss of the head (0: BCE with logits, mean -- as before) */
    int32_t loss_kind;
} mkgnn_tail_args;
int mkgnn_tail_supported(int32_t K, int32_t H, int32_t G, const int32_t num_kernels[MKGNN_MAX_DEGREE]);
size_t mkgnn_tail_workspace_bytes(int32_t K, int32_t H, int32_t G, int64_t n_atoms, int64_t n_mols);
int mkgnn_tail_fused(const mkgnn_tail_args* args, void* workspace, size_t workspace_bytes, void* stream);
/* The readout's dropout (MolKGNNNet.py:144-146, drop_ratio: between swish(lin1(h)) and lin2), drawn inside the kernels from the
 * head's generator -- the mask convention below.  A call with head dropout (args->dropout_p), readout dropout or both reads
 * args->rng_state once, copies it to args->rng_used and advances its offset by exactly one (the deferred reduction included);
 * both masks come from that one pair.  readout_dropout_p in [0, 1); 0: mkgnn_tail_fused, bit for bit. */
int mkgnn_tail_fused_readout_dropout(const mkgnn_tail_args* args, float readout_dropout_p, void* workspace, size_t workspace_bytes,
                                     void* stream);
/* The readout dropout mask convention (ABI v8, shared by mkgnn_tail_fused_readout_dropout and mkgnn_molecule_step with
 * MKGNN_MOLECULE_READOUT_DROPOUT): Philox4x32-10 keyed by seed, counter (element / 4, offset), word element % 4 -- the
 * generator of the head's dropout -- at  element = 2^62 + atom * H + h  (atom: the atom's row in the batch; the head's elements
 * are mol * G + j, below 2^62).  u = (word >> 8) / 2^24; dropped when u < p, else scaled by 1 / (1 - p).  A function of
 * (seed, offset, atom, h) alone: not of chunking, and appended padding atoms leave the real atoms' masks as they are.
 * mkgnn_readout_dropout_mask writes those multipliers, keep [n_rows, H] (row stride keep_stride), for the {seed, offset}
 * pair at rng_pair on the device (the rng_used of a call, say); it reads the pair and advances nothing. */
int mkgnn_readout_dropout_mask(const int64_t* rng_pair, int64_t n_rows, int32_t H, float p, float* keep, int64_t keep_stride,
                               void* stream);
/* Launches what a mkgnn_tail_fused call left pending on this device, on `stream` (no-op: nothing): a deferred projection
 * (mkgnn_tail_defer_projection: the full launch, grad_sim and the dW1 partials) first, then the deferred reduction. */
int mkgnn_tail_flush(void* stream);
/* (additive; the ABI version stays 8) One-shot request, per device: the NEXT mkgnn_tail_fused / mkgnn_tail_fused_readout_dropout
 * call on the current device, if it has defer_reduce set, also leaves out its projection launch
 *     grad_sim[n, block(n)] = d z[n] . W1[:, block(n)],   dW1 partials = d z^T sim
 * and keeps it pending beside the reduction.  grad_sim is then NOT written by that call.  The calling thread's next
 * mkgnn_kernelsetconv_backward takes the projection over when it is the reader of grad_sim -- grad_out == grad_sim with the same
 * stride, the streamed kernels without MKGNN_BACKWARD_THROUGH_NEIGHBOURS, MKGNN_BACKWARD_DEFER_BANK, a forked helper stream, the
 * same degree blocks and buckets: its coefficient pre-pass forms every value from d z and W1 itself, in the term order of the
 * projection kernel (its records are bit for bit those of the materialised grad_sim, which is never written), and the dW1
 * partials are launched on the helper stream, in front of the deferred reduction.  Any other mkgnn_kernelsetconv_backward on the
 * device, mkgnn_tail_flush, mkgnn_tail_score, mkgnn_atom_contributions and a further mkgnn_tail_fused* call first make the launch
 * that was left out, on their stream: behind any of them grad_sim is what it would have been.  The flag clears itself with the
 * next mkgnn_tail_fused* call whether that call defers or not.  MKGNN_TAIL_PROJECT_IN_PREPASS=0: requests are ignored. */
int mkgnn_tail_defer_projection(int32_t on);
/* diagnostics: launches since the library was loaded -- out[0] coefficient pre-passes with a projected source, out[1] projection
 * launches that write grad_sim (made by the tail call or materialised later), out[2] projection launches for the dW1 partials only */
int mkgnn_debug_tail_projection_launches(int64_t out[3]);
/* The tail in evaluation mode, forward only (additive; the ABI version stays 8): pred_g = ffn( emb_g ) and emb_g of the formulas
 * above, no dropout, no loss, no gradient -- TWO launches: z = W1 sim on the matrix cores, then the forward phases of the training
 * tail's middle kernel with its work distribution and every summation order.  For the same inputs pred and emb are BIT FOR BIT
 * what mkgnn_tail_fused writes with dropout_p = 0, batches padded to a fixed shape included.
 * Takes mkgnn_tail_args as it is and READS: sim, sim_stride, num_kernels, buckets, in_rowptr, in_col, mol_ptr, atom_mol (must not be
 * NULL; the forward phases do not need its contents), n_atoms, n_mols, n_loss_mols (the leading molecules whose pred is
 * written), readout, head_weight, head_bias (or NULL), emb + emb_stride ([n_mols, G], every row written; or NULL) and pred
 * [n_loss_mols].  EVERYTHING ELSE IS IGNORED and may be NULL / 0: out_rowptr, out_col, target, dropout_p, rng_state, rng_used, loss,
 * grad_*, defer_reduce, loss_kind -- nothing behind those pointers is read or written, and the generator does not advance.
 * Limits: those of mkgnn_tail_fused; a molecule beyond MKGNN_TAIL_MAX_ATOMS / MKGNN_TAIL_MAX_EDGES gets NaN in its pred and its
 * emb row, the others their values.  A reduction that a mkgnn_tail_fused call with defer_reduce left pending on this thread is
 * launched first, on `stream` (as mkgnn_tail_fused does: the workspace may be the one it reads).
 * workspace: mkgnn_tail_score_workspace_bytes (the z rows only; a mkgnn_tail_workspace_bytes buffer is large enough). */
size_t mkgnn_tail_score_workspace_bytes(int32_t K, int32_t H, int32_t G, int64_t n_atoms, int64_t n_mols);
int mkgnn_tail_score(const mkgnn_tail_args* args, void* workspace, size_t workspace_bytes, void* stream);
/* Monte Carlo dropout on the forward-only tail (additive; the ABI version stays 8): n_samples stochastic predictions of every
 * molecule -- evaluation-mode inputs, both dropouts left on -- with their mean, spread and an acquisition value, in TWO launches:
 * z = W1 sim on the matrix cores, then ONE middle kernel.  Both dropouts sit behind the last convolution, so per chunk of
 * molecules the window, the propagate step and swish run once; only what lies behind the masks runs per sample (with
 * readout_dropout_p == 0 only the head's mask and its row sum do; pool and lin2 run once).  No atomics, one writer per output,
 * no process-wide or thread-local state: the call is capturable.
 * The sample convention: sample s, 0 <= s < n_samples, uses the generator pair {seed, offset + s} of rng_pair ({seed, offset},
 * int64 on the device; READ, nothing is advanced).  The readout's elements are 2^62 + atom * H + h, the head's mol * G + j, the
 * keep rule the one of the readout dropout mask convention above.  samples[g * samples_stride + s] is BIT FOR BIT the pred[g]
 * that mkgnn_tail_fused_readout_dropout writes for the same inputs, the same two probabilities (args->dropout_p, the head's;
 * readout_dropout_p) and generator state {seed, offset + s}; with both probabilities 0 every sample is mkgnn_tail_score's pred.
 * A molecule's samples are sums over its own atoms in a fixed order under masks that are functions of (seed, offset + s, atom, h)
 * and (seed, offset + s, mol, j): their bits do not depend on chunking, on the grid, or on padding atoms and molecules appended
 * behind the real ones.
 * The statistics, per molecule from its samples x_0 .. x_{S-1} in sample order, every step one IEEE round-to-nearest float32
 * operation (no fused multiply-add), so that float32 arithmetic on the host reproduces them bit for bit:
 *     sum = +0;  sum = sum + x_s;   mean = sum / S;   q = +0;  d = x_s - mean;  q = q + d * d;
 *     std = S > 1 ? sqrt(q / (S - 1)) : 0  (unbiased);      acq = alpha * mean + beta * std   (two products, one sum)
 * Takes mkgnn_tail_args as mkgnn_tail_score does and reads the same fields, and dropout_p.  args->pred [n_loss_mols] and args->emb
 * are each optional here (NULL: not wanted); when given they receive exactly what mkgnn_tail_score writes, bit for bit.
 * rng_state, rng_used, target, loss, grad_*, out_*, defer_reduce and loss_kind are ignored.  Every pointer of `out` may be NULL;
 * with samples == NULL no [n, S] buffer exists anywhere (a chunk's samples live in LDS).
 * Limits: those of mkgnn_tail_score; 1 <= n_samples <= MKGNN_TAIL_MC_MAX_SAMPLES; both probabilities in [0, 1);
 * samples_stride >= n_samples.  Bad arguments, a NULL rng_pair or out and a workspace that is too small are refused before any
 * launch.  A molecule beyond MKGNN_TAIL_MAX_ATOMS / MKGNN_TAIL_MAX_EDGES gets NaN in every output of its row (samples, mean, std,
 * acq, pred, emb), the others their values.  A reduction or projection that a mkgnn_tail_fused call left pending is launched
 * first, as mkgnn_tail_score does.  workspace: mkgnn_tail_score_mc_workspace_bytes (the z rows). */
#define MKGNN_TAIL_MC_MAX_SAMPLES 64
typedef struct mkgnn_tail_mc_out {
    float* samples; int64_t samples_stride;   /* [n_loss_mols, S] or NULL */
    float* mean; float* std; float* acq;      /* [n_loss_mols] each, or NULL */
    float alpha, beta;                        /* acq = alpha * mean + beta * std */
} mkgnn_tail_mc_out;
size_t mkgnn_tail_score_mc_workspace_bytes(int32_t K, int32_t H, int32_t G, int64_t n_atoms, int64_t n_mols);
int mkgnn_tail_score_mc(const mkgnn_tail_args* args, float readout_dropout_p, int32_t n_samples, const int64_t* rng_pair,
                        const mkgnn_tail_mc_out* out, void* workspace, size_t workspace_bytes, void* stream);

/* (additive; the ABI version stays 8) Every atom's exact share of every logit of the head, in evaluation mode -- why a molecule
 * scores what it scores.  Behind the last kernel convolution lin2, the add-pool and the head are linear, so with
 *     pre_n = b1 + sum_{j -> n} W1[:, block(j)] sim[j, block(j)]        (project, then propagate: the block-row readout)
 *     V = head_weight . lin2_weight  ([T, H]),      c0[t] = head_weight[t, :] . lin2_bias
 * every logit is  pred[g, t] = head_bias[t] + sum_{n in g} c[n, t]  with
 *     contrib[n * contrib_stride + t] = c[n, t] = sum_h V[t, h] swish(pre_n[h]) + c0[t]        for every n < n_atoms, t < T
 * -- exact, additive and complete for any number of tasks; no gradient is involved.  head_bias is not part of it.
 *   sim, sim_stride, num_kernels, buckets, in_rowptr, in_col, readout: as mkgnn_tail_args (buckets: count and selected_index are
 *   read; in_*: the edges by target, columns = sources); head_weight [T, G] with rows head_stride >= G floats apart;
 *   lin1_bias / lin2_bias NULL count as zeros.  Needs neither mol_ptr nor atom_mol: molecules of any size, atoms in no degree
 *   bucket (an isolated atom, a hub of degree >= 5: their z row is zero) and atoms without in-edges (V swish(b1) + c0) included.
 * TWO launches on `stream`, capturable: z = W1 sim into the workspace (the tail's projection, on the matrix cores), then one
 * kernel over atoms.  No atomics, no process-wide or thread-local state, one writer per output; nothing of contrib is written
 * outside [n, 0..T).  A reduction that a mkgnn_tail_fused call with defer_reduce left pending on this thread is launched first
 * (the workspace may be the one it reads).
 * Evaluation order, one per output (kgnn_atom_contrib.hip): V[t][h] and c0[t] by fmaf over g = 0 .. G - 1 from +0.0, formed by
 * every workgroup from the parameters alone; s = +0.0 plus the z rows of n's in-edges, edge by edge in CSR order; pre = s + b1;
 * a = pre * sigmoid(pre) with the tail's sigmoid (v_exp_f32, v_rcp_f32: relative error <= 2^-22 + |pre| 2^-23); lane l of 8 forms
 * V[t][4 l] * a[4 l], then fmaf over 4 l + 1 .. 4 l + 3 (+0.0 at h >= H); the 8 values go through an xor tree (offsets 4, 2, 1);
 * + c0[t].  The BITS of contrib[n, t] therefore depend on the parameters, row t of head_weight and the z rows of n's
 * in-neighbours in CSR order only: not on n_atoms, the atom's place in block or grid, other atoms, T, t's index, contrib_stride
 * or head_stride.
 * Error criterion (the project's own, of the fused tail): against the float64 formula on the same sim,
 * max |got - want| <= 2e-5 max(max |want|, 1e-6) over the [n_atoms, T] result.
 * Limits: mkgnn_tail_supported(K, H, G, num_kernels) and 1 <= T <= MKGNN_ATOM_CONTRIB_MAX_TASKS; n_atoms < 2^31.  Anything else, a
 * null pointer, contrib_stride < T, head_stride < G, misaligned sim rows or a workspace below
 * mkgnn_atom_contributions_workspace_bytes (the z rows: a mkgnn_tail_workspace_bytes buffer of the batch is large enough) returns
 * non-zero with mkgnn_last_error set before any launch.  n_atoms == 0 is a no-op that returns 0. */
#define MKGNN_ATOM_CONTRIB_MAX_TASKS 32
typedef struct mkgnn_atom_contrib_args {
    const float* sim; int64_t sim_stride;
    int32_t num_kernels[MKGNN_MAX_DEGREE];
    const mkgnn_degree_bucket* buckets;      /* [MKGNN_MAX_DEGREE] */
    const int32_t* in_rowptr; const int32_t* in_col;
    int64_t n_atoms;
    mkgnn_readout_params readout;
    const float* head_weight; int64_t head_stride; int32_t T;   /* [T, G] */
    float* contrib; int64_t contrib_stride;                      /* [n_atoms, T] */
} mkgnn_atom_contrib_args;
size_t mkgnn_atom_contributions_workspace_bytes(int32_t K, int32_t H, int32_t G, int64_t n_atoms);
int mkgnn_atom_contributions(const mkgnn_atom_contrib_args* args, void* workspace, size_t workspace_bytes, void* stream);

/* BatchNorm1d over atom rows, reference MolKGNNNet.py:115 (torch.nn.BatchNorm1d semantics: biased
 * variance for the normalisation, unbiased for running_var, running <- running + momentum (batch - running)).
 * training != 0: batch statistics, running_* (may be NULL) updated in place, save_* written.
 * training == 0: running statistics; save_* (may be NULL) receive mean and 1/sqrt(var + eps).
 * inv_norm (may be NULL; needs C <= 32, C % 4 == 0 and 16-byte aligned rows of x and out): also
 * 1 / max(||out row||, 1e-8) per row, bit-identical to mkgnn_row_inv_norm
 * on out -- the first kernel convolution reads the normalised features next (MolKGNNNet.py:115-117).
 * num_batches_tracked (may be NULL): incremented when training != 0 (BatchNorm1d's counter).
 * n_valid_rows (device scalar, may be NULL): only rows [0, *n_valid_rows) enter the batch statistics; the rest of the
 * n_rows rows is padding (normalised like any row, excluded from every sum) -- a batch padded to a fixed shape so that
 * one captured graph serves every batch (molkgnn_amd.padding) keeps the statistics of its real atoms.
 * training | MKGNN_BN_SPLIT_ROWS (ABI v6; with inv_norm): `out` is written PRE-SPLIT (MKGNN_VARIANT_ROWS_SPLIT above) for a caller
 * whose only reader of it is the first mkgnn_kernelsetconv_forward / _backward. */
#define MKGNN_BN_SPLIT_ROWS 2
size_t mkgnn_batchnorm_workspace_bytes(int32_t C);
int mkgnn_batchnorm_forward(const float* x, int64_t x_stride, int64_t n_rows, int32_t C,
                            const float* weight, const float* bias,
                            float* running_mean, float* running_var, float momentum, float eps,
                            int32_t training, float* out, int64_t out_stride,
                            float* save_mean, float* save_invstd, float* inv_norm, int64_t* num_batches_tracked,
                            const int64_t* n_valid_rows, void* workspace, size_t workspace_bytes, void* stream);
/* Statistics-only companion of a batch norm (ABI v5).  The reference runs edge_batch_norm(data.edge_attr) in every
 * forward (MolKGNNNet.py:116); its OUTPUT never reaches the kernel convolution (kernels.py:610-751 ignores edge_attr,
 * SURVEY 8 a-1), but in training mode the call moves the module's running_mean / running_var / num_batches_tracked, and
 * those buffers are state-dict contents.  This is that side effect without the normalised rows: BatchNorm1d's update
 * (biased batch variance -> unbiased for running_var, running <- running + momentum (batch - running), counter + 1).
 *   row_key / key_limit (both or neither; device pointers): row r counts iff row_key[r] < *key_limit -- for a batch padded
 *   to a fixed shape (molkgnn_amd.padding) the bond rows of real atoms are those whose source id edge_index[0][r] is
 *   below n_valid_atoms.
 * mkgnn_batchnorm_update_stats runs it alone (one launch up to 64 K padded elements, three above);
 * mkgnn_batchnorm_forward_with_stats = mkgnn_batchnorm_forward with the companion's rows summed by extra blocks of the same
 * launches (training != 0 only; companion may be NULL).  Workspace: mkgnn_batchnorm_stats_workspace_bytes(companion C). */
typedef struct mkgnn_bn_stats {
    const float* x; int64_t x_stride; int64_t n_rows; int32_t C;
    float* running_mean; float* running_var;      /* [C], updated in place (either may be NULL) */
    float momentum;
    int64_t* num_batches_tracked;                 /* may be NULL */
    const int64_t* row_key; const int64_t* key_limit;
} mkgnn_bn_stats;
size_t mkgnn_batchnorm_stats_workspace_bytes(int32_t C);
int mkgnn_batchnorm_update_stats(const mkgnn_bn_stats* stats, void* workspace, size_t workspace_bytes, void* stream);
int mkgnn_batchnorm_forward_with_stats(const float* x, int64_t x_stride, int64_t n_rows, int32_t C,
                            const float* weight, const float* bias,
                            float* running_mean, float* running_var, float momentum, float eps,
                            int32_t training, float* out, int64_t out_stride,
                            float* save_mean, float* save_invstd, float* inv_norm, int64_t* num_batches_tracked,
                            const int64_t* n_valid_rows, void* workspace, size_t workspace_bytes,
                            const mkgnn_bn_stats* companion, void* companion_workspace, size_t companion_workspace_bytes,
                            void* stream);
/* grad_x (may be NULL), grad_weight, grad_bias (may be NULL) are fully overwritten. */
int mkgnn_batchnorm_backward(const float* grad_out, int64_t grad_out_stride, const float* x, int64_t x_stride,
                             int64_t n_rows, int32_t C, const float* weight,
                             const float* save_mean, const float* save_invstd, int32_t training,
                             float* grad_x, int64_t grad_x_stride, float* grad_weight, float* grad_bias,
                             const int64_t* n_valid_rows, void* workspace, size_t workspace_bytes, void* stream);
/* tests: 0 = the batch norm merges its block partials in the loop form at every width (MKGNN_BN_MERGE=0; this call wins over the
 * environment); 1 = out of registers where a thread's terms fit; negative = back to the default.  Every result of the three
 * calls above is the same bits either way. */
int mkgnn_debug_set_bn_merge(int32_t on);

/* Receptive-field builder: the per-degree tensors of a collated batch, reference
 * wrapper.py:559-672 (ToXAndPAndEdgeAttrForDeg) + PyG collation.  edge_index is [2, M] int64 (row 0 sources, row 1
 * targets), every bond stored as two consecutive directed edges with identical attributes (wrapper.py:152-156).
 *   mkgnn_rf_count  computes the out-degrees and writes the four bucket sizes N_1..N_4 to counts (device, int64[4]);
 *   mkgnn_rf_fill   (same workspace, untouched in between) fills, for d = 1..4, out[d-1]:
 *       selected_index [N_d] ascending atom ids, nei_index [N_d*d] edge targets in edge-list order,
 *       nei_edge_attr [N_d*d, E] attributes of bond 2*(e/2), p_focal [N_d, 3], nei_p [N_d*d, 3];
 *       nei_edge_unit [N_d*d, 8] (if not NULL and E <= 8) the same rows unit-normalised, as mkgnn_unit_rows8 gives them;
 *       out[d-1].count = rows allocated (>= N_d).  Atoms of out-degree 0 or > 4 are in no bucket.
 * Deterministic: integer atomics only choose slots, the <= 4 edge ids of an atom are sorted afterwards. */
size_t mkgnn_rf_workspace_bytes(int64_t n_atoms);
int mkgnn_rf_count(const int64_t* edge_index, int64_t n_atoms, int64_t n_edges,
                   void* workspace, size_t workspace_bytes, int64_t* counts, void* stream);
int mkgnn_rf_fill(const int64_t* edge_index, const float* p, const float* edge_attr,
                  int64_t n_atoms, int64_t n_edges, int32_t E, const void* workspace,
                  const mkgnn_degree_bucket out[MKGNN_MAX_DEGREE], void* stream);

/* Per-batch index plan (the host side keeps it with the batch, molkgnn_amd.plan): for every atom, in ascending original
 * order inside the atom's segment,
 *   scatter  the contribution rows of mkgnn_kernelsetconv_backward that point at it (rows numbered bucket by bucket, atom
 *            by atom, focal then neighbours): scatter_rowptr [N+1], scatter_rows [sum_d N_d (d+1)];
 *   in       the edges that end in it, by source atom: in_rowptr [N+1], in_col [M] (MolGCN.propagate's forward);
 *            in_col_packed (may be NULL): the same with the source's degree bucket in bits 28..30
 *            (mkgnn_segment_sum_block_rows mode 1);
 *   out      the edges that start from it, by target atom: out_rowptr [N+1], out_col [M] (its gradient);
 *   deg8     [N] the degree bucket of every atom (0 = in none).
 * No sort over the batch and no host synchronisation: counts with integer atomics, a scan, slots taken with integer
 * atomics, every segment sorted by one thread -- the result does not depend on the order the atomics ran in.
 * buckets: only count, selected_index and nei_index are read.  N < 2^28, M < 2^31. */
size_t mkgnn_plan_workspace_bytes(int64_t n_atoms, int64_t n_edges, int64_t n_rows);

/* Receptive fields AND index plan in one pass (ABI v5): mkgnn_rf_count + mkgnn_rf_fill + mkgnn_plan_build for a caller that knows the
 * bucket capacities up front (a batch padded to a fixed shape: molkgnn_amd.padding) -- one memset and six kernels instead of
 * two and nine, no host round trip (capturable).  Inputs as mkgnn_rf_fill; out[d-1].count = rows allocated for degree d, which
 * must equal the batch's number of atoms of out-degree d: counts[0..3] (device, int64[6]) receive the real numbers, counts[4]
 * the number of atoms that did not fit (0 for a well-formed call), counts[5] = 0; rows beyond a real size are zero-filled.
 * PRECONDITION: every capacity EQUALS the real count (what a fixed-shape batch guarantees).  With a capacity above the real count
 * the scatter CSR covers the ranked atoms only -- scatter_rowptr[n_atoms] < the allocated rows, the tail of scatter_rows is left
 * unwritten -- which is NOT what mkgnn_plan_build does with zero-filled rows; the caller checks counts[0..3] against its
 * capacities (receptive_field.check_sizes) before trusting the plan.  Outputs as
 * mkgnn_rf_fill (the 20 tensors of wrapper.py:559-672 + the unit bond rows) and as mkgnn_plan_build (contribution rows
 * numbered with the allocated row counts), entry for entry what the separate calls give.  rf_ready_event (a hipEvent_t, may be
 * NULL) is recorded on the stream where the receptive fields are complete (the plan's two kernels follow): the first
 * convolution of a step needs only those. */
size_t mkgnn_index_workspace_bytes(int64_t n_atoms, int64_t n_edges, int64_t n_rows);
int mkgnn_index_build(const int64_t* edge_index, const float* p, const float* edge_attr, int64_t n_atoms, int64_t n_edges,
                      int32_t E, const mkgnn_degree_bucket out[MKGNN_MAX_DEGREE],
                      int32_t* scatter_rowptr, int32_t* scatter_rows, int32_t* in_rowptr, int32_t* in_col,
                      int32_t* in_col_packed, int32_t* out_rowptr, int32_t* out_col, int8_t* deg8, int64_t* counts,
                      void* workspace, size_t workspace_bytes, void* rf_ready_event, void* stream);

/* A collated batch from its compact wire form (what a loader sends over PCIe, molkgnn_amd/shards.py) to the tensors the
 * reference's batch object holds (PyG collation, wrapper.py:152-156):
 *   bond_ij   [n_bonds, 2] int32 batch-local atom ids      -> edge_index [2, 2 n_bonds] int64: bond k as the consecutive
 *                                                             directed edges (i, j), (j, i);
 *   bond_attr [n_bonds, E] uint8 (0..255-valued features)  -> edge_attr [2 n_bonds, E] fp32, the same row for both directions;
 *   mol_ptr   [n_molecules + 1] int32 first atom of every molecule -> batch [n_atoms] int64 and atom_molecule [n_atoms] int32.
 * Any output may be NULL (skipped).  One launch. */
int mkgnn_expand_batch(const int32_t* bond_ij, const uint8_t* bond_attr, int64_t n_bonds, int32_t E,
                       const int32_t* mol_ptr, int64_t n_molecules, int64_t n_atoms,
                       int64_t* edge_index, float* edge_attr, int64_t* batch, int32_t* atom_molecule, void* stream);
int mkgnn_plan_build(const mkgnn_degree_bucket buckets[MKGNN_MAX_DEGREE], int64_t n_atoms, const int64_t* edge_index,
                     int64_t n_edges, int32_t* scatter_rowptr, int32_t* scatter_rows, int32_t* in_rowptr, int32_t* in_col,
                     int32_t* in_col_packed, int32_t* out_rowptr, int32_t* out_col, int8_t* deg8, void* workspace,
                     size_t workspace_bytes, void* stream);

/* (ABI v8, additive) Present blocks.  Between two layers h = propagate(sim_sc), and row n of sim_sc is non-zero only in the column
 * block of atom n's degree: block d of h[j] is +0 unless j has a bond partner of degree d, and the backward of the layer that made
 * h reads block d of d loss / d h[j] under exactly that condition.
 *   present8          [N] the blocks of atom j: the OR of 1 << (deg8[s] - 1) over the edges s -> j (edges from an atom in no bucket
 *                     add nothing; 0 for an atom without such an edge, which the kernels read as "every block");
 *   contrib_present8  [sum_d N_d (d+1)] present8 of every contribution row's target (the rows numbered as in the scatter CSR);
 *                     may be NULL (skipped): no kernel of the step reads it -- it is what a mask on the producer of the
 *                     contribution rows would read -- so it is made on request, not with every plan.
 * One launch, behind the mkgnn_plan_build / mkgnn_index_build whose in_rowptr / in_col_packed it reads (same stream).  buckets:
 * count, selected_index and nei_index are read.  in_col_packed NULL (a batch without edge_index): the arrays are zeroed. */
int mkgnn_plan_present_blocks(const mkgnn_degree_bucket buckets[MKGNN_MAX_DEGREE], int64_t n_atoms, const int32_t* in_rowptr,
                              const int32_t* in_col_packed, int8_t* present8, int8_t* contrib_present8, void* stream);
/* The NEXT mkgnn_kernelsetconv_backward of the calling thread may leave d loss / d x undefined outside the present blocks of every
 * atom: x is such an h, num_kernels the four block widths of its columns (their sum = F), present8 as above, alive until that
 * call's kernels have run.  The call takes the hint whatever it does with it; where its masked gather does not apply (the generic
 * kernels, MKGNN_GRAD_BLOCKS=0, an empty block, more than 255 columns) it writes whole rows, which is always correct.  The values
 * in the present blocks, and every other result of the call, are those of the call without the hint, bit for bit.
 * (NULL, NULL) withdraws a pending hint. */
int mkgnn_backward_grad_blocks(const int8_t* present8, const int32_t num_kernels[MKGNN_MAX_DEGREE]);
/* tests: the number of backward calls since the library was loaded whose gather ran on present blocks only;
 * mkgnn_debug_poison_backward(1): every backward call fills its contribution rows and grad_x with NaN before its first launch */
int64_t mkgnn_debug_grad_blocks_launches(void);
int mkgnn_debug_poison_backward(int32_t enable);
/* tests: which kernel family every degree of a forward / backward call with these arguments would take.  The same decision the
 * two entry points make (shapes, null-ness and alignment only: nothing is read through a pointer, nothing is launched).
 * fwd_variant / bwd_variant as the entry points take them; want_grad_x == 0: as a backward call with grad_x == NULL.
 *   out[0..3]   forward, per degree:  0 skip (no atoms or no kernels), 1 any-shape kernel, 2 LDS-bank kernel, 3 streamed kernel
 *   out[4..7]   backward, per degree: 0 skip, 1 zero fill (atoms without kernels), 2 any-shape kernels, 3 per-degree LDS pair,
 *               4 MFMA rows + LDS bank kernel, 5 streamed pair
 *   out[8..10]  bank gradients of all degrees in one launch; the streamed rows launch; the streamed bank launch */
int mkgnn_debug_conv_dispatch(const mkgnn_kernel_bank banks[MKGNN_MAX_DEGREE], const mkgnn_degree_bucket buckets[MKGNN_MAX_DEGREE],
                              const float* x, int64_t x_stride, int64_t out_stride, int64_t n_atoms, int32_t F, int32_t E,
                              int32_t fwd_variant, int32_t bwd_variant, int32_t want_grad_x, const float* grad_x,
                              int64_t grad_x_stride, int32_t out[11]);

/* Tail of the training step for a single task (reference model.py:147-148, 190-198 with data.py:37):
 *     pred = graph_embedding @ ffn.weight[0] + ffn.bias;   loss = mean(BCEWithLogits(pred, target))
 * forward writes pred [n_rows] and loss [1]; backward takes d loss (one float on the device) and fully overwrites
 * grad_emb [n_rows, H] (may be NULL), grad_weight [H], grad_bias [1] (may be NULL).  Two launches each (block
 * partials, then their sum in a fixed order).  workspace: mkgnn_bce_head_workspace_bytes bytes, not shared by calls
 * that may run concurrently. */
size_t mkgnn_bce_head_workspace_bytes(int64_t n_rows, int32_t H);
int mkgnn_bce_head_forward(const float* emb, int64_t emb_stride, int64_t n_rows, int32_t H,
                           const float* weight, const float* bias, const float* target,
                           float* pred, float* loss, void* workspace, size_t workspace_bytes, void* stream);
int mkgnn_bce_head_backward(const float* emb, int64_t emb_stride, int64_t n_rows, int32_t H,
                            const float* weight, const float* target, const float* pred, const float* grad_loss,
                            float* grad_emb, int64_t grad_emb_stride, float* grad_weight, float* grad_bias,
                            void* workspace, size_t workspace_bytes, void* stream);

/* The same with dropout on the embedding ahead of the product (reference model.py:150,169: nn.Dropout(ffn_dropout_rate)
 * before ffn), generated in the kernels: element (row, h) is zeroed with probability dropout_p in [0, 1), kept values
 * scaled by 1 / (1 - dropout_p).  Counter-based generator (Philox4x32-10) keyed by rng_state = {seed, offset} on the
 * device: forward uses the pair, copies it to rng_used (2 x int64, the backward regenerates the mask from it) and
 * advances offset by one, so a replayed graph draws a fresh mask every time.  dropout_p = 0: the functions above. */
int mkgnn_bce_head_dropout_forward(const float* emb, int64_t emb_stride, int64_t n_rows, int32_t H,
                                   const float* weight, const float* bias, const float* target, float dropout_p,
                                   int64_t* rng_state, int64_t* rng_used, float* pred, float* loss,
                                   void* workspace, size_t workspace_bytes, void* stream);
int mkgnn_bce_head_dropout_backward(const float* emb, int64_t emb_stride, int64_t n_rows, int32_t H,
                                    const float* weight, const float* target, const float* pred,
                                    const float* grad_loss, float dropout_p, const int64_t* rng_used,
                                    float* grad_emb, int64_t grad_emb_stride, float* grad_weight, float* grad_bias,
                                    void* workspace, size_t workspace_bytes, void* stream);

/* Forward of mkgnn_bce_head_dropout_forward AND the gradients of mkgnn_bce_head_dropout_backward for d loss = 1 in one
 * pass (two launches instead of four): the loss ends the graph, so its own gradient is 1 in a training step, and
 * d loss / d pred of a row needs only that row's pred.  grad_emb [n_rows, H] (may be NULL), grad_weight [H], grad_bias [1]
 * (may be NULL) are fully overwritten with the gradients a backward call with *grad_loss == 1 would give, bit for bit.
 * A caller whose d loss is something else scales them.  Same workspace, same dropout generator protocol. */
int mkgnn_bce_head_fused(const float* emb, int64_t emb_stride, int64_t n_rows, int32_t H,
                         const float* weight, const float* bias, const float* target, float dropout_p,
                         int64_t* rng_state, int64_t* rng_used, float* pred, float* loss,
                         float* grad_emb, int64_t grad_emb_stride, float* grad_weight, float* grad_bias,
                         void* workspace, size_t workspace_bytes, void* stream);

/* (ABI v8) The five entry points above for any loss kind (MKGNN_LOSS_*; an unknown kind is an error): same arguments behind
 * loss_kind, same workspace (mkgnn_bce_head_workspace_bytes), same dropout generator protocol and mask, same fixed-order
 * reductions.  loss_kind = MKGNN_LOSS_BCE_MEAN gives the mkgnn_bce_head_* results bit for bit. */
int mkgnn_head_loss_forward(int32_t loss_kind, const float* emb, int64_t emb_stride, int64_t n_rows, int32_t H,
                            const float* weight, const float* bias, const float* target,
                            float* pred, float* loss, void* workspace, size_t workspace_bytes, void* stream);
int mkgnn_head_loss_backward(int32_t loss_kind, const float* emb, int64_t emb_stride, int64_t n_rows, int32_t H,
                             const float* weight, const float* target, const float* pred, const float* grad_loss,
                             float* grad_emb, int64_t grad_emb_stride, float* grad_weight, float* grad_bias,
                             void* workspace, size_t workspace_bytes, void* stream);
int mkgnn_head_loss_dropout_forward(int32_t loss_kind, const float* emb, int64_t emb_stride, int64_t n_rows, int32_t H,
                                    const float* weight, const float* bias, const float* target, float dropout_p,
                                    int64_t* rng_state, int64_t* rng_used, float* pred, float* loss,
                                    void* workspace, size_t workspace_bytes, void* stream);
int mkgnn_head_loss_dropout_backward(int32_t loss_kind, const float* emb, int64_t emb_stride, int64_t n_rows, int32_t H,
                                     const float* weight, const float* target, const float* pred,
                                     const float* grad_loss, float dropout_p, const int64_t* rng_used,
                                     float* grad_emb, int64_t grad_emb_stride, float* grad_weight, float* grad_bias,
                                     void* workspace, size_t workspace_bytes, void* stream);
int mkgnn_head_loss_fused(int32_t loss_kind, const float* emb, int64_t emb_stride, int64_t n_rows, int32_t H,
                          const float* weight, const float* bias, const float* target, float dropout_p,
                          int64_t* rng_state, int64_t* rng_used, float* pred, float* loss,
                          float* grad_emb, int64_t grad_emb_stride, float* grad_weight, float* grad_bias,
                          void* workspace, size_t workspace_bytes, void* stream);

/* (ABI v8, additive) The task-indexed head with masked labels: weight [T, H] and bias [T] (or NULL) of a T-output ffn, and per
 * row i < n_rows ONE task  t_i = task[i]  (row_ids NULL; n_task >= n_rows entries)  or  t_i = task[row_ids[i]]  (task: a table of
 * n_task entries, e.g. one per molecule of a resident shard; row_ids int32 [n_rows]; an id outside [0, n_task) is "no label").
 * A row is labelled when 0 <= t_i < T (-1 by convention otherwise):
 *     pred_i = labelled ? (keep_i * emb_i) . weight[t_i] + bias[t_i] : +0.0
 *     loss   = sum over the labelled rows of the loss kind's term(pred_i, target_i) / max(n_labelled, 1)   (SQERR_SUM: no division)
 * keep: the single-task head's dropout multipliers (element i * H + h of the same generator, same rng_state / rng_used protocol).
 * The gradients are those of that expression: rows of grad_emb without a label, and rows of grad_weight [T, H] / grad_bias [T]
 * (or NULL) of tasks without a labelled row, are exactly zero; with no labelled row at all the loss and every gradient are
 * zero.  target is not used for unlabelled rows; nothing is read at rows >= n_rows.  forward / backward / fused mirror
 * mkgnn_head_loss_dropout_forward / _dropout_backward / _fused (backward: d loss from the device, the mask regenerated from
 * rng_used; fused: forward and the gradients for d loss = 1).  Two launches per call, fixed-order sums, bit-reproducible; T = 1
 * with every row labelled gives the pred of mkgnn_head_loss_dropout_forward bit for bit.  1 <= T <= MKGNN_TASK_HEAD_MAX_TASKS and
 * 1 <= H <= 64, anything else is an error.  workspace: mkgnn_task_head_workspace_bytes (0 outside the limits). */
#define MKGNN_TASK_HEAD_MAX_TASKS 32
size_t mkgnn_task_head_workspace_bytes(int64_t n_rows, int32_t H, int32_t T);
int mkgnn_task_head_forward(int32_t loss_kind, const float* emb, int64_t emb_stride, int64_t n_rows, int32_t H, int32_t T,
                            const float* weight, const float* bias, const float* target, const int32_t* task,
                            const int32_t* row_ids, int64_t n_task, float dropout_p, int64_t* rng_state, int64_t* rng_used,
                            float* pred, float* loss, void* workspace, size_t workspace_bytes, void* stream);
int mkgnn_task_head_backward(int32_t loss_kind, const float* emb, int64_t emb_stride, int64_t n_rows, int32_t H, int32_t T,
                             const float* weight, const float* target, const int32_t* task, const int32_t* row_ids,
                             int64_t n_task, const float* pred, const float* grad_loss, float dropout_p,
                             const int64_t* rng_used, float* grad_emb, int64_t grad_emb_stride, float* grad_weight,
                             float* grad_bias, void* workspace, size_t workspace_bytes, void* stream);
int mkgnn_task_head_fused(int32_t loss_kind, const float* emb, int64_t emb_stride, int64_t n_rows, int32_t H, int32_t T,
                          const float* weight, const float* bias, const float* target, const int32_t* task,
                          const int32_t* row_ids, int64_t n_task, float dropout_p, int64_t* rng_state, int64_t* rng_used,
                          float* pred, float* loss, float* grad_emb, int64_t grad_emb_stride, float* grad_weight,
                          float* grad_bias, void* workspace, size_t workspace_bytes, void* stream);

/* (additive; the ABI version stays 8) The task-indexed head with a weighted loss: a sample weight s_i per row and a positive
 * weight p_t per task (torch's binary_cross_entropy_with_logits(x, y, weight = s, pos_weight = p), reduction 'mean').  For a
 * labelled row with logit x, target y and task t:
 *     BCE, pos_weight NULL :  term = s_i * (max(x, 0) - x y + log1p(e^-|x|))                    d term / d x = s_i * (sigmoid(x) - y)
 *     BCE, pos_weight      :  L = 1 + (p_t - 1) y;  term = s_i * ((1 - y) x + L (log1p(e^-|x|) + max(-x, 0)))
 *                                                                                              d term / d x = s_i * ((1 - y) - L sigmoid(-x))
 *     squared error        :  term = s_i * (x - y)^2                                           d term / d x = s_i * 2 (x - y)
 *     loss = sum of the labelled rows' terms / max(n_labelled, 1)     (SQERR_SUM: no division; NOT divided by the sum of the weights)
 * Without pos_weight the term and its derivative are the unweighted entry points' multiplied by s_i FIRST (before grad_loss and
 * 1 / n_labelled), so weights that are all exactly 1.0f give the unweighted bits.  Weights are plain multipliers and constants:
 * a zero weight gives a zero contribution (and an all-zero grad_emb row), a NaN weight on a labelled row propagates, a weight of
 * an unlabelled row or of a row >= n_rows is never used.  pos_weight with a squared-error kind is an error.
 * mkgnn_task_head_weighted_forward / _backward / _fused take the arguments of mkgnn_task_head_forward / _backward / _fused and
 * `weights` before the workspace; same workspace (mkgnn_task_head_workspace_bytes), same dropout generator protocol, same two
 * launches, same fixed-order sums, same limits.  In these three entry points only, task == NULL means "every row has task 0" and
 * requires T == 1 and row_ids == NULL (n_task is then not looked at): how a single-task model uses the same kernels.  weights ==
 * NULL, or sample_weight and pos_weight both NULL, with task != NULL: the outputs of the unweighted entry point bit for bit (its
 * own kernels are launched).  Refused before any launch, with mkgnn_last_error set: an unknown loss kind, pos_weight with a
 * squared-error kind, task == NULL with T != 1, a non-NULL sample_weight with n_sample_weight < 1 (weight_ids given) or
 * < n_rows (not given), and everything the unweighted entry points refuse (n_rows < 1 among it).  No atomics, no process-wide
 * state, capturable, launched on `stream`. */
typedef struct mkgnn_loss_weights {
    const float*   sample_weight;    /* NULL: every row 1 */
    const int32_t* weight_ids;       /* NULL: sample_weight[i]; else sample_weight[weight_ids[i]], outside [0, n_sample_weight): +0.0 */
    int64_t        n_sample_weight;
    const float*   pos_weight;       /* NULL: 1; [T]; BCE only */
} mkgnn_loss_weights;
int mkgnn_task_head_weighted_forward(int32_t loss_kind, const float* emb, int64_t emb_stride, int64_t n_rows, int32_t H, int32_t T,
                                     const float* weight, const float* bias, const float* target, const int32_t* task,
                                     const int32_t* row_ids, int64_t n_task, float dropout_p, int64_t* rng_state,
                                     int64_t* rng_used, float* pred, float* loss, const mkgnn_loss_weights* weights,
                                     void* workspace, size_t workspace_bytes, void* stream);
int mkgnn_task_head_weighted_backward(int32_t loss_kind, const float* emb, int64_t emb_stride, int64_t n_rows, int32_t H, int32_t T,
                                      const float* weight, const float* target, const int32_t* task, const int32_t* row_ids,
                                      int64_t n_task, const float* pred, const float* grad_loss, float dropout_p,
                                      const int64_t* rng_used, float* grad_emb, int64_t grad_emb_stride, float* grad_weight,
                                      float* grad_bias, const mkgnn_loss_weights* weights, void* workspace,
                                      size_t workspace_bytes, void* stream);
int mkgnn_task_head_weighted_fused(int32_t loss_kind, const float* emb, int64_t emb_stride, int64_t n_rows, int32_t H, int32_t T,
                                   const float* weight, const float* bias, const float* target, const int32_t* task,
                                   const int32_t* row_ids, int64_t n_task, float dropout_p, int64_t* rng_state,
                                   int64_t* rng_used, float* pred, float* loss, float* grad_emb, int64_t grad_emb_stride,
                                   float* grad_weight, float* grad_bias, const mkgnn_loss_weights* weights, void* workspace,
                                   size_t workspace_bytes, void* stream);
/* (additive; the ABI version stays 8) The label-matrix head: the same T-output ffn, but every row carries a ROW of labels with
 * holes instead of naming one task -- the network runs once per molecule, not once per (molecule, assay) pair.  Row i < n_rows has
 * the labels  labels[i * label_stride + t]  (row_ids NULL; n_label_rows >= n_rows rows)  or  labels[row_ids[i] * label_stride + t]
 * (labels: a table of n_label_rows rows, e.g. one per molecule of a resident shard; row_ids int32 [n_rows]; an id outside
 * [0, n_label_rows) is "no label in any task").  Entry (i, t) is labelled iff its label is not NaN -- only NaN means missing, an
 * infinite label is a label:
 *     pred[i * pred_stride + t] = (keep_i * emb_i) . weight[t] + bias[t]          for EVERY i < n_rows, t < T, labelled or not
 *     loss = sum over the labelled entries of s_i * term(pred[i, t], labels[i, t]) / max(n_labelled_entries, 1)
 * (SQERR_SUM: no division; never divided by the sum of the weights).  term, s_i (weights->sample_weight, direct or through
 * weights->weight_ids, which is that same row_ids vector or NULL) and pos_weight [T] are the weighted task head's above; weights may
 * be NULL.  Sample weights that are all exactly 1.0f give the bits of a call without them.  An unlabelled entry is removed by a
 * select: its label, and the sample weight of a row without labels, reach neither a value nor a gradient.  keep: the heads' dropout
 * multipliers -- element i * H + h of the same generator, same rng_state / rng_used protocol, so a call draws the mask the other
 * heads draw from the same {seed, offset}; dropout_p in [0, 1).
 * BITS: pred[i, t] is bit for bit what mkgnn_task_head_forward writes for row i labelled with task t under the same generator
 * state (at dropout_p = 0: mkgnn_task_scores' value).  The loss and the gradients are NOT the task head's bits (a row's terms are
 * summed in an xor tree over its tasks first); they are bit-reproducible run to run, and the fused entry's gradients are the
 * forward + backward pair's at grad_loss = 1.
 * Gradients: grad_emb[i, h] = keep[i, h] * sum over t ascending of d[i, t] * weight[t, h] (grad_emb may be NULL), grad_weight [T, H],
 * grad_bias [T] or NULL.  EXACT zeros: grad_weight[t, :] and grad_bias[t] of a task without a labelled entry in the call, grad_emb[i, :]
 * of a row without one, and with no labelled entry at all the loss and every gradient (count clamped to 1); pred is still written
 * everywhere.  Nothing is read or written at rows >= n_rows, nor between padded strides.  forward / backward / fused mirror the task
 * head's (backward: d loss from the device, pred from the forward, only the mask is recomputed).  Two launches per call -- the
 * second is the task head's own final kernel --, fixed-order sums, no atomics, no process-wide state, nothing read back, capturable:
 * labels, ids and weights are device buffers a captured step may refill.
 * Limits: 1 <= T <= MKGNN_TASK_HEAD_MAX_TASKS, 1 <= H <= 64, n_rows >= 1, n_rows * T < 2^31 (the labelled-entry count stays an exact
 * int), label_stride >= T, pred_stride >= T, emb_stride >= H; anything else, an unknown loss kind, pos_weight with a squared-error
 * kind and a short sample_weight return non-zero with mkgnn_last_error set before any launch.  workspace:
 * mkgnn_label_head_workspace_bytes (0 outside the limits). */
size_t mkgnn_label_head_workspace_bytes(int64_t n_rows, int32_t H, int32_t T);
int mkgnn_label_head_forward(int32_t loss_kind, const float* emb, int64_t emb_stride, int64_t n_rows, int32_t H, int32_t T,
                             const float* weight, const float* bias, const float* labels, int64_t label_stride,
                             const int32_t* row_ids, int64_t n_label_rows, float dropout_p, int64_t* rng_state, int64_t* rng_used,
                             float* pred, int64_t pred_stride, float* loss, const mkgnn_loss_weights* weights, void* workspace,
                             size_t workspace_bytes, void* stream);
int mkgnn_label_head_backward(int32_t loss_kind, const float* emb, int64_t emb_stride, int64_t n_rows, int32_t H, int32_t T,
                              const float* weight, const float* labels, int64_t label_stride, const int32_t* row_ids,
                              int64_t n_label_rows, const float* pred, int64_t pred_stride, const float* grad_loss,
                              float dropout_p, const int64_t* rng_used, float* grad_emb, int64_t grad_emb_stride,
                              float* grad_weight, float* grad_bias, const mkgnn_loss_weights* weights, void* workspace,
                              size_t workspace_bytes, void* stream);
int mkgnn_label_head_fused(int32_t loss_kind, const float* emb, int64_t emb_stride, int64_t n_rows, int32_t H, int32_t T,
                           const float* weight, const float* bias, const float* labels, int64_t label_stride,
                           const int32_t* row_ids, int64_t n_label_rows, float dropout_p, int64_t* rng_state, int64_t* rng_used,
                           float* pred, int64_t pred_stride, float* loss, float* grad_emb, int64_t grad_emb_stride,
                           float* grad_weight, float* grad_bias, const mkgnn_loss_weights* weights, void* workspace,
                           size_t workspace_bytes, void* stream);
/* (additive; the ABI version stays 8) mkgnn_tail_fused_readout_dropout with that weighted loss: a sample weight per molecule
 * gi < args->n_loss_mols (sample_weight[gi], or sample_weight[weight_ids[gi]]) and ONE positive weight, pos_weight[0] (the tail is
 * single-task).  Only a molecule's d loss / d logit and its loss term change -- the formulas above, the sample weight first, then
 * the 1 / n_loss_mols of the mean kinds (the tail divides by the number of loss molecules: every one of them is labelled).  It
 * obeys the whole pending-work protocol of mkgnn_tail_fused (defer_reduce, mkgnn_tail_defer_projection, mkgnn_tail_flush; what an
 * earlier call left pending is launched before its own first launch), the same generator advance and the same MKGNN_TAIL_MAX_*
 * rule.  weights == NULL, or sample_weight and pos_weight both NULL: mkgnn_tail_fused_readout_dropout bit for bit (its kernels are
 * launched); sample weights that are all exactly 1.0f without pos_weight: its bits too.  Refused before any launch: pos_weight with
 * a squared-error kind, a non-NULL sample_weight with n_sample_weight < 1 (weight_ids given) or < n_loss_mols (not given), and
 * everything mkgnn_tail_fused_readout_dropout refuses. */
int mkgnn_tail_fused_weighted(const mkgnn_tail_args* args, float readout_dropout_p, const mkgnn_loss_weights* weights,
                              void* workspace, size_t workspace_bytes, void* stream);
/* (additive; the ABI version stays 8) The fused tail for SEVERAL outputs: mkgnn_tail_fused_weighted with a T-output head behind
 * the readout -- the label-matrix head's definition (labels != NULL: labels[i, t], NaN = not measured) or the task-indexed head's
 * (task != NULL: molecule i names ONE task, -1 or anything outside [0, T) = none, and its label is args->target[i]).  Exactly one
 * of labels / task is set.  args->head_weight is [T, G], args->head_bias [T] or NULL, args->grad_head_weight [T, G],
 * args->grad_head_bias [T]; args->pred is ignored and args->target only read with task.
 *     pred[i * pred_stride + t] = (keep_i * emb_i) . head_weight[t] + head_bias[t]       for EVERY i < n_loss_mols, t < T
 *     loss = sum over the labelled (i, t) of s_i * term(pred[i, t], y[i, t]) / max(n_labelled, 1)
 * (SQERR_SUM: not divided; never divided by the sum of the weights), term, s_i and pos_weight [T] as for mkgnn_label_head_*;
 * a pos_weight entry of exactly 1.0f and sample weights of exactly 1.0f give the bits of a call without them.  An unlabelled
 * entry is removed by a select: its label and its weight reach nothing.  row_ids == NULL: row i of labels / task (n_label_rows /
 * n_task >= n_loss_mols); else labels[row_ids[i]] / task[row_ids[i]] of a table with n_label_rows / n_task >= 1 rows, an id outside
 * it: no label.  The head's dropout element is mol * G + j and the readout's the convention above: the masks are the two heads' and
 * the tail's for the same {seed, offset}, and the generator advances by exactly one per call that draws.
 * EXACT: padding molecules (i >= n_loss_mols) get zero gradients; a molecule without a labelled entry exactly zero grad_sim rows,
 * a task without one exactly zero rows of grad_head_weight / grad_head_bias; no labelled entry at all: loss 0 and every gradient 0.
 * With T == 1 and a dense label column: the bits of mkgnn_tail_fused_readout_dropout on the same inputs.
 * The labelled-entry count is taken on the device by a small integer count launch in front of the middle kernel (no read-back, no
 * float atomics, nothing depends on workgroup arrival order, capturable; it counts the first n_loss_mols rows only).  The entry
 * obeys the whole pending-work protocol of mkgnn_tail_fused (defer_reduce, mkgnn_tail_defer_projection, mkgnn_tail_flush).
 * Limits: mkgnn_tail_supported, 1 <= T <= MKGNN_TASK_HEAD_MAX_TASKS, n_loss_mols * T < 2^31 and the MKGNN_TAIL_MAX_* rule (a molecule
 * beyond it: NaN loss, as in mkgnn_tail_fused).  Refused before any launch: T out of range, both or neither label source,
 * pos_weight with a squared-error kind, label_stride or pred_stride < T, emb_stride < G, a NULL pred, a table or a vector shorter
 * than stated above, and everything mkgnn_tail_fused_weighted refuses.  workspace: mkgnn_tail_labels_workspace_bytes (0 for bad
 * shapes; at least mkgnn_tail_workspace_bytes). */
typedef struct mkgnn_tail_labels {
    int32_t n_tasks;                                                       /* T */
    const float*   labels;  int64_t label_stride;  int64_t n_label_rows;   /* label matrix, NaN = not measured; OR */
    const int32_t* task;    int64_t n_task;                                /* one task per molecule (-1: none), its label in args->target */
    const int32_t* row_ids;                                                /* NULL: row i; else the row of the table */
    float* pred; int64_t pred_stride;                                      /* [n_loss_mols, T], every entry written */
} mkgnn_tail_labels;
size_t mkgnn_tail_labels_workspace_bytes(int32_t K, int32_t H, int32_t G, int64_t n_atoms, int64_t n_mols, int32_t T);
int mkgnn_tail_fused_labels(const mkgnn_tail_args* args, float readout_dropout_p, const mkgnn_tail_labels* labels,
                            const mkgnn_loss_weights* weights, void* workspace, size_t workspace_bytes, void* stream);

/* (additive; the ABI version stays 8) Every task's logit of every row -- the T-output ffn behind the readout in evaluation mode,
 * for ranking a library per assay:
 *     pred[i * pred_row_stride + t * pred_task_stride] = emb_i . weight[t] + bias[t]      for every i < n_rows, t < T
 * weight [T, H], bias [T] or NULL (then +0.0 is added).  pred[i, t] is BIT FOR BIT what mkgnn_task_head_forward writes for row i
 * when that row is labelled with task t, at dropout_p = 0, for any loss kind: the same products (lane h: emb[h] * w[t][h], then
 * fmaf(emb[32 + h], w[t][32 + h], .) for H > 32, +0.0 at lanes >= H), the same xor tree over the 32 lanes (offsets 16, 8, 4, 2, 1),
 * the bias added last.  Either output layout: [n_rows, T] rows (pred_task_stride = 1, pred_row_stride >= T) or [T, n_rows]
 * task-major (pred_row_stride = 1, pred_task_stride >= n_rows) -- any pair of positive strides under which no two (i, t) share
 * an element; nothing else of pred is written.  One launch on `stream`, capturable; no workspace, no atomics, no process-wide
 * state, one writer per output.  The task head's limits: 1 <= T <= MKGNN_TASK_HEAD_MAX_TASKS, 1 <= H <= 64, emb_stride >= H;
 * anything else returns non-zero with mkgnn_last_error set.  n_rows == 0 is a no-op that returns 0. */
int mkgnn_task_scores(const float* emb, int64_t emb_stride, int64_t n_rows, int32_t H, int32_t T,
                      const float* weight, const float* bias, float* pred, int64_t pred_row_stride, int64_t pred_task_stride,
                      void* stream);

/* (additive; the ABI version stays 8) Cosine similarity of every embedding row with every query -- analogue search over a library
 * of graph embeddings (the reference compares molecules by CosineSimilarity(dim=-1) of their graph embeddings):
 *     sim[i * sim_row_stride + q * sim_query_stride] = (emb_i . queries_q) / (max(||emb_i||, eps) * max(||queries_q||, eps))
 * for every i < n_rows, q < Q, with eps = 1e-8f: each vector is clamped on its own, as torch.nn.functional.cosine_similarity and
 * mkgnn_row_inv_norm do.  emb [n_rows, H] with emb_stride >= H, queries [Q, H] with query_stride >= H, RAW: nothing is prepared
 * ahead, every block normalises the queries itself, so one captured launch follows the contents of both inputs.  A zero row or a
 * zero query gives +0.0; a NaN in row i makes row i's Q outputs NaN and no others, a NaN in query q column q and no others.
 * DOMAIN: rows and queries whose sum of squares is finite in float32; outside it the result is whatever the arithmetic gives.
 * Evaluation order, one per element: lane h of 32 forms v[h] * w[h] (a plain multiply, +0.0 at h >= H), applies
 * fmaf(v[32 + h], w[32 + h], .) where 32 + h < H, and the 32 values go through an xor tree (offsets 16, 8, 4, 2, 1) -- for the two
 * sums of squares (v = w) and the dot product alike; inv = 1 / fmaxf(sqrtf(sum of squares), eps), correctly rounded; the dot
 * product gets + (+0.0); sim = (dot * inv_row) * inv_query.  The BITS of sim[i, q] therefore depend on the H values of row i and
 * of query q only: not on n_rows, the row's place in block or grid, Q, q's index, either input stride or the output layout.
 * Against the exact value the error is at most (2 H + 10) 2^-24 M ie iq + H 2^-149 ie iq + 2^-149, M = sum_h |e_h| |q_h|, ie and
 * iq the two inverse clamped norms.  Either output layout: [n_rows, Q] rows (sim_query_stride = 1,
 * sim_row_stride >= Q) or [Q, n_rows] query-major (sim_row_stride = 1, sim_query_stride >= n_rows) -- any pair of positive strides
 * under which no two (i, q) share an element; nothing else of sim is written.  One launch on `stream`, capturable; no workspace,
 * no atomics, no process-wide or thread-local state, one writer per output.  1 <= Q <= MKGNN_EMBED_COSINE_MAX_QUERIES (the lists
 * of one mkgnn_topk_update_tasks), 1 <= H <= 64; anything else, a negative n_rows, a null pointer or overlapping outputs returns
 * non-zero with mkgnn_last_error set before any launch.  n_rows == 0 is a no-op that returns 0. */
#define MKGNN_EMBED_COSINE_MAX_QUERIES 32
int mkgnn_embed_cosine(const float* emb, int64_t emb_stride, int64_t n_rows, int32_t H, const float* queries, int64_t query_stride,
                       int32_t Q, float* sim, int64_t sim_row_stride, int64_t sim_query_stride, void* stream);

/* AdamW step over all trainable tensors of the model in one launch (reference model.py:368-385: torch.optim.AdamW,
 * two parameter groups -- kernel banks without weight decay).  Per tensor: param / grad [numel] fp32 contiguous,
 * state [mkgnn_adamw_state_floats(numel)] = exp_avg, exp_avg_sq, step count (as a float, advanced by this call), two reserved
 * floats, then one copy of the step count per 1024 elements (every block of the update advances its own: one launch per
 * step, no counting pass; a caller that sets the step count sets every copy).  Per group: the
 * learning rate either by value (lr_device NULL) or read from a device float at run time (so that a captured graph
 * follows a scheduler), betas, eps, decoupled weight_decay, maximize, grad_scale.  The update is torch's fused AdamW formula
 * (bias corrections 1 - beta^step).  At most 4 groups; any number of tensors (80 per launch). */
/* (ABI v7) n_items small float tensors, each into its destination, in one launch (ceil(numel / 1024) blocks each): the
 * data-parallel step's gradients into the flat buffer one collective sums (dp.FlatGradAllReduce), where torch._foreach_copy_
 * takes two multi-tensor launches.  Sources and destinations must not overlap; graph-capturable (pointers are baked in). */
typedef struct mkgnn_copy_item { float* dst; const float* src; int64_t numel; } mkgnn_copy_item;
int mkgnn_flat_copy(const mkgnn_copy_item* items, int32_t n_items, void* stream);

typedef struct mkgnn_adamw_tensor {
    float* param;
    const float* grad;
    float* state;
    int64_t numel;
    int32_t group;
    int32_t reserved;
    const float* active;   /* NULL, or a device float: the tensor is skipped (no update, step count not advanced) when it
                              reads 0 -- "no rank had a gradient for it this step" in a captured data-parallel step */
} mkgnn_adamw_tensor;
typedef struct mkgnn_adamw_group {
    const float* lr_device;
    float lr, beta1, beta2, eps, weight_decay;
    int32_t maximize;
    float grad_scale;      /* every gradient is multiplied by this first (1 / world size after a summing all-reduce; else 1) */
} mkgnn_adamw_group;
int64_t mkgnn_adamw_state_floats(int64_t numel);
int mkgnn_adamw_step(const mkgnn_adamw_tensor* tensors, int32_t n_tensors, const mkgnn_adamw_group* groups,
                     int32_t n_groups, void* stream);

/* The same step with the gradients clipped by their global norm and, optionally, skipped when that norm is not finite -- both
 * decided on the device (ABI v8, additive: the three declarations above are unchanged).
 *
 * A tensor is STEPPED when its active flag is absent or does not read 0.  For a stepped tensor gg = fl32(+-grad * grad_scale),
 * element by element (maximize's sign first, then the group's scale: the value mkgnn_adamw_step forms).  S = sum of gg^2 over all
 * elements of all stepped tensors of the WHOLE table (not per launch of 80 tensors), accumulated in float64 in a fixed order;
 * norm = sqrt(S), non-finite if and only if some gg is; coef = fl32(min(1, max_norm / (norm + 1e-6))) evaluated in double, a NaN
 * kept: torch.nn.utils.clip_grad_norm_'s formula.  The update is mkgnn_adamw_step's with fl32(gg * coef) in place of gg: one
 * more float32 multiply, nothing else reordered -- a step with coef = 1 is bit for bit mkgnn_adamw_step's (tested over three
 * steps of a 161-tensor table).  grad is NOT written back (unlike clip_grad_norm_, the clip lives in the step).
 * max_norm = +inf: coef = 1, the norm and the guard without clipping.
 *
 * skip_nonfinite != 0 and norm not finite: the step does not happen -- no parameter, moment, canonical or per-block step count
 * changes by a bit, stats[2] goes up by one, and the next finite step continues from the old counts.  skip_nonfinite == 0: as
 * torch does, an infinite norm gives coef = 0 (the infinite elements become NaN, the rest 0), a NaN norm coef = NaN.
 *
 * stats [4 floats, device]: [0] fl32(norm), the pre-clip norm clip_grad_norm_ returns; [1] coef; [2] the running count of skipped
 * steps (the caller zeroes it once; this call only ever adds one); [3] reserved, not touched.  One workgroup writes them.
 *
 * workspace [mkgnn_adamw_clip_workspace_bytes(tensors, n_tensors) bytes, 8-byte aligned, device]: one float64 partial per
 * 1024-element block of the table and one more double.  Every byte of it that a call reads the same call has written: it needs
 * no initialisation and may be shared by calls that do not overlap in time.  The size is a function of the numel fields alone
 * (host only, no GPU needed; 0 for an empty table).
 *
 * Launches, all on `stream`, all capturable, no atomics, no cooperative launch, no flag a workgroup waits on, no host round
 * trip: one partial-sum launch per 80 tensors; then, only when the table has more than MKGNN_ADAMW_CLIP_PROLOGUE_BLOCKS blocks,
 * a one-workgroup launch that reduces the partials to one double; then one update launch per 80 tensors, every block of which
 * adds up the partials (or reads that double) in its prologue.  So a model of up to 80 tensors takes two launches.
 *
 * max_norm must be > 0 or +inf; a NaN, zero or negative max_norm, a workspace that is null, misaligned or shorter than
 * mkgnn_adamw_clip_workspace_bytes says, a null stats, and everything mkgnn_adamw_step refuses return non-zero with
 * mkgnn_last_error set before any launch. */
#define MKGNN_ADAMW_CLIP_PROLOGUE_BLOCKS 512
size_t mkgnn_adamw_clip_workspace_bytes(const mkgnn_adamw_tensor* tensors, int32_t n_tensors);
int mkgnn_adamw_step_clipped(const mkgnn_adamw_tensor* tensors, int32_t n_tensors, const mkgnn_adamw_group* groups,
                             int32_t n_groups, float max_norm, int32_t skip_nonfinite, void* workspace, size_t workspace_bytes,
                             float* stats, void* stream);

/* The same steps with an average of the weights kept inside the update launch (ABI v8, additive: every declaration above is
 * unchanged): Polyak / EMA averaging, or the equal-weight mean of the iterates (torch.optim.swa_utils.AveragedModel), with no
 * launch of its own, and decided on the device -- a step that the guard skipped or a tensor whose flag read 0 is not averaged.
 *
 * Per tensor the average lies directly behind the packed state: `state` holds mkgnn_adamw_state_floats(numel) +
 * mkgnn_adamw_average_floats(numel) floats, the second part [avg (numel) | n_averaged | one n_averaged per 1024 elements]
 * (numel + 1 + ceil(numel / 1024) floats; 0 for numel < 1).  The counts are floats, exact to 2^24, one copy per block of the
 * update as for the step count: no block reads what another writes; block 0 also writes the canonical copy.  The caller
 * initialises avg (to the parameter) and zeroes the counts; a caller that sets the count sets every copy.
 *
 * A tensor's step is TAKEN when mkgnn_adamw_step / mkgnn_adamw_step_clipped would change it.  After a taken step that produced
 * p_new and the step count t:
 *   t <= start:                  avg = p_new (the same bits), n_averaged stays 0
 *   t >  start, n_averaged == 0: avg = p_new, n_averaged = 1
 *   t >  start, n = n_averaged:  avg = avg + fl32(w * fl32(p_new - avg)), n_averaged = n + 1 -- three float32 operations, each
 *                                rounded, no fused multiply-add; w == 1 copies p_new instead
 * w is formed per block in double and rounded once to float32: mean: 1 / (n + 1); ema: 1 - d with d = decay, or with warmup
 * d = min(decay, (1 + n) / (10 + n)).  A step that is not taken changes neither avg nor any count by a bit.
 *
 * Parameters, moments, step counts and stats are bit for bit those of mkgnn_adamw_step (when max_norm == +inf, skip_nonfinite ==
 * 0 and stats == NULL: one launch per 80 tensors, workspace ignored) and of mkgnn_adamw_step_clipped (otherwise: that entry's
 * launches, checks, workspace and stats).  The two reserved floats of the state stay as they are.  Capturable, no atomics.
 * A null `avg`, a mode that is neither constant, decay outside [0, 1) or NaN, start < 0 and everything the underlying entry
 * refuses return non-zero with mkgnn_last_error set before any launch. */
#define MKGNN_ADAMW_AVERAGE_EMA 0
#define MKGNN_ADAMW_AVERAGE_MEAN 1
typedef struct { int32_t mode; float decay; int32_t warmup; int32_t start; } mkgnn_adamw_average;
int64_t mkgnn_adamw_average_floats(int64_t numel);
int mkgnn_adamw_step_averaged(const mkgnn_adamw_tensor* tensors, int32_t n_tensors, const mkgnn_adamw_group* groups,
                              int32_t n_groups, const mkgnn_adamw_average* avg, float max_norm, int32_t skip_nonfinite,
                              void* workspace, size_t workspace_bytes, float* stats, void* stream);

/* n_items pairs of small float tensors, the contents of each pair exchanged, in one launch per 120 items (ceil(numel / 1024)
 * blocks each; both loads, then both stores): the averaged weights into the model and the live ones out, and back.  No two
 * tensors of a call may overlap -- not a and b of one item, not tensors of different items.  Capturable (pointers are baked in).
 * A negative n_items, a null pointer or numel outside 1 .. 2^30 returns non-zero with mkgnn_last_error set before any launch. */
typedef struct mkgnn_swap_item { float* a; float* b; int64_t numel; } mkgnn_swap_item;
int mkgnn_flat_swap(const mkgnn_swap_item* items, int32_t n_items, void* stream);

/* ---- Molecule-resident small-batch step (ABI v4).
 *
 * At the reference's own batch sizes (README.md:81 `--batch_size 16`, data.py:236 default 17; BASELINE configs[0] / [2]) a
 * step of one launch per operator is a chain of ~30 dependent launches of a few microseconds each.  Nothing on the path
 * crosses a molecule boundary after the batch-norm statistics (edge_index is block-diagonal), so here ONE launch runs, for
 * a chunk of whole molecules per workgroup (at most 64 atoms, its rows resident in LDS):
 *
 *   node_batch_norm -> num_layers x (KernelSetConv -> propagate) -> lin1, swish, add-pool, lin2   (MolKGNNNet.py:115-146,
 *                                                                                                  KernelLayer.py:109-120)
 *   [-> dropout -> ffn -> BCEWithLogitsLoss                                                       (model.py:150, 169, 190-198)]
 *   [-> the backward of all of it, back to the batch norm's weight and bias]
 *
 * followed by one reduction launch that sums the per-workgroup partial gradients in a fixed order (no float atomics) and
 * undoes the unit normalisation of the kernel rows, and preceded by one preparation launch (unit-normalised kernel rows,
 * mixing weights, chirality tables of every layer; partial batch-norm statistics).  Same arithmetic as the per-operator
 * entry points above -- cosines of unit rows, every neighbour order scored ((c0+c1)+c2)+c3 then / d, strict '>' scan in
 * table order, chirality sign -- so the parity criteria of the per-operator path apply unchanged; results are not
 * bit-identical to it (other summation orders inside a dot product).
 *
 * Shapes taken: 1..4 layers; first layer's input width <= 32, every layer's kernel count K <= 112 with at most 64
 * kernels per degree and (L_1 + 2 L_2 + 3 L_3) + (L_1 + L_2 + L_3) <= 256, 5 L_4 <= 256; E <= 8; H, G <= 64; every
 * molecule <= 64 atoms, atoms of a molecule contiguous, every atom's degree <= 4 and its bonds stored in both
 * directions (as the reference stores them, wrapper.py:152-156), unit bond rows present.  mkgnn_molecule_supported says
 * whether a model shape is taken; the batch conditions are the caller's (molkgnn_amd.molecule checks them once per batch). */
#define MKGNN_MOLECULE_MAX_LAYERS 4
#define MKGNN_MOLECULE_MAX_ATOMS 64      /* atoms per chunk (and so per molecule) */
#define MKGNN_MOLECULE_MAX_MOLS 16       /* molecules per chunk */

typedef struct mkgnn_molecule_layer {
    mkgnn_kernel_bank bank[MKGNN_MAX_DEGREE];        /* this layer's KernelSetConv (kernels.py:759-778) */
    mkgnn_kernel_bank_grad grad[MKGNN_MAX_DEGREE];   /* backward: where the bank gradients go (a NULL x_center: skipped) */
    mkgnn_saved saved[MKGNN_MAX_DEGREE];             /* pair records [N_d, L_d, 4] (+ chirality, last layer, d = 4):
                                                        written by the forward, needed by the backward */
    int32_t F;                                       /* input width of the layer (x_dim, then the previous layer's K) */
    int32_t reserved;
    float* sim_out;                                  /* optional [n_atoms, sim_stride]: this layer's sim_sc (tests) */
    int64_t sim_stride;
} mkgnn_molecule_layer;

typedef struct mkgnn_molecule_net {
    int32_t num_layers, E;
    mkgnn_molecule_layer layer[MKGNN_MOLECULE_MAX_LAYERS];
    /* node_batch_norm (MolKGNNNet.py:26, 115) */
    const float* bn_weight; const float* bn_bias;    /* [F0] or NULL */
    float* bn_running_mean; float* bn_running_var;   /* [F0]; updated when bn_training */
    int64_t* bn_num_batches_tracked;                 /* or NULL */
    float bn_eps, bn_momentum;
    int32_t bn_training, reserved;
    float* grad_bn_weight; float* grad_bn_bias;      /* backward outputs (NULL: skipped) */
    /* readout (MolKGNNNet.py:144-146): lin1 [H, K_last], lin2 [G, H] */
    mkgnn_readout_params readout;
    float* grad_lin1_weight; float* grad_lin1_bias; float* grad_lin2_weight; float* grad_lin2_bias;
    /* head (model.py:149-150, 169): ffn [1, G], dropout in front of it */
    const float* ffn_weight; const float* ffn_bias;
    float* grad_ffn_weight; float* grad_ffn_bias;
    float head_dropout;                              /* 0 = none */
    float readout_dropout;                           /* (ABI v8) read with MKGNN_MOLECULE_READOUT_DROPOUT only: p in [0, 1) */
    int64_t* rng_state;                              /* {seed, offset} of the head's and the readout's dropout (offset advanced
                                                        by the call; not with GRAD_EMB: see MKGNN_MOLECULE_READOUT_DROPOUT) */
    int64_t* rng_used;                               /* optional: the {seed, offset} this call's mask was drawn with */
    /* edge_batch_norm's side effect (MolKGNNNet.py:116; ABI v5): when not NULL
     * (the caller leaves it NULL on a backward-only call), the bond rows' statistics -- 1..8192 rows, C <= 8; anything else
     * is an error: use mkgnn_batchnorm_update_stats -- are taken by one extra block of the preparation launch and the
     * module's buffers updated as mkgnn_batchnorm_update_stats would */
    const mkgnn_bn_stats* edge_stats;
} mkgnn_molecule_net;

typedef struct mkgnn_molecule_batch {
    int64_t n_atoms, n_mols, n_chunks;
    int64_t max_chunk_atoms;                         /* atoms of the largest chunk (<= 32: the half-size kernel variant) */
    const int32_t* chunk_mol_ptr;                    /* [n_chunks + 1] first molecule of every chunk */
    const int64_t* mol_atom_ptr;                     /* [n_mols + 1] first atom of every molecule */
    const int8_t* atom_degree;                       /* [n_atoms] out-degree, 0..4 */
    const int32_t* atom_rank;                        /* [n_atoms] position of the atom in its degree bucket */
    mkgnn_degree_bucket buckets[MKGNN_MAX_DEGREE];   /* nei_index, nei_edge_unit; p_focal / nei_p for d = 4 */
    const float* x; int64_t x_stride;                /* [n_atoms, F0] raw node features */
} mkgnn_molecule_batch;

#define MKGNN_MOLECULE_HEAD      1   /* dropout -> ffn -> BCE-with-logits against `target`; writes pred, loss */
#define MKGNN_MOLECULE_BACKWARD  2   /* gradients of every parameter (d loss = 1 with HEAD, else from grad_emb) */
#define MKGNN_MOLECULE_GRAD_EMB  4   /* BACKWARD without HEAD: d loss / d graph embedding is given */
#define MKGNN_MOLECULE_SQERR     8   /* (ABI v8) with HEAD: squared error in place of BCE-with-logits (MKGNN_LOSS_SQERR_MEAN) */
#define MKGNN_MOLECULE_SUM      16   /* (ABI v8) with SQERR: summed, not averaged, over the molecules (MKGNN_LOSS_SQERR_SUM) */
/* (ABI v8) the readout's dropout, net->readout_dropout in [0, 1), its mask the convention of mkgnn_readout_dropout_mask; needs
 * rng_state.  Without GRAD_EMB the call draws it from rng_state and advances the offset by one (once, with head dropout too),
 * rng_used receiving the pair.  With GRAD_EMB -- the backward of a forward-only call -- it reads rng_state and advances
 * nothing: the caller passes the pair that forward recorded, and the recomputed forward draws the same mask. */
#define MKGNN_MOLECULE_READOUT_DROPOUT 32

int mkgnn_molecule_supported(const mkgnn_molecule_net* net, int32_t x_dim);
size_t mkgnn_molecule_workspace_bytes(const mkgnn_molecule_net* net, int32_t x_dim, int64_t n_atoms, int64_t n_chunks);
/* emb [n_mols, G] is always written.  target [n_mols] and pred [n_mols] / loss [1] with HEAD; grad_emb [n_mols, G] with
 * GRAD_EMB.  The workspace is scratch between calls (the backward of a call recomputes what it needs). */
int mkgnn_molecule_step(const mkgnn_molecule_net* net, const mkgnn_molecule_batch* batch, int32_t mode,
                        const float* target, const float* grad_emb, float* emb, float* pred, float* loss,
                        void* workspace, size_t workspace_bytes, void* stream);

/* ---- host side of the packed-shard loader (no device work): a fixed-shape batch of molecules [m0, m1) of a shard in the
 * compact wire form that mkgnn_expand_batch takes -- features and coordinates as they are, every bond once as an int32
 * pair with byte-valued attributes, labels, molecule pointers; padding atoms / bonds / molecules as molkgnn_amd.padding
 * defines them.  Replaces PyG's Python collation (reference data.py:168-203: DataLoader workers) on the loader threads;
 * one call per batch, so a Python caller's interpreter lock is released for all of it.  `shape` = {atoms, directed edges,
 * N_1, N_2, N_3, N_4} of the epoch's common shape; out: the staging buffer (mkgnn_collate_compact_bytes, fields 256-byte
 * aligned in the order x, p, bond_ij, bond_attr, y, mol_ptr, n_valid_atoms).  The shard's bonds must be stored as reversed
 * pairs (i, j), (j, i) with shared byte-valued attributes (the shard writer's `compact` flag). */
typedef struct mkgnn_shard_view {
    const float* x;                 /* [n_atoms, x_dim] */
    const float* p;                 /* [n_atoms, p_dim] */
    const int32_t* edge_src;        /* [n_edges] shard-global atom ids */
    const int32_t* edge_dst;
    const float* edge_attr;         /* [n_edges, e_dim] */
    const float* y;                 /* [n_molecules] */
    const int64_t* mol_atom_ptr;    /* [n_molecules + 1] */
    const int64_t* mol_edge_ptr;    /* [n_molecules + 1] */
    const int64_t* mol_deg_ptr;     /* [n_molecules + 1, 5] prefix sums of the atoms of degree 1..4 / in no bucket */
    int64_t n_molecules;
    int32_t x_dim, p_dim, e_dim, reserved;
} mkgnn_shard_view;
size_t mkgnn_collate_compact_bytes(const int64_t shape[6], int64_t n_molecules, int32_t pad_molecules, int32_t x_dim,
                                   int32_t p_dim, int32_t e_dim);
int mkgnn_collate_compact(const mkgnn_shard_view* shard, int64_t m0, int64_t m1, const int64_t shape[6],
                          int32_t pad_molecules, void* out, size_t out_bytes);

/* ---- gather-collate from a device-resident shard (additive; the ABI version stays 8): an ARBITRARY list of molecules of a shard that lives in device
 * memory -- repeats allowed, order kept: a draw with replacement (reference data.py:136-166, WeightedRandomSampler) -- into the
 * compact wire form above, exactly what mkgnn_collate_compact writes for a shard that holds those molecules in that order as
 * its range [0, n_ids).  The only per-batch traffic from the host is the id list.
 *
 * All pointers of mkgnn_resident_shard are DEVICE pointers.  Every bond is stored once (the even-indexed directed edges of the
 * shard file) with shard-global endpoints; mol_deg[m][d] is the number of atoms of degree d + 1 in molecule m (a shard with
 * atoms in no degree bucket cannot be resident).
 *
 * Two launches on `stream`, capturable, no host round trip, integer arithmetic only, no atomics: a single-workgroup scan over
 * the slots (exclusive atom / bond offsets and the slots' first source atom / bond into the workspace; y, mol_ptr and
 * n_valid_atoms into the wire buffer), then a grid-wide fill in which every element of x, p, bond_ij and bond_attr has exactly
 * one writer.  Every byte of every wire field is written; the 256-byte alignment gaps between fields are not touched.
 *
 * Errors the device finds are reported in the int32 status word at the start of the workspace, written by every launch:
 *   MKGNN_GATHER_BAD_ID   an id was outside [0, n_molecules); it is clamped before use
 *   MKGNN_GATHER_MISFIT   the molecules do not fit `shape` (a degree over its target, or the padding does not pair up);
 *                         every copy is clamped to its field's extent and every index written stays inside the batch
 * `shape` as for mkgnn_collate_compact; wire_bytes >= mkgnn_collate_compact_bytes(shape, n_ids, pad_molecules, dims). */
#define MKGNN_GATHER_BAD_ID 1
#define MKGNN_GATHER_MISFIT 2
typedef struct mkgnn_resident_shard {
    const float* x;                 /* [n_atoms, x_dim] */
    const float* p;                 /* [n_atoms, p_dim] */
    const int32_t* bond_ij;         /* [n_bonds, 2] shard-global atom ids, every bond once */
    const uint8_t* bond_attr;       /* [n_bonds, e_dim] */
    const float* y;                 /* [n_molecules] */
    const int32_t* mol_atom_ptr;    /* [n_molecules + 1] */
    const int32_t* mol_bond_ptr;    /* [n_molecules + 1] */
    const int32_t* mol_deg;         /* [n_molecules, 4] atoms of degree 1, 2, 3, 4 */
    int64_t n_molecules;
    int32_t x_dim, p_dim, e_dim, reserved;
} mkgnn_resident_shard;
size_t mkgnn_gather_compact_workspace_bytes(int64_t n_ids);
int mkgnn_gather_compact(const mkgnn_resident_shard* shard, const int32_t* ids, int64_t n_ids, const int64_t shape[6],
                         int32_t pad_molecules, void* wire, size_t wire_bytes, void* workspace, void* stream);

/* ---- the same gather from a shard whose atom features are PACKED (additive; the ABI version stays 8): every column of x whose
 * values, over the whole shard, are integers in [-128, 127] and never -0.0 is held as one int8, the other columns as fp32, bit
 * for bit (NaN payloads, infinities, denormals, -0.0).  The decode is exact, so the wire buffer is byte for byte what
 * mkgnn_gather_compact writes for the same shard held unpacked, and the status word agrees.
 *
 * One record of rec_bytes per atom, atom a at x_rec + a * rec_bytes:
 *   the nf fp32 columns in column order | the nq int8 columns in column order | zero bytes up to a multiple of 4
 *   rec_bytes = 4 * nf + 4 * ceil(nq / 4)
 * The column table x_col[x_dim] says where column c lives in the record:
 *   x_col[c] >= 0   an fp32 at byte offset x_col[c] (a multiple of 4)
 *   x_col[c] <  0   an int8 at byte offset -x_col[c] - 1
 * nq == 0 and nf == 0 are both legal.  molkgnn_amd/shards.py::pack_x / unpack_x are the definition.
 *
 * x_rec is a DEVICE pointer, 4-byte aligned (the records are read in dwords).  x_col is a HOST pointer: the entry point checks
 * the table against rec_bytes (every entry inside the record, fp32 offsets multiples of 4, rec_bytes as the layout makes it) and
 * hands it to the kernel with the launch arguments, so nothing of it is read after the call returns and a captured graph holds
 * its own copy.  x_dim <= MKGNN_PACKED_MAX_X_DIM.  Everything else -- the other arrays, ids, shape, wire, the workspace
 * (mkgnn_gather_compact_workspace_bytes) and the status word -- is as for mkgnn_gather_compact. */
#define MKGNN_PACKED_MAX_X_DIM 160
typedef struct mkgnn_resident_shard_packed {
    const uint8_t* x_rec;           /* [n_atoms, rec_bytes] packed records (device) */
    const int32_t* x_col;           /* [x_dim] column table (HOST) */
    const float* p;                 /* [n_atoms, p_dim] */
    const int32_t* bond_ij;         /* [n_bonds, 2] shard-global atom ids, every bond once */
    const uint8_t* bond_attr;       /* [n_bonds, e_dim] */
    const float* y;                 /* [n_molecules] */
    const int32_t* mol_atom_ptr;    /* [n_molecules + 1] */
    const int32_t* mol_bond_ptr;    /* [n_molecules + 1] */
    const int32_t* mol_deg;         /* [n_molecules, 4] atoms of degree 1, 2, 3, 4 */
    int64_t n_molecules;
    int32_t x_dim, p_dim, e_dim, rec_bytes;
} mkgnn_resident_shard_packed;
int mkgnn_gather_compact_packed(const mkgnn_resident_shard_packed* shard, const int32_t* ids, int64_t n_ids,
                                const int64_t shape[6], int32_t pad_molecules, void* wire, size_t wire_bytes, void* workspace,
                                void* stream);

/* ---- running top-k on the device (additive; the ABI version stays 8): the ranking of a screen, kept sorted across batches and
 * shards inside the captured scoring step.  The list (top_score, top_shard, top_mol)[K] is updated IN PLACE to the best K entries
 * of the multiset  old list  U  {(scores[i], *shard_tag, ids[i]) : i < min(max(*n_valid, 0), B)}  and is always fully sorted.
 * n_valid and shard_tag are device int32 scalars read by the kernels, so one captured launch serves every batch and shard;
 * scores and ids past n_valid are not read.
 *
 * The order is total:
 *   1. occupied slots before empty slots.  An empty slot is (-inf, -1, -1); a real entry whose score is -inf ranks before it
 *      (a real entry with score -inf, shard -1 AND molecule -1 cannot be told from an empty slot: tags and ids are >= 0 in use)
 *   2. non-NaN scores before NaN scores (all NaNs rank alike, whatever their payload)
 *   3. score descending; -0.0 and +0.0 compare equal
 *   4. shard ascending, then molecule id ascending (signed)
 *   5. entries alike in all of that keep their order of arrival: the old list first, then the batch by slot
 * Repeated (shard, molecule) pairs are kept, not de-duplicated.  Score bits are copied, never recomputed (a NaN keeps its
 * payload, a zero its sign).  A list starts out as K empty slots.
 *
 * Launches on `stream` (one launch for B <= 1024, two beyond), capturable; integer comparisons only, no atomics, no
 * process-wide state; the result is a function of the inputs alone and every output has one writer.  Any B >= 1;
 * 1 <= K <= MKGNN_TOPK_MAX_K, anything else is rejected (non-zero, mkgnn_last_error), never truncated.  The workspace
 * (16-byte aligned, mkgnn_topk_workspace_bytes(B, K) bytes; 0 for rejected sizes) needs no initialisation: it is read only where the same call wrote it. */
#define MKGNN_TOPK_MAX_K 1024
size_t mkgnn_topk_workspace_bytes(int32_t B, int32_t K);
int mkgnn_topk_update(const float* scores, const int32_t* ids, int32_t B, const int32_t* n_valid, const int32_t* shard_tag,
                      int32_t K, float* top_score, int32_t* top_shard, int32_t* top_mol, void* workspace,
                      size_t workspace_bytes, void* stream);

/* (additive; the ABI version stays 8) T running lists in one update -- a library ranked per assay of a multi-task model.  List t
 * is slots [t * K, (t + 1) * K) of top_score / top_shard / top_mol ([T, K], contiguous); after the call it is exactly what
 * mkgnn_topk_update would make of that list and the scores  scores[i * score_row_stride + t * score_task_stride]  (a [B, T] or a
 * [T, B] tensor, or any other strides; a negative stride is rejected): the same total order, empty slots, copied score bits and
 * stability rule.  ids, *n_valid and *shard_tag are the same for every task: every molecule enters every task's list.  The
 * kernels of mkgnn_topk_update with the task on the grid's second dimension: one launch for B <= 1024, two beyond; blocks of
 * different tasks share nothing, the runs of task t lie at their own offset of the workspace (16-byte aligned,
 * mkgnn_topk_tasks_workspace_bytes(B, K, T) bytes, read only where the same call wrote it).  Any B >= 1, 1 <= K <= MKGNN_TOPK_MAX_K,
 * 1 <= T <= MKGNN_TASK_HEAD_MAX_TASKS; everything else is rejected before a launch and has workspace size 0. */
size_t mkgnn_topk_tasks_workspace_bytes(int32_t B, int32_t K, int32_t T);
int mkgnn_topk_update_tasks(const float* scores, int64_t score_row_stride, int64_t score_task_stride, const int32_t* ids,
                            int32_t B, int32_t T, const int32_t* n_valid, const int32_t* shard_tag, int32_t K,
                            float* top_score, int32_t* top_shard, int32_t* top_mol, void* workspace, size_t workspace_bytes,
                            void* stream);

/* ---- the nearest reference of every library molecule (additive; the ABI version stays 8): how close each embedding row lies to a
 * set of known molecules -- the known actives, the training set, a patent set -- for a novelty filter or an applicability domain
 * in front of the running list.  With sim(i, r) the float32 value mkgnn_embed_cosine writes for row i and query refs[r], BIT FOR
 * BIT (its evaluation order above: the two-values-per-lane products, the xor tree with offsets 16, 8, 4, 2, 1, the + 0.0,
 * (dot * inv(e)) * inv(q); the tree is a fixed binary tree of commutative adds, which one thread evaluates serially in the same
 * association), the winner of row i is the first r in the order mkgnn_topk_update ranks by:
 *   1. non-NaN similarities before NaN ones
 *   2. larger similarities first; -0.0 and +0.0 compare equal
 *   3. then the lower r
 * max_sim[i] carries the winner's bits (when the winner is a NaN: some NaN) and arg_ref[i] = r.  A row of NaN, or a set of NaN
 * references, gives (NaN, 0).  emb [n_rows, H] with emb_stride >= H, refs [R, H] with ref_stride >= H, both RAW: the inverse norms
 * of the references and of the rows are computed inside the call, into the workspace, so one captured call follows new contents
 * of emb and of refs.  max_sim [n_rows] and arg_ref [n_rows] are contiguous; nothing else is written outside the workspace.
 *
 * Two launches on `stream`, three when the references are split over the grid (the per-part winners go through the workspace and
 * a finishing launch combines them in reference order); capturable, no host round trip, no float atomics, no process-wide
 * state, one writer per output.  The workspace (4-byte aligned, mkgnn_embed_max_cosine_workspace_bytes(n_rows, R) bytes; 0 for
 * rejected sizes) needs no initialisation: it is read only where the same call wrote it.  The bits of (max_sim[i], arg_ref[i])
 * depend on row i and on the reference set alone: not on n_rows, the row's place in the grid, the strides, or how the launch
 * splits the references (the winner is the first element of a total order).  Plain FP32: the bit contract forbids the matrix
 * instructions' summation order.  Against the exact cosine every sim(i, r) carries mkgnn_embed_cosine's error bound.
 *
 * Limits: 1 <= H <= 64; 1 <= R <= MKGNN_MAX_COSINE_MAX_REFS; 0 <= n_rows < 2^31.  MKGNN_MAX_COSINE_MAX_REFS is 2^20: a training set
 * of a large assay fits in one call, while one thread's walk stays at R / 256 <= 4 096 references when the batch is small (the
 * references are split into at most 256 parts, and no more than bring the grid to 2 048 blocks), R + n_rows and every index
 * derived from r stay far inside int32, and the workspace stays at 4 (R + n_rows) bytes of norms plus 8 n_rows per part -- at
 * most 4 MiB of winners, whatever n_rows.  More references: call per chunk and combine by the order above.
 * n_rows == 0 is a no-op that returns 0, even with null pointers.  Anything else -- a limit, a stride below H, a null pointer, a
 * workspace that is too small -- returns non-zero with mkgnn_last_error set, before any launch. */
#define MKGNN_MAX_COSINE_MAX_REFS 1048576
size_t mkgnn_embed_max_cosine_workspace_bytes(int64_t n_rows, int32_t R);
int mkgnn_embed_max_cosine(const float* emb, int64_t emb_stride, int64_t n_rows, int32_t H, const float* refs, int64_t ref_stride,
                           int32_t R, float* max_sim, int32_t* arg_ref, void* workspace, size_t workspace_bytes, void* stream);

/* (additive; the ABI version stays 8) Stable compaction of a batch by a key -- the filter between a scoring step and
 * mkgnn_topk_update.  The rows i < min(max(*n_valid, 0), B) with bounds[0] <= key[i] <= bounds[1] are kept (a NaN key fails both
 * comparisons and is never kept; a key equal to a bound is kept; infinite bounds are allowed): their (scores[i], ids[i]) are written
 * in order to out_scores[0 .. *n_kept) and out_ids[0 .. *n_kept), score bits carried over, and *n_kept is written by the launch.
 * Slots from *n_kept on are not written.  n_valid (int32) and bounds (float[2]: lo, hi) are DEVICE scalars read when the launch
 * runs, so one captured launch serves every batch and every pair of bounds.  What the launch writes -- out_scores, out_ids and
 * *n_kept -- must not overlap scores, ids, key, *n_valid, bounds or each other (rejected).  Any B >= 1 in ONE launch of one workgroup (a block scan per 1 024 slots, looping over B: a batch
 * is a few thousand slots); capturable, no atomics, no workspace, no state.  B < 1 or a null pointer returns non-zero with
 * mkgnn_last_error set before the launch.  mkgnn_topk_update(out_scores, out_ids, B, n_kept, ...) takes the result as it is: it
 * reads its count on the device and accepts a count of zero. */
int mkgnn_select_rows(const float* scores, const int32_t* ids, const float* key, int32_t B, const int32_t* n_valid,
                      const float* bounds, float* out_scores, int32_t* out_ids, int32_t* n_kept, void* stream);

/* ---- diverse hits (additive; the ABI version stays 8): leader clustering of a ranked list -- the best molecule of every chemical
 * series among the top of a screen, and the series every other hit belongs to.  emb [n_rows, H] (emb_stride >= H, RAW) holds the
 * embeddings in RANK ORDER, best first.  The similarity is S[i, p] for p <= i: the float32 value mkgnn_embed_cosine writes for
 * row i as the ROW and row p as the QUERY, BIT FOR BIT -- (dot * inv(e_i)) * inv(e_p); the orientation matters, the two
 * multiplications do not commute in their last bit.  Only the lower triangle and the diagonal are read.  Walk i = 0, 1, ...:
 *   1. S[i, i] is NaN (a NaN, infinite or overflowing row): row i is never picked and covers nothing -- leader[i] = -1,
 *      leader_sim[i] = NaN -- whatever its similarity to a pick is
 *   2. otherwise let p be the FIRST pick so far, in pick order, with S[i, p] > max_sim (strict: a similarity equal to max_sim
 *      does not cover, a NaN never does): row i is covered, leader[i] = p (a row index), leader_sim[i] = S[i, p]
 *   3. otherwise, while fewer than k_max picks exist, row i becomes a pick: it is appended to picks, leader[i] = i,
 *      leader_sim[i] = S[i, i]
 *   4. otherwise the list is full and nothing covers the row: leader[i] = -1, leader_sim[i] = NaN
 * Rows behind the last pick are still assigned to the picks that cover them, so the cluster sizes count the whole list.
 * Outputs, all contiguous: picks int32 [k_max] (unused slots -1), *n_picks, leader int32 [n_rows], leader_sim float32 [n_rows];
 * nothing else is written outside the workspace.  They must not overlap emb, the workspace or each other (rejected).
 *
 * The rows go in tiles of 1 024 in rank order: one workgroup decides a tile (one thread per row, the alive
 * set as one ballot word per wave), then a grid-wide launch lets every row behind the tile meet the picks the tile added; the
 * pick count lives in device memory.  1 + 2 * tiles - 1 launches on `stream`, capturable, no host round trip, no atomics on
 * global memory, no state between calls; the inverse norms and S[i, i] are computed inside the call, so a captured call follows
 * new contents of emb.  The result is a function of emb, max_sim and k_max alone: not of the tile size, the stride or the grid.
 * The workspace (4-byte aligned, mkgnn_diverse_pick_workspace_bytes(n_rows) bytes -- 8 per row and 16 more; 0 for rejected sizes)
 * needs no initialisation.
 *
 * Limits: 1 <= H <= 64; 1 <= n_rows <= MKGNN_DIVERSE_MAX_ROWS (2^20: the selection is quadratic in the worst case -- every row a
 * pick -- and every index fits an int); 1 <= k_max <= n_rows; max_sim finite.  n_rows == 0 is a no-op that returns 0, even with
 * null pointers.  Anything else -- a limit, a NaN or infinite max_sim, a stride below H, a null pointer, a workspace that is too
 * small or misaligned, overlapping buffers -- returns non-zero with mkgnn_last_error set, before any launch. */
#define MKGNN_DIVERSE_MAX_ROWS 1048576
size_t mkgnn_diverse_pick_workspace_bytes(int64_t n_rows);
int mkgnn_diverse_pick(const float* emb, int64_t emb_stride, int64_t n_rows, int32_t H, float max_sim, int32_t k_max,
                       int32_t* picks, int32_t* n_picks, int32_t* leader, float* leader_sim, void* workspace,
                       size_t workspace_bytes, void* stream);

/* ---- what each kernel learned (additive; the ABI version stays 8): C running lists, one per kernel column of a convolution
 * layer's output sim [n_atoms, C] (row n holds the num_kernels[d] scores of its own degree d + 1 in the columns [col_begin[d],
 * col_begin[d] + num_kernels[d]); what lies elsewhere in the row is never read), each the K atoms of a library that column matches
 * best.  List c is slots [c K, (c + 1) K) of top_score / top_shard / top_mol / top_atom ([C, K], contiguous), updated IN PLACE
 * and always fully sorted.  An empty slot is (-inf, -1, -1, -1); a list starts out as K of them.
 *
 * The candidates come from the degree buckets of the batch: slot s < buckets[d].count names atom n = buckets[d].selected_index[s]
 * (only count and selected_index of a bucket are read).  It is a candidate of every column of [col_begin[d], col_begin[d] +
 * num_kernels[d]) and of no other, if  n < *n_valid_atoms  (a device int64 scalar; NULL: every atom) and  g = atom_mol[n] <
 * min(max(*n_live, 0), B)  -- live molecules come first in a batch; fillers, padding molecules and padding atoms never enter,
 * whatever they score.  Its entry in column c is (the bits of sim[n * sim_stride + c], *shard_tag, mol_ids[g], n - mol_ptr[g]):
 * the atom's index inside its molecule.  atom_mol int32 [n_atoms], mol_ptr int32 [B + 1], mol_ids int32 [B]; n_live and shard_tag
 * are device int32 scalars as in mkgnn_topk_update, so one captured launch serves every batch and shard.
 *
 * After the call list c holds the first K entries, sorted, of  old list c  U  the candidates of c  under mkgnn_topk_update's
 * total order extended by the atom: occupied before empty (a real entry whose score is -inf ranks before an empty slot), non-NaN
 * before NaN, score descending with -0.0 == +0.0, shard ascending, molecule ascending, atom ascending, and entries alike in all
 * of that in their order of arrival -- the old list first, then degree-bucket slot order.  Score bits are copied, never recomputed.
 *
 * Two launches on `stream`, capturable: one workgroup per (tile of 128 slots of one degree, chunk of 64 of its columns) reads the
 * atoms' scores once, decides per column whether any candidate of the tile displaces the list's last entry under the full order
 * and, only then, leaves the tile's best entries as a sorted run; one wave per column merges the flagged runs into its list in
 * tile order.  No host round trip, no atomics, no process-wide state; integer comparisons only; every output has one writer; the
 * result is a function of the inputs alone.  The workspace (16-byte aligned, mkgnn_kernel_exemplars_workspace_bytes(counts,
 * num_kernels, K, C) bytes; 0 for rejected sizes) needs no initialisation: it is read only where the same call wrote it.
 *
 * Limits: 1 <= K <= MKGNN_EXEMPLARS_MAX_K (K need not be a power of two); 1 <= C <= MKGNN_EXEMPLARS_MAX_COLUMNS; the four column
 * blocks lie inside [0, C) and do not overlap (num_kernels[d] = 0 and count = 0 are allowed); sim_stride >= C; B >= 1;
 * 1 <= n_atoms <= 2^30.  Anything else -- a null pointer, a negative count or one above n_atoms, a workspace that is too small or
 * misaligned, an output aliasing an input or another output -- returns non-zero with mkgnn_last_error set, before any launch. */
#define MKGNN_EXEMPLARS_MAX_K 64
#define MKGNN_EXEMPLARS_MAX_COLUMNS 256
size_t mkgnn_kernel_exemplars_workspace_bytes(const int64_t count[MKGNN_MAX_DEGREE], const int32_t num_kernels[MKGNN_MAX_DEGREE],
                                              int32_t K, int32_t C);
int mkgnn_kernel_exemplars_update(const float* sim, int64_t sim_stride, int64_t n_atoms,
                                  const mkgnn_degree_bucket buckets[MKGNN_MAX_DEGREE], const int32_t col_begin[MKGNN_MAX_DEGREE],
                                  const int32_t num_kernels[MKGNN_MAX_DEGREE], const int32_t* atom_mol, const int32_t* mol_ptr,
                                  const int32_t* mol_ids, int32_t B, const int32_t* n_live, const int64_t* n_valid_atoms,
                                  const int32_t* shard_tag, int32_t K, int32_t C, float* top_score, int32_t* top_shard,
                                  int32_t* top_mol, int32_t* top_atom, void* workspace, size_t workspace_bytes, void* stream);

/* ---- analogue search for any number of queries (additive; the ABI version stays 8): fused cosine and top-k.  Q running lists of
 * K slots each, one per query -- top_sim / top_shard / top_mol ([Q, K], contiguous), updated IN PLACE and always fully sorted; an
 * empty slot is (-inf, -1, -1) and a list starts out as K of them -- take raw candidate embeddings and raw queries in; no [n, Q]
 * similarity matrix exists.  Let s_q[i] be the float32 value mkgnn_embed_cosine writes for row i of emb as the ROW and
 * queries[q] as the QUERY, BIT FOR BIT (its evaluation order above: the two-values-per-lane products, the xor tree with offsets
 * 16, 8, 4, 2, 1 as a fixed binary tree, the + (+0.0), (dot * inv(row)) * inv(query) in that orientation).  After the call list
 * q holds the first K entries, sorted, of  old list q  U  {(s_q[i], *shard_tag, ids[i]) : i < min(max(*n_valid, 0), n_rows)}
 * under mkgnn_topk_update's total order:
 *   1. occupied slots before empty ones (a real entry whose similarity is -inf ranks before an empty slot)
 *   2. non-NaN similarities before NaN ones
 *   3. larger similarities first; -0.0 and +0.0 compare equal
 *   4. then the lower shard, then the lower id
 *   5. entries alike in all of that in their order of arrival: the old list first, then the candidates by row
 * Similarity bits are carried over; repeated (shard, id) pairs are kept; among NaN entries only NaN-ness is specified, not the
 * payload.  A zero row or a zero query gives +0.0, so a zero query's list holds the lowest (shard, id) pairs; fewer candidates
 * than K leave empty slots at the end.  ids int32 [n_rows] (NULL: the row index), n_valid and shard_tag DEVICE int32 scalars read
 * when the launches run (NULL: every row; tag 0), so one captured call serves every batch of every shard.  emb [n_rows, H] with
 * emb_stride >= H and queries [Q, H] with query_stride >= H, both RAW: the inverse norms are computed inside the call, into the
 * workspace, so a captured call follows new contents of both.
 *
 * The lists of query q depend only on the old list q, the values and ids of the first min(max(*n_valid, 0), n_rows) rows, the
 * tag and the H values of query q: not on Q or q's index, the rows behind n_valid (never read for their values), either stride,
 * a row's place in block or grid, or how the launch splits the candidates.  Feeding the same candidates in one call or in
 * several gives the same lists.
 *
 * Two launches on `stream`, three when the candidates are split: the norms; one wave per (query, part of the candidates) -- a
 * lane takes a candidate, the four waves of a block share every tile of 64 rows through LDS, the list lives one slot per lane,
 * a ballot under the full order finds the few lanes that get in; and, when Q is too small to fill the chip, a finishing launch
 * that merges the old list and the parts' lists in part order.  The split: parts of whole tiles, at least two tiles each, at
 * most 32 parts, and no more than bring the grid to 1 024 blocks of four queries -- so the candidates are split only where
 * Q <= 4 092, and the parts' lists in the workspace never exceed 32 times the lists' own size, nor 2 047 * 4 * K entries of 12
 * bytes (6 MiB at K = 64) whatever Q.  Capturable, no host round trip, no atomics, no process-wide or thread-local state, one
 * writer per output; integer comparisons on the order's key.  The workspace (4-byte aligned,
 * mkgnn_embed_knn_workspace_bytes(n_rows, Q, K) bytes -- 4 (Q + n_rows) of norms plus the parts' lists; 0 for rejected sizes)
 * needs no initialisation: it is read only where the same call wrote it.  Plain FP32: the bit contract forbids the matrix
 * instructions' summation order.
 *
 * Limits: 1 <= H <= 64; 1 <= K <= MKGNN_KNN_MAX_K (one slot per lane of a wave); 1 <= Q <= MKGNN_KNN_MAX_QUERIES;
 * 0 <= n_rows <= MKGNN_KNN_MAX_ROWS (more rows: call per chunk -- the lists run on).  n_rows == 0 is a no-op that returns 0, even
 * with null pointers.  Anything else -- a limit, a stride below H, a null emb, queries, list or workspace, a workspace that is too
 * small or misaligned, list arrays that overlap an input, the workspace or each other -- returns non-zero with mkgnn_last_error
 * set, before any launch. */
#define MKGNN_KNN_MAX_K       64
#define MKGNN_KNN_MAX_QUERIES 1048576
#define MKGNN_KNN_MAX_ROWS    1048576
size_t mkgnn_embed_knn_workspace_bytes(int64_t n_rows, int32_t Q, int32_t K);
int mkgnn_embed_knn_update(const float* emb, int64_t emb_stride, int64_t n_rows, int32_t H, const int32_t* ids,
                           const int32_t* n_valid, const int32_t* shard_tag, const float* queries, int64_t query_stride, int32_t Q,
                           int32_t K, float* top_sim, int32_t* top_shard, int32_t* top_mol, void* workspace,
                           size_t workspace_bytes, void* stream);

/* ---- neighbour counts (additive; the ABI version stays 8): how many references lie within a similarity threshold of every
 * embedding row -- the count a Taylor-Butina clustering ranks its rows by (refs = emb, then mkgnn_diverse_pick in count order),
 * and the number of catalogue analogues of a hit.
 *   counts[i] = #{ r in [0, R) : sim(i, r) > min_sim }
 * with sim(i, r) the float32 value mkgnn_embed_cosine writes for row i as the ROW and refs[r] as the QUERY, BIT FOR BIT --
 * (dot * inv(e_i)) * inv(refs[r]); the orientation matters, the two multiplications do not commute in their last bit.  It is the
 * value mkgnn_diverse_pick compares, so a neighbour in the count is a neighbour in the walk.  The comparison is strict, as in
 * mkgnn_diverse_pick; a NaN similarity never counts (a NaN, infinite or overflowing row counts nothing; a NaN reference is
 * counted by no row).  The operator knows no "self": with refs = emb (the same pointer is allowed) the diagonal is a pair like
 * any other.  min_sim is passed by value and must be finite.  emb [n_rows, H] with emb_stride >= H, refs [R, H] with ref_stride
 * >= H, both RAW: the inverse norms are computed inside the call, into the workspace, so one captured call follows new contents
 * of both.  counts [n_rows] is contiguous; nothing else is written outside the workspace, and counts and the workspace must
 * overlap neither emb nor refs nor each other (rejected).
 *
 * It is mkgnn_embed_max_cosine's walk with another reduction: the same two launches on `stream`, three when the references are
 * split over the grid (every part writes its partial count to the workspace and a finishing launch adds them); capturable, no
 * host round trip, no atomics, no process-wide state, one writer per output.  counts[i] is a sum of integers: it depends on row
 * i and on the reference SET alone -- not on n_rows, the row's place in the grid, the strides, the order of the references, how
 * the launch splits them, or whether refs aliases emb.  The workspace (4-byte aligned,
 * mkgnn_embed_count_within_workspace_bytes(n_rows, R) bytes; 0 for rejected sizes) is
 *   [inverse norms: R + n_rows floats, padded to a multiple of 4][parts x n_rows int32 partial counts, when parts > 1]
 * and needs no initialisation: it is read only where the same call wrote it.
 *
 * Limits as for mkgnn_embed_max_cosine: 1 <= H <= 64; 1 <= R <= MKGNN_MAX_COSINE_MAX_REFS; 0 <= n_rows < 2^31 (a count fits
 * int32 with room to spare).  More references: call per slice and add.  n_rows == 0 is a no-op that returns 0, even with null
 * pointers.  Anything else -- a limit, a stride below H, a min_sim that is NaN or infinite, a null pointer, a workspace that is
 * too small or misaligned, an overlap -- returns non-zero with mkgnn_last_error set, before any launch. */
size_t mkgnn_embed_count_within_workspace_bytes(int64_t n_rows, int32_t R);
int mkgnn_embed_count_within(const float* emb, int64_t emb_stride, int64_t n_rows, int32_t H, const float* refs, int64_t ref_stride,
                             int32_t R, float min_sim, int32_t* counts, void* workspace, size_t workspace_bytes, void* stream);

/* ---- neighbour lists (additive; the ABI version stays 8): WHICH references lie within a similarity threshold of every embedding
 * row -- the pairs mkgnn_embed_count_within counts, written into a CSR whose row pointers the caller made from those counts.
 *   for row i, the r in [0, R) with sim(i, r) > min_sim, in ASCENDING r, as (nbr_ref, nbr_sim) = (r, sim(i, r)) in the slots
 *   row_ptr[i], row_ptr[i] + 1, ...;   found[i] = the number of such r, whether written or not
 * sim(i, r), the strict comparison and the NaN rule are mkgnn_embed_count_within's, BIT FOR BIT: nbr_sim holds the float32 values
 * mkgnn_embed_cosine writes for row i as the ROW and refs[r] as the QUERY, and found is what the count returns.  With row_ptr the
 * exclusive sum of the count's result for the same inputs and threshold (row_ptr[n_rows] <= capacity), every slot of
 * [0, row_ptr[n_rows]) is written exactly once.  emb, refs, the strides, min_sim: as for the count (refs may be emb: the self-join,
 * the diagonal a pair like any other).  row_ptr int64 [n_rows + 1] on the DEVICE, read when the launches run; nbr_ref int32 and
 * nbr_sim float32 [capacity] each, found int32 [n_rows], contiguous.
 *
 * THE GUARD.  Row i writes only slots s with  0 <= row_ptr[i] <= s < min(row_ptr[i + 1], capacity)  -- WHATEVER row_ptr holds:
 * counts of another threshold or of other contents, negative, non-monotone or huge values.  A row whose row_ptr[i] lies outside
 * [0, capacity), or whose segment is empty or runs backwards, writes nothing; pairs beyond the end of a segment are counted in
 * found and dropped, so found[i] > row_ptr[i + 1] - row_ptr[i] is how a caller sees that a list was cut (the prefix that was
 * written is right).  Segments that overlap because row_ptr is not monotone are written by more than one row, inside those
 * bounds.  capacity == 0 with null nbr_ref / nbr_sim is legal: found is still written.
 *
 * The count's walk with a third reduction.  References not split over the grid: the norms and ONE walk, which writes found itself.
 * Split: the norms, the COUNT walk into the workspace's [parts][n_rows] partials, a small launch that turns each row's partials
 * into exclusive offsets over the parts and writes found, then the FILL walk, every part starting at its offset -- so a split
 * call walks the references twice (on top of the caller's own count).  Capturable, no host round trip, no atomics, no
 * process-wide state, one writer per slot; plain FP32.  The lists depend on row i, the references and row_ptr alone -- not on
 * n_rows, the row's place in the grid, the strides, how the launch splits the references, or whether refs aliases emb.  The
 * workspace (4-byte aligned, mkgnn_embed_neighbours_within_workspace_bytes(n_rows, R) bytes; 0 for rejected sizes) is the count's:
 *   [inverse norms: R + n_rows floats, padded to a multiple of 4][parts x n_rows int32, when parts > 1]
 * and needs no initialisation.
 *
 * Limits as for the count: 1 <= H <= 64; 1 <= R <= MKGNN_MAX_COSINE_MAX_REFS; 0 <= n_rows < 2^31; 0 <= capacity.  n_rows == 0 is a
 * no-op that returns 0, even with null pointers.  Anything else -- a limit, a stride below H, a min_sim that is NaN or infinite,
 * a null emb, refs, row_ptr, found or workspace (or a null list with capacity > 0), a workspace that is too small or misaligned,
 * an output (the lists, found, the workspace) that overlaps emb, refs, row_ptr or another output -- returns non-zero with
 * mkgnn_last_error set, before any launch. */
size_t mkgnn_embed_neighbours_within_workspace_bytes(int64_t n_rows, int32_t R);
int mkgnn_embed_neighbours_within(const float* emb, int64_t emb_stride, int64_t n_rows, int32_t H, const float* refs,
                                  int64_t ref_stride, int32_t R, float min_sim, const int64_t* row_ptr, int64_t capacity,
                                  int32_t* nbr_ref, float* nbr_sim, int32_t* found, void* workspace, size_t workspace_bytes,
                                  void* stream);

/* ---- connected components of CSR neighbour lists (additive; the ABI version stays 8): the single-linkage clusters of a
 * threshold graph -- the finest partition with no linked pair across its parts.
 *   labels[v] = the smallest vertex of v's component, in the graph on [0, n) where u and v are linked if col holds v in u's
 *   segment [row_ptr[u], row_ptr[u + 1]) OR u in v's
 * The union matters: sim(i, j) and sim(j, i) of the lists above round their two scalings in different orders, so a threshold
 * graph can hold an edge in one direction only.  Self-loops and duplicate edges are harmless.  row_ptr int64 [n + 1] and col
 * int32 [row_ptr[n]] on the device; labels int32 [n].
 *
 * Nothing is indexed with input that was not checked: a segment is walked only if 0 <= row_ptr[v] <= row_ptr[v + 1] <= row_ptr[n]
 * and an edge used only if 0 <= col[e] < n; anything else is skipped and sets state[2] (so col must hold row_ptr[n] entries: that,
 * the operator cannot check).  With resume = 1 a label outside [0, v] is replaced by v and sets state[2] too.
 *
 * Hook and compress, in rounds of two launches: the hook reads both endpoints' parents of the previous round (roots, after its
 * compression; a snapshot) and lowers the larger root's entry of a copy to the smaller root with atomicMin; the compress makes
 * every vertex point at its root.  The fixpoint is unique, so the result is deterministic although the atomics' order is not.  A
 * call enqueues 2 ceil(log2 max(n, 2)) + 1 rounds; a per-round device flag makes every launch behind a round
 * that changed nothing return at once.  No host round trip; capturable.  state int32 [4] on the device:
 *   state[0] the rounds of this call that changed a label, state[1] 1 if the last enqueued round changed nothing (converged:
 *   labels is the answer), state[2] 1 if something was skipped as described, state[3] 0
 * resume: 0 starts from every vertex as its own label; 1 goes on from labels as an earlier call on the SAME graph left them --
 * what a caller does while state[1] == 0 (every such call lowers a label or converges).  Bits 8 and up of resume, when non-zero,
 * cap the rounds of the call below the number above (diagnostics: that is how the tests reach state[1] == 0).
 * The workspace (4-byte aligned, mkgnn_graph_components_workspace_bytes(n) = 4 (2 n + 72) bytes; 0 for a rejected n) needs no
 * initialisation.  0 <= n <= MKGNN_COMPONENTS_MAX_VERTICES; n == 0 writes state alone.  A limit, a resume that is neither, a null
 * row_ptr, state or workspace (or labels with n > 0), a workspace that is too small or misaligned, an output that overlaps
 * row_ptr or another output: non-zero with mkgnn_last_error set, before any launch. */
#define MKGNN_COMPONENTS_MAX_VERTICES 134217728
size_t mkgnn_graph_components_workspace_bytes(int32_t n);
int mkgnn_graph_components(const int64_t* row_ptr, const int32_t* col, int32_t n, int32_t* labels, int32_t* state, int32_t resume,
                           int32_t* workspace, size_t workspace_bytes, void* stream);

/* ---- MaxMin picking (additive; the ABI version stays 8): the farthest-first traversal of stored embeddings -- k_max rows that
 * are as different from each other as possible (RDKit's MaxMinPicker), the similarity at which each was taken, and the pick every
 * other row lies nearest to.  emb [n_rows, H] (emb_stride >= H, RAW).  The similarity is S[i, p]: the float32 value
 * mkgnn_embed_cosine writes for row i as the ROW and row p as the QUERY, BIT FOR BIT -- (dot * inv(e_i)) * inv(e_p), the
 * orientation and text mkgnn_diverse_pick uses.  molkgnn_amd/screening.py::maxmin_pick_reference is the definition:
 *   a row is VALID when S[i, i] is not NaN (a NaN, infinite or overflowing row is never picked, takes no part and keeps leader
 *   -1, leader_sim NaN).  cur[i] starts at start_sim[i] (the row's similarity to what the caller already owns: the first output of
 *   mkgnn_embed_max_cosine, say), or at -inf with start_sim null; a valid row whose start value is NaN is EXCLUDED: never picked,
 *   but assigned like any other.  leader[i] starts at -1.  Round t = 0 .. k_max - 1: the candidate is the valid, not excluded, not
 *   yet picked row with the SMALLEST cur (-0.0 == +0.0; among equals the lower row); without one, or unless cur < stop_sim
 *   (strict), the rounds end.  picks[t] = i, pick_sim[t] = cur[i] (its bits), leader[i] = i, cur[i] = S[i, i] (final).  Every valid,
 *   not picked row j then meets the pick: s = S[j, i] replaces cur[j], and i leader[j], when s is not NaN and cur[j] is NaN or
 *   s > cur[j] (strict: among equally near picks the EARLIER one leads).
 * Afterwards leader_sim[j] = cur[j] for the valid rows (a row nothing came nearer to than its start keeps -1 and its start
 * value's bits); unused slots of picks are -1, of pick_sim NaN; *n_picks is the number of picks (device memory).  pick_sim is
 * non-decreasing: it is the threshold a leader clustering would need for that many picks.
 *
 * Up to 1 024 rows ONE workgroup runs every round in one launch behind the init (a thread per row, the row in registers).  Beyond,
 * a round is two launches: a one-workgroup select (reduces the blocks' partial arg-mins, applies the stop rule, stages the pick)
 * and a grid-wide update (one pass over emb; every block leaves its new partial arg-min); 1 + 2 k_max launches are enqueued, and
 * once the rounds have ended a device flag makes the remaining ones return at once.  The launch boundary is the only thing that
 * orders workgroups against each other.  Everything runs on `stream`, is capturable, has no host round trip, no atomics and no
 * state between calls; the inverse norms and S[i, i] are computed inside the call, so a captured call follows new contents of emb
 * and start_sim.  The result is a function of emb, start_sim, stop_sim and k_max alone: not of the block size, the stride or which
 * of the two forms ran.  The workspace (4-byte aligned, mkgnn_maxmin_pick_workspace_bytes(n_rows) =
 * 4 (3 ceil4(n_rows) + 2 ceil4(ceil(n_rows / 256)) + 72) bytes, ceil4 rounding up to a multiple of 4; 0 for rejected sizes) needs no
 * initialisation.
 *
 * Limits: 1 <= H <= 64; 1 <= n_rows <= MKGNN_MAXMIN_MAX_ROWS (2^20); 1 <= k_max <= min(n_rows, MKGNN_MAXMIN_MAX_PICKS); stop_sim
 * not NaN (+inf: no stop; -inf: no pick).  n_rows == 0 is a no-op that returns 0, even with null pointers.  Anything else -- a
 * limit, a NaN stop_sim, a stride below H, a null pointer other than start_sim, a workspace that is too small or misaligned,
 * overlapping buffers -- returns non-zero with mkgnn_last_error set, before any launch. */
#define MKGNN_MAXMIN_MAX_ROWS  1048576
#define MKGNN_MAXMIN_MAX_PICKS 4096
size_t mkgnn_maxmin_pick_workspace_bytes(int64_t n_rows);
int mkgnn_maxmin_pick(const float* emb, int64_t emb_stride, int64_t n_rows, int32_t H, const float* start_sim /* [n_rows] or null */,
                      float stop_sim, int32_t k_max, int32_t* picks, float* pick_sim, int32_t* n_picks, int32_t* leader,
                      float* leader_sim, void* workspace, size_t workspace_bytes, void* stream);

/* ---- Bootstrap replicates of AUC and logAUC (additive; the ABI version stays 8): B resamples of n scored rows, evaluated without
 * sorting any of them.  The caller sorts ONCE (scores descending, stable) and passes
 *   rank [n] int32     the rank of row i, the rows in the caller's order or, for a stratified bootstrap, class-major: the `split`
 *                      actives first, then the inactives
 *   y_sorted [n] uint8    non-zero where the row at a rank is active
 *   group_last [n] uint8  non-zero where a rank ends its tie group (the next rank's score differs)
 * Replicate b (b = 0 .. B - 1) draws, for every row i, the row
 *   j = lo + ((uint64) philox_word(seed, offset + b, i) * size >> 32),   (lo, size) = (0, split) for i < split, (split, n - split) else
 * (philox_word as the dropout kernels draw it: Philox4x32-10 keyed by seed, counter (i / 4, offset + b), word i % 4), and
 * c[rank[j]] grows by one.  The call consumes the offsets offset .. offset + B - 1; with split = n the bootstrap is unstratified.
 * molkgnn_amd/evaluation.py::bootstrap_reference is the definition of what follows: per tie group gt and gf, the drawn actives
 * and inactives; a group with none does not exist in the replicate; the ROC points are the running sums (fps, tps) at the end of
 * each remaining group; T and F the totals.
 *   n_pos[b] = T (F = n - T)
 *   two_u[b] = sum over the groups of gf * (2 * tps_before + gt), an exact integer
 *   auc[b]   = (double) two_u / (double) (2 T F): one float64 division, bit for bit on every route
 *   logauc[b] = the area under the curve over log10(FPR) in [lower, upper], divided by log10(upper) - log10(lower): the points
 *               thinned as sklearn.roc_curve(drop_intermediate=True) thins them (the first and last stay, an interior point iff its
 *               group's (gf, gt) differs from the next existing group's), (0, 0) in front, every consecutive pair clipped to
 *               [lower, upper] in linear FPR with np.interp's formula, then (log10(b) - log10(a)) * (ya + yb) / 2
 *   T == 0 or F == 0: auc[b] and logauc[b] are NaN.
 * A replicate's four outputs are a function of (rank, y_sorted, group_last, n, split, seed, offset + b, lower, upper) alone: not
 * of B, of where the call's replicates start, of the workspace's size, of which form ran or of the run.  The integers and the
 * AUC are exact; the log-area is a float64 sum in one fixed order (tiles of 1 024 ranks in rank order, a tile's trapezoids by a
 * fixed tree).  A rank outside [0, n) is skipped, never used as an address (its replicate's totals then fall short of n).
 *
 * Up to 8 192 rows ONE launch does everything: one workgroup per replicate holds the multiplicities in LDS, draws, counts and
 * walks; the workspace is not touched.  Beyond, the call passes over the replicates, as many at a time as the workspace holds --
 * floor(workspace_bytes / (4 ceil4(n))), at least one --: a launch that clears the pass's multiplicities and n_pos, a grid-wide draw-and-
 * count launch (integer atomicAdd; no float atomics anywhere) and a walk launch of one workgroup per replicate.  The launch
 * boundary is the only thing that orders workgroups against each other.  Everything runs on `stream`, is capturable, has no host
 * round trip and no state between calls.  mkgnn_bootstrap_roc_workspace_bytes(n, replicates_per_pass) = 4 ceil4(n) *
 * replicates_per_pass bytes beyond 8 192 rows, 16 up to there, 0 for rejected sizes; it is host arithmetic only.  Callers keep the
 * workspace at or under MKGNN_BOOTSTRAP_WORKSPACE_CAP (1 GiB: 256 replicates of 2^20 rows in flight, 64 of 2^22) and let the call
 * chunk B; the workspace is 16-byte aligned and needs no initialisation.
 *
 * Limits: 1 <= n <= MKGNN_BOOTSTRAP_MAX_ROWS (2^22: every count and 2 T F stay exact); 1 <= B <= MKGNN_BOOTSTRAP_MAX_REPLICATES
 * per call; 0 <= split <= n; 0 < lower < upper <= 1.  Anything else -- a limit, a null pointer, a workspace that is misaligned or
 * holds no replicate, overlapping buffers -- returns non-zero with mkgnn_last_error set, before any launch. */
#define MKGNN_BOOTSTRAP_MAX_ROWS       4194304
#define MKGNN_BOOTSTRAP_MAX_REPLICATES 4096
#define MKGNN_BOOTSTRAP_WORKSPACE_CAP  1073741824
size_t mkgnn_bootstrap_roc_workspace_bytes(int64_t n, int32_t replicates_per_pass);
int mkgnn_bootstrap_roc(const int32_t* rank, const uint8_t* y_sorted, const uint8_t* group_last, int64_t n, int64_t split, int32_t B,
                        uint64_t seed, uint64_t offset, double lower, double upper, double* auc, double* logauc, int64_t* two_u,
                        int32_t* n_pos, void* workspace, size_t workspace_bytes, void* stream);

/* ---- Early-recognition functionals of the same replicates (additive; the ABI version stays 8): mkgnn_bootstrap_roc's call with
 * three more outputs per replicate, formed in the same walk behind the same draw -- the same clear and draw kernels, the same
 * number of launches, only the walk kernel differs.  molkgnn_amd/evaluation.py::early_reference is the definition.  With the
 * groups of the replicate as above, P_g the drawn rows in front of group g, sg = gt + gf its rows, tps_g the actives up to and
 * including it, N = n:
 *   ap[b]          = sum over the groups with gt > 0 of (gt / (double) T) * (tps_g / (double) (P_g + sg))
 *                    (sklearn.metrics.average_precision_score with the multiplicities as sample weights; 0 without an active)
 *   hits[b, j]     = (double) (tps_g - gt) + (double) gt * (double) (cuts[j] - P_g) / (double) sg  for the ONE group with
 *                    P_g < cuts[j] <= P_g + sg: the expected actives among the first cuts[j] drawn rows when a tie group's rows
 *                    are in random order.  Bit for bit the definition's
 *   rie[b, a]      = sum over the groups with gt > 0 of
 *                    gt * exp(-(alpha (P_g + 1)) / N) * (-expm1(-(alpha sg) / N)) / (-expm1(-alpha / N)) / sg
 *                    (the sum over the drawn actives of exp(-alpha r / N), a tied active taking the mean over its group's positions)
 * ap and rie are float64 sums in the log-area's fixed order; they agree with the definition within a relative (m + 16) 2^-53 for m
 * positive terms plus the device's exp and expm1.  The enrichment factor, BEDROC and average precision follow from them, T and N
 * on the host (evaluation.early_derived).  The points are taken BEFORE the thinning, which concerns the logAUC alone.
 *   cuts [J] int32 and alphas [A] float64 are DEVICE arrays (a captured call follows new values written into them);
 *   0 <= J <= MKGNN_BOOTSTRAP_MAX_CUTS, 0 <= A <= MKGNN_BOOTSTRAP_MAX_ALPHAS; with J == 0 cuts and hits may be null, with A == 0
 *   alphas and rie.  hits is [B, J] and rie [B, A], row-major.
 * A cut outside [1, n], and an alpha outside (0, 500] or not finite, is never an address and enters no sum: its column of hits or
 * rie is NaN and nothing else changes.  auc, logauc, two_u and n_pos are bit for bit mkgnn_bootstrap_roc's for the same arguments,
 * and a replicate's outputs are a function of (rank, y_sorted, group_last, n, split, seed, offset + b, lower, upper, cuts,
 * alphas) alone.  The workspace rule is mkgnn_bootstrap_roc_workspace_bytes'.  The limits and refusals are mkgnn_bootstrap_roc's,
 * with J, A, the five new pointers (8-byte aligned; cuts 4-byte) and the aliasing of ap, hits and rie against everything else. */
#define MKGNN_BOOTSTRAP_MAX_CUTS   8
#define MKGNN_BOOTSTRAP_MAX_ALPHAS 4
int mkgnn_bootstrap_early(const int32_t* rank, const uint8_t* y_sorted, const uint8_t* group_last, int64_t n, int64_t split, int32_t B,
                          uint64_t seed, uint64_t offset, double lower, double upper, const int32_t* cuts, int32_t J,
                          const double* alphas, int32_t A, double* auc, double* logauc, int64_t* two_u, int32_t* n_pos, double* ap,
                          double* hits, double* rie, void* workspace, size_t workspace_bytes, void* stream);

/* ---- Bootstrap replicates of the regression metrics (additive; the ABI version stays 8): the raw sums of RMSE, MAE, R2, Pearson,
 * Spearman and top-fraction recall of B resamples of n rows with a prediction p and a truth t each, none of which is ever sorted.
 * The caller sorts BOTH vectors once (best first, stable, the same direction for both) and passes
 *   rank_p [n] int32                 row i -> its prediction rank (what the draw scatters through)
 *   first_p, last_p [n] int32        by prediction rank: the first and the last rank of the rank's tie group
 *   cross [n] int32                  truth rank -> the prediction rank of the same row
 *   first_t, last_t [n] int32        by truth rank: the first and the last rank of the rank's tie group
 *   p_sorted, t_by_prank [n] float64 by prediction rank: the row's prediction and its truth
 *   centre [2] float64, DEVICE       the values the moments are centred on (the full sample's mean of p and of t)
 *   cuts [J] int32, DEVICE           the top-k sizes, 0 <= J <= MKGNN_BOOTSTRAP_MAX_CUTS (J == 0: cuts and hits may be null)
 * Replicate b draws as the unstratified mkgnn_bootstrap_roc does (split = n): row i draws row j = (uint64) philox_word(seed,
 * offset + b, i) * n >> 32 and c[rank_p[j]] grows by one, so a regression fold and a classification fold with the same (seed,
 * offset, n) see the same rows.  With Cp and Ct the inclusive prefix sums of c by prediction rank and by truth rank (Cp[-1] = 0)
 * and N = the drawn rows, molkgnn_amd/evaluation.py::regression_reference_sorted is the definition of
 *   mom[b, 0..6]       sum c dp, sum c dt, sum c dp^2, sum c dt^2, sum c dp dt, sum c |p - t|, sum c (p - t)^2 with dp = p -
 *                      centre[0], dt = t - centre[1]; every term (double) c * (product), the product formed first, over the rows
 *                      with c > 0.  float64 sums in one fixed order (tiles of 1 024 prediction ranks in rank order, a tile's terms
 *                      by a fixed tree): |mom - definition| <= (m + 16) 2^-53 sum c |term| for m terms
 *   rank_sums[b, 0..2] sum c a b, sum c a^2, sum c b^2 with a = 2 midrank_p - (N + 1) = Cp[first_p - 1] + Cp[last_p] - N of the
 *                      row's tie group in prediction order and b the same in truth order: exact integers (|sum| <= n (n - 1)^2 <
 *                      2^63 up to MKGNN_BOOTSTRAP_REG_MAX_ROWS).  Spearman = xy / sqrt(xx yy)
 *   hits[b, j]         sum over the rows of min(clamp(cuts[j] - (Cp[q] - c), 0, c), clamp(cuts[j] - (Ct[r] - c), 0, c)), q and r the
 *                      row's two ranks: the drawn copies that lie among the first cuts[j] copies in BOTH orders, copies ordered by
 *                      (stable rank, copy number).  Exact.  A cut outside [1, n] is never used: its column is -1, nothing else changes
 *   n_drawn[b]         N (n, unless a rank_p entry was out of range)
 * evaluation.regression_derived turns them into the metrics.  A replicate's outputs are a function of (the ten arrays, n, seed,
 * offset + b) alone: not of B, of where the call's replicates start, of the workspace's size or of the run.  Every index read from
 * rank_p, cross, first_* and last_* is compared against n before it is an address: a drawn row whose rank_p is out of range is
 * not drawn, a truth rank whose cross is out of range holds no copy, and a row with a first_* or last_* out of range enters no
 * integer sum.
 *
 * The call passes over the replicates, as many at a time as the workspace holds -- floor(workspace_bytes / (8 ceil4(n))), at least
 * one; mkgnn_bootstrap_regression_workspace_bytes(n, replicates_per_pass) = 2 * 4 ceil4(n) * replicates_per_pass, 0 for rejected
 * sizes --: mkgnn_bootstrap_roc's clear and draw launches (integer atomicAdd; no float atomics anywhere), then ONE walk launch of one
 * workgroup per replicate that sweeps the ranks three times -- prediction order (Cp in place of c, the moments), truth order (Ct),
 * truth order again (the gathers and the integer sums).  The launch boundary is the only thing that orders workgroups against
 * each other; no cooperative launch, no flag a workgroup waits on, no host round trip, no state between calls; capturable, and a
 * captured call follows new values in every array, centre and cuts included.  The workspace is 16-byte aligned, needs no
 * initialisation and stays at or under MKGNN_BOOTSTRAP_WORKSPACE_CAP by the caller's choice of replicates per pass.
 *
 * Limits: 1 <= n <= MKGNN_BOOTSTRAP_REG_MAX_ROWS (2^20); 1 <= B <= MKGNN_BOOTSTRAP_MAX_REPLICATES per call; 0 <= J <=
 * MKGNN_BOOTSTRAP_MAX_CUTS.  Anything else -- a limit, a null pointer, a misaligned array (4 bytes for int32, 8 for float64 and
 * int64, 16 for the workspace), a workspace that holds no replicate, overlapping buffers -- returns non-zero with mkgnn_last_error
 * set, before any launch. */
#define MKGNN_BOOTSTRAP_REG_MAX_ROWS 1048576
size_t mkgnn_bootstrap_regression_workspace_bytes(int64_t n, int32_t replicates_per_pass);
int mkgnn_bootstrap_regression(const int32_t* rank_p, const int32_t* first_p, const int32_t* last_p, const int32_t* cross,
                               const int32_t* first_t, const int32_t* last_t, const double* p_sorted, const double* t_by_prank,
                               const double* centre, const int32_t* cuts, int32_t J, int64_t n, int32_t B, uint64_t seed,
                               uint64_t offset, double* mom, int64_t* rank_sums, int64_t* hits, int32_t* n_drawn, void* workspace,
                               size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MOLKGNN_HIP_H */
