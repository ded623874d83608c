// The fused tail for SEVERAL outputs (mkgnn_tail_fused_labels, kgnn_readout.hip): the training form of
// tail_middle_kernel (kgnn_tail.hip) with a T-output head behind the readout -- the label-matrix head (labels [n, T], NaN = not
// measured; readout.label_head_reference) or the task-indexed head (one task per molecule; readout.task_head_reference):
//     pred[i, t] = (keep_i * emb_i) . w_t + b_t                                   for EVERY (i, t)
//     loss       = sum over the labelled (i, t) of s_i * term(pred[i, t], y[i, t]) / max(n_labelled, 1)      (SQERR_SUM: not divided)
// Same windows, chunks, phases P1 to P6, work distribution (tail_group_size / tail_middle_blocks: functions of n_loss alone, so
// a padded batch gives the unpadded batch's bits) and slab epilogue; kgnn_tail.hip's instantiations are not touched.  Only the
// per-molecule phase differs: the 32 lanes of a row slot hold the molecule's emb * keep, so
//     logit t  = the xor tree of emb_j keep_j w[t][j] + b_t, kept by lane t -- which also keeps entry (i, t)'s label, its term and d_t;
//     d emb_j  = keep_j * sum over t ASCENDING of d_t * w[t][j];
//     d W_head[t][j] += d_t * emb_j keep_j and d b_head[t] += d_t as per-thread partials, the loss as a per-lane partial.
// The head matrix lives in REGISTERS (lane j: column j, w[0 .. T)[j]) and so do the d W_head partials: 2 TB VGPRs for a task
// bound TB (a template parameter), no LDS -- the training form's 52 468 bytes of LDS stay what they are.  Up to TB3 = 10 tasks
// the kernel keeps the 168 VGPRs of three workgroups per CU; a wider head (TB = 32) is bounded for two, knowingly (DESIGN 4.4p
// has the compiler's figures and the measurement).
// With T = 1 and a dense label column every statement that reaches a result is the single-task kernel's: the bits are its bits.
//
// THE DIVISOR.  n_labelled depends on the data and d z leaves this kernel final, so the count is on the device before any d is
// formed: tail_label_count_kernel (a few blocks, integer partial counts of the first n_loss rows) runs in front, and every
// workgroup of the middle kernel adds the partials up in its prologue.  Integers: exact in any order, no atomics, no read-back,
// nothing depends on the order in which workgroups arrive, capturable.
// An unlabelled entry is removed by a select: its label and its weight reach nothing; a molecule without a label gets d = 0 in
// every task and with it exactly zero d z rows.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <math.h>

#include "kgnn_common.h"
#include "kgnn_launch.h"
#include "kgnn_philox.h"
#include "kgnn_sigmoid.h"
#include "kgnn_tail_shared.h"
#include "../../include/molkgnn_hip.h"

namespace mkgnn {
namespace tail {

constexpr int LLDS_FLOATS = 32 * WP + 2 * AC * HP + 3 * MC * HP + 96;      // (the training form's: kgnn_tail.hip)
constexpr int LLDS_INTS = AC + 2 * (AC + 1) + 2 * EC + 3 * (MC + 1) + 4;
constexpr int TMAX = MKGNN_TASK_HEAD_MAX_TASKS;
constexpr int TB3 = 10;                 // the widest head whose register arrays fit beside three workgroups per CU (see the launcher)
static_assert(TMAX == 32, "one lane of a row slot per task");
static_assert(8 * TMAX * 32 <= 2 * AC * HP, "the epilogue's d W_head image fits the two atom-row images");

// gather_rows<AC / 32> as two passes of half as many atoms: the same sums atom by atom (so the same bits), half the rows in
// flight -- 32 VGPRs less at the kernel's widest point, which the head's register arrays need
__device__ __forceinline__ void gather_halves(const int* rp, const int* ec, const float* rows, int at0, int A, int l, f32x4 (&out)[AC / 32]) {
    static_assert(AC / 32 == 4, "two passes of two atoms");
    f32x4 h[2];
    gather_rows<2>(rp, ec, rows, at0, A, l, h);
    out[0] = h[0]; out[1] = h[1];
    asm volatile("" ::: "memory");                       // (keeps the scheduler from merging the passes again)
    gather_rows<2>(rp, ec, rows, at0 + 64, A, l, h);
    out[2] = h[0]; out[3] = h[1];
}

// entry (i, tk), i < n_loss: labelled?  y: its label (only read where labelled)
__device__ __forceinline__ bool label_of(const TailLabelArgs& la, int64_t i, int tk, float& y) {
    int64_t r = i;
    bool in = true;
    if (la.row_ids) {
        r = la.row_ids[i];
        in = r >= 0 && r < (la.labels ? la.n_label_rows : la.n_task);      // (an id outside the table: no label in any task)
        if (!in) r = 0;
    }
    if (la.labels) {
        y = la.labels[r * la.ls + tk];
        return in && y == y;                             // only NaN means missing
    }
    const int tsk = la.task[r];
    y = la.m.y[i];
    return in && tsk == tk;
}

__global__ void __launch_bounds__(256) tail_label_count_kernel(TailLabelArgs la) {
    __shared__ int part[4];
    const int T = la.T;
    const int64_t total = la.m.n_loss * T;
    int c = 0;
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < total; q += (int64_t)gridDim.x * 256) {
        const int64_t i = q / T;
        float y;
        c += label_of(la, i, (int)(q - i * T), y) ? 1 : 0;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) la.counts[blockIdx.x] = part[0] + part[1] + part[2] + part[3];
}

// LK, RD: as tail_middle_kernel's.  The weights (la.m.sw, la.m.pw) are looked at at run time.
template <int LK, bool RD, int TB>
__global__ void __launch_bounds__(NT, TB > TB3 ? 2 : 3) tail_labels_middle_kernel(TailLabelArgs la) {
    const TailMidArgs& a = la.m;
    __shared__ __align__(16) float lds[LLDS_FLOATS + LLDS_INTS];
    float* const W2s = lds;                              // [32][HP]
    float* const zp = W2s + 32 * WP;                     // [AC][HP]: pre, later d pre
    float* const dzb = zp + AC * HP;                     // [AC][HP]: z, then swish(pre), then d z
    float* const emol = dzb + AC * HP;                   // [MC][HP]: d e_g
    float* const emol_e = emol + MC * HP;                // [MC][HP]: e_g
    float* const emol_d = emol_e + MC * HP;              // [MC][HP]: d emb_g
    float* const vec = emol_d + MC * HP;                 // b1 | b2 | (free)
    int* const amol = (int*)(vec + 96);                  // [AC] molecule of the chunk
    int* const rpin = amol + AC;                         // [AC + 1] local edge offsets, by target
    int* const rpout = rpin + AC + 1;                    // [AC + 1] by source
    int* const ecin = rpout + AC + 1;                    // [EC] local source of every in-edge (-1: outside the chunk)
    int* const ecout = ecin + EC;                        // [EC]
    int* const mptr = ecout + EC;                        // [MC + 1] first atom of every molecule of the window
    int* const mein = mptr + MC + 1;                     // [MC + 1] first in-edge
    int* const meout = mein + MC + 1;                    // [MC + 1] first out-edge
    int* const ctl = meout + MC + 1;                     // [0] molecules of this chunk, [1] labelled entries of the call
    const int t = threadIdx.x, j = t & 31, slot = t >> 5;      // the per-molecule phase: (row slot of 8, hidden unit / task)
    const int l = t & 7, as = t >> 3;                          // the per-atom phases: (atom slot of 32, 16-byte lane of 8)
    const int H = a.H, G = a.G, T = la.T;

    // ---- once: the weights (every load first, then the stores), the head matrix's column j, the labelled-entry count
    float w2r[4], vr = 0.f;
#pragma unroll
    for (int u = 0; u < 4; ++u) { const int i = t + NT * u; w2r[u] = a.w2[i < G * H ? i : 0]; }
    {
        const float* vp = t < 32 ? a.b1 : a.b2;
        const int lim = t < 32 ? H : G, k = t & 31;
        if (t < 64 && vp && k < lim) vr = vp[k];
    }
    float whc[TB];                                       // w[tk][j] (0 at j >= G and tk >= T)
#pragma unroll
    for (int tk = 0; tk < TB; ++tk) { whc[tk] = 0.f; if (tk < T && j < G) whc[tk] = a.wh[tk * G + j]; }
    const int jt = j < T ? j : 0;
    int cnt_part = 0;
    if (t < 64 && t < la.n_counts) cnt_part = la.counts[t];
    const bool drop = a.drop_p > 0.f;
    const bool weighted = a.sw || a.pw;
    const uint64_t seed = (drop || RD) ? (uint64_t)a.rng[0] : 0, offset = (drop || RD) ? (uint64_t)a.rng[1] : 0;
    if (t < 64) {                                        // (wave 0: the partial counts, integers -- exact in any order)
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) cnt_part += __shfl_xor(cnt_part, o, 64);
        if (t == 0) ctl[1] = cnt_part;
    }
    for (int i = t; i < 32 * WP; i += NT) W2s[i] = 0.f;
    if (t < 96) vec[t] = vr;
    __syncthreads();
#pragma unroll
    for (int u = 0; u < 4; ++u) { const int i = t + NT * u; if (i < G * H) { const int r = i / H, c = i - r * H; W2s[r * WP + c] = w2r[u]; } }
    const int n_lab = ctl[1];
    const float invB = 1.f / (float)(n_lab > 1 ? n_lab : 1);

    // this workgroup's molecules: as tail_middle_kernel (groups of MG molecules, group g to workgroup g mod gridDim.x)
    const int MG = a.mg;
    const int64_t n_groups = (a.n_mols + MG - 1) / MG;
    int64_t grp = blockIdx.x;
    int64_t m_next = grp * MG;
    int64_t m_hi = m_next + MG < a.n_mols ? m_next + MG : a.n_mols;
    if (grp >= n_groups) m_next = m_hi = 0;

    float accW2[4] = {0.f, 0.f, 0.f, 0.f};
    f32x4 acc_b1 = {0.f, 0.f, 0.f, 0.f};
    float acc_b2 = 0.f, acc_bh = 0.f, acc_loss = 0.f;    // acc_bh, acc_loss: lane t holds task t's
    float acc_wh[TB];                                    // d W_head[tk][j], this row slot's molecules
#pragma unroll
    for (int tk = 0; tk < TB; ++tk) acc_wh[tk] = 0.f;

    __syncthreads();
    while (true) {
        if (m_next >= m_hi) {                            // (block-uniform) this group is done: the next one of this workgroup
            grp += gridDim.x;
            if (grp >= n_groups) break;
            m_next = grp * MG;
            m_hi = m_next + MG < a.n_mols ? m_next + MG : a.n_mols;
        }
        const int64_t m0 = m_next;
        // ---- the window: first atom and first edges of the next MC + 1 molecules
        if (t <= MC) {
            const int64_t m = m0 + t < a.n_mols ? m0 + t : a.n_mols;
            const int at = a.mol_ptr[m];
            mptr[t] = at;
            mein[t] = a.rin[at];
            meout[t] = a.rout[at];
        }
        __syncthreads();
        if (t == 0) {
            int nm = 0;
            const int lim = (int)(m_hi - m0 < MC ? m_hi - m0 : MC);
            while (nm < lim && mptr[nm + 1] - mptr[0] <= AC && mein[nm + 1] - mein[0] <= EC && meout[nm + 1] - meout[0] <= EC) ++nm;
            ctl[0] = nm;
        }
        __syncthreads();
        const int nm = ctl[0];
        if (nm == 0) {                                   // (block-uniform) one molecule beyond a chunk: skipped, reported as NaN.
            // Its atoms still get a d z row (zero): the projection kernel behind this one reads every row.
            const int a0 = mptr[0], A = mptr[1] - a0;
            for (int i = t; i < A * 32; i += NT) a.dz[(int64_t)a0 * 32 + i] = 0.f;
            if (t == 0) acc_loss = __builtin_nanf("");
            if (m0 < a.n_loss && t < T) la.pred[m0 * la.ps + t] = __builtin_nanf("");      // (every entry of pred is written)
            m_next = m0 + 1;
            __syncthreads();
            continue;
        }
        m_next = m0 + nm;
        const int a0 = mptr[0], A = mptr[nm] - a0;
        const int ein0 = mein[0], nin = mein[nm] - ein0, eout0 = meout[0], nout = meout[nm] - eout0;
        // (A == 0: a chunk of empty molecules only -- see tail_middle_kernel: no load below leaves the arrays then)
        // ---- P1: per atom -- molecule, edge offsets; the z rows
        if (t <= A) {
            const int n = A > 0 ? a0 + (t < A ? t : A - 1) : 0;
            const int mol = a.atom_mol[n] - (int)m0;
            const int ri = a.rin[a0 + t] - ein0, ro = a.rout[a0 + t] - eout0;      // (t == A: the end of the last atom's edges)
            if (t < A) amol[t] = mol;
            rpin[t] = ri; rpout[t] = ro;
        }
        {
            f32x4 zr[AC / 32];
            const int zlast = A > 0 ? a0 + A - 1 : 0;
#pragma unroll
            for (int q = 0; q < AC / 32; ++q) { const int at = as + 32 * q; zr[q] = *(const f32x4*)(a.z + (int64_t)(at < A ? a0 + at : zlast) * 32 + 4 * l); }
#pragma unroll
            for (int q = 0; q < AC / 32; ++q) { const int at = as + 32 * q; if (at < A) *(f32x4*)(dzb + at * HP + 4 * l) = zr[q]; }
        }
        {
            int ci[EC / NT], co[EC / NT];
#pragma unroll
            for (int u = 0; u < EC / NT; ++u) {          // (no edge one way: nothing to read -- ein0 may be the end of cin)
                const int i = t + NT * u;
                ci[u] = a.cin[nin > 0 ? ein0 + (i < nin ? i : 0) : 0];
                co[u] = a.cout[nout > 0 ? eout0 + (i < nout ? i : 0) : 0];
            }
#pragma unroll
            for (int u = 0; u < EC / NT; ++u) {
                const int i = t + NT * u;
                if (i < nin) { const int s = ci[u] - a0; ecin[i] = (s >= 0 && s < A) ? s : -1; }
                if (i < nout) { const int s = co[u] - a0; ecout[i] = (s >= 0 && s < A) ? s : -1; }
            }
        }
        __syncthreads();
        // ---- P3: pre = b1 + sum of z over the in-edges; swish (times the readout's keep with RD)
        f32x4 sw[AC / 32];
        {
            const f32x4 b1v = *(const f32x4*)(vec + 4 * l);
            f32x4 p[AC / 32];
            gather_halves(rpin, ecin, dzb, as, A, l, p);
#pragma unroll
            for (int u = 0; u < AC / 32; ++u) {
                const int at = as + 32 * u;
                const f32x4 pv = b1v + p[u];
                sw[u] = f32x4{0.f, 0.f, 0.f, 0.f};
                if (at < A) {
                    *(f32x4*)(zp + at * HP + 4 * l) = pv;
#pragma unroll
                    for (int c = 0; c < 4; ++c) sw[u][c] = pv[c] * sigmoidf_(pv[c]);
                    if constexpr (RD) {
                        float ks[4];
                        readout_keep4(seed, offset, (int64_t)a0 + at, H, l, a.rdrop_p, ks);
#pragma unroll
                        for (int c = 0; c < 4; ++c) sw[u][c] *= ks[c];
                    }
                }
            }
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < AC / 32; ++q) { const int at = as + 32 * q; if (at < A) *(f32x4*)(dzb + at * HP + 4 * l) = sw[q]; }
        __syncthreads();
        // ---- P4: per molecule -- pool, lin2, the T logits, their terms, and the way back to d e_g
        for (int g = slot; g < nm; g += 8) {
            const int64_t gi = m0 + g;
            const bool counted = gi < a.n_loss;
            int jv = j;                                  // (opaque per molecule: the 32 "lane == task" masks are formed where they are
            asm volatile("" : "+v"(jv) :: "memory");     // used -- hoisted out of the loop they cost 64 SGPRs, spilled; and W2's row and
                                                         // column are read from LDS per molecule, not kept in 64 VGPRs across the loop)
            // (this molecule's label, task and weight first: they are in flight while the atoms are pooled)
            float yv = 0.f, s = 1.f;
            bool lab = false;
            const float bhl = a.bh ? a.bh[jt] : 0.f;     // lane t: b_t, and the positive weight of task t (per molecule, not kept: two
            const float pwl = a.pw ? a.pw[jt] : 1.f;     // registers the per-atom phases need)
            if (counted && j < T) {
                lab = label_of(la, gi, j, yv);
                if (a.sw) {
                    if (a.wids) {
                        const int64_t r = a.wids[gi];
                        const bool in = r >= 0 && r < a.n_sw;      // (an id outside the table: weight +0.0)
                        s = a.sw[in ? r : 0];
                        if (!in) s = 0.f;
                    } else {
                        s = a.sw[gi];
                    }
                }
            }
            const int b0 = mptr[g] - a0, b1_ = mptr[g + 1] - a0;
            float e = 0.f;
            for (int at = b0; at < b1_; at += 8) {       // (eight reads in flight; the order of the sum stays atom by atom)
                float v[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) v[u] = dzb[(at + u < b1_ ? at + u : b1_ - 1) * HP + j];
#pragma unroll
                for (int u = 0; u < 8; ++u) if (at + u < b1_) e += v[u];
            }
            const float cnt = (float)(b1_ - b0);
            float emb = vec[32 + j] * cnt;
#pragma unroll
            for (int k = 0; k < 32; ++k) emb = fmaf(W2s[j * WP + k], lane_of(e, k), emb);
            if (a.emb && j < G) a.emb[gi * a.es + j] = emb;
            const float ks = (drop && j < G) ? keep_scale_of(seed, offset, (uint64_t)(counted ? gi : 0) * G + j, a.drop_p) : 1.f;
            // the T logits: lane tk keeps logit tk (the single-task kernel's product, tree and bias, task by task)
            float x = 0.f;
#pragma unroll
            for (int tk = 0; tk < TB; ++tk) {
                if (tk < T) {                            // (block-uniform)
                    const float v = half_sum(j < G ? emb * ks * whc[tk] : 0.f);
                    if (jv == tk) x = v + bhl;
                }
            }
            if (counted && j < T) la.pred[gi * la.ps + j] = x;
            // lane tk: entry (gi, tk)'s d and term -- the single-task kernel's statements, unweighted and weighted
            float d = 0.f;
            if (weighted) {
                if (lab) {
                    float d0, t0;
                    if constexpr (LK == MKGNN_LOSS_BCE_MEAN) {
                        if (a.pw && pwl != 1.f) {        // (a positive weight of exactly 1: the unweighted statements and their bits)
                            const float L = fmaf(pwl - 1.f, yv, 1.f);
                            d0 = fmaf(-L, sigmoidf_(-x), 1.f - yv);
                            t0 = fmaf(L, log1pf(expf(-fabsf(x))) + fmaxf(-x, 0.f), (1.f - yv) * x);
                        } else {
                            d0 = sigmoidf_(x) - yv;
                            t0 = fmaxf(x, 0.f) - x * yv + log1pf(expf(-fabsf(x)));
                        }
                    } else {
                        const float r = x - yv;
                        d0 = 2.f * r;
                        t0 = r * r;
                    }
                    d = LK == MKGNN_LOSS_SQERR_SUM ? s * d0 : invB * (s * d0);
                    acc_loss += LK == MKGNN_LOSS_SQERR_SUM ? s * t0 : invB * (s * t0);
                    acc_bh += d;
                }
            } else if (lab) {
                if constexpr (LK == MKGNN_LOSS_BCE_MEAN) {
                    d = invB * (sigmoidf_(x) - yv);
                    acc_loss += invB * (fmaxf(x, 0.f) - x * yv + log1pf(expf(-fabsf(x))));      // torch's stable form
                    acc_bh += d;
                } else {                                 // squared error: d = 2 (x - y), / n_labelled for the mean
                    const float r = x - yv;
                    d = LK == MKGNN_LOSS_SQERR_MEAN ? invB * (2.f * r) : 2.f * r;
                    acc_loss += LK == MKGNN_LOSS_SQERR_MEAN ? invB * (r * r) : r * r;
                    acc_bh += d;
                }
            }
            // d emb_j = keep_j * sum over tk ascending of d_tk w[tk][j];  d W_head[tk][j] += d_tk * emb_j keep_j
            const float ek = emb * ks;
            float dsum = 0.f;
#pragma unroll
            for (int tk = 0; tk < TB; ++tk) {
                if (tk < T) {
                    const float dt = lane_of(d, tk);
                    acc_wh[tk] = fmaf(dt, ek, acc_wh[tk]);
                    dsum = tk == 0 ? dt * whc[0] : fmaf(dt, whc[tk], dsum);
                }
            }
            const float demb = j < G ? dsum * ks : 0.f;
            acc_b2 = fmaf(demb, cnt, acc_b2);
            float de = 0.f;                              // d e_g[j] = sum_i W2[i][j] d emb_i
#pragma unroll
            for (int i = 0; i < 32; ++i) de = fmaf(W2s[i * WP + j], lane_of(demb, i), de);
            emol[g * HP + j] = de;
            emol_e[g * HP + j] = e;
            emol_d[g * HP + j] = demb;
        }
        __syncthreads();
        int tv = t;                                      // (opaque: the eight LDS addresses below are formed here, per chunk, instead of
        asm volatile("" : "+v"(tv));                     // living in registers -- spilled ones -- from the prologue on)
#pragma unroll
        for (int u = 0; u < 4; ++u) {                    // dW2[i][k] += sum over the chunk's molecules of d emb_g[i] e_g[k]
            const int i = (tv + NT * u) >> 5, k = (tv + NT * u) & 31;
            for (int g = 0; g < nm; ++g) accW2[u] = fmaf(emol_d[g * HP + i], emol_e[g * HP + k], accW2[u]);
        }
        // ---- P5: d pre = d e_g * swish'(pre)   (in place of pre; times the readout's keep, drawn again, with RD) -- two atoms of
        // a slot at a time: half the rows in flight
#pragma unroll
        for (int hf = 0; hf < AC / 64; ++hf) {
            f32x4 p[2], de[2];
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int at = as + 32 * (2 * hf + u), ac = at < A ? at : A - 1;        // (A == 0: row -1 of zp is W2s' last, inside LDS)
                p[u] = *(const f32x4*)(zp + ac * HP + 4 * l);
                de[u] = *(const f32x4*)(emol + (A > 0 ? amol[ac] : 0) * HP + 4 * l);
            }
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int at = as + 32 * (2 * hf + u);
                if (at < A) {
                    if constexpr (RD) {
                        float ks[4];
                        readout_keep4(seed, offset, (int64_t)a0 + at, H, l, a.rdrop_p, ks);
#pragma unroll
                        for (int c = 0; c < 4; ++c) de[u][c] *= ks[c];
                    }
                    f32x4 dp;
#pragma unroll
                    for (int c = 0; c < 4; ++c) { const float sg = sigmoidf_(p[u][c]); dp[c] = de[u][c] * (sg * (1.f + p[u][c] * (1.f - sg))); }
                    *(f32x4*)(zp + at * HP + 4 * l) = dp;
                    acc_b1 += dp;
                }
            }
            asm volatile("" ::: "memory");
        }
        __syncthreads();
        // ---- P6: d z = sum of d pre over the out-edges, straight to memory
        {
            f32x4 v[AC / 32];
            gather_halves(rpout, ecout, zp, as, A, l, v);
#pragma unroll
            for (int u = 0; u < AC / 32; ++u) {
                const int at = as + 32 * u;
                if (at < A) *(f32x4*)(a.dz + (int64_t)(a0 + at) * 32 + 4 * l) = v[u];
            }
        }
        // (a barrier that does not wait for the d z stores: see tail_middle_kernel)
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    }
    __syncthreads();

    // ---- the workgroup's slab: everything summed over the eight row slots in slot order
    float* const so = a.slab + (size_t)blockIdx.x * a.slab_stride;
#pragma unroll
    for (int u = 0; u < 4; ++u) so[TAILL_W2 + t + NT * u] = accW2[u];
    float* const red = zp;                               // [8 slots][32][4]: b2, bh of the per-molecule phase
    float* const redb = dzb;                             // [32 atom slots][32]: b1 of the per-atom phases
    const float slot_loss = half_sum(acc_loss);          // (T = 1: lane 0's value plus exact zeros)
    red[(slot * 32 + j) * 4 + 1] = acc_b2;
    red[(slot * 32 + j) * 4 + 3] = acc_bh;               // (lanes from T on never added to it)
    *(f32x4*)(redb + as * 32 + 4 * l) = acc_b1;
    if (j == 0) vec[slot] = slot_loss;                   // (b1's copy is no longer needed)
    __syncthreads();
    if (t < 128) {
        const int r = t >> 2, c = t & 3;
        float v = 0.f;
        if (c == 0) {
#pragma unroll
            for (int s32 = 0; s32 < 32; ++s32) v += redb[s32 * 32 + r];
            so[TAILL_B1 + r] = v;
        } else if (c != 2) {
#pragma unroll
            for (int s8 = 0; s8 < 8; ++s8) v += red[(s8 * 32 + r) * 4 + c];
            if (c == 1) so[TAILL_B2 + r] = v;
            else so[TAILL_BH + r] = v;
        }
    }
    if (t == 0) {
        float v = 0.f;
        for (int s8 = 0; s8 < 8; ++s8) v += vec[s8];
        so[TAILL_LOSS] = v;                              // (already divided by the labelled-entry count for the mean kinds)
    }
    __syncthreads();
    float* const redw = zp;                              // [8 slots][T][32]: d W_head, over both atom-row images
#pragma unroll
    for (int tk = 0; tk < TB; ++tk) if (tk < T) redw[(slot * T + tk) * 32 + j] = acc_wh[tk];
    __syncthreads();
    for (int q = t; q < T * 32; q += NT) {
        float v = 0.f;
#pragma unroll
        for (int s8 = 0; s8 < 8; ++s8) v += redw[s8 * T * 32 + q];
        so[TAILL_WH + q] = v;
    }
}

}  // namespace tail

int tail_label_count_blocks(int64_t n_loss_mols, int T) {
    const int64_t nb = (n_loss_mols * T + 1023) / 1024;   // (four entries a thread, at most one wave of partials for the prologue)
    return (int)(nb < 1 ? 1 : (nb > TAIL_LABEL_MAX_COUNTS ? TAIL_LABEL_MAX_COUNTS : nb));
}

// TB: the task bound of the register arrays (the head matrix's column and the d W_head partials, 2 TB VGPRs): up to 16 tasks the
// kernel stays inside the 168 VGPRs of three workgroups per CU; beyond, it is bounded for two
template <bool RD, int TB>
static hipError_t launch_tail_labels_rd(const TailLabelArgs& a, int nb, int loss_kind, hipStream_t st) {
    switch (loss_kind) {
    case MKGNN_LOSS_BCE_MEAN: tail::tail_labels_middle_kernel<MKGNN_LOSS_BCE_MEAN, RD, TB><<<nb, tail::NT, 0, st>>>(a); break;
    case MKGNN_LOSS_SQERR_MEAN: tail::tail_labels_middle_kernel<MKGNN_LOSS_SQERR_MEAN, RD, TB><<<nb, tail::NT, 0, st>>>(a); break;
    case MKGNN_LOSS_SQERR_SUM: tail::tail_labels_middle_kernel<MKGNN_LOSS_SQERR_SUM, RD, TB><<<nb, tail::NT, 0, st>>>(a); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}
template <int TB>
static hipError_t launch_tail_labels_tb(const TailLabelArgs& a, int nb, int loss_kind, hipStream_t st) {
    return a.m.rdrop_p > 0.f ? launch_tail_labels_rd<true, TB>(a, nb, loss_kind, st) : launch_tail_labels_rd<false, TB>(a, nb, loss_kind, st);
}

hipError_t launch_tail_labels_middle(const TailLabelArgs& a, int nb, int loss_kind, hipStream_t st) {
    const TailMidArgs& m = a.m;
    if (m.mg < tail::MG_MIN || m.mg > tail::MG_MAX || m.mg > tail::MC) return hipErrorInvalidValue;
    if (m.rdrop_p > 0.f && !m.rng) return hipErrorInvalidValue;
    if (a.T < 1 || a.T > tail::TMAX || !a.counts || !a.pred || (a.labels == nullptr) == (a.task == nullptr)) return hipErrorInvalidValue;
    if (m.pw && loss_kind != MKGNN_LOSS_BCE_MEAN) return hipErrorInvalidValue;
    if (a.n_counts != tail_label_count_blocks(m.n_loss, a.T)) return hipErrorInvalidValue;
    tail::tail_label_count_kernel<<<a.n_counts, 256, 0, st>>>(a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (a.T <= tail::TB3) return launch_tail_labels_tb<tail::TB3>(a, nb, loss_kind, st);
    return launch_tail_labels_tb<32>(a, nb, loss_kind, st);
}

}  // namespace mkgnn
