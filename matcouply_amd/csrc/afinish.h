// The A-phase finish of the AO-ADMM engine (gfx950): per slab the fp64 system Q_i + (rho n + l2) I, its register
// Gauss-Jordan inverse, the fused inner ADMM loop on the row a_i, the terms of the fast reconstruction-error formula and the
// systems of the next B-phase - in a column-per-lane layout (k_A_finish) and a row-split one (k_A_finish_rows*).
//
// Included by admm.hip, whose code object these kernels share: as a translation unit of its own (a separate code object) the
// file cost config 2 a further 0.25 % (profiles/finish_refactor.txt, section 6).
//
// Reference sites: A1/A3-A6 (decomposition.py:138,155-213), E1 (:445-452), B1/B3-B5 (:240-256).
#pragma once
#include <string>
#include <type_traits>

#include "mcl_internal.h"
#include "gj_inverse.h"

// What the A-phase finish absorbs from its predecessor on the sweep path: Mpart != nullptr - the sweep left
// M_bseg = X_bseg^T B_bseg per bseg (C-fragment order) and the wave forms rhs_i = sum_bsegs coldot(M_bseg, C) itself
// (decomposition.py:147-152): one launch (k_A_rhs_from_M) and its boundary less per outer iteration.
// (Measured and NOT kept: letting the last workgroup to finish also reduce the diagnostics tables - the 256-way ticket
// fan-in on one counter plus the epilogue cost 9 us, the k_diag_final launch it replaced 4.8 us.)
struct AFuse {
    const float *Mpart, *Cfrag;
    int MS, NBm;
    // the C-phase finish over several workgroups (k_C_finish_multi) leaves C^T C as ctc_parts partial 16 x 16 fp64 blocks:
    // the finish sums them (fixed order) and slab 0 writes the totals out for everybody else
    int ctc_parts;
    const double *CtCpart;
    double *CtC64_out;
    float *CtC_out;
    double *LinvB64;  // fp64 copy of the next B-phase's inverses (fp64 row passes of PARAFAC2 stacks: mcl_rows64), or NULL
    double *LinvA64, *rhsA64, *Q64;  // fp64 systems / right-hand sides / cross products of a host- or wide-driven inner loop (fused_inner = 0), or NULL
    int wide_inner;            // small problems (exact-products mode): the inner loop keeps the row and its ADMM variables in fp64
};

// The argument list of the three finish kernels and of the row-split slab function, written once (AF_PARAMS) with the list of
// its names for handing it on (AF_ARGS).  The kernels take separate kernel arguments, not one by-value struct: of a struct
// the compiler loads every field up front and keeps it live (SGPR spills through VGPR lanes, 1.3 % of a config-2 iteration),
// separate arguments are re-loaded from the kernarg segment where they are used.
//   BtB [I, r, r] out: Q_i = BtB_i o CtC (the `cross_products` by-product); constant: rho_max[1] instead of the slab's own rho;
//   the per-slab Gram and right-hand side arrive as fp64 per-segment partials (seg_btb / seg_rhs; slab_seg_ptr == nullptr:
//   one entry per slab) and stay fp64 through Q_i, the system and the solve: only the stored by-products are rounded;
//   fused_inner == 0: only Q_i, rho_i and L_i^-1 are produced (the generic inner loop follows);
//   next_B: also build and invert the next B-phase's systems (l2_B, n_regs_B -> rhoB, LinvB); rhsA_out: the `rhses` by-product.
#define AF_PARAMS                                                                                                        \
    float *__restrict__ BtB, const double *__restrict__ CtC, int I, int r, float scale, float l2, int constant,          \
        const float *__restrict__ rho_max, float *__restrict__ rhoA, float *__restrict__ LinvA, float *__restrict__ A,   \
        RegSet regs, int inner, int fused_inner, double *__restrict__ e1, double *__restrict__ diag_row, int next_B,     \
        float l2_B, int n_regs_B, float *__restrict__ rhoB, float *__restrict__ LinvB,                                   \
        const int *__restrict__ slab_seg_ptr, const double *__restrict__ seg_rhs, const double *__restrict__ seg_btb,    \
        float *__restrict__ rhsA_out, AFuse F
#define AF_ARGS                                                                                                          \
    BtB, CtC, I, r, scale, l2, constant, rho_max, rhoA, LinvA, A, regs, inner, fused_inner, e1, diag_row, next_B, l2_B,  \
        n_regs_B, rhoB, LinvB, slab_seg_ptr, seg_rhs, seg_btb, rhsA_out, F

// =========================================================================================================
// the parts of the finish as functions: the column kernel k_A_finish is assembled from them, k_A_e1 uses the statistics.
// How a lane gets f_c = sum_d t_d M[d][c] for its column c (MatVec) and how the per-column terms are summed over the
// slab (Red) are passed in.  (The row-split kernels further down keep the text they had: see the note there.)
// =========================================================================================================
// one column per lane: t_d by v_readlane, the whole sum in the lane
template <int RP>
struct ColMatVec {
    const double (&col)[RP];
    int r;
    __device__ __forceinline__ double operator()(double t) const {
        double acc = 0.0;
#pragma unroll
        for (int d = 0; d < RP; ++d) {
            if (d < r) acc = fma(readlane_f64_u(t, d), col[d], acc);
        }
        return acc;
    }
};

struct WaveSum {
    __device__ __forceinline__ double operator()(double v) const { return wave_sum(v); }
};

// The inner loop is branch-free: absent penalties (and the lanes without a column) are masked out of the sum.
static __device__ __forceinline__ void a_prox_setup(const RegSet &regs, bool act, float rho, float (&z)[MCL_MAX_REGS],
                                                    float (&u)[MCL_MAX_REGS], float (&on)[MCL_MAX_REGS],
                                                    ProxClamp (&prox)[MCL_MAX_REGS]) {
    const int n = regs.n;
#pragma unroll
    for (int k = 0; k < MCL_MAX_REGS; ++k) {
        if (!(k < n && act)) z[k] = u[k] = 0.f;
        on[k] = (k < n) ? 1.f : 0.f;
        if (k < n) prox[k].set(regs.kind[k], regs.nonneg[k], regs.p0[k], regs.p1[k], regs.p0[k] / rho);
        else prox[k].set(0, 0, 0.f, 0.f, 0.f);
    }
}

// n_it inner iterations on the row (decomposition.py:188-213): t = rhs + rho sum_k (z_k - u_k), a = t L^-1 (fp64 product,
// rounded), z_k = prox_k(a + u_k), u_k = a - (z_k - u_k)
template <class MatVec>
static __device__ __forceinline__ void a_inner_f32(int n, int n_it, float rho, double rhs, const float (&on)[MCL_MAX_REGS],
                                                   const ProxClamp (&prox)[MCL_MAX_REGS], float &a, float (&z)[MCL_MAX_REGS],
                                                   float (&u)[MCL_MAX_REGS], const MatVec &mv) {
    for (int it = 0; it < n_it; ++it) {
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < MCL_MAX_REGS; ++k) s = fmaf(on[k], z[k] - u[k], s);  // = s + (z - u) exactly when on
        const double t = (n > 0) ? fma((double)rho, (double)s, rhs) : rhs;
        a = (float)mv(t);
#pragma unroll
        for (int k = 0; k < MCL_MAX_REGS; ++k) {
            const float y = a + u[k];
            const float zn = prox[k](y);
            u[k] = a - (zn - u[k]);
            z[k] = zn;
        }
    }
}

// the same for small problems (exact-products mode): the row, its auxiliary and dual variables in fp64, rounded once
template <class MatVec>
static __device__ __forceinline__ void a_inner_f64(const RegSet &regs, bool act, int n_it, float rho, double rhs, float &a,
                                                   float (&z)[MCL_MAX_REGS], float (&u)[MCL_MAX_REGS], const MatVec &mv) {
    const int n = regs.n;
    double zd[MCL_MAX_REGS], ud[MCL_MAX_REGS], ad = (double)a;
    ProxClampD pd[MCL_MAX_REGS];
#pragma unroll
    for (int k = 0; k < MCL_MAX_REGS; ++k) {
        zd[k] = (double)z[k], ud[k] = (double)u[k];
        if (k < n) pd[k].set(regs.kind[k], regs.nonneg[k], regs.p0d[k], regs.p1d[k], regs.p0d[k] / (double)rho);
        else pd[k].set(0, 0, 0.0, 0.0, 0.0);
    }
    for (int it = 0; it < n_it; ++it) {
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < MCL_MAX_REGS; ++k)
            if (k < n) s += zd[k] - ud[k];
        const double t = (n > 0) ? fma((double)rho, s, rhs) : rhs;
        ad = mv(t);
        if (!act) ad = 0.0;
#pragma unroll
        for (int k = 0; k < MCL_MAX_REGS; ++k) {
            const double zn = pd[k](ad + ud[k]);
            ud[k] = ad - (zn - ud[k]);
            zd[k] = zn;
        }
    }
    a = (float)ad;
#pragma unroll
    for (int k = 0; k < MCL_MAX_REGS; ++k) z[k] = (float)zd[k], u[k] = (float)ud[k];
}

// the fused inner loop of one slab: a, z, u hold the loaded row on entry and the new one on return (0 in lanes without a column)
template <class MatVec>
static __device__ __forceinline__ void a_inner_loop(const RegSet &regs, int inner, int wide_inner, bool act, float rho,
                                                    double rhs, float &a, float (&z)[MCL_MAX_REGS], float (&u)[MCL_MAX_REGS],
                                                    const MatVec &mv) {
    float on[MCL_MAX_REGS];
    ProxClamp prox[MCL_MAX_REGS];
    a_prox_setup(regs, act, rho, z, u, on, prox);
    if (!act) a = 0.f;
    const int n = regs.n;
    const int n_it = (n == 0 && inner > 1) ? 1 : inner;  // without penalties every inner solve is identical
    if (wide_inner) a_inner_f64(regs, act, n_it, rho, rhs, a, z, u, mv);
    else a_inner_f32(n, n_it, rho, rhs, on, prox, a, z, u, mv);
    if (!act) a = 0.f;
}

// own: the lane stores column c of slab i
static __device__ __forceinline__ void a_store_row(float *__restrict__ A, const RegSet &regs, int r, int i, int c, bool own,
                                                   float a, const float (&z)[MCL_MAX_REGS], const float (&u)[MCL_MAX_REGS]) {
    if (own) {
        A[(long)i * r + c] = a;
#pragma unroll
        for (int k = 0; k < MCL_MAX_REGS; ++k) {
            if (k < regs.n) {
                regs.aux[k][(long)i * r + c] = z[k];
                regs.dual[k][(long)i * r + c] = u[k];
            }
        }
    }
}

// Slab i's terms of the fast reconstruction-error formula (decomposition.py:445-449): <X_i, M_i> = rhs_i . a_i and
// ||M_i||^2 = a_i^T Q_i a_i (qa: the lane's (Q_i a_i)_c), and its row of the mode-0 diagnostics.  own: the lane contributes
// column c; red sums over the slab's columns and leaves the total (at least) in lane 0, which stores.
template <class Red>
static __device__ __forceinline__ void a_stats_store(double *__restrict__ e1, double *__restrict__ diag_row, int i, int lane,
                                                     bool own, int n, double rhs, float a, double qa,
                                                     const float (&z)[MCL_MAX_REGS], const Red &red) {
    const double inner_i = red(own ? rhs * (double)a : 0.0);
    const double model_i = red(own ? (double)a * qa : 0.0);
    const double nf = red(own ? (double)a * (double)a : 0.0);
    const double na = red(own ? fabs((double)a) : 0.0);
    double gap[MCL_MAX_REGS];
#pragma unroll
    for (int k = 0; k < MCL_MAX_REGS; ++k) {
        const double dlt = (own && k < n) ? (double)z[k] - (double)a : 0.0;
        gap[k] = red(dlt * dlt);
    }
    if (lane == 0) {
        e1[2 * i] = inner_i;
        e1[2 * i + 1] = model_i;
        diag_row_store(diag_row + (long)i * DIAG_COLS, nf, na, gap);
    }
}

// The next B-phase's systems depend only on the a_i just computed and on CtC (unchanged until the next C-phase):
// L_i = CtC o a_i a_i^T + (rho_i n_B + l2_B) I (decomposition.py:243-256) - built and inverted in the finish.  trb: the
// lane's diagonal entry of CtC o a_i a_i^T (0 elsewhere); returns the shift of the diagonal, rb: rho_i.
static __device__ __forceinline__ double next_b_shift(double trb, float scale, int n_regs_B, float l2_B, float &rb) {
    trb = wave_sum(trb);
    rb = rho_of_trace(trb, scale);
    return (double)rb * n_regs_B + (double)l2_B;
}

// ---------------------------------------------------------------------------------------------------------
// A-phase finish, one wave per slab i (decomposition.py:155-219), everything in registers:
//   lane c owns column c of Q_i = BtB_i o CtC (stored back as cross_products) and of L_i = Q_i + (rho n + l2) I;
//   L_i^-1 by the register Gauss-Jordan; fused inner loop on the row a_i with row-separable penalties
//   (a_c = sum_d t_d L^-1[d][c], t_d fetched with v_readlane); per-slab terms of the fast reconstruction-error
//   formula (:445-449) and the mode-0 diagnostics.
// ---------------------------------------------------------------------------------------------------------
template <int RP>
__global__ __launch_bounds__(256) void k_A_finish(AF_PARAMS) {
    MCL_GATE(regs.gate);
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= I) return;
    const bool act = lane < r;
    const int c = act ? lane : 0;
    double qcol[RP];
    double col[RP];
    double tr = 0.0;
    int sg0 = i, sg1 = i + 1;
    if (slab_seg_ptr != nullptr) {
        sg0 = slab_seg_ptr[i];
        sg1 = slab_seg_ptr[i + 1];
    }
    // Every global load of the kernel is issued up front, unconditionally (clamped column, masked at use): the loads
    // of one stage are all in flight together instead of one dependent L2 round trip per matrix row.
    double ctc[RP], btbv[RP];
#pragma unroll
    for (int d = 0; d < RP; ++d) {
        const int dd = d < r ? d : r - 1;
        ctc[d] = CtC[dd * r + c];
        btbv[d] = 0.0;
    }
    double rhs_pre = 0.0;
    float z[MCL_MAX_REGS], u[MCL_MAX_REGS];
#pragma unroll
    for (int k = 0; k < MCL_MAX_REGS; ++k) {
        z[k] = u[k] = 0.f;
        if (k < regs.n) {
            z[k] = regs.aux[k][(long)i * r + c];
            u[k] = regs.dual[k][(long)i * r + c];
        }
    }
    float a = A[(long)i * r + c];
    for (int sg = sg0; sg < sg1; ++sg) {  // per-segment partial Grams / right-hand sides of this slab (fixed order)
        double v[RP];
#pragma unroll
        for (int d = 0; d < RP; ++d) v[d] = seg_btb[((long)sg * r + (d < r ? d : r - 1)) * r + c];
        const double rv = seg_rhs[(long)sg * r + c];
#pragma unroll
        for (int d = 0; d < RP; ++d) btbv[d] += v[d];
        rhs_pre += rv;
    }
#pragma unroll
    for (int d = 0; d < RP; ++d) {
        double q = 0.0;
        if (act && d < r) {
            q = btbv[d] * ctc[d];
            BtB[((long)i * r + d) * r + c] = (float)q;
        }
        qcol[d] = q;
        if (d == lane) tr = q;
    }
    tr = wave_sum(act ? tr : 0.0);
    float rho = rho_of_trace(tr, scale);
    if (constant) rho = rho_max[1];
    const double shift = (double)rho * regs.n + (double)l2;
#pragma unroll
    for (int d = 0; d < RP; ++d) {
        double v = (d == lane) ? 1.0 : 0.0;
        if (act && d < r) v = qcol[d] + (d == lane ? shift : 0.0);
        col[d] = v;
    }
    gj_inverse_reg<RP>(col, r, lane);
    if (lane == 0) rhoA[i] = rho;
    const double rhs = act ? rhs_pre : 0.0;
    if (act) rhsA_out[(long)i * r + c] = (float)rhs;
    if (!fused_inner) {
#pragma unroll
        for (int d = 0; d < RP; ++d)
            if (act && d < r) {
                LinvA[((long)i * r + d) * r + c] = (float)col[d];
                if (F.LinvA64 != nullptr) F.LinvA64[((long)i * r + d) * r + c] = col[d];
            }
        if (act && F.rhsA64 != nullptr) F.rhsA64[(long)i * r + c] = rhs;
#pragma unroll
        for (int d = 0; d < RP; ++d)
            if (act && d < r && F.Q64 != nullptr) F.Q64[((long)i * r + d) * r + c] = qcol[d];
        return;
    }
    a_inner_loop(regs, inner, F.wide_inner, act, rho, rhs, a, z, u, ColMatVec<RP>{col, r});
    a_store_row(A, regs, r, i, c, act, a, z, u);
    // (Q symmetric: column c of Q = row c)
    double qa = 0.0;
#pragma unroll
    for (int d = 0; d < RP; ++d) {
        if (d < r) {
            const float ad = readlane_f32(a, d);
            qa += qcol[d] * (double)ad;
        }
    }
    a_stats_store(e1, diag_row, i, lane, act, regs.n, rhs, a, qa, z, WaveSum{});
    if (next_B) {
        double trb = 0.0;
#pragma unroll
        for (int d = 0; d < RP; ++d) {
            const float ad = (d < r) ? readlane_f32(a, d) : 0.f;
            double v = (d == lane) ? 1.0 : 0.0;
            if (act && d < r) v = ctc[d] * (double)ad * (double)a;
            if (d == lane && act) trb = v;
            col[d] = v;
        }
        float rb;
        const double shiftb = next_b_shift(trb, scale, n_regs_B, l2_B, rb);
        if (act) {
#pragma unroll
            for (int d = 0; d < RP; ++d)
                if (d == lane) col[d] += shiftb;
        }
        gj_inverse_reg<RP>(col, r, lane);
#pragma unroll
        for (int d = 0; d < RP; ++d)
            if (act && d < r) LinvB[((long)i * r + d) * r + c] = (float)col[d];
        if (lane == 0) rhoB[i] = rb;
    }
}

// ---------------------------------------------------------------------------------------------------------
// k_A_finish with the rows of every system split over the lane groups of GJRows<RP> (all 64 lanes busy; the Gauss-Jordan
// sweeps, the matrix-vector products of the inner loop and of the error terms are ~4x shorter for rank 9..16).
// Lane l = g * RP + c: column c, rows d = g * RL + j.  Per-column quantities (rhs, a, aux, dual) are replicated in
// every group; group 0 stores them.  Same arithmetic as k_A_finish up to the association of the fp64 sums over d.
// ---------------------------------------------------------------------------------------------------------
// The row-split kernels keep their own copy of the inner loops, the statistics and the next-B build instead of the shared parts
// above: routed through those (force-inlined, the same expressions in the same order) their instruction streams came out
// 0.5 - 2 % longer with another register allocation, and config 2, whose iteration is 34 us, lost 0.7 %.
// sum of a value that is non-zero only in lanes [0, RP), RP <= 32: butterfly inside the 16-lane DPP row (quad_perm xor 1,
// xor 2, row_half_mirror, row_mirror), one cross-row step for RP = 32; every lane of the row(s) ends with the total
template <int RP>
static __device__ __forceinline__ double lead_sum(double v) {
    static_assert(RP <= 32, "lead lanes must fit two DPP rows");
    v += dpp_mov_f64<0xB1>(v);
    v += dpp_mov_f64<0x4E>(v);
    v += dpp_mov_f64<0x141>(v);
    v += dpp_mov_f64<0x140>(v);
    if (RP > 16) v += __shfl_xor(v, 16);
    return v;
}

// sum_k M[k][c] C[k][c] over the bsegs sgA, sgA + step, ... < sgB, both operands in C-fragment order (element
// ((chunk * NB + nb) * 64 + l) * 4 + m <-> k = 16 chunk + 4 (l >> 4) + m, column 16 nb + (l & 15)): the wave streams
// M_bseg with 1 KB loads, fp64 accumulation (products of fp32 values are exact), the four lane quarters of a column are
// summed by two butterfly steps: every lane ends with the sums of columns (l & 15) and 16 + (l & 15) in acc0 / acc1.
template <int NQ>  // chunks of 256 floats per trip: 16 (partial images of K >= 256: MS is a multiple of 4096) or 8 (K <= 128: MS = 2048)
static __device__ __forceinline__ void m_coldot_q(const AFuse &F, int sgA, int sgB, int step, int lane, double (&pa)[2][2]) {
    for (int sg = sgA; sg < sgB; sg += step) {
        const float *mp = F.Mpart + (long)sg * F.MS;
        for (int e0 = 0; e0 < F.MS; e0 += 256 * NQ) {  // 2 NQ loads in flight
            f32x4 mv[NQ], cv[NQ];
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                mv[q] = *reinterpret_cast<const f32x4 *>(mp + e0 + 256 * q + 4 * lane);
                cv[q] = *reinterpret_cast<const f32x4 *>(F.Cfrag + e0 + 256 * q + 4 * lane);
            }
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                double d = (double)mv[q][0] * (double)cv[q][0];
                d = fma((double)mv[q][1], (double)cv[q][1], d);
                d = fma((double)mv[q][2], (double)cv[q][2], d);
                d = fma((double)mv[q][3], (double)cv[q][3], d);
                // chunk index = e >> 8 = NQ * trip + q: nb = chunk % NB
                if (F.NBm == 2 && (q & 1)) pa[1][(q >> 1) & 1] += d;
                else pa[0][(q >> (F.NBm == 2 ? 1 : 0)) & 1] += d;
            }
        }
    }
}

static __device__ __forceinline__ void m_coldot(const AFuse &F, int sgA, int sgB, int step, int lane, double &acc0,
                                                double &acc1) {
    double pa[2][2] = {{0.0, 0.0}, {0.0, 0.0}};  // [nb][chain]: two chains per column block shorten the FMA dependency
    if ((F.MS & 4095) == 0) m_coldot_q<16>(F, sgA, sgB, step, lane, pa);
    else m_coldot_q<8>(F, sgA, sgB, step, lane, pa);
    acc0 = pa[0][0] + pa[0][1], acc1 = pa[1][0] + pa[1][1];
    acc0 += __shfl_xor(acc0, 16), acc1 += __shfl_xor(acc1, 16);
    acc0 += __shfl_xor(acc0, 32), acc1 += __shfl_xor(acc1, 32);
}

// one wave = one slab
template <int RP>
static __device__ __forceinline__ void a_finish_rows_slab(const int i, const int lane, float *__restrict__ BtB,
                                                          const double *__restrict__ CtC, int r, float scale, float l2,
                                                          int constant, const float *__restrict__ rho_max,
                                                          float *__restrict__ rhoA, float *__restrict__ LinvA,
                                                          float *__restrict__ A, const RegSet &regs, int inner,
                                                          int fused_inner, double *__restrict__ e1,
                                                          double *__restrict__ diag_row, int next_B, float l2_B,
                                                          int n_regs_B, float *__restrict__ rhoB,
                                                          float *__restrict__ LinvB, const int *__restrict__ slab_seg_ptr,
                                                          const double *__restrict__ seg_rhs,
                                                          const double *__restrict__ seg_btb,
                                                          float *__restrict__ rhsA_out, const AFuse &F,
                                                          const double *rhs_lds = nullptr) {
    constexpr int RL = GJRows<RP>::RL, G = GJRows<RP>::G;
    const int cc = lane % RP, g = lane / RP;
    const bool in_range = lane < GJRows<RP>::LANES;  // RP = 4 uses 16 lanes only
    const bool act = in_range && cc < r;
    const bool lead = act && g == 0;                 // the lanes that own the per-column results
    const int c = act ? cc : 0;
    int drow[RL];
    bool dok[RL];
#pragma unroll
    for (int j = 0; j < RL; ++j) {
        const int d = (in_range ? g : 0) * RL + j;
        dok[j] = act && d < r;
        drow[j] = d < r ? d : r - 1;  // clamped: every load is unconditional
    }
    int sg0 = i, sg1 = i + 1;
    if (slab_seg_ptr != nullptr) {
        sg0 = slab_seg_ptr[i];
        sg1 = slab_seg_ptr[i + 1];
    }
    // all global loads up front
    double ctc[RL], btbv[RL];
    if (F.ctc_parts > 0) {
        for (int pb = 0; pb < F.ctc_parts; pb += 4) {  // four partial blocks per trip: independent clamped loads, added in order
            double v[4][RL];
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int j = 0; j < RL; ++j) v[u][j] = F.CtCpart[(long)min(pb + u, F.ctc_parts - 1) * 256 + drow[j] * 16 + c];
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (pb + u < F.ctc_parts) {
#pragma unroll
                    for (int j = 0; j < RL; ++j) ctc[j] = (pb + u == 0) ? v[u][j] : ctc[j] + v[u][j];
                }
        }
        if (i == 0) {
#pragma unroll
            for (int j = 0; j < RL; ++j)
                if (dok[j]) {
                    F.CtC64_out[drow[j] * r + c] = ctc[j];
                    F.CtC_out[drow[j] * r + c] = (float)ctc[j];
                }
        }
#pragma unroll
        for (int j = 0; j < RL; ++j) btbv[j] = 0.0;
    } else {
#pragma unroll
        for (int j = 0; j < RL; ++j) {
            ctc[j] = CtC[drow[j] * r + c];
            btbv[j] = 0.0;
        }
    }
    double rhs_pre = 0.0;
    float z[MCL_MAX_REGS], u[MCL_MAX_REGS], on[MCL_MAX_REGS];
    ProxClamp prox[MCL_MAX_REGS];
    const int n = regs.n;
#pragma unroll
    for (int k = 0; k < MCL_MAX_REGS; ++k) {
        z[k] = u[k] = 0.f;
        if (k < n) {
            z[k] = regs.aux[k][(long)i * r + c];
            u[k] = regs.dual[k][(long)i * r + c];
        }
    }
    float a = A[(long)i * r + c];
    {  // fp64 per-segment partial Grams / right-hand sides of this slab, fixed order
        constexpr int SGB = 4;  // segments fetched per batch: independent clamped loads, summed in segment order
        for (int sb = sg0; sb < sg1; sb += SGB) {
            double v[SGB][RL], rv[SGB];
#pragma unroll
            for (int q = 0; q < SGB; ++q) {
                const long sg = min(sb + q, sg1 - 1);
#pragma unroll
                for (int j = 0; j < RL; ++j) v[q][j] = seg_btb[(sg * r + drow[j]) * r + c];
                rv[q] = (F.Mpart == nullptr) ? seg_rhs[sg * r + c] : 0.0;
            }
#pragma unroll
            for (int q = 0; q < SGB; ++q)
                if (sb + q < sg1) {
#pragma unroll
                    for (int j = 0; j < RL; ++j) btbv[j] += v[q][j];
                    rhs_pre += rv[q];
                }
        }
    }
    if (rhs_lds != nullptr) {
        // k_A_finish_rows_wide: the slab's other wave(s) stream its partials of M while this wave builds and inverts the
        // system; their column sums are picked up behind the workgroup barrier after the Gauss-Jordan
    } else if (F.Mpart != nullptr) {
        // rhs_i[c] = sum_k M_i[k][c] C[k][c] over the slab's bsegs; the column's sum is fetched into the lanes that own it
        double acc0, acc1;
        m_coldot(F, sg0, sg1, 1, lane, acc0, acc1);
        const double v0 = bperm_f64(cc & 15, acc0), v1 = bperm_f64(cc & 15, acc1);
        rhs_pre = (cc < 16) ? v0 : v1;
    }
    double qf[RL];
    double tr = 0.0;
#pragma unroll
    for (int j = 0; j < RL; ++j) {
        double q = 0.0;
        if (dok[j]) {
            q = btbv[j] * ctc[j];
            BtB[((long)i * r + drow[j]) * r + c] = (float)q;
            if (drow[j] == c) tr = q;
        }
        qf[j] = q;
    }
    tr = wave_sum(tr);
    float rho = rho_of_trace(tr, scale);
    if (constant) rho = rho_max[1];
    const double shift = (double)rho * n + (double)l2;
    double col[RL];
#pragma unroll
    for (int j = 0; j < RL; ++j) {
        const int d = g * RL + j;
        double v = (d == cc) ? 1.0 : 0.0;  // identity padding (also for the idle lanes of RP = 4)
        if (dok[j]) v = qf[j] + (d == cc ? shift : 0.0);
        col[j] = v;
    }
    gj_inverse_rows<RP>(col, r, in_range ? lane : cc);
    if (lane == 0) rhoA[i] = rho;
    if (rhs_lds != nullptr) {
        __syncthreads();
        rhs_pre = (rhs_lds[cc] + rhs_lds[32 + cc]) + rhs_lds[64 + cc];
    }
    const double rhs = act ? rhs_pre : 0.0;
    if (lead) rhsA_out[(long)i * r + c] = (float)rhs;  // the `rhses` by-product
    if (!fused_inner) {
#pragma unroll
        for (int j = 0; j < RL; ++j)
            if (dok[j]) {
                LinvA[((long)i * r + drow[j]) * r + c] = (float)col[j];
                if (F.LinvA64 != nullptr) F.LinvA64[((long)i * r + drow[j]) * r + c] = col[j];
            }
        if (lead && F.rhsA64 != nullptr) F.rhsA64[(long)i * r + c] = rhs;
#pragma unroll
        for (int j = 0; j < RL; ++j)
            if (dok[j] && F.Q64 != nullptr) F.Q64[((long)i * r + drow[j]) * r + c] = qf[j];
        return;
    }
#pragma unroll
    for (int k = 0; k < MCL_MAX_REGS; ++k) {
        if (!(k < n && act)) z[k] = u[k] = 0.f;
        on[k] = (k < n) ? 1.f : 0.f;
        if (k < n) prox[k].set(regs.kind[k], regs.nonneg[k], regs.p0[k], regs.p1[k], regs.p0[k] / rho);
        else prox[k].set(0, 0, 0.f, 0.f, 0.f);
    }
    if (!act) a = 0.f;
    // sum over the G row groups of one column: lanes c, RP + c, ... (fixed association)
    auto group_sum = [&](double v) -> double {
#pragma unroll
        for (int o = RP; o < 64 && o < RP * G; o <<= 1) v += __shfl_xor(v, o);
        return v;
    };
    const int n_it = (n == 0 && inner > 1) ? 1 : inner;
    if (F.wide_inner) {  // (see k_A_finish)
        double zd[MCL_MAX_REGS], ud[MCL_MAX_REGS], ad = (double)a;
        ProxClampD pd[MCL_MAX_REGS];
#pragma unroll
        for (int k = 0; k < MCL_MAX_REGS; ++k) {
            zd[k] = (double)z[k], ud[k] = (double)u[k];
            if (k < n) pd[k].set(regs.kind[k], regs.nonneg[k], regs.p0d[k], regs.p1d[k], regs.p0d[k] / (double)rho);
            else pd[k].set(0, 0, 0.0, 0.0, 0.0);
        }
        for (int it = 0; it < n_it; ++it) {
            double s = 0.0;
#pragma unroll
            for (int k = 0; k < MCL_MAX_REGS; ++k)
                if (k < n) s += zd[k] - ud[k];
            const double t = (n > 0) ? fma((double)rho, s, rhs) : rhs;
            double acc = 0.0;
#pragma unroll
            for (int j = 0; j < RL; ++j) {
                const double td = bperm_f64(g * RP + g * RL + j, t);
                if (g * RL + j < r) acc = fma(td, col[j], acc);
            }
            ad = group_sum(acc);  // (every lane takes part in the shuffles)
            if (!act) ad = 0.0;
#pragma unroll
            for (int k = 0; k < MCL_MAX_REGS; ++k) {
                const double zn = pd[k](ad + ud[k]);
                ud[k] = ad - (zn - ud[k]);
                zd[k] = zn;
            }
        }
        a = (float)ad;
#pragma unroll
        for (int k = 0; k < MCL_MAX_REGS; ++k) z[k] = (float)zd[k], u[k] = (float)ud[k];
    } else
    for (int it = 0; it < n_it; ++it) {
        float sacc = 0.f;
#pragma unroll
        for (int k = 0; k < MCL_MAX_REGS; ++k) sacc = fmaf(on[k], z[k] - u[k], sacc);  // = sacc + (z - u) exactly when on
        const double t = (n > 0) ? fma((double)rho, (double)sacc, rhs) : rhs;
        double acc = 0.0;
#pragma unroll
        for (int j = 0; j < RL; ++j) {
            const double td = bperm_f64(g * RP + g * RL + j, t);  // t_d, d = g RL + j (column d of my own group)
            if (g * RL + j < r) acc = fma(td, col[j], acc);
        }
        a = (float)group_sum(acc);
#pragma unroll
        for (int k = 0; k < MCL_MAX_REGS; ++k) {
            const float y = a + u[k];
            const float zn = prox[k](y);
            u[k] = a - (zn - u[k]);
            z[k] = zn;
        }
    }
    if (!act) a = 0.f;
    if (lead) {
        A[(long)i * r + c] = a;
#pragma unroll
        for (int k = 0; k < MCL_MAX_REGS; ++k) {
            if (k < n) {
                regs.aux[k][(long)i * r + c] = z[k];
                regs.dual[k][(long)i * r + c] = u[k];
            }
        }
    }
    // <X_i, M_i> = rhs_i . a_i ;  ||M_i||^2 = a_i^T Q_i a_i
    float ad[RL];
    double qa = 0.0;
#pragma unroll
    for (int j = 0; j < RL; ++j) {
        ad[j] = bperm_f32(g * RP + g * RL + j, a);  // a_d
        if (g * RL + j < r) qa += qf[j] * (double)ad[j];
    }
    qa = group_sum(qa);
    // the contributions live in the lead lanes [0, RP): DPP row reductions (no LDS round trips), result in lane 0
    const double inner_i = lead_sum<RP>(lead ? rhs * (double)a : 0.0);
    const double model_i = lead_sum<RP>(lead ? (double)a * qa : 0.0);
    const double nf = lead_sum<RP>(lead ? (double)a * (double)a : 0.0);
    const double na = lead_sum<RP>(lead ? fabs((double)a) : 0.0);
    double gap[MCL_MAX_REGS];
#pragma unroll
    for (int k = 0; k < MCL_MAX_REGS; ++k) {
        const double dlt = (lead && k < n) ? (double)z[k] - (double)a : 0.0;
        gap[k] = lead_sum<RP>(dlt * dlt);
    }
    if (lane == 0) {
        e1[2 * i] = inner_i;
        e1[2 * i + 1] = model_i;
        double *o = diag_row + (long)i * DIAG_COLS;
        o[0] = nf;
        o[1] = na;
#pragma unroll
        for (int k = 0; k < MCL_MAX_REGS; ++k) o[2 + k] = gap[k];
    }
    if (next_B) {
        // systems of the next B-phase: L_i = CtC o a_i a_i^T + (rho_i n_B + l2_B) I (decomposition.py:243-256)
        double trb = 0.0;
#pragma unroll
        for (int j = 0; j < RL; ++j) {
            const int d = g * RL + j;
            double v = (d == cc) ? 1.0 : 0.0;
            if (dok[j]) v = ctc[j] * (double)ad[j] * (double)a;
            if (dok[j] && d == cc) trb = v;
            col[j] = v;
        }
        trb = wave_sum(trb);
        const float rb = rho_of_trace(trb, scale);
        const double shiftb = (double)rb * n_regs_B + (double)l2_B;
#pragma unroll
        for (int j = 0; j < RL; ++j)
            if (dok[j] && g * RL + j == cc) col[j] += shiftb;
        gj_inverse_rows<RP>(col, r, in_range ? lane : cc);
#pragma unroll
        for (int j = 0; j < RL; ++j)
            if (dok[j]) {
                LinvB[((long)i * r + drow[j]) * r + c] = (float)col[j];
                if (F.LinvB64 != nullptr) F.LinvB64[((long)i * r + drow[j]) * r + c] = col[j];
            }
        if (lane == 0) rhoB[i] = rb;
    }
}

template <int RP>
__global__ __launch_bounds__(256) void k_A_finish_rows(AF_PARAMS) {
    MCL_GATE(regs.gate);
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= I) return;
    a_finish_rows_slab<RP>(i, lane, BtB, CtC, r, scale, l2, constant, rho_max, rhoA, LinvA, A, regs, inner, fused_inner, e1,
                           diag_row, next_B, l2_B, n_regs_B, rhoB, LinvB, slab_seg_ptr, seg_rhs, seg_btb, rhsA_out, F);
}

// One workgroup per slab: waves 1..3 stream the slab's partials of M (rhs_i = sum over partials of coldot(M_part, C)) WHILE
// wave 0 loads, builds and inverts the slab's system; one workgroup barrier behind the Gauss-Jordan hands the column sums
// over, then wave 0 finishes the slab as in k_A_finish_rows.  Used whenever the finish forms rhs_i itself (1..8 partials
// per slab): the M stream (16 KB per partial at K = 256, two 32-load trips) leaves the critical path of the iteration.
// SPB = 2 (more than 512 slabs, one partial per slab - config 3): two slabs per workgroup, one system wave and one streaming
// wave each, so that 1024 slabs still fit the device in one round (two workgroups per CU).
template <int RP, int SPB>
__global__ __launch_bounds__(256) void k_A_finish_rows_wide(AF_PARAMS) {
    MCL_GATE(regs.gate);
    __shared__ double part[SPB][3][32];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    constexpr int WPS = 4 / SPB;                  // waves per slab: one system wave + WPS - 1 streaming waves
    const int sl = wave / WPS, role = wave % WPS;  // role 0: the system wave
    const int i = blockIdx.x * SPB + sl;
    if (role != 0) {
        double a0 = 0.0, a1 = 0.0;
        if (i < I) m_coldot(F, slab_seg_ptr[i] + role - 1, slab_seg_ptr[i + 1], WPS - 1, lane, a0, a1);
        if (lane < 16) {
            part[sl][role - 1][lane] = a0, part[sl][role - 1][16 + lane] = a1;
            if (SPB == 2) part[sl][1][lane] = part[sl][1][16 + lane] = part[sl][2][lane] = part[sl][2][16 + lane] = 0.0;
        }
        __syncthreads();  // pairs with the barrier of the system wave behind its Gauss-Jordan (a_finish_rows_slab)
        return;
    }
    if (i >= I) {  // the odd slab out of a two-slab workgroup
        __syncthreads();
        return;
    }
    a_finish_rows_slab<RP>(i, lane, BtB, CtC, r, scale, l2, constant, rho_max, rhoA, LinvA, A, regs, inner, fused_inner, e1,
                           diag_row, next_B, l2_B, n_regs_B, rhoB, LinvB, slab_seg_ptr, seg_rhs, seg_btb, rhsA_out, F,
                           &part[sl][0][0]);
}

// rho_i of the A-phase alone (needed before the systems when the feasibility penalty is constant)
__global__ void k_A_rho(const double *__restrict__ BtB, const double *__restrict__ CtC, int I, int r, float scale,
                        float *__restrict__ rhoA, float *__restrict__ rho_max) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= I) return;
    double s = 0.0;
    for (int c = 0; c < r; ++c) s += BtB[((long)i * r + c) * r + c] * CtC[c * r + c];
    const float rho = rho_of_trace(s, scale);
    rhoA[i] = rho;
    atomicMax(reinterpret_cast<int *>(rho_max + 1), __float_as_int(rho));
}

// e1 / row diagnostics of mode 0 from (rhsA, BtB or Q, A) - used when the A-phase inner loop was not fused
// or when the by-products are recomputed for an error evaluation without an A update (decomposition.py:430-444)
__global__ __launch_bounds__(64) void k_A_e1(const float *__restrict__ rhsA, const float *__restrict__ BtB,
                                             const float *__restrict__ CtC, int btb_is_q, const float *__restrict__ A,
                                             RegSet regs, int r, double *__restrict__ e1,
                                             double *__restrict__ diag_row, const double *__restrict__ rhs64,
                                             const double *__restrict__ Q64) {
    // rhs64 / Q64: the fp64 right-hand sides / cross products the systems were built from (exact-products mode): the fast
    // error formula ||X||^2 - 2 <X, M> + ||M||^2 cancels to rec^2, so the fp32 rounding of rhs_i and Q_i (6e-8) would reach
    // the reconstruction error multiplied by ||X||^2 / rec^2
    MCL_GATE(regs.gate);
    const int i = blockIdx.x, lane = threadIdx.x;
    const bool act = lane < r;
    const int c = act ? lane : 0;
    const float a = A[(long)i * r + c];
    double qa = 0.0;
    for (int d = 0; d < r; ++d) {
        double q = Q64 != nullptr ? Q64[((long)i * r + c) * r + d] : (double)BtB[((long)i * r + c) * r + d];
        if (!btb_is_q) q *= (double)CtC[c * r + d];
        qa += q * (double)A[(long)i * r + d];
    }
    const double rhs_c = rhs64 != nullptr ? rhs64[(long)i * r + c] : (double)rhsA[(long)i * r + c];
    float z[MCL_MAX_REGS];
#pragma unroll
    for (int k = 0; k < MCL_MAX_REGS; ++k) z[k] = (act && k < regs.n) ? regs.aux[k][(long)i * r + c] : 0.f;
    a_stats_store(e1, diag_row, i, lane, act, regs.n, rhs_c, a, qa, z, WaveSum{});
}

// =========================================================================================================
// host launchers
// =========================================================================================================
int mcl_launch_A_rho(mcl_context *c) {
    ProfScope prof_(c, MCL_PROF_OTHER);
    MCL_CHECK_HIP(c, hipMemsetAsync(c->rho_max + 1, 0, sizeof(float), c->stream));
    if (c->I == 0) return 0;
    hipLaunchKernelGGL(k_A_rho, dim3((unsigned)((c->I + 255) / 256)), dim3(256), 0, c->stream, c->seg_btb, c->CtC64,
                       (int)c->I, c->r, (float)c->opt.feasibility_penalty_scale, c->rhoA, c->rho_max);
    MCL_CHECK_HIP(c, hipGetLastError());
    return 0;
}

// f(integral_constant<RP>) for the context's padded rank, out of the listed instantiations; false: RP is not among them
template <int... RPs, class Fn>
static bool dispatch_rp(int RP, Fn &&f) {
    return ((RP == RPs ? (f(std::integral_constant<int, RPs>{}), true) : false) || ...);
}

int mcl_launch_A_finish(mcl_context *c, bool fuse_inner) {
    if (c->I == 0) return 0;
    const bool rows_kernel = mcl_a_finish_rows(c);
    // (a B-phase with fp64 row passes also needs the fp64 inverses: only the row-split kernels write them)
    const bool b_needs_64 = mcl_rows64(c) || c->exact;  // the B-phase reads the fp64 inverses (fp64 row passes / wide.hip)
    const APlan &plan = c->a_plan;
    const bool seg = plan.use_seg_gram;
    // the kernels' arguments under the kernels' names (AF_PARAMS), handed over with AF_ARGS
    float *BtB = c->BtB, *rhoA = c->rhoA, *LinvA = c->LinvA, *A = c->A, *rhoB = c->rhoB, *LinvB = c->LinvB, *rhsA_out = c->rhsA;
    const double *CtC = c->CtC64, *seg_rhs = c->seg_rhs, *seg_btb = (seg && plan.seg_from_sweep) ? c->part_btb : c->seg_btb;
    const float *rho_max = c->rho_max;
    const int *slab_seg_ptr = seg ? (plan.seg_from_sweep ? c->slab_part_ptr : c->slab_seg_ptr) : nullptr;
    const int I = (int)c->I, r = c->r, constant = c->opt.constant_A, inner = c->opt.inner_n_iter_max, n_regs_B = c->regs[1].n;
    const int fused_inner = fuse_inner ? 1 : 0;
    const float scale = (float)c->opt.feasibility_penalty_scale, l2 = (float)c->opt.l2_penalty[0], l2_B = (float)c->opt.l2_penalty[1];
    const RegSet &regs = c->regs[0];
    double *e1 = c->e1, *diag_row = c->diagA_row;
    // also prepare the next B-phase's systems when that is exact: fused inner loop, per-slab rho for B
    const int next_B = (fuse_inner && !c->opt.constant_B && c->regs[1].n > 0 && !c->sw.no_next_b &&
                        (rows_kernel || !b_needs_64)) ? 1 : 0;
    // what the row-split kernel absorbs: rhs_i from the sweep's M_bseg
    AFuse F{};
    F.ctc_parts = c->bp.ctc_parts, F.CtCpart = c->CtCpart, F.CtC64_out = c->CtC64, F.CtC_out = c->CtC;
    if (plan.rhs_from_M) {
        F.Mpart = c->Mpart, F.Cfrag = c->CfragS, F.NBm = c->NB;
        F.MS = mcl_sweep_KC(c) * 64 * 16 * c->NB;
    }
    F.LinvB64 = b_needs_64 ? c->LinvB64 : nullptr;
    F.LinvA64 = c->LinvA64, F.rhsA64 = c->rhsA64, F.Q64 = c->Q64;  // (allocated in the exact-products mode only)
    F.wide_inner = (c->exact && !c->sw.no_wide) ? 1 : 0;
    if (!rows_kernel && c->bp.ctc_parts > 0)
        if (int rc = mcl_launch_ctc_fold(c)) return rc;
    const dim3 block(256), per_wave((unsigned)((c->I + 3) / 4)), per_pair((unsigned)((c->I + 1) / 2)), per_slab((unsigned)c->I);
    bool launched;
    // ranks 5..32: rows of every system split over the lane groups (all 64 lanes busy); 64 columns fill the wave anyway
    if (!rows_kernel) {
        launched = dispatch_rp<4, 8, 16, 32, 64>(c->RP, [&](auto rp) {
            hipLaunchKernelGGL((k_A_finish<decltype(rp)::value>), per_wave, block, 0, c->stream, AF_ARGS);
        });
    } else {
        launched = dispatch_rp<8, 16, 32>(c->RP, [&](auto rp) {
            constexpr int RP = decltype(rp)::value;
            if (plan.rhs_wide && plan.rhs_pairs)  // two slabs per workgroup (one partial per slab, many slabs)
                hipLaunchKernelGGL((k_A_finish_rows_wide<RP, 2>), per_pair, block, 0, c->stream, AF_ARGS);
            else if (plan.rhs_wide)
                hipLaunchKernelGGL((k_A_finish_rows_wide<RP, 1>), per_slab, block, 0, c->stream, AF_ARGS);
            else
                hipLaunchKernelGGL((k_A_finish_rows<RP>), per_wave, block, 0, c->stream, AF_ARGS);
        });
    }
    if (!launched) {
        c->err = "internal: no A-finish kernel for padded rank " + std::to_string(c->RP);
        return 1;
    }
    MCL_CHECK_HIP(c, hipGetLastError());
    if (!fuse_inner && c->Q64 != nullptr) c->bp.made(BP_A64);  // rhsA64 / Q64 / LinvA64 hold this phase's systems
    c->variant[MCL_PROF_A_FINISH] = !rows_kernel ? "k_A_finish" : (plan.rhs_wide ? (plan.rhs_pairs ? "k_A_finish_rows_wide<SPB=2>" : "k_A_finish_rows_wide<SPB=1>") : "k_A_finish_rows");
    c->bp.ctc_parts = 0;  // the rows kernels wrote the totals
    if (next_B != 0) c->bp.made(BP_B_SYSTEMS);
    return 0;
}

int mcl_launch_A_e1(mcl_context *c, bool btb_is_q) {
    ProfScope prof_(c, MCL_PROF_OTHER);
    if (c->I == 0) return 0;
    // (the fp64 copies exist in the exact-products mode and are current when the systems were just built from them)
    const bool wide = btb_is_q && c->exact && c->bp.has(BP_A64);
    hipLaunchKernelGGL(k_A_e1, dim3((unsigned)c->I), dim3(64), 0, c->stream, c->rhsA, c->BtB, c->CtC, btb_is_q ? 1 : 0,
                       c->A, c->regs[0], c->r, c->e1, c->diagA_row, wide ? (const double *)c->rhsA64 : nullptr,
                       wide ? (const double *)c->Q64 : nullptr);
    MCL_CHECK_HIP(c, hipGetLastError());
    return 0;
}
