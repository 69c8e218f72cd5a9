// cmf_aoadmm_multistart (decomposition.py): many random starts of ONE problem fitted at once, one workgroup per start.
//
// A start of the examples' size (150 .. 500 rows, K = 15 .. 20, rank 3 .. 4) leaves almost the whole device idle and spends its
// time on launches and host set-up.  Its phases need cross-workgroup synchronisation only because one problem is spread over
// many workgroups; here a start lives in ONE workgroup (256 threads = 4 wave64s), so the whole fit - every outer iteration, its
// B, C and A phases with their inner ADMM loops, the diagnostics and the stopping rule - runs inside one launch with nothing but
// workgroup barriers.  Starts are independent: blockIdx.x is the start, and a finished workgroup frees its CU for the next.
//
// Order per outer iteration (reference decomposition.py): B phase :222-292, C phase :295-344, A phase :120-219, feasibility
// gaps :351-417, reconstruction error from the A phase's by-products :445-449 (:430-444 when A is not updated), loss and the
// stopping rule of the outer loop :945-1053 - the rule of mcl_run / k_diag_verdict: the relative criterion against the last
// RECORDED loss, the absolute one on the newest, both only on feasible iterates and only when `tol` is set.
//
// Numerics: fp64 throughout; X is read in its stored type and converted exactly (xload.h: ld1), then widened.  The r x r systems
// are inverted by Cholesky in LDS (one thread per system, a batch of systems at a time), the PARAFAC2 polar factor of
// M_i = Y_i Delta^T is M_i (M_i^T M_i)^{-1/2} from a cyclic Jacobi eigen-decomposition of the r x r Gram in LDS (the rotation of
// symeig_lds.h, one thread per slab: the I Grams are independent, and one workgroup-wide solve per slab would cost ~60
// barriers each).  No atomics; every sum runs in a fixed order that depends only on the problem's shape, so a start's result
// is bitwise independent of how many starts share the launch and of which.
//
// Memory: X, row_ptr and the row -> slab map are shared.  Each start owns a slice of `state` (factors, aux, duals: the caller's
// layout, matcouply_hip.h) and a slice of the scratch workspace (right-hand sides, inverses, X C, ...), all fp64.  At the sizes
// this serves, the slices stay in L2 / MALL.
//
// cmf_aoadmm_resample (resampling.py): k_multistart_weighted is the same fit with a weight per matrix and
// job in the data term (mcl_multistart_run_weighted) - bootstrap, jackknife and K-fold jobs over the matrices share the one X.
//
// cmf_aoadmm_grid: the same launch with options of its own for every workgroup (mcl_multistart_run_grid).  The workgroup copies
// jobs[blockIdx.x] over the options of its LDS copy of the arguments, which is where every helper reads them; the jobs share X
// and one state layout (ms_check_grid), everything else - strengths, tolerances, iteration limits - is per job.
//
// cmf_aoadmm_missing (missing.py): k_multistart_missing is the same fit on data with missing entries, by
// expectation-maximisation.  Every job owns an fp64 copy X~ of X in the workspace (k_missing_copy_in: X where the job's mask
// says observed, the fill elsewhere), the phases read X~ through the fp64 loader of xload.h, and the diagnostics of every outer
// iteration are ONE pass over the job's entries that sums (X - M)^2 over the observed ones and stores the model M = B_i D_i C^T
// into the others (mcl_multistart_run_missing).
#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "entry_host.h"
#include "mcl_internal.h"
#include "wg_fp64.h"
#include "xload.h"

namespace {

static ErrorSlot g_ms_error;
constexpr int MS_MAX_RANK = 16;
constexpr int MS_SYS_BYTES = 40960;  // LDS for a batch of r x r systems (two r x r matrices per thread)

struct MsArgs {
    const void *X;
    const int64_t *row_ptr;
    const int32_t *slab_of_row;
    int64_t I, N, K;
    int64_t state_len, scratch_len, diag_stride;
    double *state, *scratch, *diag;
    int32_t *n_iter, *stop;
    int64_t off_aux[3][MCL_MAX_REGS], off_dual[3][MCL_MAX_REGS], off_delta[3][MCL_MAX_REGS];
    mcl_multistart_options o;
    const mcl_multistart_options *jobs;  // mcl_multistart_run_grid: options of workgroup s at jobs[s]; NULL: `o` for all
};
static_assert(sizeof(mcl_multistart_options) % sizeof(int32_t) == 0, "the options are copied to LDS word by word");

// scratch of one start, in doubles
struct MsScratch {
    int64_t rhsB, XC, RC, LinvB, rhoB, LinvA, rhoA, Q, rhsA, PF, colsq, small, total;
};

static __host__ __device__ inline MsScratch ms_scratch(int64_t I, int64_t N, int64_t K, int r) {
    MsScratch s{};
    int64_t o = 0;
    auto take = [&](int64_t n) { const int64_t at = o; o += (n + 31) & ~int64_t(31); return at; };
    s.rhsB = take(N * r);
    s.XC = take(N * r);
    s.RC = take(K * r);
    s.LinvB = take(I * r * r);
    s.rhoB = take(I);
    s.LinvA = take(I * r * r);
    s.rhoA = take(I);
    s.Q = take(I * r * r);
    s.rhsA = take(I * r);
    s.PF = take(I * r * r);
    s.colsq = take(I * r);
    s.small = take(8 * r * r + 64);
    s.total = o;
    return s;
}

// the prox of a row-separable kind on one value (oracle prox_elementwise; rho: the row's feasibility penalty)
static __device__ inline double prox_value(const mcl_multistart_penalty &p, double y, double rho) {
    if (p.kind == MCL_PEN_NN) return fmax(y, 0.0);
    if (p.kind == MCL_PEN_BOX) return fmin(fmax(y, p.p0), p.p1);
    if (p.kind == MCL_PEN_L1) {
        const double thr = p.p0 / rho;
        if (p.non_negativity) return fmax(y - thr, 0.0);
        const double m = fmax(fabs(y) - thr, 0.0);
        return y > 0.0 ? m : (y < 0.0 ? -m : 0.0);
    }
    return y;
}

// WEIGHTED: the job minimises the loss with the data term sum_i w_i |X_i - B_i D_i C^T|^2 / sum_i w_i |X_i|^2 (resampling over
// the matrices): every per-matrix Gram and right-hand side is multiplied by w_i, a matrix of weight 0 is
// not in the job (its rows of A, B and of every aux and dual are zeros on entry and stay exact zeros).  A weight multiplies ONE
// factor of a product and never a product that feeds an add, so that the contraction into fused multiply-adds is the
// unweighted kernel's and a weight of 1.0 changes no bit.  Without WEIGHTED `w` is never read.
//
// MISSING: X is the job's own fp64 copy X~ (XL = XF64), `obs` the job's mask [N, K] (1 = observed).  The phases are the
// complete-data ones on X~; impute_pass replaces model_terms.  Nothing computed from X~ lives from one outer iteration to the
// next: every phase rebuilds its right-hand side and X C from X~, and rhs_A / Q of the A phase feed nothing here.  Without
// MISSING `obs` and `fill_model` are never read.
template <int R, class XL, bool WEIGHTED, bool MISSING = false>
struct Start {
    const MsArgs &a;
    const typename XL::T *X;
    const int64_t *rp;
    const int32_t *slab;
    int64_t I, N, K;
    const double *w;  // WEIGHTED: the job's weight per slab [I]
    double *A, *B, *C, *ws;
    MsScratch sc;
    double *red, *sys, *sh;  // LDS: reduction scratch, system batch, small shared values
    int nb;                  // systems per batch
    const uint8_t *obs;      // MISSING: the job's mask [N, K], 1 = observed
    bool fill_model;         // MISSING: the missing entries of X~ start as the start's model (row 0 of the diagnostics stores it)

    __device__ int64_t rows_of(int m) const { return m == 0 ? I : (m == 1 ? N : K); }
    __device__ __forceinline__ double *F(int m) const { return m == 0 ? A : (m == 1 ? B : C); }
    __device__ __forceinline__ double *aux(int m, int k) const { return A + a.off_aux[m][k]; }
    __device__ __forceinline__ double *dual(int m, int k) const { return A + a.off_dual[m][k]; }
    __device__ __forceinline__ double *delta(int m, int k) const { return A + a.off_delta[m][k]; }
    __device__ __forceinline__ double x(int64_t j, int64_t c) const { return (double)XL::ld1(X + j * K + c); }
    // the weight of slab i (1 without WEIGHTED, folded away), and whether the slab is in the job
    __device__ __forceinline__ double wt(int64_t i) const {
        if constexpr (WEIGHTED) return w[i];
        return 1.0;
    }
    __device__ __forceinline__ bool in_job(int64_t i) const {
        if constexpr (WEIGHTED) return w[i] != 0.0;
        return true;
    }
    // the maximum of rho over the slabs of the job into every slab of the job (constant feasibility penalty); 0 outside it
    __device__ __forceinline__ void constant_rho(double *rho) {
        const int t = threadIdx.x;
        if (t == 0) {
            double mx = rho[0];
            if constexpr (WEIGHTED) {
                bool any = false;
                for (int64_t i = 0; i < I; ++i)
                    if (in_job(i)) mx = any ? fmax(mx, rho[i]) : rho[i], any = true;
            } else {
                for (int64_t i = 1; i < I; ++i) mx = fmax(mx, rho[i]);
            }
            sh[2 * R * R] = mx;
        }
        __syncthreads();
        const double mx = sh[2 * R * R];
        for (int64_t i = t; i < I; i += MS_THREADS) rho[i] = in_job(i) ? mx : 0.0;
        __syncthreads();
    }

    // aux of penalty k of mode m as a packed matrix, element (j, l): P Delta for PARAFAC2 (Delta copied to sh_delta first)
    __device__ __forceinline__ double auxp(int m, int k, int64_t j, int l, const double *dl) const {
        if (a.o.regs[m][k].kind == MCL_PEN_PARAFAC2) {
            const double *P = aux(m, k) + j * R;
            double v = 0.0;
            for (int q = 0; q < R; ++q) v += P[q] * dl[q * R + l];
            return v;
        }
        return aux(m, k)[j * R + l];
    }

    // invert the systems of the n = I slabs: build(i, S) writes system i into S (one thread), the inverse goes to out + i R R
    template <class Build>
    __device__ __forceinline__ void invert_systems(int64_t n, double *out, Build build) {
        const int t = threadIdx.x;
        for (int64_t base = 0; base < n; base += nb) {
            const int64_t i = base + t;
            if (t < nb && i < n) {
                double *S = sys + t * 2 * R * R, *W = S + R * R;
                if (in_job(i)) {
                    build(i, S);
                    spd_inverse<R>(S, W);
                    for (int e = 0; e < R * R; ++e) out[i * R * R + e] = S[e];
                } else {  // not (0 + l2) I inverted: the slab's rows stay zeros
                    for (int e = 0; e < R * R; ++e) out[i * R * R + e] = 0.0;
                }
            }
        }
        __syncthreads();
    }

    // C^T C into cc (global scratch), rows_reduce order
    __device__ __forceinline__ void ctc(double *cc) {
        rows_reduce(R * R, K, cc, red, [&](int64_t c, int e) { return C[c * R + e / R] * C[c * R + e % R]; });
    }

    // ---- prox + dual update of penalty k of mode m; F is the new factor, rho_row(j) the row's penalty, rho_mat(seg) a matrix's
    __device__ __forceinline__ void prox_mode(int m, int k, const double *rho_rows_slab, double rho_scalar) {
        const mcl_multistart_penalty &p = a.o.regs[m][k];
        const int t = threadIdx.x;
        const int64_t rows = rows_of(m);
        double *Fm = F(m), *Z = aux(m, k), *U = dual(m, k);
        auto rho_of = [&](int64_t j) {
            if (m == 1) return rho_rows_slab[slab[j]];
            if (m == 0) return rho_rows_slab[j];
            return rho_scalar;
        };
        // a row of a slab outside the job keeps its zeros: no prox, no dual step (a Box with a positive lower bound would move it)
        auto live = [&](int64_t j) {
            if (m == 1) return in_job(slab[j]);
            if (m == 0) return in_job(j);
            return true;
        };
        if (p.kind == MCL_PEN_NN || p.kind == MCL_PEN_BOX || p.kind == MCL_PEN_L1) {
            for (int64_t e = t; e < rows * R; e += MS_THREADS) {
                const int64_t j = e / R;
                if (!live(j)) continue;
                const double f = Fm[e], u = U[e];
                const double z = prox_value(p, f + u, rho_of(j));
                Z[e] = z;
                U[e] = f - (z - u);
            }
            __syncthreads();
            return;
        }
        if (p.kind == MCL_PEN_L2BALL) {
            for (int64_t e = t; e < rows * R; e += MS_THREADS) {
                const double y = Fm[e] + U[e];
                Z[e] = p.non_negativity ? fmax(y, 0.0) : y;
            }
            __syncthreads();
            double *cs = ws + sc.colsq;
            if (m == 1) {  // column norms per matrix B_i
                for (int64_t e = t; e < I * R; e += MS_THREADS) {
                    const int64_t i = e / R;
                    const int l = (int)(e % R);
                    double s = 0.0;
                    for (int64_t j = rp[i]; j < rp[i + 1]; ++j) s += Z[j * R + l] * Z[j * R + l];
                    cs[e] = s;
                }
                __syncthreads();
            } else {
                rows_reduce(R, rows, cs, red, [&](int64_t j, int l) { return Z[j * R + l] * Z[j * R + l]; });
            }
            for (int64_t e = t; e < rows * R; e += MS_THREADS) {
                const int64_t j = e / R;
                const int l = (int)(e % R);
                if (!live(j)) continue;
                const double nrm = sqrt(m == 1 ? cs[slab[j] * R + l] : cs[l]);
                const double z = Z[e] * p.p0 / fmax(nrm, p.p0);
                Z[e] = z;
                U[e] = Fm[e] - (z - U[e]);
            }
            __syncthreads();
            return;
        }
        // PARAFAC2 (mode 1): P_i = polar(Y_i Delta^T), Delta <- sum_i rho_i P_i^T Y_i / sum_i rho_i, Y = B + U
        double *P = Z, *D = delta(m, k);
        double *dl = sh;  // Delta (old) in LDS
        for (int e = t; e < R * R; e += MS_THREADS) dl[e] = D[e];
        __syncthreads();
        double *PF = ws + sc.PF;
        // Gram of M_i = Y_i Delta^T per slab
        for (int64_t e = t; e < I * R * R; e += MS_THREADS) {
            const int64_t i = e / (R * R);
            const int ab = (int)(e % (R * R)), ra = ab / R, rb = ab % R;
            double s = 0.0;
            for (int64_t j = rp[i]; j < rp[i + 1]; ++j) {
                double ma = 0.0, mb = 0.0;
                #pragma unroll
                for (int l = 0; l < R; ++l) {
                    const double y = B[j * R + l] + U[j * R + l];
                    ma += y * dl[ra * R + l];
                    mb += y * dl[rb * R + l];
                }
                s += ma * mb;
            }
            PF[e] = s;
        }
        __syncthreads();
        for (int64_t base = 0; base < I; base += nb) {
            const int64_t i = base + t;
            if (t < nb && i < I) {
                double *S = sys + t * 2 * R * R, *W = S + R * R;
                for (int e = 0; e < R * R; ++e) S[e] = PF[i * R * R + e];
                gram_inv_sqrt<R>(S, W, 1e-13);
                for (int e = 0; e < R * R; ++e) PF[i * R * R + e] = S[e];
            }
        }
        __syncthreads();
        for (int64_t j = t; j < N; j += MS_THREADS) {  // P_j = (Y_j Delta^T) G_i^{-1/2}
            double mrow[R];
            #pragma unroll
            for (int q = 0; q < R; ++q) {
                double v = 0.0;
                for (int l = 0; l < R; ++l) v += (B[j * R + l] + U[j * R + l]) * dl[q * R + l];
                mrow[q] = v;
            }
            const double *G = PF + (int64_t)slab[j] * R * R;
            #pragma unroll 1
            for (int l = 0; l < R; ++l) {
                double v = 0.0;
                #pragma unroll
                for (int q = 0; q < R; ++q) v += mrow[q] * G[q * R + l];
                P[j * R + l] = v;
            }
        }
        __syncthreads();
        for (int64_t e = t; e < I * R * R; e += MS_THREADS) {  // rho_i P_i^T Y_i per slab
            const int64_t i = e / (R * R);
            const int ab = (int)(e % (R * R)), ra = ab / R, rb = ab % R;
            double s = 0.0;
            for (int64_t j = rp[i]; j < rp[i + 1]; ++j) s += P[j * R + ra] * (B[j * R + rb] + U[j * R + rb]);
            PF[e] = rho_rows_slab[i] * s;
        }
        __syncthreads();
        if (t < R * R) {
            double s = 0.0, rs = 0.0;
            for (int64_t i = 0; i < I; ++i) s += PF[i * R * R + t], rs += rho_rows_slab[i];
            D[t] = s / rs;
            dl[t] = s / rs;
        }
        __syncthreads();
        for (int64_t e = t; e < N * R; e += MS_THREADS) {
            const int64_t j = e / R;
            const int l = (int)(e % R);
            double v = 0.0;
            for (int q = 0; q < R; ++q) v += P[j * R + q] * dl[q * R + l];
            U[e] = B[e] - (v - U[e]);
        }
        __syncthreads();
    }

    // ||F_m||^2, ||aux_k - F_m||^2 per penalty and sum |F_m| (L1 values), in fixed order
    __device__ __forceinline__ void mode_stats(int m, double *nf, double *gap, double *abs_sum) {
        const int t = threadIdx.x;
        const int64_t n = rows_of(m) * R;
        const double *Fm = F(m);
        double v = 0.0, w = 0.0;
        for (int64_t e = t; e < n; e += MS_THREADS) v += Fm[e] * Fm[e], w += fabs(Fm[e]);
        *nf = wg_sum(v, red);
        *abs_sum = wg_sum(w, red);
#pragma unroll
        for (int k = 0; k < MCL_MAX_REGS; ++k) {
            if (k >= a.o.n_regs[m]) break;
            double *dl = sh + R * R;
            if (a.o.regs[m][k].kind == MCL_PEN_PARAFAC2) {
                for (int e = t; e < R * R; e += MS_THREADS) dl[e] = delta(m, k)[e];
                __syncthreads();
            }
            double g = 0.0;
            for (int64_t e = t; e < n; e += MS_THREADS) {
                const double d = auxp(m, k, e / R, (int)(e % R), dl) - Fm[e];
                g += d * d;
            }
            gap[k] = wg_sum(g, red);
        }
    }

    // inner_tol (decomposition.py:90-117): relative change <= tol and every gap of the mode < tol
    __device__ __forceinline__ bool inner_converged(int m, double diff_partial) {
        const double tol = a.o.inner_tol;
        const double diff = wg_sum(diff_partial, red);
        double nf, gp[MCL_MAX_REGS], as;
        mode_stats(m, &nf, gp, &as);
        if (sqrt(diff) > tol * sqrt(nf)) return false;
        double worst = -INFINITY;
#pragma unroll
        for (int k = 0; k < MCL_MAX_REGS; ++k)
            if (k < a.o.n_regs[m]) worst = fmax(worst, sqrt(gp[k]) / sqrt(nf));
        return a.o.n_regs[m] == 0 || worst < tol;
    }

    // ---- B phase ----------------------------------------------------------------------------------------------------------
    __device__ __forceinline__ void phase_B() {
        const int t = threadIdx.x;
        const int n = a.o.n_regs[1];
        double *cc = ws + sc.small, *rhs = ws + sc.rhsB, *Linv = ws + sc.LinvB, *rho = ws + sc.rhoB;
        ctc(cc);
        for (int64_t j = t; j < N; j += MS_THREADS) {  // rhs_i = w_i X_i (C * a_i)
            const double *ai = A + (int64_t)slab[j] * R;
            double acc[R];
            #pragma unroll
            for (int l = 0; l < R; ++l) acc[l] = 0.0;
            if (in_job(slab[j]))  // a slab outside the job: no pass over its X
                for (int64_t c = 0; c < K; ++c) {
                    const double xv = x(j, c);
                    #pragma unroll
                    for (int l = 0; l < R; ++l) acc[l] += xv * (C[c * R + l] * ai[l]);
                }
            #pragma unroll
            for (int l = 0; l < R; ++l) {
                if constexpr (WEIGHTED) acc[l] *= w[slab[j]];
                rhs[j * R + l] = acc[l];
            }
        }
        for (int64_t i = t; i < I; i += MS_THREADS) {
            double tr = 0.0;
            for (int l = 0; l < R; ++l) tr += cc[l * R + l] * A[i * R + l] * A[i * R + l];
            if constexpr (WEIGHTED) tr *= w[i];
            rho[i] = 0.5 * tr * a.o.feasibility_penalty_scale;
        }
        __syncthreads();
        if (a.o.constant_B) constant_rho(rho);
        invert_systems(I, Linv, [&](int64_t i, double *S) {
            const double *ai = A + i * R;
            const double shift = rho[i] * n + a.o.l2_penalty[1];
            for (int p = 0; p < R; ++p)
                for (int q = 0; q < R; ++q) {
                    double g = cc[p * R + q];
                    if constexpr (WEIGHTED) g *= w[i];
                    S[p * R + q] = g * ai[p] * ai[q] + (p == q ? shift : 0.0);
                }
        });
        for (int it = 0; it < a.o.inner_n_iter_max; ++it) {
            // Delta of every PARAFAC2 penalty into LDS for the right-hand side
            for (int k = 0; k < n; ++k)
                if (a.o.regs[1][k].kind == MCL_PEN_PARAFAC2)
                    for (int e = t; e < R * R; e += MS_THREADS) sh[3 * R * R + 8 + k * R * R + e] = delta(1, k)[e];
            __syncthreads();
            double diff = 0.0;
            for (int64_t j = t; j < N; j += MS_THREADS) {
                const int64_t i = slab[j];
                double T[R];
                #pragma unroll
                for (int l = 0; l < R; ++l) {
                    double s = 0.0;
                    for (int k = 0; k < n; ++k) s += auxp(1, k, j, l, sh + 3 * R * R + 8 + k * R * R) - dual(1, k)[j * R + l];
                    T[l] = n ? rho[i] * s + rhs[j * R + l] : rhs[j * R + l];
                }
                const double *L = Linv + i * R * R;
                #pragma unroll 1
                for (int l = 0; l < R; ++l) {
                    double v = 0.0;
                    #pragma unroll
                    for (int q = 0; q < R; ++q) v += T[q] * L[q * R + l];
                    const double d = v - B[j * R + l];
                    diff += d * d;
                    B[j * R + l] = v;
                }
            }
            __syncthreads();
            for (int k = 0; k < n; ++k) prox_mode(1, k, rho, 0.0);
            if (a.o.inner_tol > 0.0 && inner_converged(1, diff)) break;
        }
    }

    // ---- C phase ----------------------------------------------------------------------------------------------------------
    __device__ __forceinline__ void phase_C() {
        const int t = threadIdx.x;
        const int n = a.o.n_regs[2];
        double *G = ws + sc.small + R * R, *Linv = ws + sc.small + 2 * R * R, *RC = ws + sc.RC;
        auto ba = [&](int64_t j, int l) { return B[j * R + l] * A[(int64_t)slab[j] * R + l]; };
        auto wba = [&](int64_t j, int l) {  // w_i (B_i D_i)
            if constexpr (WEIGHTED) return w[slab[j]] * ba(j, l);
            else return ba(j, l);
        };
        // G = sum_i w_i D_i B_i^T B_i D_i, RC = sum_i w_i X_i^T B_i D_i (a slab outside the job: no pass over its X)
        rows_reduce(R * R, N, G, red, [&](int64_t j, int e) { return wba(j, e / R) * ba(j, e % R); });
        // (the product itself is returned, not 0.0 on another path: a select between the multiply and rows_reduce's add would
        // keep the two from being contracted as they are in the unweighted kernel)
        rows_reduce((int)(K * R), N, RC, red, [&](int64_t j, int e) {
            const double xv = in_job(slab[j]) ? x(j, e / R) : 0.0;
            return xv * wba(j, e % R);
        });
        double tr = 0.0;
        for (int l = 0; l < R; ++l) tr += G[l * R + l];
        const double rho = 0.5 * tr * a.o.feasibility_penalty_scale;
        if (t == 0) {
            double *S = sys, *W = sys + R * R;
            for (int e = 0; e < R * R; ++e) S[e] = G[e] + ((e / R == e % R) ? rho * n + a.o.l2_penalty[2] : 0.0);
            spd_inverse<R>(S, W);
            for (int e = 0; e < R * R; ++e) Linv[e] = S[e];
        }
        __syncthreads();
        for (int it = 0; it < a.o.inner_n_iter_max; ++it) {
            double diff = 0.0;
            for (int64_t c = t; c < K; c += MS_THREADS) {
                double T[R];
                #pragma unroll
                for (int l = 0; l < R; ++l) {
                    double s = 0.0;
                    for (int k = 0; k < n; ++k) s += aux(2, k)[c * R + l] - dual(2, k)[c * R + l];
                    T[l] = n ? s * rho + RC[c * R + l] : RC[c * R + l];
                }
                #pragma unroll 1
                for (int l = 0; l < R; ++l) {
                    double v = 0.0;
                    #pragma unroll
                    for (int q = 0; q < R; ++q) v += T[q] * Linv[q * R + l];
                    const double d = v - C[c * R + l];
                    diff += d * d;
                    C[c * R + l] = v;
                }
            }
            __syncthreads();
            for (int k = 0; k < n; ++k) prox_mode(2, k, nullptr, rho);
            if (a.o.inner_tol > 0.0 && inner_converged(2, diff)) break;
        }
    }

    // ---- A phase (leaves rhs_A and Q for the reconstruction error) ---------------------------------------------------------
    __device__ __forceinline__ void phase_A() {
        const int t = threadIdx.x;
        const int n = a.o.n_regs[0];
        double *cc = ws + sc.small, *XC = ws + sc.XC, *rhsA = ws + sc.rhsA, *Q = ws + sc.Q, *Linv = ws + sc.LinvA, *rho = ws + sc.rhoA;
        ctc(cc);
        x_times_C(XC);
        for (int64_t e = t; e < I * R; e += MS_THREADS) {
            const int64_t i = e / R;
            const int l = (int)(e % R);
            double s = 0.0;
            for (int64_t j = rp[i]; j < rp[i + 1]; ++j) s += B[j * R + l] * XC[j * R + l];
            if constexpr (WEIGHTED) s *= w[i];
            rhsA[e] = s;
        }
        for (int64_t e = t; e < I * R * R; e += MS_THREADS) {
            const int64_t i = e / (R * R);
            const int ab = (int)(e % (R * R)), p = ab / R, q = ab % R;
            double s = 0.0;
            for (int64_t j = rp[i]; j < rp[i + 1]; ++j) s += B[j * R + p] * B[j * R + q];
            if constexpr (WEIGHTED) s *= w[i];
            Q[e] = s * cc[ab];
        }
        __syncthreads();
        for (int64_t i = t; i < I; i += MS_THREADS) {
            double tr = 0.0;
            for (int l = 0; l < R; ++l) tr += Q[i * R * R + l * R + l];
            rho[i] = 0.5 * tr * a.o.feasibility_penalty_scale;
        }
        __syncthreads();
        if (a.o.constant_A) constant_rho(rho);
        invert_systems(I, Linv, [&](int64_t i, double *S) {
            const double shift = rho[i] * n + a.o.l2_penalty[0];
            for (int e = 0; e < R * R; ++e) S[e] = Q[i * R * R + e] + ((e / R == e % R) ? shift : 0.0);
        });
        for (int it = 0; it < a.o.inner_n_iter_max; ++it) {
            double diff = 0.0;
            for (int64_t i = t; i < I; i += MS_THREADS) {
                double T[R];
                #pragma unroll
                for (int l = 0; l < R; ++l) {
                    double s = 0.0;
                    for (int k = 0; k < n; ++k) s += aux(0, k)[i * R + l] - dual(0, k)[i * R + l];
                    T[l] = n ? rho[i] * s + rhsA[i * R + l] : rhsA[i * R + l];
                }
                const double *L = Linv + i * R * R;
                #pragma unroll 1
                for (int l = 0; l < R; ++l) {
                    double v = 0.0;
                    #pragma unroll
                    for (int q = 0; q < R; ++q) v += T[q] * L[q * R + l];
                    const double d = v - A[i * R + l];
                    diff += d * d;
                    A[i * R + l] = v;
                }
            }
            __syncthreads();
            for (int k = 0; k < n; ++k) prox_mode(0, k, rho, 0.0);
            if (a.o.inner_tol > 0.0 && inner_converged(0, diff)) break;
        }
    }

    __device__ __forceinline__ void x_times_C(double *XC) {
        for (int64_t j = threadIdx.x; j < N; j += MS_THREADS) {
            double acc[R];
            #pragma unroll
            for (int l = 0; l < R; ++l) acc[l] = 0.0;
            if (in_job(slab[j]))  // a slab outside the job: zeros, no pass over its X
                for (int64_t c = 0; c < K; ++c) {
                    const double xv = x(j, c);
                    #pragma unroll
                    for (int l = 0; l < R; ++l) acc[l] += xv * C[c * R + l];
                }
            #pragma unroll
            for (int l = 0; l < R; ++l) XC[j * R + l] = acc[l];
        }
        __syncthreads();
    }

    // (<X, model>, ||model||^2): from the A phase's rhs and Q (decomposition.py:445-449), or with a pass over X (:430-444).
    // WEIGHTED: sum_i w_i <X_i, model_i> and sum_i w_i ||model_i||^2 (rhs_A and Q carry w_i already)
    __device__ __forceinline__ void model_terms(bool from_A, double *inner, double *model) {
        const int t = threadIdx.x;
        double *Q = ws + sc.Q, *rhsA = ws + sc.rhsA;
        if (from_A) {
            double s = 0.0, m = 0.0;
            for (int64_t e = t; e < I * R; e += MS_THREADS) s += rhsA[e] * A[e];
            for (int64_t i = t; i < I; i += MS_THREADS) {
                const double *ai = A + i * R, *Qi = Q + i * R * R;
                double v = 0.0;
                for (int p = 0; p < R; ++p) {
                    double w = 0.0;
                    for (int q = 0; q < R; ++q) w += Qi[p * R + q] * ai[q];
                    v += ai[p] * w;
                }
                m += v;
            }
            *inner = wg_sum(s, red);
            *model = wg_sum(m, red);
            return;
        }
        double *cc = ws + sc.small, *XC = ws + sc.XC;
        ctc(cc);
        x_times_C(XC);
        double s = 0.0;
        for (int64_t j = t; j < N; j += MS_THREADS) {
            const double *ai = A + (int64_t)slab[j] * R;
            for (int l = 0; l < R; ++l) {
                double b = B[j * R + l] * ai[l];
                if constexpr (WEIGHTED) b *= w[slab[j]];
                s += XC[j * R + l] * b;
            }
        }
        double m = 0.0;
        for (int64_t e = t; e < I * R * R; e += MS_THREADS) {
            const int64_t i = e / (R * R);
            const int ab = (int)(e % (R * R)), p = ab / R, q = ab % R;
            double g = 0.0;
            for (int64_t j = rp[i]; j < rp[i + 1]; ++j) g += (B[j * R + p] * A[i * R + p]) * (B[j * R + q] * A[i * R + q]);
            if constexpr (WEIGHTED) g *= w[i];
            m += g * cc[ab];
        }
        *inner = wg_sum(s, red);
        *model = wg_sum(m, red);
    }

    // MISSING: one pass over the job's entries with M = B_i D_i C^T at (j, c): the sum of (X - M)^2 over the observed ones is
    // returned, and with `store` the others get X~(j, c) = M.  Thread t takes the entries t, t + 256, ... (row-major), wg_sum adds
    // the 256 partials: a fixed order.  The mask selects; the value of X~ at a missing entry is never used in arithmetic.
    __device__ __forceinline__ double impute_pass(bool store) {
        double *Xt = const_cast<double *>(reinterpret_cast<const double *>(X));
        const int64_t n = N * K, dj = MS_THREADS / K, dc = MS_THREADS % K;
        int64_t j = threadIdx.x / K, c = threadIdx.x % K;
        double ss = 0.0;
        for (int64_t e = threadIdx.x; e < n; e += MS_THREADS) {
            const double *bj = B + j * R, *ai = A + (int64_t)slab[j] * R, *cc = C + c * R;
            double m = 0.0;
            #pragma unroll
            for (int l = 0; l < R; ++l) m += (bj[l] * ai[l]) * cc[l];
            if (obs[e]) {
                const double d = Xt[e] - m;
                ss += d * d;
            } else if (store) {
                Xt[e] = m;
            }
            j += dj, c += dc;
            if (c >= K) c -= K, ++j;
        }
        return wg_sum(ss, red);  // (its barriers: the stores are visible to the workgroup's next pass over X~)
    }

    // one diagnostics row: rec_error, loss, flags, regularisation, gaps; returns the flags.  MISSING: `store` as in impute_pass
    __device__ __forceinline__ int diagnostics(bool from_A, double x_sq, double *row, bool store = false) {
        double inner = 0.0, model = 0.0, resid = 0.0;
        if constexpr (MISSING) resid = impute_pass(store);
        else model_terms(from_A, &inner, &model);
        double reg = 0.0, worst = -INFINITY, gaps[3][MCL_MAX_REGS];
#pragma unroll
        for (int m = 0; m < 3; ++m) {
            double nf, gp[MCL_MAX_REGS], as;
            mode_stats(m, &nf, gp, &as);
#pragma unroll
            for (int k = 0; k < MCL_MAX_REGS; ++k) {
                gaps[m][k] = 0.0;
                if (k >= a.o.n_regs[m]) continue;
                gaps[m][k] = sqrt(gp[k]) / sqrt(nf);
                worst = fmax(worst, gaps[m][k]);
                if (a.o.regs[m][k].kind == MCL_PEN_L1) reg += a.o.regs[m][k].p0 * as;
            }
            if (a.o.l2_penalty[m] != 0.0) reg += 0.5 * a.o.l2_penalty[m] * nf;
        }
        double rec;
        if constexpr (MISSING) rec = sqrt(resid) / sqrt(x_sq);
        else rec = sqrt(fmax(0.0, x_sq - 2.0 * inner + model)) / sqrt(x_sq);
        const double loss = 0.5 * rec * rec + reg;
        const bool feasible = a.o.feasibility_tol > 0.0 && worst < a.o.feasibility_tol;
        if (threadIdx.x == 0) {
            row[0] = rec, row[1] = loss, row[3] = reg;
#pragma unroll
            for (int m = 0; m < 3; ++m)
#pragma unroll
                for (int k = 0; k < MCL_MAX_REGS; ++k) row[4 + m * MCL_MAX_REGS + k] = gaps[m][k];
        }
        return feasible ? 1 : 0;
    }

    // the whole fit of job s: the body of k_multistart and of k_multistart_weighted
    __device__ __forceinline__ void fit(int64_t s) {
        double *diag = a.diag + s * a.diag_stride;
        const int t = threadIdx.x;

        // ||X||^2 (every start: the same order, the same bits); WEIGHTED: sum_i w_i ||X_i||^2, in that order too
        double xs = 0.0;
        for (int64_t e = t; e < a.N * a.K; e += MS_THREADS) {
            if constexpr (MISSING) {  // the observed entries alone
                if (obs[e]) {
                    const double v = (double)XL::ld1(X + e);
                    xs += v * v;
                }
            } else if constexpr (WEIGHTED) {
                const double wi = w[slab[e / a.K]];
                if (wi != 0.0) {
                    const double v = (double)XL::ld1(X + e);
                    xs += (wi * v) * v;
                }
            } else {
                const double v = (double)XL::ld1(X + e);
                xs += v * v;
            }
        }
        const double x_sq = wg_sum(xs, red);

        int f0 = diagnostics(false, x_sq, diag, fill_model);
        if (t == 0) diag[2] = (double)(f0 | 2);
        __syncthreads();
        const mcl_multistart_options &o = a.o;
        const bool active = o.tol > 0.0 || o.absolute_tol > 0.0;
        double prev = diag[1];
        int it = 0, code = 0;
        for (; it < o.n_iter_max && !code; ++it) {
            if (o.update_B) phase_B();
            if (o.update_C) phase_C();
            if (o.update_A) phase_A();
            double *row = diag + (int64_t)(it + 1) * MCL_MS_DIAG;
            const int feasible = diagnostics(o.update_A != 0, x_sq, row, true);
            __syncthreads();
            const double loss = row[1];
            const bool evaluated = !active || feasible || o.evaluate_loss_always;
            if (active && evaluated && o.tol > 0.0 && feasible) {
                if (fabs(prev - loss) < o.tol * prev) code = MCL_STOP_RELATIVE;
                else if (loss < o.absolute_tol) code = MCL_STOP_ABSOLUTE;
            }
            if (evaluated) prev = loss;
            __syncthreads();
            if (t == 0) row[2] = (double)(feasible | (evaluated ? 2 : 0));
        }
        if (t == 0) a.n_iter[s] = it, a.stop[s] = code;
    }
};

// The LDS, the arguments' LDS copy and the start object are declared in the kernels themselves, not in a function the two share:
// where they are declared moves the register allocation of the unweighted instantiations (DESIGN.md sections 17 and 18).
// MORE: statements on the start object `st` of job `s` before the fit (k_multistart_missing: its slice of X~ and its mask).
#define MS_START(WEIGHTED, MISSING, WPTR, MORE)                                                                               \
    __shared__ double red[MS_THREADS];                                                                                        \
    __shared__ double sys[MS_SYS_BYTES / 8];                                                                                  \
    __shared__ double sh[4 * R * R + 16 + MCL_MAX_REGS * R * R];                                                              \
    __shared__ MsArgs sa; /* the arguments in LDS: the helpers keep a reference to them (no private copy of the kernarg) */  \
    if (threadIdx.x == 0) sa = a0;                                                                                            \
    __syncthreads();                                                                                                          \
    const int64_t s = blockIdx.x;                                                                                             \
    if (a0.jobs) { /* a grid: this workgroup's own options replace the shared ones (uniform branch: a0 is the kernarg) */    \
        const int32_t *src = reinterpret_cast<const int32_t *>(a0.jobs + s);                                                  \
        int32_t *dst = reinterpret_cast<int32_t *>(&sa.o);                                                                    \
        for (int e = threadIdx.x; e < (int)(sizeof(mcl_multistart_options) / sizeof(int32_t)); e += MS_THREADS) dst[e] = src[e]; \
        __syncthreads();                                                                                                      \
    }                                                                                                                         \
    const MsArgs &a = sa;                                                                                                     \
    Start<R, XL, WEIGHTED, MISSING> st{a, static_cast<const typename XL::T *>(a.X), a.row_ptr, a.slab_of_row, a.I, a.N, a.K, WPTR}; \
    st.A = a.state + s * a.state_len;                                                                                         \
    st.B = st.A + a.I * R;                                                                                                    \
    st.C = st.B + a.N * R;                                                                                                    \
    st.ws = a.scratch + s * a.scratch_len;                                                                                    \
    st.sc = ms_scratch(a.I, a.N, a.K, R);                                                                                     \
    st.red = red, st.sys = sys, st.sh = sh;                                                                                   \
    st.nb = std::min(MS_THREADS, MS_SYS_BYTES / (2 * R * R * 8));                                                             \
    MORE                                                                                                                      \
    st.fit(s);

template <int R, class XL>
__global__ __launch_bounds__(MS_THREADS) void k_multistart(MsArgs a0) {
    MS_START(false, false, nullptr, )
}

// job blockIdx.x under its own row of slab_weight [n_jobs, I] (fp64, device)
template <int R, class XL>
__global__ __launch_bounds__(MS_THREADS) void k_multistart_weighted(MsArgs a0, const double *slab_weight) {
    MS_START(true, false, slab_weight + (int64_t)blockIdx.x * a0.I, )
}

// job blockIdx.x on its own copy X~ (a0.X: fp64 [n_jobs, N, K], k_missing_copy_in) under mask blockIdx.x % n_masks of
// observed [n_masks, N, K]
template <int R>
__global__ __launch_bounds__(MS_THREADS) void k_multistart_missing(MsArgs a0, const uint8_t *observed, int32_t n_masks, int32_t fill_model) {
    using XL = XF64;
    MS_START(false, true, nullptr,
             st.X += s * (a.N * a.K);
             st.obs = observed + (s % n_masks) * (a.N * a.K);
             st.fill_model = fill_model != 0;)
}
#undef MS_START

// X~ of every job: block s copies X (stored type, converted exactly) where mask s % n_masks says observed; elsewhere the mask's
// row of fill_values [n_masks, K], or 0.0 without fill_values (k_multistart_missing stores the start's model there before any
// phase reads it).  A select, never a product: X may hold NaN or anything else at a missing entry.
template <class XL>
__global__ __launch_bounds__(MS_THREADS) void k_missing_copy_in(const typename XL::T *X, const uint8_t *observed, int32_t n_masks,
                                                                const double *fill_values, int64_t NK, int64_t K, double *Xt) {
    const int64_t s = blockIdx.x, m = s % n_masks;
    const uint8_t *ob = observed + m * NK;
    double *out = Xt + s * NK;
    for (int64_t e = threadIdx.x; e < NK; e += MS_THREADS) {
        const double fill = fill_values ? fill_values[m * K + e % K] : 0.0;
        out[e] = ob[e] ? (double)XL::ld1(X + e) : fill;
    }
}

std::string ms_check(const int64_t *row_ptr, int64_t I, int64_t K, int32_t rank, const mcl_multistart_options *o, int32_t n_starts) {
    if (!row_ptr || !o || I < 1 || K < 1) return "need row_ptr, options, I >= 1, K >= 1";
    if (rank < 1 || rank > MS_MAX_RANK) return "need 1 <= rank <= 16";
    if (n_starts < 1) return "need n_starts >= 1";
    if (row_ptr[0] != 0) return "row_ptr[0] must be 0";
    int64_t Jmin = INT64_MAX;
    for (int64_t i = 0; i < I; ++i) {
        if (row_ptr[i + 1] < row_ptr[i]) return "row_ptr must be non-decreasing";
        Jmin = std::min(Jmin, row_ptr[i + 1] - row_ptr[i]);
    }
    if (row_ptr[I] >= (int64_t(1) << 31)) return "more than 2^31 packed rows are not supported";
    if (o->inner_n_iter_max < 0 || o->n_iter_max < 0) return "need inner_n_iter_max >= 0 and n_iter_max >= 0";
    for (int m = 0; m < 3; ++m) {
        if (o->n_regs[m] < 0 || o->n_regs[m] > MCL_MAX_REGS) return "at most MCL_MAX_REGS penalties per mode";
        for (int k = 0; k < o->n_regs[m]; ++k) {
            const int kind = o->regs[m][k].kind;
            if (kind == MCL_PEN_PARAFAC2) {
                if (m != 1) return "PARAFAC2 only on mode 1";
                if (Jmin < rank) return "PARAFAC2 needs every J_i >= rank";
            } else if (kind == MCL_PEN_L2BALL) {
                if (m == 0 && !o->constant_A) return "an L2 ball on mode 0 needs constant_A";
            } else if (kind != MCL_PEN_NN && kind != MCL_PEN_BOX && kind != MCL_PEN_L1) {
                return "penalty kind " + std::to_string(kind) + " is not served (NN, Box, L1, L2 ball, PARAFAC2)";
            }
        }
    }
    return "";
}

// the state slice of one start, in doubles: A, B, C, then aux (+ Delta for PARAFAC2) and dual of every penalty
void ms_state_layout(MsArgs &a, int rank, const mcl_multistart_options *o) {
    const int64_t r = rank, rows[3] = {a.I, a.N, a.K};
    int64_t off = (a.I + a.N + a.K) * r;
    for (int m = 0; m < 3; ++m)
        for (int k = 0; k < o->n_regs[m]; ++k) {
            a.off_aux[m][k] = off;
            off += rows[m] * r;
            if (o->regs[m][k].kind == MCL_PEN_PARAFAC2) {
                a.off_delta[m][k] = off;
                off += r * r;
            }
            a.off_dual[m][k] = off;
            off += rows[m] * r;
        }
    a.state_len = off;
}

StartsPlan ms_plan(void *workspace, const int64_t *row_ptr, int64_t I, int64_t K, int rank, int32_t n_starts) {
    return starts_plan(workspace, row_ptr, I, ms_scratch(I, row_ptr[I], K, rank).total, n_starts);
}

// the options of a grid's jobs in the workspace, behind the plan of mcl_multistart_run
int64_t ms_jobs_bytes(int32_t n_jobs) { return (int64_t(n_jobs) * (int64_t)sizeof(mcl_multistart_options) + 255) & ~int64_t(255); }

// a grid: every job passes ms_check, and all jobs have ONE state layout and one set of phases (what ms_plan and the kernel's
// uniform branches follow): the number, kind and non-negativity flag of the penalties, constant_A / B and update_A / B / C
std::string ms_check_grid(const int64_t *row_ptr, int64_t I, int64_t K, int32_t rank, const mcl_multistart_options *o, int32_t n_jobs) {
    if (!o || n_jobs < 1) return "need options and n_jobs >= 1";
    for (int32_t s = 0; s < n_jobs; ++s) {
        const std::string bad = ms_check(row_ptr, I, K, rank, o + s, n_jobs);
        if (!bad.empty()) return "job " + std::to_string(s) + ": " + bad;
        const mcl_multistart_options &a = o[0], &b = o[s];
        bool same = a.constant_A == b.constant_A && a.constant_B == b.constant_B && a.update_A == b.update_A &&
                    a.update_B == b.update_B && a.update_C == b.update_C;
        for (int m = 0; m < 3 && same; ++m) {
            same = a.n_regs[m] == b.n_regs[m];
            for (int k = 0; same && k < a.n_regs[m]; ++k)
                same = a.regs[m][k].kind == b.regs[m][k].kind && a.regs[m][k].non_negativity == b.regs[m][k].non_negativity;
        }
        if (!same)
            return "job " + std::to_string(s) + " differs from job 0 in n_regs, a penalty's kind or non_negativity, constant_A/B or "
                   "update_A/B/C: the jobs of a grid share one state layout";
    }
    return "";
}

// the weights of mcl_multistart_run_weighted in the workspace, behind the plan of mcl_multistart_run
int64_t ms_weights_bytes(int32_t n_jobs, int64_t I) { return (int64_t(n_jobs) * I * 8 + 255) & ~int64_t(255); }

// slab_weights [n_jobs, I] on the host: finite, >= 0, a positive one in every job
std::string ms_check_weights(const double *w, int32_t n_jobs, int64_t I) {
    if (!w) return "NULL slab_weights";
    for (int32_t s = 0; s < n_jobs; ++s) {
        bool any = false;
        for (int64_t i = 0; i < I; ++i) {
            const double v = w[int64_t(s) * I + i];
            if (!std::isfinite(v) || v < 0.0)
                return "slab_weights[" + std::to_string(s) + "][" + std::to_string(i) + "] is negative or not finite";
            any = any || v > 0.0;
        }
        if (!any) return "job " + std::to_string(s) + " has no positive weight";
    }
    return "";
}

// the X~ slices of mcl_multistart_run_missing in the workspace, behind the plan of mcl_multistart_run
int64_t ms_filled_bytes(int32_t n_jobs, int64_t N, int64_t K) { return (int64_t(n_jobs) * N * K * 8 + 255) & ~int64_t(255); }

// mcl_multistart_run (per_job false: *opt for every workgroup, passed in the kernarg), mcl_multistart_run_grid (per_job true:
// opt[s] for workgroup s, uploaded to the workspace) and mcl_multistart_run_weighted (weighted true: *opt for every workgroup
// and the host array slab_weights [n_starts, I], uploaded to the workspace) and mcl_multistart_run_missing (observed set: *opt for
// every workgroup, the device mask observed [n_masks, N, K] and device fill_values [n_masks, K] or NULL)
int ms_run(const char *who, const char *sizer, const void *X, int32_t x_type, const int64_t *row_ptr, int64_t I, int64_t K, int32_t rank,
           const mcl_multistart_options *opt, int32_t n_starts, bool per_job, bool weighted, const double *slab_weights,
           bool missing, const uint8_t *observed, int32_t n_masks, const double *fill_values, double *state, double *diag,
           int32_t *n_iter, int32_t *stop, void *workspace, int64_t workspace_bytes, void *hip_stream) {
    ErrorSlot &fail = g_ms_error.named(who);
    std::string bad = per_job ? ms_check_grid(row_ptr, I, K, rank, opt, n_starts) : ms_check(row_ptr, I, K, rank, opt, n_starts);
    if (bad.empty() && weighted) bad = ms_check_weights(slab_weights, n_starts, I);
    if (!bad.empty()) return fail(bad);
    if (missing && n_masks != 1 && n_masks != n_starts) return fail("need n_masks = 1 or n_masks = n_jobs");
    if (missing && !observed) return fail("NULL observed mask");
    if (!X || !state || !diag || !n_iter || !stop || !workspace) return fail("NULL argument");
    if (!x_type_error(x_type).empty()) return fail(x_type_error(x_type));
    const StartsPlan p = ms_plan(workspace, row_ptr, I, K, rank, n_starts);
    const int64_t jobs_bytes = per_job    ? ms_jobs_bytes(n_starts)
                               : weighted ? ms_weights_bytes(n_starts, I)
                               : missing  ? ms_filled_bytes(n_starts, p.N, K)
                                          : 0;
    if (workspace_refused(fail, workspace, workspace_bytes, p.total + jobs_bytes, sizer)) return 1;
    hipStream_t s = reinterpret_cast<hipStream_t>(hip_stream);
    char *extra = static_cast<char *>(workspace) + p.total;  // the jobs' options, weights or X~ slices, behind the plan
    std::vector<int32_t> slab;
    if (upload_starts(p, row_ptr, I, slab, s) != hipSuccess ||
        (per_job && hipMemcpyAsync(extra, opt, int64_t(n_starts) * sizeof(mcl_multistart_options), hipMemcpyHostToDevice, s) != hipSuccess) ||
        (weighted && hipMemcpyAsync(extra, slab_weights, int64_t(n_starts) * I * 8, hipMemcpyHostToDevice, s) != hipSuccess) ||
        hipStreamSynchronize(s) != hipSuccess)
        return fail(per_job ? "upload of row_ptr and the options failed"
                            : (weighted ? "upload of row_ptr and the weights failed" : "upload of row_ptr failed"));
    int32_t n_iter_most = opt->n_iter_max;  // the diagnostics stride: that of the longest job
    for (int32_t j = 1; per_job && j < n_starts; ++j) n_iter_most = std::max(n_iter_most, opt[j].n_iter_max);
    MsArgs a{};
    a.X = X;
    a.row_ptr = p.row_ptr;
    a.slab_of_row = p.slab_of_row;
    a.I = I, a.N = p.N, a.K = K;
    ms_state_layout(a, rank, opt);
    a.scratch_len = ms_scratch(I, p.N, K, rank).total;
    a.diag_stride = int64_t(n_iter_most + 1) * MCL_MS_DIAG;
    a.state = state, a.scratch = p.scratch, a.diag = diag;
    a.n_iter = n_iter, a.stop = stop;
    a.o = *opt;
    a.jobs = per_job ? reinterpret_cast<const mcl_multistart_options *>(extra) : nullptr;
    const double *slab_weight = weighted ? reinterpret_cast<const double *>(extra) : nullptr;
    if (missing) {  // the typed copy into the fp64 slices, then the fit on them: 16 instantiations, not 48
        double *Xt = reinterpret_cast<double *>(extra);
        mcl_x_dispatch(x_type, [&](auto xl) {
            using XL = decltype(xl);
            hipLaunchKernelGGL((k_missing_copy_in<XL>), dim3(n_starts), dim3(MS_THREADS), 0, s, static_cast<const typename XL::T *>(X),
                               observed, n_masks, fill_values, p.N * K, K, Xt);
            return 0;
        });
        a.X = Xt;
        rank_exact<MS_MAX_RANK>(rank, [&](auto rc) {
            constexpr int R = decltype(rc)::value;
            hipLaunchKernelGGL((k_multistart_missing<R>), dim3(n_starts), dim3(MS_THREADS), 0, s, a, observed, n_masks,
                               int32_t(fill_values == nullptr));
        });
    } else mcl_x_dispatch(x_type, [&](auto xl) {
        using XL = decltype(xl);
        rank_exact<MS_MAX_RANK>(rank, [&](auto rc) {
            constexpr int R = decltype(rc)::value;
            if (slab_weight) hipLaunchKernelGGL((k_multistart_weighted<R, XL>), dim3(n_starts), dim3(MS_THREADS), 0, s, a, slab_weight);
            else hipLaunchKernelGGL((k_multistart<R, XL>), dim3(n_starts), dim3(MS_THREADS), 0, s, a);
        });
        return 0;
    });
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(std::string("launch failed: ") + hipGetErrorString(e));
    return 0;
}

}  // namespace

extern "C" {

const char *mcl_multistart_last_error(void) { return g_ms_error.c_str(); }

int64_t mcl_multistart_workspace_bytes(const int64_t *row_ptr, int64_t I, int64_t K, int32_t rank, const mcl_multistart_options *opt,
                                       int32_t n_starts) {
    if (!ms_check(row_ptr, I, K, rank, opt, n_starts).empty()) return -1;
    return ms_plan(nullptr, row_ptr, I, K, rank, n_starts).total;
}

int mcl_multistart_run(const void *X, int32_t x_type, const int64_t *row_ptr, int64_t I, int64_t K, int32_t rank,
                       const mcl_multistart_options *opt, int32_t n_starts, double *state, double *diag, int32_t *n_iter, int32_t *stop,
                       void *workspace, int64_t workspace_bytes, void *hip_stream) {
    return ms_run("mcl_multistart_run: ", "mcl_multistart_workspace_bytes", X, x_type, row_ptr, I, K, rank, opt, n_starts, false, false,
                  nullptr, false, nullptr, 0, nullptr, state, diag, n_iter, stop, workspace, workspace_bytes, hip_stream);
}

int64_t mcl_multistart_grid_workspace_bytes(const int64_t *row_ptr, int64_t I, int64_t K, int32_t rank,
                                            const mcl_multistart_options *options, int32_t n_jobs) {
    if (!ms_check_grid(row_ptr, I, K, rank, options, n_jobs).empty()) return -1;
    return ms_plan(nullptr, row_ptr, I, K, rank, n_jobs).total + ms_jobs_bytes(n_jobs);
}

int mcl_multistart_run_grid(const void *X, int32_t x_type, const int64_t *row_ptr, int64_t I, int64_t K, int32_t rank,
                            const mcl_multistart_options *options, int32_t n_jobs, double *state, double *diag, int32_t *n_iter,
                            int32_t *stop, void *workspace, int64_t workspace_bytes, void *hip_stream) {
    return ms_run("mcl_multistart_run_grid: ", "mcl_multistart_grid_workspace_bytes", X, x_type, row_ptr, I, K, rank, options, n_jobs, true,
                  false, nullptr, false, nullptr, 0, nullptr, state, diag, n_iter, stop, workspace, workspace_bytes, hip_stream);
}

int64_t mcl_multistart_weighted_workspace_bytes(const int64_t *row_ptr, int64_t I, int64_t K, int32_t rank,
                                                const mcl_multistart_options *opt, int32_t n_jobs) {
    if (!ms_check(row_ptr, I, K, rank, opt, n_jobs).empty()) return -1;
    return ms_plan(nullptr, row_ptr, I, K, rank, n_jobs).total + ms_weights_bytes(n_jobs, I);
}

int mcl_multistart_run_weighted(const void *X, int32_t x_type, const int64_t *row_ptr, int64_t I, int64_t K, int32_t rank,
                                const mcl_multistart_options *opt, int32_t n_jobs, const double *slab_weights, double *state,
                                double *diag, int32_t *n_iter, int32_t *stop, void *workspace, int64_t workspace_bytes,
                                void *hip_stream) {
    return ms_run("mcl_multistart_run_weighted: ", "mcl_multistart_weighted_workspace_bytes", X, x_type, row_ptr, I, K, rank, opt, n_jobs,
                  false, true, slab_weights, false, nullptr, 0, nullptr, state, diag, n_iter, stop, workspace, workspace_bytes, hip_stream);
}

int64_t mcl_multistart_missing_workspace_bytes(const int64_t *row_ptr, int64_t I, int64_t K, int32_t rank,
                                               const mcl_multistart_options *opt, int32_t n_jobs) {
    if (!ms_check(row_ptr, I, K, rank, opt, n_jobs).empty()) return -1;
    return ms_plan(nullptr, row_ptr, I, K, rank, n_jobs).total + ms_filled_bytes(n_jobs, row_ptr[I], K);
}

int mcl_multistart_run_missing(const void *X, int32_t x_type, const int64_t *row_ptr, int64_t I, int64_t K, int32_t rank,
                               const mcl_multistart_options *opt, int32_t n_jobs, const uint8_t *observed, int32_t n_masks,
                               const double *fill_values, double *state, double *diag, int32_t *n_iter, int32_t *stop,
                               void *workspace, int64_t workspace_bytes, void *hip_stream) {
    return ms_run("mcl_multistart_run_missing: ", "mcl_multistart_missing_workspace_bytes", X, x_type, row_ptr, I, K, rank, opt, n_jobs,
                  false, false, nullptr, true, observed, n_masks, fill_values, state, diag, n_iter, stop, workspace, workspace_bytes,
                  hip_stream);
}

}  // extern "C"
