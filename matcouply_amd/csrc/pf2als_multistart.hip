// parafac2_als_multistart (decomposition.py): many random starts of ONE unconstrained PARAFAC2-ALS problem fitted at once, one
// workgroup per start (the layout of csrc/multistart.hip).
//
// At the sizes PARAFAC2 users fit from many starts (about 100 matrices of ~100 x 20, rank 2-4) one parafac2_als call is
// launch-bound and keeps a few CUs busy.  Here a start lives in ONE workgroup (256 threads): every outer iteration, its CP sweeps
// and the stopping rule run inside one launch with nothing but workgroup barriers; blockIdx.x is the start.
//
// One outer iteration, as tests/parafac2_als_restatement.py states it:
//   W_i = X_i C, WtW_i = W_i^T W_i, G_i = B D_i WtW_i D_i B^T, T_i = D_i B^T G_i^-1/2 (eigenvalues <= 1e-12 lam_max dropped),
//   Y_i = T_i^T (W_i^T X_i) [r, K], then n_iter_parafac CP sweeps on Y over the modes A, B, C: ALS (Cholesky; the pseudo-inverse
//   from a Jacobi eigen-decomposition when the Cholesky fails) or one Gauss-Seidel HALS column pass for the modes in nn_modes.
//   With tol > 0: e^2 = (|X|^2 - 2 <M_C, C> + sum_i sum((D_i B^T P_i^T P_i B D_i) o C^T C)) / |X|^2, P_i^T P_i = T_i^T WtW_i T_i
//   (no third read of X); stop after t >= 1 when |e_{t-1}^2 - e_t^2| <= tol e_{t-1}^2 or e_t^2 < absolute_tol.
// The projections P_i = W_i T_i are written once, from the last iteration's W and T.
//
// Numerics: fp64 throughout; X is read in its stored type and converted exactly (xload.h).  No atomics; every sum runs in a
// fixed order that depends only on the problem's shape (wg_fp64.h), so a start's result is bitwise independent of how many
// starts share the launch and of which.
//
// parafac2_als_resample (resampling.py): k_ms_pf2als_weighted is the same fit of the matrices
// scale[s][i] X_i, job s reading its own I factors - bootstrap, jackknife and K-fold jobs over the matrices share the one X.
//
// Memory: X, row_ptr and the row -> slab map are shared.  Each start owns its factors (the caller's fp64 [I + r + K, r]), its
// projections and errors, and a slice of the fp64 scratch workspace: W [N, r], Y [I, r, K], T / WtW / V [I, r, r], M_A [I, r],
// M_C [K, r].  The r x r matrices of the sweeps (B, the Grams, M_B) live in LDS.
#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "entry_host.h"
#include "mcl_internal.h"
#include "wg_fp64.h"
#include "xload.h"

namespace {

static ErrorSlot g_pm_error;
constexpr int PM_MAX_RANK = 16;
constexpr int PM_SYS_BYTES = 40960;  // LDS for a batch of per-slab r x r polar steps (two r x r matrices per thread)
constexpr double PM_DROP = 1e-12;    // eigenvalues at or below PM_DROP lam_max are dropped (polar factor, pseudo-inverse)

struct PmArgs {
    const void *X;
    const int64_t *row_ptr;
    const int32_t *slab_of_row;
    int64_t I, N, K;
    int64_t scratch_len;
    double *factors, *P, *errors, *scratch;
    int32_t *n_iter;
    int32_t n_iter_max, n_iter_parafac, nn_modes;
    double tol, absolute_tol;
};

// scratch of one start, in doubles (decomposition.py / _engine.pf2als_multistart_scratch_len restate it)
struct PmScratch {
    int64_t W, Y, T, WtW, V, MA, MC, total;
};

static __host__ __device__ inline PmScratch pm_scratch(int64_t I, int64_t N, int64_t K, int r) {
    PmScratch s{};
    int64_t o = 0;
    auto take = [&](int64_t n) { const int64_t at = o; o += (n + 31) & ~int64_t(31); return at; };
    s.W = take(N * r);
    s.Y = take(I * r * K);
    s.T = take(I * r * r);
    s.WtW = take(I * r * r);
    s.V = take(I * r * r);
    s.MA = take(I * r);
    s.MC = take(K * r);
    s.total = o;
    return s;
}

// SCALED: the job fits the matrices scale_i X_i (resampling over the matrices): every element of X_i is
// multiplied by the job's factor of slab i after the exact conversion to double.  Without SCALED `scale` is never read.
template <int R, class XL, bool SCALED>
struct Pf2Start {
    static constexpr int RR = R * R;
    const typename XL::T *X;
    const int64_t *rp;
    const int32_t *slab;
    int64_t I, N, K;
    double *A, *B, *C;                   // the start's factors (global, in/out)
    double *W, *Y, *T, *WtW, *V, *MA, *MC;  // scratch (global)
    double *red, *sys, *Bs, *BtB, *CtC, *AtA, *MB;  // LDS
    int nb;                              // polar steps per batch

    __device__ __forceinline__ double x(int64_t j, int64_t c) const { return (double)XL::ld1(X + j * K + c); }

    // out (LDS, R x R) = F^T F for a factor of n rows
    __device__ __forceinline__ void gram(const double *F, int64_t n, double *out) {
        rows_reduce(RR, n, out, red, [&](int64_t j, int e) { return F[j * R + e / R] * F[j * R + e % R]; });
    }

    // G (LDS) = G1 o G2; then, for ALS, G <- G^-1: Cholesky, or the pseudo-inverse (Jacobi, eigenvalues <= 1e-12 lam_max dropped,
    // (G^+1/2)^2) when a pivot is not positive.  HALS keeps G.
    __device__ __forceinline__ void system(const double *G1, const double *G2, bool hals) {
        double *G = sys, *Wk = sys + RR, *Gsave = sys + 2 * RR;
        if (threadIdx.x == 0) {
            for (int e = 0; e < RR; ++e) G[e] = G1[e] * G2[e], Gsave[e] = G[e];
            if (!hals && !spd_inverse<R>(G, Wk)) {
                for (int e = 0; e < RR; ++e) G[e] = Gsave[e];
                gram_inv_sqrt<R>(G, Wk, PM_DROP);
                for (int p = 0; p < R; ++p)
                    for (int q = 0; q < R; ++q) {
                        double v = 0.0;
                        for (int u = 0; u < R; ++u) v += G[p * R + u] * G[u * R + q];
                        Gsave[p * R + q] = v;
                    }
                for (int e = 0; e < RR; ++e) G[e] = Gsave[e];
            }
        }
        __syncthreads();
    }

    // rows of F (n x R) from their right-hand sides M with the system of system(): ALS F = M G^-1, HALS one column pass
    __device__ __forceinline__ void update_rows(const double *M, double *F, int64_t n, bool hals) {
        const double *G = sys;
        for (int64_t i = threadIdx.x; i < n; i += MS_THREADS) {
            if (hals) {
                #pragma unroll 1
                for (int q = 0; q < R; ++q) {
                    const double gqq = G[q * R + q];
                    if (gqq == 0.0) continue;
                    double fg = 0.0;
                    #pragma unroll
                    for (int p = 0; p < R; ++p) fg += F[i * R + p] * G[p * R + q];
                    F[i * R + q] = fmax(0.0, F[i * R + q] + (M[i * R + q] - fg) / gqq);
                }
            } else {
                double m[R];
                #pragma unroll
                for (int q = 0; q < R; ++q) m[q] = M[i * R + q];
                #pragma unroll 1
                for (int l = 0; l < R; ++l) {
                    double v = 0.0;
                    #pragma unroll
                    for (int q = 0; q < R; ++q) v += m[q] * G[q * R + l];
                    F[i * R + l] = v;
                }
            }
        }
        __syncthreads();
    }

    // W = X C, WtW_i, then per slab T_i = D_i B^T G_i^-1/2 (one thread per slab, a batch at a time in LDS), then Y_i
    // (scale: the job's factor per slab [I], SCALED only)
    __device__ __forceinline__ void project(const double *scale) {
        const int t = threadIdx.x;
        for (int64_t j = t; j < N; j += MS_THREADS) {
            double acc[R];
            #pragma unroll
            for (int l = 0; l < R; ++l) acc[l] = 0.0;
            if constexpr (SCALED) {
                const double f = scale[slab[j]];
                if (f != 0.0)  // a slab of scale 0 has W = 0 either way: its pass over X is skipped
                    for (int64_t c = 0; c < K; ++c) {
                        const double xv = x(j, c) * f;
                        #pragma unroll
                        for (int l = 0; l < R; ++l) acc[l] += xv * C[c * R + l];
                    }
            } else {
                for (int64_t c = 0; c < K; ++c) {
                    const double xv = x(j, c);
                    #pragma unroll
                    for (int l = 0; l < R; ++l) acc[l] += xv * C[c * R + l];
                }
            }
            #pragma unroll
            for (int l = 0; l < R; ++l) W[j * R + l] = acc[l];
        }
        __syncthreads();
        for (int64_t e = t; e < I * RR; e += MS_THREADS) {
            const int64_t i = e / RR;
            const int p = (int)(e % RR) / R, q = (int)(e % RR) % R;
            double s = 0.0;
            for (int64_t j = rp[i]; j < rp[i + 1]; ++j) s += W[j * R + p] * W[j * R + q];
            WtW[e] = s;
        }
        __syncthreads();
        for (int64_t base = 0; base < I; base += nb) {
            const int64_t i = base + t;
            if (t < nb && i < I) {
                double *S = sys + t * 2 * RR, *H = S + RR;
                const double *a = A + i * R, *Wt = WtW + i * RR;
                for (int p = 0; p < R; ++p)  // H = D WtW D B^T
                    for (int y = 0; y < R; ++y) {
                        double v = 0.0;
                        for (int q = 0; q < R; ++q) v += a[p] * a[q] * Wt[p * R + q] * Bs[y * R + q];
                        H[p * R + y] = v;
                    }
                for (int u = 0; u < R; ++u)  // G = B H
                    for (int y = 0; y < R; ++y) {
                        double v = 0.0;
                        for (int p = 0; p < R; ++p) v += Bs[u * R + p] * H[p * R + y];
                        S[u * R + y] = v;
                    }
                for (int u = 0; u < R; ++u)  // (G + G^T) / 2
                    for (int y = u + 1; y < R; ++y) {
                        const double v = 0.5 * (S[u * R + y] + S[y * R + u]);
                        S[u * R + y] = v, S[y * R + u] = v;
                    }
                gram_inv_sqrt<R>(S, H, PM_DROP);
                double *Ti = T + i * RR;
                for (int p = 0; p < R; ++p)  // T = D B^T G^-1/2
                    for (int q = 0; q < R; ++q) {
                        double v = 0.0;
                        for (int u = 0; u < R; ++u) v += Bs[u * R + p] * S[u * R + q];
                        Ti[p * R + q] = a[p] * v;
                    }
            }
        }
        __syncthreads();
        for (int64_t e = t; e < I * K; e += MS_THREADS) {  // Y_i[:, k] = T_i^T (W_i^T X_i[:, k])
            const int64_t i = e / K, k = e % K;
            double z[R];
            #pragma unroll
            for (int p = 0; p < R; ++p) z[p] = 0.0;
            if constexpr (SCALED) {
                const double f = scale[i];
                if (f != 0.0)  // W_i = 0 and T_i = 0: Y_i is written as zeros below
                    for (int64_t j = rp[i]; j < rp[i + 1]; ++j) {
                        const double xv = x(j, k) * f;
                        #pragma unroll
                        for (int p = 0; p < R; ++p) z[p] += W[j * R + p] * xv;
                    }
            } else {
                for (int64_t j = rp[i]; j < rp[i + 1]; ++j) {
                    const double xv = x(j, k);
                    #pragma unroll
                    for (int p = 0; p < R; ++p) z[p] += W[j * R + p] * xv;
                }
            }
            const double *Ti = T + i * RR;
            #pragma unroll 1
            for (int q = 0; q < R; ++q) {
                double v = 0.0;
                #pragma unroll
                for (int p = 0; p < R; ++p) v += Ti[p * R + q] * z[p];
                Y[(i * R + q) * K + k] = v;
            }
        }
        __syncthreads();
    }

    // one CP sweep on Y over the modes A, B, C; leaves M_C in MC
    __device__ __forceinline__ void sweep(bool hals_a, bool hals_c) {
        const int t = threadIdx.x;
        gram(C, K, CtC);
        if (t < RR) {
            double v = 0.0;
            for (int q = 0; q < R; ++q) v += Bs[q * R + t / R] * Bs[q * R + t % R];
            BtB[t] = v;
        }
        for (int64_t e = t; e < I * RR; e += MS_THREADS) {  // V_i = Y_i C
            const int64_t i = e / RR;
            const int q = (int)(e % RR) / R, s = (int)(e % RR) % R;
            const double *y = Y + (i * R + q) * K;
            double v = 0.0;
            for (int64_t k = 0; k < K; ++k) v += y[k] * C[k * R + s];
            V[e] = v;
        }
        __syncthreads();
        for (int64_t e = t; e < I * R; e += MS_THREADS) {  // M_A[i][s] = sum_q B[q][s] V_i[q][s]
            const int64_t i = e / R;
            const int s = (int)(e % R);
            double v = 0.0;
            for (int q = 0; q < R; ++q) v += Bs[q * R + s] * V[i * RR + q * R + s];
            MA[e] = v;
        }
        system(BtB, CtC, hals_a);
        update_rows(MA, A, I, hals_a);
        gram(A, I, AtA);
        rows_reduce(RR, I, MB, red, [&](int64_t i, int e) { return V[i * RR + e] * A[i * R + e % R]; });  // M_B = sum_i V_i D_i
        system(AtA, CtC, false);
        update_rows(MB, B, R, false);
        if (t < RR) Bs[t] = B[t];
        __syncthreads();
        if (t < RR) {
            double v = 0.0;
            for (int q = 0; q < R; ++q) v += Bs[q * R + t / R] * Bs[q * R + t % R];
            BtB[t] = v;
        }
        // M_C[k][s] = sum_i a_i[s] sum_q Y_i[q][k] B[q][s]
        rows_reduce((int)(K * R), I, MC, red, [&](int64_t i, int e) {
            const int64_t k = e / R;
            const int s = e % R;
            double v = 0.0;
            for (int q = 0; q < R; ++q) v += Y[(i * R + q) * K + k] * Bs[q * R + s];
            return v * A[i * R + s];
        });
        system(AtA, BtB, hals_c);
        update_rows(MC, C, K, hals_c);
    }

    // e^2 after the sweeps (every thread gets it): |X|^2 - 2 <M_C, C> + sum_i a_i^T ((B^T P_i^T P_i B) o C^T C) a_i, over |X|^2.
    // Uses V and WtW as scratch (P_i^T P_i overwrites WtW_i).
    __device__ __forceinline__ double error_sq(double x_sq) {
        const int t = threadIdx.x;
        double cr = 0.0;
        for (int64_t e = t; e < K * R; e += MS_THREADS) cr += MC[e] * C[e];
        const double cross = wg_sum(cr, red);
        gram(C, K, CtC);
        for (int64_t e = t; e < I * RR; e += MS_THREADS) {  // V_i = WtW_i T_i
            const int64_t i = e / RR;
            const int p = (int)(e % RR) / R, y = (int)(e % RR) % R;
            double v = 0.0;
            for (int u = 0; u < R; ++u) v += WtW[i * RR + p * R + u] * T[i * RR + u * R + y];
            V[e] = v;
        }
        __syncthreads();
        for (int64_t e = t; e < I * RR; e += MS_THREADS) {  // P_i^T P_i = T_i^T V_i (into WtW)
            const int64_t i = e / RR;
            const int x0 = (int)(e % RR) / R, y = (int)(e % RR) % R;
            double v = 0.0;
            for (int p = 0; p < R; ++p) v += T[i * RR + p * R + x0] * V[i * RR + p * R + y];
            WtW[e] = v;
        }
        __syncthreads();
        for (int64_t e = t; e < I * RR; e += MS_THREADS) {  // V_i = P_i^T P_i B
            const int64_t i = e / RR;
            const int p = (int)(e % RR) / R, s = (int)(e % RR) % R;
            double v = 0.0;
            for (int u = 0; u < R; ++u) v += WtW[i * RR + p * R + u] * Bs[u * R + s];
            V[e] = v;
        }
        __syncthreads();
        double f = 0.0;
        for (int64_t e = t; e < I * RR; e += MS_THREADS) {
            const int64_t i = e / RR;
            const int x0 = (int)(e % RR) / R, s = (int)(e % RR) % R;
            double v = 0.0;
            for (int p = 0; p < R; ++p) v += Bs[p * R + x0] * V[i * RR + p * R + s];
            f += A[i * R + x0] * A[i * R + s] * v * CtC[x0 * R + s];
        }
        const double fit = wg_sum(f, red);
        return x_sq > 0.0 ? fmax(0.0, x_sq - 2.0 * cross + fit) / x_sq : 0.0;
    }

    // the factors, the scratch slice and the LDS of start blockIdx.x
    __device__ __forceinline__ void bind(const PmArgs a, double *red_, double *sys_, double *small) {
        const int64_t s = blockIdx.x;
        X = static_cast<const typename XL::T *>(a.X), rp = a.row_ptr, slab = a.slab_of_row, I = a.I, N = a.N, K = a.K;
        A = a.factors + s * (a.I + R + a.K) * R;
        B = A + a.I * R;
        C = B + RR;
        double *ws = a.scratch + s * a.scratch_len;
        const PmScratch sc = pm_scratch(a.I, a.N, a.K, R);
        W = ws + sc.W, Y = ws + sc.Y, T = ws + sc.T, WtW = ws + sc.WtW, V = ws + sc.V, MA = ws + sc.MA, MC = ws + sc.MC;
        red = red_, sys = sys_;
        Bs = small, BtB = small + RR, CtC = small + 2 * RR, AtA = small + 3 * RR, MB = small + 4 * RR;
        nb = std::min(MS_THREADS, PM_SYS_BYTES / (2 * RR * 8));
    }

    // the whole fit of the start: the body of k_ms_pf2als (SCALED false, scale unused) and of k_ms_pf2als_weighted (SCALED true,
    // scale: the job's factor per slab [I])
    __device__ __forceinline__ void fit(const PmArgs a, const double *scale) {
        const int64_t s = blockIdx.x;
        const int t = threadIdx.x;
        if (t < RR) Bs[t] = B[t];

        double xs = 0.0;  // |X|^2 (every start: the same order, the same bits); SCALED: sum_i scale_i^2 |X_i|^2, in that order too
        for (int64_t e = t; e < N * K; e += MS_THREADS) {
            double v = x(0, e);
            if constexpr (SCALED) v *= scale[slab[e / K]];
            xs += v * v;
        }
        const double x_sq = wg_sum(xs, red);  // (its barriers also publish Bs)

        const bool hals_a = a.nn_modes & 1, hals_c = (a.nn_modes >> 2) & 1;
        double *errors = a.errors ? a.errors + s * a.n_iter_max : nullptr;
        double prev = 0.0;
        int it = 0;
        while (it < a.n_iter_max) {
            project(scale);
            for (int sw = 0; sw < a.n_iter_parafac; ++sw) sweep(hals_a, hals_c);
            ++it;
            if (a.tol > 0.0) {
                const double e2 = error_sq(x_sq);
                if (t == 0) errors[it - 1] = sqrt(e2);
                const bool stop = it >= 2 && (fabs(prev - e2) <= a.tol * prev || e2 < a.absolute_tol);
                prev = e2;
                if (stop) break;
            }
        }
        double *P = a.P + s * N * R;
        for (int64_t e = t; e < N * R; e += MS_THREADS) {  // P = W T, from the last iteration's W and T
            const int64_t j = e / R;
            const int q = (int)(e % R);
            const double *Ti = T + (int64_t)slab[j] * RR;
            double v = 0.0;
            for (int p = 0; p < R; ++p) v += W[j * R + p] * Ti[p * R + q];
            P[e] = v;
        }
        if (t == 0) a.n_iter[s] = it;
    }
};

// The LDS of a start is declared in the kernels, and `st` lives in them: with either inside a function both kernels call, the
// unweighted instantiations no longer get the registers they had (rank 14: 382 VGPRs for 168).
#define PM_START_LDS                       \
    __shared__ double red[MS_THREADS];     \
    __shared__ double sys[PM_SYS_BYTES / 8]; \
    __shared__ double small[5 * R * R];

template <int R, class XL>
__global__ __launch_bounds__(MS_THREADS) void k_ms_pf2als(PmArgs a) {
    PM_START_LDS
    Pf2Start<R, XL, false> st;
    st.bind(a, red, sys, small);
    st.fit(a, nullptr);
}

// slab_scale: fp64 [gridDim.x, I]; job blockIdx.x reads its own row and nothing of its neighbours'
template <int R, class XL>
__global__ __launch_bounds__(MS_THREADS) void k_ms_pf2als_weighted(PmArgs a, const double *slab_scale) {
    PM_START_LDS
    Pf2Start<R, XL, true> st;
    st.bind(a, red, sys, small);
    st.fit(a, slab_scale + (int64_t)blockIdx.x * a.I);
}
#undef PM_START_LDS

std::string pm_check(const int64_t *row_ptr, int64_t I, int64_t K, int32_t rank, int32_t n_starts) {
    const std::string bad = packed_args_error(row_ptr, I, K, rank, PM_MAX_RANK);
    if (!bad.empty()) return bad;
    if (n_starts < 1) return "need n_starts >= 1";
    return packed_rows_error(row_ptr, I, K, rank, 31);
}

StartsPlan pm_plan(void *workspace, const int64_t *row_ptr, int64_t I, int64_t K, int rank, int32_t n_starts) {
    return starts_plan(workspace, row_ptr, I, pm_scratch(I, row_ptr[I], K, rank).total, n_starts);
}

// mcl_pf2als_multistart_run (weighted false, slab_scale unused) and mcl_pf2als_multistart_run_weighted
int pm_run(const char *who, bool weighted, const double *slab_scale, const void *X, int32_t x_type, const int64_t *row_ptr, int64_t I,
           int64_t K, int32_t rank, int32_t n_starts, int32_t n_iter_max, int32_t n_iter_parafac, double tol, double absolute_tol,
           int32_t nn_modes, double *factors, double *P, double *errors, int32_t *n_iter, void *workspace, int64_t workspace_bytes,
           void *hip_stream) {
    ErrorSlot &fail = g_pm_error.named(who);
    const std::string bad = pm_check(row_ptr, I, K, rank, n_starts);
    if (!bad.empty()) return fail(bad);
    if (weighted && !slab_scale) return fail("slab_scale is NULL (a device array [n_starts, I] of the square roots of the weights)");
    if (!X || !factors || !P || !n_iter || !workspace || (tol > 0.0 && !errors)) return fail("NULL argument");
    if (!x_type_error(x_type).empty()) return fail(x_type_error(x_type));
    if (nn_modes & ~5) return fail("nn_modes may hold modes 0 and 2 only (bits 1 and 4)");
    if (n_iter_max < 1 || n_iter_parafac < 1 || !(tol >= 0.0) || !(absolute_tol >= 0.0))
        return fail("need n_iter_max >= 1, n_iter_parafac >= 1, tol >= 0 and absolute_tol >= 0");
    const StartsPlan p = pm_plan(workspace, row_ptr, I, K, rank, n_starts);
    if (workspace_refused(fail, workspace, workspace_bytes, p.total, "mcl_pf2als_multistart_workspace_bytes")) return 1;
    hipStream_t s = reinterpret_cast<hipStream_t>(hip_stream);
    std::vector<int32_t> slab;
    if (upload_starts(p, row_ptr, I, slab, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess) return fail("upload of row_ptr failed");
    PmArgs a{};
    a.X = X;
    a.row_ptr = p.row_ptr;
    a.slab_of_row = p.slab_of_row;
    a.I = I, a.N = p.N, a.K = K;
    a.scratch_len = pm_scratch(I, p.N, K, rank).total;
    a.factors = factors, a.P = P, a.errors = tol > 0.0 ? errors : nullptr;
    a.scratch = p.scratch;
    a.n_iter = n_iter;
    a.n_iter_max = n_iter_max, a.n_iter_parafac = n_iter_parafac, a.nn_modes = nn_modes;
    a.tol = tol, a.absolute_tol = absolute_tol;
    mcl_x_dispatch(x_type, [&](auto xl) {
        using XL = decltype(xl);
        rank_exact<PM_MAX_RANK>(rank, [&](auto rc) {
            constexpr int R = decltype(rc)::value;
            if (weighted) hipLaunchKernelGGL((k_ms_pf2als_weighted<R, XL>), dim3(n_starts), dim3(MS_THREADS), 0, s, a, slab_scale);
            else hipLaunchKernelGGL((k_ms_pf2als<R, XL>), dim3(n_starts), dim3(MS_THREADS), 0, s, a);
        });
        return 0;
    });
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(std::string("launch failed: ") + hipGetErrorString(e));
    return 0;
}

}  // namespace

extern "C" {

const char *mcl_pf2als_multistart_last_error(void) { return g_pm_error.c_str(); }

int64_t mcl_pf2als_multistart_workspace_bytes(const int64_t *row_ptr, int64_t I, int64_t K, int32_t rank, int32_t n_starts) {
    if (!pm_check(row_ptr, I, K, rank, n_starts).empty()) return -1;
    return pm_plan(nullptr, row_ptr, I, K, rank, n_starts).total;
}

int mcl_pf2als_multistart_run(const void *X, int32_t x_type, const int64_t *row_ptr, int64_t I, int64_t K, int32_t rank, int32_t n_starts,
                              int32_t n_iter_max, int32_t n_iter_parafac, double tol, double absolute_tol, int32_t nn_modes,
                              double *factors, double *P, double *errors, int32_t *n_iter, void *workspace, int64_t workspace_bytes,
                              void *hip_stream) {
    return pm_run("mcl_pf2als_multistart_run: ", false, nullptr, X, x_type, row_ptr, I, K, rank, n_starts, n_iter_max, n_iter_parafac, tol,
                  absolute_tol, nn_modes, factors, P, errors, n_iter, workspace, workspace_bytes, hip_stream);
}

int mcl_pf2als_multistart_run_weighted(const void *X, int32_t x_type, const int64_t *row_ptr, int64_t I, int64_t K, int32_t rank,
                                       int32_t n_starts, const double *slab_scale, int32_t n_iter_max, int32_t n_iter_parafac, double tol,
                                       double absolute_tol, int32_t nn_modes, double *factors, double *P, double *errors, int32_t *n_iter,
                                       void *workspace, int64_t workspace_bytes, void *hip_stream) {
    return pm_run("mcl_pf2als_multistart_run_weighted: ", true, slab_scale, X, x_type, row_ptr, I, K, rank, n_starts, n_iter_max,
                  n_iter_parafac, tol, absolute_tol, nn_modes, factors, P, errors, n_iter, workspace, workspace_bytes, hip_stream);
}

}  // extern "C"
