// parafac2_als (decomposition.py): unconstrained PARAFAC2-ALS (TensorLy's parafac2, restated in tests/parafac2_als_restatement.py)
// for data resident in HBM.  Model X_i ~ P_i B diag(a_i) C^T with P_i^T P_i = I; A [I, r], B [r, r], C [K, r] kept in fp64.
//
// One iteration:
//   pass 1 (X):  W = X C on the fp32 MFMA (k_pf2als_xc: xc_segment of cp_passes.h, which alsinit.hip runs too)
//   per slab:    WtW_i = W_i^T W_i, G_i = B D_i WtW_i D_i B^T, T_i = D_i B^T G_i^-1/2 (cyclic Jacobi, eigenvalues <= 1e-12 lam_max
//                dropped), P_i^T P_i = T_i^T WtW_i T_i, all fp64 (k_pf2als_polar); the projection is P_i = W_i T_i
//   pass 2 (X):  Y_i = T_i^T (W_i^T X_i) [r, K], W_i^T X_i on the fp32 MFMA (xtw_segments of cp_passes.h), the rest fp64
//                (k_pf2als_y); Y is stored [I][K][r]
//   n_iter_parafac CP sweeps on the I x r x K tensor Y, modes A, B, C (ALS normal equations, or one HALS column pass for the
//   modes in nn_modes), five launches per sweep:
//     k_pf2als_ab    V_i = Y_i C, M_A[i] = diag(B^T V_i), A[i] <- update; partials of A^T A and M_B = sum_i V_i diag(a_i)
//     k_pf2als_b     (one workgroup) A^T A, M_B; B <- update; B^T B; the next system G_C = A^T A o B^T B
//     k_pf2als_mc    partials of M_C = sum_i Y_i^T B diag(a_i) per slab group
//     k_pf2als_c     M_C rows; C <- update; fp32 fragments of C; partials of C^T C and <M_C, C>
//     k_pf2als_prep  (one workgroup) C^T C, <M_C, C>; the next system G_A = B^T B o C^T C
//   error (tol > 0): e^2 = (|X|^2 - 2 <M_C, C> + sum_i sum((D_i B^T P_i^T P_i B D_i) o C^T C)) / |X|^2 (k_pf2als_fit, k_pf2als_err);
//   k_pf2als_err also evaluates the stopping rule and raises the device stop flag that gates every launch of the iteration.
// Every reduction has a fixed order and no float atomics are used: two runs are bitwise equal.  The r x r inverse, the row update
// and the fixed-order sum of partials are cp_passes.h's as well.
#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "cp_passes.h"

namespace {

static ErrorSlot g_pf2als_error{"mcl_parafac2_als: "};
constexpr int PA_BLOCK = 16;   // iterations enqueued between two reads of the stop flag
constexpr int PA_MAX_RANK = 32;

// ---- |X|^2: per-slab partials (threads strided over the slab's elements, then a fixed tree) --------------------------------------
template <class XL>
__global__ __launch_bounds__(256) void k_pf2als_norm(const typename XL::T *__restrict__ X, const int *__restrict__ ext, int K,
                                                     double *__restrict__ nxp) {
    __shared__ double red[256];
    const int i = blockIdx.x, tid = threadIdx.x;
    const long b = (long)ext[i] * K, n = (long)(ext[i + 1] - ext[i]) * K;
    double s = 0.0;
    for (long e = tid; e < n; e += 256) {
        const double x = (double)XL::ld1(X + b + e);
        s = fma(x, x, s);
    }
    red[tid] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) red[tid] += red[tid + o];
        __syncthreads();
    }
    if (tid == 0) nxp[i] = red[0];
}

// ---- pass 1: W = X C -------------------------------------------------------------------------------------------------------
// One wave per segment (xc_segment, cp_passes.h); the epilogue stores the rows of W.
template <class XL, int NB, bool VEC>
__global__ __launch_bounds__(256) void k_pf2als_xc(const typename XL::T *__restrict__ X, const int4 *__restrict__ segs, int nseg, int K, int r,
                                                   const float *__restrict__ Cfrag, float *__restrict__ W, const int *__restrict__ gate) {
    if (*gate) return;
    __shared__ f32x4 tiles[4][16 * 16];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, seg = blockIdx.x * 4 + w;
    if (seg >= nseg) return;  // whole waves; no barrier below
    const int4 sg = segs[seg];
    const int row0 = sg.y, n = sg.z;
    const int row16 = lane & 15, g = lane >> 4;
    f32x4 acc[4][NB];
    xc_segment<XL, NB, VEC>(X, sg, K, Cfrag, tiles[w], acc);
#pragma unroll
    for (int rb = 0; rb < 4; ++rb) {
        const int loc = 16 * rb + row16;
        if (loc >= n) continue;
#pragma unroll
        for (int hp = 0; hp < NB; ++hp)
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int q = 16 * hp + 4 * g + v;
                if (q < r) W[(long)(row0 + loc) * r + q] = acc[rb][hp][v];
            }
    }
}

// ---- per slab: WtW_i, G_i, Jacobi, T_i, P_i^T P_i (one workgroup per slab) -------------------------------------------------------
template <int RMAX>
__global__ __launch_bounds__(256) void k_pf2als_polar(const float *__restrict__ W, const int *__restrict__ ext, int r,
                                                      const double *__restrict__ A64, const double *__restrict__ B64,
                                                      double *__restrict__ Tout, double *__restrict__ PtP, const int *__restrict__ gate) {
    if (*gate) return;
    constexpr int RR = RMAX * RMAX, NE = (RR + 255) / 256;
    __shared__ float Ws[64][RMAX + 1];
    __shared__ double WtW[RR], Bs[RR], H[RR], S[RR], V[RR], cs[RMAX + 2], a[RMAX];
    const int i = blockIdx.x, tid = threadIdx.x, rr = r * r;
    const int s0 = ext[i], n = ext[i + 1] - s0;
    for (int e = tid; e < rr; e += 256) Bs[e] = B64[e];
    if (tid < r) a[tid] = A64[(long)i * r + tid];
    double acc[NE];
#pragma unroll
    for (int u = 0; u < NE; ++u) acc[u] = 0.0;
    for (int j0 = 0; j0 < n; j0 += 64) {
        const int cnt = min(64, n - j0);
        __syncthreads();
        for (int e = tid; e < cnt * r; e += 256) {
            const int jj = e / r, q = e - jj * r;
            Ws[jj][q] = W[(long)(s0 + j0 + jj) * r + q];
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < NE; ++u) {
            const int e = tid + 256 * u;
            if (e >= rr) continue;
            const int p = e / r, q = e - p * r;
            double s = acc[u];
            for (int jj = 0; jj < cnt; ++jj) s = fma((double)Ws[jj][p], (double)Ws[jj][q], s);
            acc[u] = s;
        }
    }
#pragma unroll
    for (int u = 0; u < NE; ++u)
        if (tid + 256 * u < rr) WtW[tid + 256 * u] = acc[u];
    __syncthreads();
    // H = (D WtW D) B^T: H[p][y] = sum_q a_p a_q WtW[p][q] B[y][q]
    for (int e = tid; e < rr; e += 256) {
        const int p = e / r, y = e - p * r;
        double s = 0.0;
        for (int q = 0; q < r; ++q) s = fma(a[p] * a[q] * WtW[p * r + q], Bs[y * r + q], s);
        H[e] = s;
    }
    __syncthreads();
    // G = B H, symmetrised
    for (int e = tid; e < rr; e += 256) {
        const int x = e / r, y = e - x * r;
        double s = 0.0;
        for (int p = 0; p < r; ++p) s = fma(Bs[x * r + p], H[p * r + y], s);
        V[e] = s;
    }
    __syncthreads();
    for (int e = tid; e < rr; e += 256) {
        const int x = e / r, y = e - x * r;
        S[e] = 0.5 * (V[x * r + y] + V[y * r + x]);
    }
    __syncthreads();
    jacobi_lds(S, V, cs, r);
    double lmax = 0.0;
    for (int k = 0; k < r; ++k) lmax = fmax(lmax, S[k * r + k]);
    // H = G^-1/2 on the kept eigenvalues
    for (int e = tid; e < rr; e += 256) {
        const int x = e / r, y = e - x * r;
        double s = 0.0;
        for (int k = 0; k < r; ++k) {
            const double l = S[k * r + k];
            if (l > 0.0 && l > 1e-12 * lmax) s += V[x * r + k] * V[y * r + k] / sqrt(l);
        }
        H[e] = s;
    }
    __syncthreads();
    // T = D B^T H: T[p][q] = a_p sum_s B[s][p] H[s][q]  (into V)
    for (int e = tid; e < rr; e += 256) {
        const int p = e / r, q = e - p * r;
        double s = 0.0;
        for (int x = 0; x < r; ++x) s = fma(Bs[x * r + p], H[x * r + q], s);
        V[e] = a[p] * s;
        Tout[(long)i * rr + e] = a[p] * s;
    }
    __syncthreads();
    // P^T P = T^T (WtW T): S = WtW T, then T^T S
    for (int e = tid; e < rr; e += 256) {
        const int p = e / r, q = e - p * r;
        double s = 0.0;
        for (int u = 0; u < r; ++u) s = fma(WtW[p * r + u], V[u * r + q], s);
        S[e] = s;
    }
    __syncthreads();
    for (int e = tid; e < rr; e += 256) {
        const int x = e / r, y = e - x * r;
        double s = 0.0;
        for (int p = 0; p < r; ++p) s = fma(V[p * r + x], S[p * r + y], s);
        PtP[(long)i * rr + e] = s;
    }
}

// ---- pass 2: Y_i = T_i^T (W_i^T X_i), one workgroup per (slab, 64-column block) ---------------------------------------------------
// xtw_segments (cp_passes.h) over the slab's segments with the weights W[row][q] (fp32, exact).  The four waves' fixed-order fp64
// sum fills Z [64][r] (LDS); then Y[i][k][q] = sum_p T_i[p][q] Z[k][p].
template <class XL, int NB, bool VEC>
__global__ __launch_bounds__(256) void k_pf2als_y(const typename XL::T *__restrict__ X, const int4 *__restrict__ segs,
                                                  const int *__restrict__ slab_seg, int K, int r, const float *__restrict__ W,
                                                  const double *__restrict__ Tm, double *__restrict__ Y, const int *__restrict__ gate) {
    if (*gate) return;
    constexpr int RMAX = 16 * NB;
    __shared__ float red[3][NB * 16][64];
    __shared__ double Zs[64][RMAX + 1], Ts[RMAX * RMAX];
    const int tid = threadIdx.x, c16 = tid & 15, i = blockIdx.x, kb = blockIdx.y;
    for (int e = tid; e < r * r; e += 256) Ts[e] = Tm[(long)i * r * r + e];
    f32x4 acc[4][NB];
    float wn[4][NB];
    auto wload = [&](const int4 sg, const int(&loc)[4]) {
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) wn[u][nb] = W[(long)(sg.y + loc[u]) * r + min(16 * nb + c16, r - 1)];
    };
    xtw_segments<XL, NB, VEC>(X, segs, slab_seg[i], slab_seg[i + 1], K, r, kb, wload, [&](int u, int nb) { return wn[u][nb]; }, acc);
    xtw_wave_sum<NB>(acc, red, [&](int kl, int q, double s) { Zs[kl][q] = s; });
    __syncthreads();
    for (int e = tid; e < 64 * r; e += 256) {
        const int kl = e / r, q = e - kl * r, k = 64 * kb + kl;
        if (k >= K) continue;
        double s = 0.0;
        for (int p = 0; p < r; ++p) s = fma(Ts[p * r + q], Zs[kl][p], s);
        Y[((long)i * K + k) * r + q] = s;
    }
}

// ---- mode A (+ the M_B partials): one wave per slab, slabs lo + w, lo + w + 4, ... of the workgroup's group ----------------------
// Lane (qb = l >> 3, sb = l & 7) holds the RMAX/8 x RMAX/8 block V[qb * BQ + x][sb * BQ + y] of V_i = Y_i C.
template <int RMAX>
__global__ __launch_bounds__(256) void k_pf2als_ab(const double *__restrict__ Y, const double *__restrict__ C64, double *__restrict__ A64,
                                                   const double *__restrict__ B64, const double *__restrict__ Gm, int I, int K, int r,
                                                   int ngrp, int hals, double *__restrict__ Pab, const int *__restrict__ gate) {
    if (*gate) return;
    constexpr int BQ = RMAX / 8, RR = RMAX * RMAX;
    __shared__ double Gs[RR], Bs[RR], Vs[4][RR], ms[4][RMAX], as[4][RMAX];
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, rr = r * r;
    const int qb = lane >> 3, sb = lane & 7;
    const int lo = (int)((long)I * blockIdx.x / ngrp), hi = (int)((long)I * (blockIdx.x + 1) / ngrp);
    for (int e = tid; e < rr; e += 256) Gs[e] = Gm[e], Bs[e] = B64[e];
    double mb[BQ][BQ], ata[BQ][BQ];
#pragma unroll
    for (int x = 0; x < BQ; ++x)
#pragma unroll
        for (int y = 0; y < BQ; ++y) mb[x][y] = 0.0, ata[x][y] = 0.0;
    __syncthreads();
    for (int base = lo; base < hi; base += 4) {
        const int i = base + w;
        const bool act = i < hi;
        double v[BQ][BQ];
#pragma unroll
        for (int x = 0; x < BQ; ++x)
#pragma unroll
            for (int y = 0; y < BQ; ++y) v[x][y] = 0.0;
        if (act) {
            const double *Yi = Y + (long)i * K * r;
#pragma unroll 8
            for (int k = 0; k < K; ++k) {  // (unrolled: eight iterations' loads in flight)
                double yq[BQ], cs[BQ];
#pragma unroll
                for (int x = 0; x < BQ; ++x) {
                    const int q = qb * BQ + x;
                    yq[x] = q < r ? Yi[(long)k * r + q] : 0.0;
                    cs[x] = sb * BQ + x < r ? C64[(long)k * r + sb * BQ + x] : 0.0;
                }
#pragma unroll
                for (int x = 0; x < BQ; ++x)
#pragma unroll
                    for (int y = 0; y < BQ; ++y) v[x][y] = fma(yq[x], cs[y], v[x][y]);
            }
#pragma unroll
            for (int x = 0; x < BQ; ++x)
#pragma unroll
                for (int y = 0; y < BQ; ++y) {
                    const int q = qb * BQ + x, s = sb * BQ + y;
                    if (q < r && s < r) Vs[w][q * r + s] = v[x][y];
                }
        }
        __syncthreads();
        if (act && lane < r) {  // M_A[i][s] = sum_q B[q][s] V[q][s]
            double m = 0.0;
            for (int q = 0; q < r; ++q) m = fma(Bs[q * r + lane], Vs[w][q * r + lane], m);
            ms[w][lane] = m;
        }
        __syncthreads();
        if (act && (hals ? lane == 0 : lane < r)) {
            double m[RMAX], f[RMAX];
#pragma unroll
            for (int q = 0; q < RMAX; ++q) m[q] = q < r ? ms[w][q] : 0.0, f[q] = q < r ? A64[(long)i * r + q] : 0.0;
            factor_row_update<RMAX>(m, f, Gs, r, hals);
            if (hals) {
#pragma unroll
                for (int q = 0; q < RMAX; ++q)
                    if (q < r) as[w][q] = f[q];
            } else {
                double fl = 0.0;
#pragma unroll
                for (int q = 0; q < RMAX; ++q)
                    if (q == lane) fl = f[q];
                as[w][lane] = fl;
            }
        }
        __syncthreads();
        if (act) {
            if (lane < r) A64[(long)i * r + lane] = as[w][lane];
#pragma unroll
            for (int x = 0; x < BQ; ++x)
#pragma unroll
                for (int y = 0; y < BQ; ++y) {
                    const int q = qb * BQ + x, s = sb * BQ + y;
                    if (q < r && s < r) {
                        mb[x][y] = fma(as[w][s], v[x][y], mb[x][y]);
                        ata[x][y] = fma(as[w][q], as[w][s], ata[x][y]);
                    }
                }
        }
        __syncthreads();
    }
    // the partials of the four waves, (w0 + w1) + (w2 + w3): A^T A, then M_B (through Vs)
    for (int h = 0; h < 2; ++h) {
#pragma unroll
        for (int x = 0; x < BQ; ++x)
#pragma unroll
            for (int y = 0; y < BQ; ++y) {
                const int q = qb * BQ + x, s = sb * BQ + y;
                if (q < r && s < r) Vs[w][q * r + s] = h ? mb[x][y] : ata[x][y];
            }
        __syncthreads();
        for (int e = tid; e < rr; e += 256) Pab[((long)blockIdx.x * 2 + h) * rr + e] = (Vs[0][e] + Vs[1][e]) + (Vs[2][e] + Vs[3][e]);
        __syncthreads();
    }
}

// ---- mode B (one workgroup): A^T A and M_B from the partials, B <- update, B^T B, the system of mode C ------------------------------
template <int RMAX>
__global__ __launch_bounds__(1024) void k_pf2als_b(const double *__restrict__ Pab, int ngrp, int r, int hals_c,
                                                   double *__restrict__ B64, double *__restrict__ Gram, double *__restrict__ Gm,
                                                   const int *__restrict__ gate) {
    if (*gate) return;
    constexpr int RR = RMAX * RMAX;
    __shared__ double sums[2 * RR], S[RR], Wj[RR], cs[RMAX + 2], Bn[RR], red[1024];
    const int tid = threadIdx.x, rr = r * r;
    fixed_order_sum<1024>(Pab, ngrp, 2 * rr, 2 * rr, sums, red);  // sums = [A^T A | M_B]
    for (int e = tid; e < rr; e += 1024) {
        Gram[e] = sums[e];
        S[e] = sums[e] * Gram[2 * rr + e];  // G_B = A^T A o C^T C
    }
    __syncthreads();
    spd_inverse_lds<1024>(S, Wj, cs, r, [&](int e) { return sums[e] * Gram[2 * rr + e]; });  // (mode B is never non-negative: ALS)
    for (int e = tid; e < rr; e += 1024) {  // B[q][s] = sum_p M_B[q][p] G_B^-1[p][s]
        const int q = e / r, c = e - q * r;
        double t = 0.0;
        for (int p = 0; p < r; ++p) t = fma(sums[rr + q * r + p], S[p * r + c], t);
        Bn[e] = t;
    }
    __syncthreads();
    for (int e = tid; e < rr; e += 1024) {
        B64[e] = Bn[e];
        const int a = e / r, c = e - a * r;
        double s = 0.0;
        for (int q = 0; q < r; ++q) s = fma(Bn[q * r + a], Bn[q * r + c], s);
        Gram[rr + e] = s;
        S[e] = sums[e] * s;  // G_C = A^T A o B^T B
    }
    __syncthreads();
    if (!hals_c) spd_inverse_lds<1024>(S, Wj, cs, r, [&](int e) { return sums[e] * Gram[rr + e]; });
    for (int e = tid; e < rr; e += 1024) Gm[e] = S[e];
}

// ---- mode C right-hand sides: Pc[g][k][s] = sum over the slabs of group g (ascending) of sum_q Y[i][k][q] B[q][s] a_i[s] ------------
// Workgroup (64-row block kb, group g); thread (kl = tid >> 2, sb = tid & 3) holds the entries s = sb * RMAX/4 + y of row kl.
template <int RMAX>
__global__ __launch_bounds__(256) void k_pf2als_mc(const double *__restrict__ Y, const double *__restrict__ A64, const double *__restrict__ B64,
                                                   int I, int K, int r, int ngrp, double *__restrict__ Pc, const int *__restrict__ gate) {
    if (*gate) return;
    constexpr int SB = RMAX / 4;
    __shared__ double Bs[RMAX * RMAX], Us[RMAX][RMAX];
    const int tid = threadIdx.x, kl = tid >> 2, sb = tid & 3, kb = blockIdx.x, g = blockIdx.y, k = 64 * kb + kl;
    const int lo = (int)((long)I * g / ngrp), hi = (int)((long)I * (g + 1) / ngrp);
    for (int e = tid; e < r * r; e += 256) Bs[e] = B64[e];
    double acc[SB];
#pragma unroll
    for (int y = 0; y < SB; ++y) acc[y] = 0.0;
    for (int i = lo; i < hi; ++i) {
        __syncthreads();
        for (int e = tid; e < RMAX * RMAX; e += 256) {
            const int q = e / RMAX, s = e - q * RMAX;
            Us[q][s] = (q < r && s < r) ? Bs[q * r + s] * A64[(long)i * r + s] : 0.0;
        }
        __syncthreads();
        if (k < K) {
            const double *Yk = Y + ((long)i * K + k) * r;
#pragma unroll 8
            for (int q = 0; q < r; ++q) {
                const double yq = Yk[q];
#pragma unroll
                for (int y = 0; y < SB; ++y) acc[y] = fma(yq, Us[q][sb * SB + y], acc[y]);
            }
        }
    }
    if (k < K)
#pragma unroll
        for (int y = 0; y < SB; ++y) {
            const int s = sb * SB + y;
            if (s < r) Pc[((long)g * K + k) * r + s] = acc[y];
        }
}

// ---- mode C: rows of C (RPW = 256 / RMAX per workgroup, thread (row, s)) -------------------------------------------------------
// M_C[k][s] = the partials in group order; ALS: thread (row, s) forms f[s] = M_C[k] Gm[:, s], HALS: thread (row, 0) walks the columns.
template <int RMAX>
__global__ __launch_bounds__(256) void k_pf2als_c(const double *__restrict__ Pc, int ngrp, int K, int r, int NB, int hals,
                                                  const double *__restrict__ Gm, double *__restrict__ C64, float *__restrict__ Cfrag,
                                                  double *__restrict__ Pcc, double *__restrict__ Pdot, const int *__restrict__ gate) {
    if (*gate) return;
    constexpr int RPW = 256 / RMAX;
    __shared__ double Gs[RMAX * RMAX], Ms[RPW][RMAX], Fs[RPW][RMAX], Ds[RPW][RMAX];
    const int tid = threadIdx.x, row = tid / RMAX, s = tid - row * RMAX, k = blockIdx.x * RPW + row, rr = r * r;
    const bool ok = k < K && s < r;
    for (int e = tid; e < rr; e += 256) Gs[e] = Gm[e];
    double m = 0.0;
    if (ok)
        for (int g = 0; g < ngrp; ++g) m += Pc[((long)g * K + k) * r + s];
    Ms[row][s] = m;
    Fs[row][s] = ok ? C64[(long)k * r + s] : 0.0;
    __syncthreads();
    double fnew = 0.0;
    if (k < K && (hals ? s == 0 : s < r)) {
        double mv[RMAX], f[RMAX];
#pragma unroll
        for (int q = 0; q < RMAX; ++q) mv[q] = Ms[row][q], f[q] = Fs[row][q];
        factor_row_update<RMAX>(mv, f, Gs, r, hals);
        if (hals) {
#pragma unroll
            for (int q = 0; q < RMAX; ++q)
                if (q < r) Fs[row][q] = f[q];
        } else {
#pragma unroll
            for (int q = 0; q < RMAX; ++q)
                if (q == s) fnew = f[q];
        }
    }
    __syncthreads();
    if (!hals && ok) Fs[row][s] = fnew;
    __syncthreads();
    Ds[row][s] = ok ? m * Fs[row][s] : 0.0;
    if (ok) {
        const double f = Fs[row][s];
        C64[(long)k * r + s] = f;
        Cfrag[cfrag_index(k, s, NB)] = (float)f;
    }
    __syncthreads();
    for (int e = tid; e < rr; e += 256) {
        const int a = e / r, c = e - a * r;
        double t = 0.0;
        for (int w = 0; w < RPW; ++w) t = fma(Fs[w][a], Fs[w][c], t);
        Pcc[(long)blockIdx.x * rr + e] = t;
    }
    if (tid == 0) {  // <M_C, C> of the block: rows in order, then columns
        double t = 0.0;
        for (int w = 0; w < RPW; ++w)
            for (int q = 0; q < r; ++q) t += Ds[w][q];
        Pdot[blockIdx.x] = t;
    }
}

// ---- after mode C (one workgroup): C^T C, <M_C, C>, the system of mode A ---------------------------------------------------------
template <int RMAX>
__global__ __launch_bounds__(1024) void k_pf2als_prep(const double *__restrict__ Pcc, const double *__restrict__ Pdot, int nwg, int r,
                                                      int hals_a, double *__restrict__ Gram, double *__restrict__ Gm,
                                                      double *__restrict__ small, const int *__restrict__ gate) {
    if (*gate) return;
    constexpr int RR = RMAX * RMAX;
    __shared__ double ctc[RR], S[RR], Wj[RR], cs[RMAX + 2], red[1024];
    const int tid = threadIdx.x, rr = r * r;
    fixed_order_sum<1024>(Pcc, nwg, rr, rr, ctc, red);
    if (tid == 0) {
        double t = 0.0;
        for (int w = 0; w < nwg; ++w) t += Pdot[w];
        small[1] = t;
    }
    for (int e = tid; e < rr; e += 1024) {
        Gram[2 * rr + e] = ctc[e];
        S[e] = Gram[rr + e] * ctc[e];  // G_A = B^T B o C^T C
    }
    __syncthreads();
    if (!hals_a) spd_inverse_lds<1024>(S, Wj, cs, r, [&](int e) { return Gram[rr + e] * ctc[e]; });
    for (int e = tid; e < rr; e += 1024) Gm[e] = S[e];
}

// ---- the start (one workgroup): |X|^2, B^T B, C^T C, the fragments of C, the system of mode A, the stop flag and counters --------
template <int RMAX>
__global__ __launch_bounds__(1024) void k_pf2als_start(const double *__restrict__ nxp, int I, int K, int r, int NB, int hals_a,
                                                       const double *__restrict__ B64, const double *__restrict__ C64,
                                                       float *__restrict__ Cfrag, double *__restrict__ Gram, double *__restrict__ Gm,
                                                       double *__restrict__ small, int *__restrict__ gate) {
    constexpr int RR = RMAX * RMAX;
    __shared__ double S[RR], Wj[RR], cs[RMAX + 2];
    const int tid = threadIdx.x, rr = r * r;
    if (tid == 0) {
        double t = 0.0;
        for (int i = 0; i < I; ++i) t += nxp[i];
        small[0] = t, small[1] = 0.0, small[2] = 0.0;
        gate[0] = 0, gate[1] = 0;
    }
    for (long e = tid; e < (long)K * r; e += 1024) {
        const int k = (int)(e / r), s = (int)(e - (long)k * r);
        Cfrag[cfrag_index(k, s, NB)] = (float)C64[e];
    }
    for (int e = tid; e < rr; e += 1024) {
        const int a = e / r, c = e - a * r;
        double sb = 0.0, sc = 0.0;
        for (int q = 0; q < r; ++q) sb = fma(B64[q * r + a], B64[q * r + c], sb);
        for (int k = 0; k < K; ++k) sc = fma(C64[(long)k * r + a], C64[(long)k * r + c], sc);
        Gram[rr + e] = sb, Gram[2 * rr + e] = sc;
        S[e] = sb * sc;
    }
    __syncthreads();
    if (!hals_a) spd_inverse_lds<1024>(S, Wj, cs, r, [&](int e) { return Gram[rr + e] * Gram[2 * rr + e]; });
    for (int e = tid; e < rr; e += 1024) Gm[e] = S[e];
}

// ---- error: Pfit[g] = sum over the slabs of group g of a_i^T ((B^T P_i^T P_i B) o C^T C) a_i --------------------------------------
template <int RMAX>
__global__ __launch_bounds__(256) void k_pf2als_fit(const double *__restrict__ PtP, const double *__restrict__ A64, const double *__restrict__ B64,
                                                    const double *__restrict__ Gram, int I, int r, int ngrp, double *__restrict__ Pfit,
                                                    const int *__restrict__ gate) {
    if (*gate) return;
    constexpr int RR = RMAX * RMAX;
    __shared__ double Bs[RR], Cc[RR], Ps[RR], Tm[RR], Hs[RR], a[RMAX];
    const int tid = threadIdx.x, rr = r * r;
    const int lo = (int)((long)I * blockIdx.x / ngrp), hi = (int)((long)I * (blockIdx.x + 1) / ngrp);
    for (int e = tid; e < rr; e += 256) Bs[e] = B64[e], Cc[e] = Gram[2 * rr + e];
    double tot = 0.0;
    for (int i = lo; i < hi; ++i) {
        __syncthreads();
        for (int e = tid; e < rr; e += 256) Ps[e] = PtP[(long)i * rr + e];
        if (tid < r) a[tid] = A64[(long)i * r + tid];
        __syncthreads();
        for (int e = tid; e < rr; e += 256) {  // Tm = P^T P B
            const int p = e / r, s = e - p * r;
            double t = 0.0;
            for (int u = 0; u < r; ++u) t = fma(Ps[p * r + u], Bs[u * r + s], t);
            Tm[e] = t;
        }
        __syncthreads();
        for (int e = tid; e < rr; e += 256) {  // Hs = a_x a_s (B^T Tm)[x][s] C^T C[x][s]
            const int x = e / r, s = e - x * r;
            double t = 0.0;
            for (int p = 0; p < r; ++p) t = fma(Bs[p * r + x], Tm[p * r + s], t);
            Hs[e] = a[x] * a[s] * t * Cc[e];
        }
        __syncthreads();
        if (tid == 0)
            for (int e = 0; e < rr; ++e) tot += Hs[e];
    }
    if (tid == 0) Pfit[blockIdx.x] = tot;
}

// e_t and the stopping rule (one thread): stop after iteration t >= 1 when |e_{t-1}^2 - e_t^2| <= tol e_{t-1}^2 or e_t^2 < absolute_tol
__global__ void k_pf2als_err(const double *__restrict__ Pfit, int ngrp, int t, double tol, double absolute_tol, double *__restrict__ small,
                             double *__restrict__ errors, int *__restrict__ gate) {
    if (*gate || threadIdx.x != 0) return;
    double fit = 0.0;
    for (int g = 0; g < ngrp; ++g) fit += Pfit[g];
    const double nx2 = small[0], cross = small[1];
    const double e2 = nx2 > 0.0 ? fmax(0.0, nx2 - 2.0 * cross + fit) / nx2 : 0.0;
    errors[t] = sqrt(e2);
    const double prev = small[2];
    if (t >= 1 && (fabs(prev - e2) <= tol * prev || e2 < absolute_tol)) gate[0] = 1;
    small[2] = e2;
    gate[1] = t + 1;
}

// outputs in fp32: the projections P = W T (rows of X), A, B, C
__global__ __launch_bounds__(256) void k_pf2als_out(const float *__restrict__ W, const double *__restrict__ Tm, const double *__restrict__ A64,
                                                    const double *__restrict__ B64, const double *__restrict__ C64, const int *__restrict__ ext,
                                                    int I, int N, int K, int r, float *__restrict__ P, float *__restrict__ A,
                                                    float *__restrict__ B, float *__restrict__ C) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (blockIdx.y == 0) {
        if (e >= (long)N * r) return;
        const int row = (int)(e / r), q = (int)(e - (long)row * r);
        const double *T = Tm + (long)slab_of_row(ext, I, row) * r * r;
        double s = 0.0;
        for (int p = 0; p < r; ++p) s = fma((double)W[(long)row * r + p], T[p * r + q], s);
        P[e] = (float)s;
    } else if (blockIdx.y == 1) {
        if (e < (long)I * r) A[e] = (float)A64[e];
    } else if (blockIdx.y == 2) {
        if (e < (long)r * r) B[e] = (float)B64[e];
    } else {
        if (e < (long)K * r) C[e] = (float)C64[e];
    }
}

struct PaPlan {
    int64_t N;
    int nseg, nkb, NB, KH, RMAX, ngrp_ab, ngrp_mc, wgC;
    int4 *segs;
    int *slab_seg, *ext, *gate, *info;
    double *A, *B, *C, *T, *PtP, *Y, *Pab, *Pc, *Pcc, *Pdot, *Pfit, *nxp, *Gram, *Gm, *small;
    float *Cfrag, *W;
    char *scratch;
    int64_t svd_ws, total;
};

// workspace NULL: the parts are null and `total` is the size (mcl_parafac2_als_workspace_bytes)
PaPlan pa_plan(void *workspace, const int64_t *row_ptr, int64_t I, int64_t K, int rank) {
    PaPlan p{};
    p.N = row_ptr[I];
    const int64_t nseg = seg_count(row_ptr, I);
    const int64_t r = rank;
    p.nseg = (int)nseg;
    p.nkb = (int)((K + 63) / 64);
    p.NB = rank <= 16 ? 1 : 2;
    p.RMAX = 16 * p.NB;
    p.KH = 4 * p.nkb;
    p.ngrp_ab = (int)std::max<int64_t>(1, std::min<int64_t>(128, (I + 7) / 8));
    p.ngrp_mc = (int)std::max<int64_t>(1, std::min<int64_t>(I, std::max<int64_t>(1, 256 / p.nkb)));
    p.wgC = (int)((K + (256 / p.RMAX) - 1) / (256 / p.RMAX));
    WsCursor ws(workspace);
    p.segs = ws.take<int4>(std::max<int64_t>(nseg, 1) * 16);
    p.slab_seg = ws.take<int>((I + 1) * 4);
    p.ext = ws.take<int>((I + 1) * 4);
    p.A = ws.take<double>(I * r * 8);
    p.B = ws.take<double>(r * r * 8);
    p.C = ws.take<double>(K * r * 8);
    p.Cfrag = ws.take<float>((int64_t)p.KH * p.NB * 64 * 4 * 4);
    p.W = ws.take<float>(p.N * r * 4);
    p.T = ws.take<double>(I * r * r * 8);
    p.PtP = ws.take<double>(I * r * r * 8);
    p.Y = ws.take<double>(I * K * r * 8);
    p.Pab = ws.take<double>((int64_t)p.ngrp_ab * 2 * r * r * 8);
    p.Pc = ws.take<double>((int64_t)p.ngrp_mc * K * r * 8);
    p.Pcc = ws.take<double>((int64_t)p.wgC * r * r * 8);
    p.Pdot = ws.take<double>((int64_t)p.wgC * 8);
    p.Pfit = ws.take<double>((int64_t)p.ngrp_ab * 8);
    p.nxp = ws.take<double>(I * 8);
    p.Gram = ws.take<double>(3 * r * r * 8);
    p.Gm = ws.take<double>(r * r * 8);
    p.small = ws.take<double>(4 * 8);  // |X|^2, <M_C, C>, e_{t-1}^2
    p.gate = ws.take<int>(4 * 4);      // stop flag, iterations used
    p.info = ws.take<int>((I + 2) * 4);
    // the svd start: mcl_svd_init's workspace + C0 (fp32)
    p.svd_ws = (mcl_svd_stack_workspace_bytes(row_ptr, I, K, rank) + 255) & ~int64_t(255);
    p.scratch = ws.take<char>(p.svd_ws + K * r * 4);
    p.total = ws.off;
    return p;
}

template <class XL, int RMAX>
int pf2als_run(const typename XL::T *X, int32_t x_type, const int64_t *row_ptr, int64_t I, int64_t K, int32_t rank, const double *A0,
               const double *B0, const double *C0, int32_t n_iter_max, int32_t n_iter_parafac, double tol, double absolute_tol,
               int32_t nn_modes, float *A, float *B, float *C, float *P, double *errors, int32_t *info, const PaPlan &p, hipStream_t s) {
    constexpr int NB = RMAX / 16;
    auto fail = [](const std::string &msg) { return g_pf2als_error.as_is(msg); };  // (a HIP call's or the svd start's message)
    const int r = rank, N = (int)p.N;
    const bool hals_a = nn_modes & 1, hals_c = (nn_modes >> 2) & 1;

    const SegTables h = seg_tables(row_ptr, I);
    CP_HIP(upload_tables(h, p.segs, p.slab_seg, p.ext, s));
    CP_HIP(hipMemsetAsync(p.Cfrag, 0, (size_t)p.KH * p.NB * 64 * 4 * 4, s));
    CP_HIP(hipMemsetAsync(p.gate, 0, 4 * sizeof(int), s));
    CP_HIP(hipStreamSynchronize(s));  // (the tables are locals)

    // ---- start: the given factors, or A = 1, B = I, C = the C of mcl_svd_init
    if (A0) {
        CP_HIP(hipMemcpyAsync(p.A, A0, sizeof(double) * I * r, hipMemcpyDeviceToDevice, s));
        CP_HIP(hipMemcpyAsync(p.B, B0, sizeof(double) * r * r, hipMemcpyDeviceToDevice, s));
        CP_HIP(hipMemcpyAsync(p.C, C0, sizeof(double) * K * r, hipMemcpyDeviceToDevice, s));
    } else {
        float *C32 = reinterpret_cast<float *>(p.scratch + p.svd_ws);
        std::string err;
        if (mcl_svd_stack_right(X, x_type, row_ptr, I, K, rank, 0, C32, p.scratch, p.svd_ws, p.info, s, err)) return fail(err);
        std::vector<double> h_A((size_t)I * r, 1.0), h_B((size_t)r * r, 0.0);
        for (int q = 0; q < r; ++q) h_B[(size_t)q * r + q] = 1.0;
        CP_HIP(upload(p.A, h_A, s));
        CP_HIP(upload(p.B, h_B, s));
        std::vector<float> h_C((size_t)K * r);
        std::vector<double> h_C64((size_t)K * r);
        CP_HIP(hipMemcpyAsync(h_C.data(), C32, sizeof(float) * h_C.size(), hipMemcpyDeviceToHost, s));
        CP_HIP(hipStreamSynchronize(s));
        for (size_t e = 0; e < h_C.size(); ++e) h_C64[e] = (double)h_C[e];
        CP_HIP(upload(p.C, h_C64, s));
        CP_HIP(hipStreamSynchronize(s));  // (the host copies are locals)
    }
    hipLaunchKernelGGL(k_pf2als_norm<XL>, dim3((unsigned)I), dim3(256), 0, s, X, (const int *)p.ext, (int)K, p.nxp);
    hipLaunchKernelGGL(k_pf2als_start<RMAX>, dim3(1), dim3(1024), 0, s, (const double *)p.nxp, (int)I, (int)K, r, NB, (int)hals_a,
                       (const double *)p.B, (const double *)p.C, p.Cfrag, p.Gram, p.Gm, p.small, p.gate);
    CP_HIP(hipGetLastError());

    const bool vec = K % 4 == 0 && mcl_x_vec_aligned(X, x_type);
    auto pass = [&](bool second) {  // W = X C, or Y = T^T W^T X
        vec_dispatch(vec, [&](auto v) {
            constexpr bool VEC = decltype(v)::value;
            if (!second)
                hipLaunchKernelGGL((k_pf2als_xc<XL, NB, VEC>), dim3((unsigned)((p.nseg + 3) / 4)), dim3(256), 0, s, X, (const int4 *)p.segs, p.nseg,
                                   (int)K, r, (const float *)p.Cfrag, p.W, (const int *)p.gate);
            else
                hipLaunchKernelGGL((k_pf2als_y<XL, NB, VEC>), dim3((unsigned)I, (unsigned)p.nkb), dim3(256), 0, s, X, (const int4 *)p.segs,
                                   (const int *)p.slab_seg, (int)K, r, (const float *)p.W, (const double *)p.T, p.Y, (const int *)p.gate);
        });
    };
    const bool check = tol > 0.0;
    int used = n_iter_max;
    for (int t = 0; t < n_iter_max; ++t) {
        pass(false);
        hipLaunchKernelGGL(k_pf2als_polar<RMAX>, dim3((unsigned)I), dim3(256), 0, s, (const float *)p.W, (const int *)p.ext, r,
                           (const double *)p.A, (const double *)p.B, p.T, p.PtP, (const int *)p.gate);
        pass(true);
        for (int sw = 0; sw < n_iter_parafac; ++sw) {
            hipLaunchKernelGGL(k_pf2als_ab<RMAX>, dim3((unsigned)p.ngrp_ab), dim3(256), 0, s, (const double *)p.Y, (const double *)p.C, p.A,
                               (const double *)p.B, (const double *)p.Gm, (int)I, (int)K, r, p.ngrp_ab, (int)hals_a, p.Pab, (const int *)p.gate);
            hipLaunchKernelGGL(k_pf2als_b<RMAX>, dim3(1), dim3(1024), 0, s, (const double *)p.Pab, p.ngrp_ab, r, (int)hals_c, p.B, p.Gram, p.Gm,
                               (const int *)p.gate);
            hipLaunchKernelGGL(k_pf2als_mc<RMAX>, dim3((unsigned)p.nkb, (unsigned)p.ngrp_mc), dim3(256), 0, s, (const double *)p.Y,
                               (const double *)p.A, (const double *)p.B, (int)I, (int)K, r, p.ngrp_mc, p.Pc, (const int *)p.gate);
            hipLaunchKernelGGL(k_pf2als_c<RMAX>, dim3((unsigned)p.wgC), dim3(256), 0, s, (const double *)p.Pc, p.ngrp_mc, (int)K, r, NB, (int)hals_c,
                               (const double *)p.Gm, p.C, p.Cfrag, p.Pcc, p.Pdot, (const int *)p.gate);
            hipLaunchKernelGGL(k_pf2als_prep<RMAX>, dim3(1), dim3(1024), 0, s, (const double *)p.Pcc, (const double *)p.Pdot, p.wgC, r, (int)hals_a,
                               p.Gram, p.Gm, p.small, (const int *)p.gate);
        }
        if (check) {
            hipLaunchKernelGGL(k_pf2als_fit<RMAX>, dim3((unsigned)p.ngrp_ab), dim3(256), 0, s, (const double *)p.PtP, (const double *)p.A,
                               (const double *)p.B, (const double *)p.Gram, (int)I, r, p.ngrp_ab, p.Pfit, (const int *)p.gate);
            hipLaunchKernelGGL(k_pf2als_err, dim3(1), dim3(64), 0, s, (const double *)p.Pfit, p.ngrp_ab, t, tol, absolute_tol, p.small, errors, p.gate);
        }
        CP_HIP(hipGetLastError());
        if (check && ((t + 1) % PA_BLOCK == 0 || t + 1 == n_iter_max)) {  // the verdict, read in blocks: later launches are gated
            int g[2] = {0, 0};
            CP_HIP(hipMemcpyAsync(g, p.gate, sizeof(g), hipMemcpyDeviceToHost, s));
            CP_HIP(hipStreamSynchronize(s));
            used = g[1];
            if (g[0]) break;
        }
    }
    const long big = std::max<long>((long)N, std::max<long>((long)I, (long)K)) * r;
    hipLaunchKernelGGL(k_pf2als_out, dim3((unsigned)((big + 255) / 256), 4), dim3(256), 0, s, (const float *)p.W, (const double *)p.T,
                       (const double *)p.A, (const double *)p.B, (const double *)p.C, (const int *)p.ext, (int)I, N, (int)K, r, P, A, B, C);
    CP_HIP(hipGetLastError());
    CP_HIP(hipMemcpyAsync(info, &used, sizeof(int32_t), hipMemcpyHostToDevice, s));
    CP_HIP(hipStreamSynchronize(s));  // (`used` is a local)
    return 0;
}

std::string check_args(const int64_t *row_ptr, int64_t I, int64_t K, int32_t rank) {
    std::string bad = packed_args_error(row_ptr, I, K, rank, PA_MAX_RANK);
    if (bad.empty()) bad = packed_rows_error(row_ptr, I, K, rank, 26);  // rows x PA_MAX_RANK in 32 bits
    if (bad.empty() && I >= (int64_t(1) << 31) / 64) bad = "more than 2^25 matrices are not supported";
    return bad;
}

}  // namespace

extern "C" {

const char *mcl_parafac2_als_last_error(void) { return g_pf2als_error.c_str(); }

int64_t mcl_parafac2_als_workspace_bytes(const int64_t *row_ptr, int64_t I, int64_t K, int32_t rank) {
    if (!check_args(row_ptr, I, K, rank).empty()) return -1;
    return pa_plan(nullptr, row_ptr, I, K, rank).total;
}

int mcl_parafac2_als_typed(const void *X, int32_t x_type, const int64_t *row_ptr, int64_t I, int64_t K, int32_t rank, const double *A0,
                           const double *B0, const double *C0, int32_t n_iter_max, int32_t n_iter_parafac, double tol,
                           double absolute_tol, int32_t nn_modes, float *A, float *B, float *C, float *P, double *errors,
                           int32_t *info, void *workspace, int64_t workspace_bytes, void *hip_stream) {
    ErrorSlot &fail = g_pf2als_error;
    const std::string bad = check_args(row_ptr, I, K, rank);
    if (!bad.empty()) return fail(bad);
    if (!X || !A || !B || !C || !P || !info || !workspace || (tol > 0.0 && !errors)) return fail("NULL argument");
    if ((A0 || B0 || C0) && !(A0 && B0 && C0)) return fail("give all of A0, B0, C0 or none");
    if (!A0 && K > 2048) return fail("the svd start needs K <= 2048");
    if (!x_type_error(x_type).empty()) return fail(x_type_error(x_type));
    if (nn_modes & ~5) return fail("nn_modes may hold modes 0 and 2 only (bits 1 and 4)");
    if (n_iter_max < 1 || n_iter_parafac < 1 || !(tol >= 0.0) || !(absolute_tol >= 0.0))
        return fail("need n_iter_max >= 1, n_iter_parafac >= 1, tol >= 0 and absolute_tol >= 0");
    const PaPlan p = pa_plan(workspace, row_ptr, I, K, rank);
    if (workspace_refused(fail, workspace, workspace_bytes, p.total, "mcl_parafac2_als_workspace_bytes")) return 1;
    hipStream_t s = reinterpret_cast<hipStream_t>(hip_stream);
    return mcl_x_dispatch(x_type, [&](auto xl) {
        using XL = decltype(xl);
        return rank_bucket(rank, [&](auto rmax) {
            return pf2als_run<XL, decltype(rmax)::value>(static_cast<const typename XL::T *>(X), x_type, row_ptr, I, K, rank, A0, B0, C0,
                                                         n_iter_max, n_iter_parafac, tol, absolute_tol, nn_modes, A, B, C, P, errors, info, p, s);
        });
    });
}

}  // extern "C"
