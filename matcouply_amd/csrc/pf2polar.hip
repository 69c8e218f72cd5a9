// The PARAFAC2 penalty of mode 1 (penalties.py:1224-1250, 1280-1281) apart from its row passes: the polar factors per slab
// (Newton-Schulz on the fp64 MFMA, Jacobi and QR behind it), the cross-slab coordinate matrix, and the policy that chooses
// between the three routes.  rows.hip applies T_i to the rows (k_pf2_apply, or the fused finish pass) and updates the dual.
#include <string>

#include "rows_launch.h"

// ---------------------------------------------------------------------------------------------------------
// PARAFAC2 prox (mode 1):  Y_i = B_i + U_i,  P_i = polar(Y_i Delta^T),  Delta <- sum rho_i P_i^T Y_i / sum rho_i
// Gram route in fp64:  S_i = Y_i^T Y_i,  G_i = Delta S_i Delta^T = V L V^T,  W_i = V L^-1/2 V^T,
//                      T_i = Delta^T W_i,  P_i = Y_i T_i,  P_i^T Y_i = T_i^T S_i.
// ---------------------------------------------------------------------------------------------------------
typedef double f64x4 __attribute__((ext_vector_type(4)));

// S_i = Y_i^T Y_i on the fp64 MFMA (v_mfma_f64_16x16x4_f64): one workgroup per slab, lane (rsub = l>>4, c16 = l&15)
// reads Y[4g + rsub][16nb + c16] (256 contiguous bytes per wave-load for r = 16); fp32 x fp32 products are exact in
// fp64, so only the final rounding of the sums remains.  D layout of the f64 form: col = l&15, row = (l>>4) + 4 reg.
template <int NB>
__global__ __launch_bounds__(256) void k_pf2_gram(const int *__restrict__ ext, const float *__restrict__ F,
                                                  const float *__restrict__ U, int r, double *__restrict__ S) {
    constexpr int W = 16 * NB;
    __shared__ double sm[W * W];
    const int slab = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int rsub = lane >> 4, c16 = lane & 15;
    const int s = ext[slab], e = ext[slab + 1];
    const int n_groups = (e - s + 3) >> 2;
    f64x4 acc[NB][NB];
#pragma unroll
    for (int a = 0; a < NB; ++a)
#pragma unroll
        for (int b = 0; b < NB; ++b) acc[a][b] = f64x4{0.0, 0.0, 0.0, 0.0};
    for (int gq = wave; gq < n_groups; gq += 4) {
        const long j = (long)s + 4 * gq + rsub;
        double y[NB];
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
            const int col = 16 * nb + c16;
            // the EXACT sum of the two stored values (an fp32 sum would round Y by 6e-8: times cond(Y Delta^T) in the polar factor)
            y[nb] = (j < e && col < r) ? (double)F[j * r + col] + (double)U[j * r + col] : 0.0;
        }
#pragma unroll
        for (int a = 0; a < NB; ++a)
#pragma unroll
            for (int b = 0; b < NB; ++b) acc[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(y[a], y[b], acc[a][b], 0, 0, 0);
    }
    for (int wv = 0; wv < 4; ++wv) {
        if (wave == wv) {
#pragma unroll
            for (int a = 0; a < NB; ++a)
#pragma unroll
                for (int b = 0; b < NB; ++b)
#pragma unroll
                    for (int v = 0; v < 4; ++v) {
                        const int idx = (16 * a + rsub + 4 * v) * W + 16 * b + c16;
                        sm[idx] = (wv == 0) ? acc[a][b][v] : sm[idx] + acc[a][b][v];
                    }
        }
        __syncthreads();
    }
    for (int t = threadIdx.x; t < W * W; t += 256) {
        const int a = t / W, b = t - a * W;
        if (a < r && b < r) S[((long)slab * r + a) * r + b] = sm[t];
    }
}

// Synchronisation of ONE wave with itself around its LDS traffic.  The LDS operations of a wave are executed in the order
// they were issued, so a value written by one lane is there for the next read of another lane of the same wave: what is needed is
// that the compiler keeps that order.  (A workgroup barrier would also do in a one-wave workgroup - where the compiler drops it -
// but the Newton-Schulz kernel runs FOUR independent slabs per workgroup at rank <= 16, each wave on its own way through the
// fallbacks: a real barrier there would wait for waves that never come.)
static __device__ __forceinline__ void wave_sync_lds() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// One slab through the Jacobi route (one wave; `smd` = 4 r^2 + r doubles of LDS, `Ssrc` = the slab's S in any address
// space).  Called by the stand-alone kernel below and by k_pf2_algebra_ns for the slabs it cannot handle.
static __device__ void pf2_jacobi_slab(double *smd, const double *Ssrc, const float *__restrict__ Delta, double rh, int r,
                                       int slab, int lane, float *__restrict__ T, double *__restrict__ acc_out,
                                       double *__restrict__ T64 = nullptr, int *__restrict__ qr_flag = nullptr,
                                       bool full_rank_expected = false, const double *__restrict__ Delta64 = nullptr) {
    double *Sm = smd, *G = smd + r * r, *V = G + r * r, *lam = V + r * r, *D = lam + r;  // D: Delta in fp64 [r*r]
    const int n2 = r * r;
    for (int e = lane; e < n2; e += 64) {
        Sm[e] = Ssrc[e];
        D[e] = Delta64 != nullptr ? Delta64[e] : (double)Delta[e];  // (the fp64 state of wide.hip, or the caller's fp32 matrix)
        V[e] = ((e / r) == (e % r)) ? 1.0 : 0.0;
    }
    wave_sync_lds();
    // G = D S D^T  (via tmp = S D^T stored in V's place is not possible: V must stay I) -> two-step through lam-free loop
    for (int e = lane; e < n2; e += 64) {
        const int a = e / r, b = e - a * r;
        double sum = 0.0;
        for (int k = 0; k < r; ++k) {
            double inner = 0.0;
            for (int l = 0; l < r; ++l) inner += Sm[k * r + l] * D[b * r + l];
            sum += D[a * r + k] * inner;
        }
        G[e] = sum;
    }
    wave_sync_lds();
    // Jacobi eigen-decomposition of the symmetric G (fp64); V accumulates the eigenvectors.  Round 6: PARALLEL ordering - in
    // each of the n - 1 steps of a sweep the n / 2 disjoint index pairs of a round-robin tournament are rotated at once
    // (Brent-Luk), where rounds 2-5 walked the r (r - 1) / 2 pairs of a cyclic sweep one after the other: every rotation is two
    // barriers and a division / square-root chain (~1000 cycles), so a rank-16 matrix took ~1 M cycles - 436 us per call on the
    // 48-matrix problems of the exact arithmetic, 75 % of their iteration (rocprof, gpurun_out/r6).  A lane keeps ONE pair for the
    // whole step (its rotation computed redundantly by the lanes that share it, from the same LDS values: identical bits), applies
    // it to its rows of G J and V J, then to its columns of J^T (G J).
    {
        const int n = r + (r & 1);      // an odd rank plays with a bye (index r)
        const int npairs = n >> 1;
        int P = 1;
        while (P < npairs) P <<= 1;     // lanes per row group: pair i = lane % P (P <= 32 for rank <= 64)
        const int pi = lane % P, kstep = 64 / P, k0 = lane / P;
        for (int sweep = 0; sweep < 30; ++sweep) {
            double off = 0.0, dg = 0.0;
            for (int e = lane; e < n2; e += 64) {
                const int a = e / r, b = e - a * r;
                if (a == b) dg += G[e] * G[e];
                else off += G[e] * G[e];
            }
            off = wave_sum_d(off);
            dg = wave_sum_d(dg);
            if (off <= 1e-30 * dg) break;
            for (int st = 0; st < n - 1; ++st) {
                // the pair of this lane in step st: (n - 1, st) for i = 0, ((st + i) mod (n - 1), (st - i) mod (n - 1)) otherwise
                int p = -1, q = -1;
                if (pi < npairs) {
                    int a = pi == 0 ? n - 1 : (st + pi) % (n - 1), b = pi == 0 ? st : (st - pi + (n - 1)) % (n - 1);
                    p = min(a, b), q = max(a, b);
                    if (q >= r) p = -1;  // the bye
                }
                wave_sync_lds();
                double cs = 1.0, sn = 0.0, dpp = 0.0, dqq = 0.0;
                bool rot = false;
                if (p >= 0) {
                    const double apq = G[p * r + q], app = G[p * r + p], aqq = G[q * r + q];
                    if (fabs(apq) > 1e-300) {
                        const double tau = (aqq - app) / (2.0 * apq);
                        const double tt = (tau >= 0.0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(1.0 + tau * tau));
                        cs = 1.0 / sqrt(1.0 + tt * tt), sn = tt * cs;
                        dpp = app - tt * apq, dqq = aqq + tt * apq;
                        rot = true;
                    }
                }
                wave_sync_lds();
                if (rot)  // columns p, q of G and V:  X <- X J
                    for (int k = k0; k < r; k += kstep) {
                        const double gkp = G[k * r + p], gkq = G[k * r + q], vkp = V[k * r + p], vkq = V[k * r + q];
                        G[k * r + p] = cs * gkp - sn * gkq, G[k * r + q] = sn * gkp + cs * gkq;
                        V[k * r + p] = cs * vkp - sn * vkq, V[k * r + q] = sn * vkp + cs * vkq;
                    }
                wave_sync_lds();
                if (rot)  // rows p, q of G:  G <- J^T G
                    for (int k = k0; k < r; k += kstep) {
                        const double gpk = G[p * r + k], gqk = G[q * r + k];
                        G[p * r + k] = cs * gpk - sn * gqk, G[q * r + k] = sn * gpk + cs * gqk;
                    }
                wave_sync_lds();
                if (rot && k0 == 0) {  // the rotated 2 x 2 block in closed form (exact zero off the diagonal)
                    G[p * r + p] = dpp, G[q * r + q] = dqq;
                    G[p * r + q] = 0.0, G[q * r + p] = 0.0;
                }
            }
            wave_sync_lds();
        }
    }
    wave_sync_lds();
    double lmax = 0.0, lmin = 1e300;
    for (int k = 0; k < r; ++k) lmax = fmax(lmax, G[k * r + k]), lmin = fmin(lmin, G[k * r + k]);
    // G = (Y Delta^T)^T (Y Delta^T) squares the condition number: beyond cond(Y Delta^T) ~ 1e5 its small eigenvalues are
    // rounding (at 1e7 the pseudo-inverse threshold below removes them and the factor comes out rank-deficient: errors of
    // 0.2 in P, tools/parity_probe.py fuzz:133).  A slab with at least r rows is flagged for k_pf2_polar_qr, which works on
    // Y Delta^T itself; what is written below is then overwritten.
    if (qr_flag != nullptr && lane == 0) qr_flag[slab] = (full_rank_expected && !(lmin > 1e-10 * lmax)) ? 2 : 0;
    if (lane < r) {
        const double l = G[lane * r + lane];
        lam[lane] = (l > 1e-14 * lmax && l > 0.0) ? 1.0 / sqrt(l) : 0.0;  // pseudo-inverse square root
    }
    wave_sync_lds();
    // W = V diag(lam) V^T -> G
    for (int e = lane; e < n2; e += 64) {
        const int a = e / r, b = e - a * r;
        double sum = 0.0;
        for (int k = 0; k < r; ++k) sum += V[a * r + k] * lam[k] * V[b * r + k];
        G[e] = sum;
    }
    wave_sync_lds();
    // T = D^T W -> V
    for (int e = lane; e < n2; e += 64) {
        const int a = e / r, b = e - a * r;
        double sum = 0.0;
        for (int k = 0; k < r; ++k) sum += D[k * r + a] * G[k * r + b];
        V[e] = sum;
    }
    wave_sync_lds();
    for (int e = lane; e < n2; e += 64) {
        const int a = e / r, b = e - a * r;
        double sum = 0.0;
        for (int k = 0; k < r; ++k) sum += V[k * r + a] * Sm[k * r + b];
        acc_out[(long)slab * (n2 + 1) + e] = rh * sum;
        T[(long)slab * n2 + e] = (float)V[e];
        if (T64 != nullptr) T64[(long)slab * n2 + e] = V[e];
    }
    if (lane == 0) acc_out[(long)slab * (n2 + 1) + n2] = rh;
}

// Is a Gram matrix on which Newton-Schulz converged too ill-conditioned for the Gram route?  zn = ||(G / tr)^-1/2||_F^2 =
// sum_i tr / lambda_i bounds cond(G) from both sides, zn / r^2 <= cond(G) <= zn; the middle, zn / r, is held against the 1e10 of
// the Jacobi route's test.  A slab flagged here goes to the QR route, which is exact at any conditioning; a well-conditioned
// one (cond(Y Delta^T) <= 1e5 / sqrt(r) whatever its spectrum) never is.
static __device__ __forceinline__ bool pf2_ill_conditioned(double zn, int r) { return zn >= 1e10 * r; }

__global__ __launch_bounds__(64) void k_pf2_algebra(const double *__restrict__ S, const float *__restrict__ Delta,
                                                    const float *__restrict__ rho, int r, float *__restrict__ T,
                                                    double *__restrict__ acc_out, int *__restrict__ status, int use_status,
                                                    double *__restrict__ T64, const int *__restrict__ ext,
                                                    const double *__restrict__ Delta64 = nullptr,
                                                    const float *__restrict__ xmin_est = nullptr) {
    extern __shared__ double smd[];
    // use_status: entries <= 0 were done by the Newton-Schulz kernel (-iterations); this kernel leaves 2 (k_pf2_polar_qr takes
    // the slab) or 0 in the entry of every slab it handles.  xmin_est (rank 32): a slab on which Newton-Schulz converged although
    // the estimate 1 / ||Z||_F it left says that the Gram matrix is too ill-conditioned for the Gram route is flagged as well
    // (its factor stands until the QR kernel has redone it)
    if (use_status && status[blockIdx.x] <= 0) {
        if (xmin_est != nullptr && threadIdx.x == 0) {
            const double est = (double)xmin_est[blockIdx.x];
            if (est > 0.0 && pf2_ill_conditioned(1.0 / (est * est), r)) status[blockIdx.x] = 2;
        }
        return;
    }
    const int slab = blockIdx.x;
    pf2_jacobi_slab(smd, S + (long)slab * r * r, Delta, (double)rho[slab], r, slab, threadIdx.x, T, acc_out, T64, status,
                    ext[slab + 1] - ext[slab] >= r, Delta64);
}

// ---------------------------------------------------------------------------------------------------------
// Polar factor of an ill-conditioned slab without squaring its condition number (the slabs k_pf2_algebra flags with 2):
//   A = Y_i Delta^T (J_i x r, fp64, Y_i = F + U exactly)  ->  Householder QR in place  ->  R (r x r)
//   ->  one-sided Jacobi on the columns of R (Hestenes): R V = U Sigma  ->  (A^T A)^-1/2 = V Sigma^-1 V^T = W
//   ->  T_i = Delta^T W,  acc_i = rho_i T_i^T S   (what pf2_jacobi_slab writes, decomposition of penalties.py:1224-1250's SVD)
// R inherits the singular values of A to eps * cond relative accuracy (the Gram route: eps * cond^2), the one-sided Jacobi
// keeps it.  One workgroup per flagged slab; rare by construction (cond >= 1e5: typically the first inner iteration from a
// random dual), so simplicity beats speed: the reflections are applied column-parallel, the rotations by one wave.
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_pf2_polar_qr(const int *__restrict__ ext, const float *__restrict__ F,
                                                      const float *__restrict__ U, const float *__restrict__ Delta,
                                                      const float *__restrict__ rho, int r, const double *__restrict__ S,
                                                      const int *__restrict__ status, double *__restrict__ Aws,
                                                      float *__restrict__ T, double *__restrict__ acc_out,
                                                      double *__restrict__ T64, const int *__restrict__ gate,
                                                      const double *__restrict__ F64 = nullptr, const double *__restrict__ U64 = nullptr,
                                                      const double *__restrict__ Delta64 = nullptr) {
    MCL_GATE(gate);
    const int slab = blockIdx.x;
    if (status[slab] != 2) return;
    const int s = ext[slab], n = ext[slab + 1] - s;
    if (n < r) return;  // (never flagged)
    extern __shared__ double sq[];
    const int n2 = r * r;
    double *D = sq, *R = D + n2, *V = R + n2, *red = V + n2, *lam = red + 4 * 64;  // red: 4 row chunks x 64 columns
    __shared__ double sh_alpha, sh_beta, sh_vkk;
    const int tid = threadIdx.x, lane = tid & 63, chunk = tid >> 6;
    for (int e = tid; e < n2; e += 256) D[e] = Delta64 != nullptr ? Delta64[e] : (double)Delta[e];
    __syncthreads();
    double *A = Aws + (long)s * r;
    for (long idx = tid; idx < (long)n * r; idx += 256) {
        const long j = idx / r;
        const int c = (int)(idx - j * r);
        double acc = 0.0;
        if (F64 != nullptr) {  // the fp64 state of wide.hip
            const double *f = F64 + ((long)s + j) * r, *u = U64 + ((long)s + j) * r;
            for (int k = 0; k < r; ++k) acc = fma(f[k] + u[k], D[c * r + k], acc);
        } else {
            const float *f = F + ((long)s + j) * r, *u = U + ((long)s + j) * r;
            for (int k = 0; k < r; ++k) acc = fma((double)f[k] + (double)u[k], D[c * r + k], acc);
        }
        A[idx] = acc;
    }
    __syncthreads();
    for (int k = 0; k < r; ++k) {
        // ||A[k:n, k]||^2
        double p = 0.0;
        for (int j = k + tid; j < n; j += 256) p = fma(A[(long)j * r + k], A[(long)j * r + k], p);
        p = wave_sum_d(p);
        if (lane == 0) red[chunk] = p;
        __syncthreads();
        if (tid == 0) {
            const double nrm2 = (red[0] + red[1]) + (red[2] + red[3]);
            const double xk = A[(long)k * r + k];
            const double alpha = -copysign(sqrt(nrm2), xk);
            const double vkk = xk - alpha;
            const double vtv = (nrm2 - xk * xk) + vkk * vkk;
            sh_alpha = alpha, sh_vkk = vkk, sh_beta = vtv > 0.0 ? 2.0 / vtv : 0.0;
        }
        __syncthreads();
        const double vkk = sh_vkk, beta = sh_beta;
        // w_c = beta v^T A[k:n, c] for the columns c > k: thread (chunk, lane) sums rows k + chunk, k + chunk + 4, ... of column k + 1 + lane
        for (int c0 = k + 1; c0 < r; c0 += 64) {
            const int c = c0 + lane;
            double dot = 0.0;
            if (c < r)
                for (int j = k + chunk; j < n; j += 4) {
                    const double vj = (j == k) ? vkk : A[(long)j * r + k];
                    dot = fma(vj, A[(long)j * r + c], dot);
                }
            red[chunk * 64 + lane] = dot;
            __syncthreads();
            if (c < r) {
                const double w = beta * ((red[lane] + red[64 + lane]) + (red[128 + lane] + red[192 + lane]));
                for (int j = k + chunk; j < n; j += 4) {
                    const double vj = (j == k) ? vkk : A[(long)j * r + k];
                    A[(long)j * r + c] = fma(-vj, w, A[(long)j * r + c]);
                }
            }
            __syncthreads();
        }
        if (tid == 0) A[(long)k * r + k] = sh_alpha;  // row k of A now holds row k of R
        __syncthreads();
    }
    for (int e = tid; e < n2; e += 256) {
        const int a = e / r, b = e - a * r;
        R[e] = (b >= a) ? A[(long)a * r + b] : 0.0;
        V[e] = (a == b) ? 1.0 : 0.0;
    }
    __syncthreads();
    if (chunk == 0) {  // one wave: lane i owns row i of R and of V (r <= 64)
        const bool act = lane < r;
        const int i = act ? lane : 0;
        for (int sweep = 0; sweep < 40; ++sweep) {
            int rotated = 0;
            for (int pc = 0; pc < r - 1; ++pc)
                for (int qc = pc + 1; qc < r; ++qc) {
                    const double rp = act ? R[i * r + pc] : 0.0, rq = act ? R[i * r + qc] : 0.0;
                    const double al = wave_sum_d(rp * rp), be = wave_sum_d(rq * rq), ga = wave_sum_d(rp * rq);
                    if (fabs(ga) > 1e-15 * sqrt(al * be) && ga != 0.0) {  // wave-uniform
                        const double zeta = (be - al) / (2.0 * ga);
                        const double tt = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                        const double cs = 1.0 / sqrt(1.0 + tt * tt), sn = cs * tt;
                        if (act) {
                            R[i * r + pc] = cs * rp - sn * rq;
                            R[i * r + qc] = sn * rp + cs * rq;
                            const double vp = V[i * r + pc], vq = V[i * r + qc];
                            V[i * r + pc] = cs * vp - sn * vq;
                            V[i * r + qc] = sn * vp + cs * vq;
                        }
                        rotated = 1;
                    }
                }
            if (!rotated) break;
        }
        double smax = 0.0;
        for (int c = 0; c < r; ++c) {
            const double rc = act ? R[i * r + c] : 0.0;
            const double sg = sqrt(wave_sum_d(rc * rc));
            if (lane == 0) lam[c] = sg;
            smax = fmax(smax, sg);
        }
        if (act) lam[lane] = (lam[lane] > 1e-14 * smax && lam[lane] > 0.0) ? 1.0 / lam[lane] : 0.0;  // pseudo-inverse
    }
    __syncthreads();
    // W = V diag(lam) V^T -> R;  T = D^T W -> V's place is still needed for W, so T goes to the red-free part of A's first rows?  no:
    // r x r results fit the LDS arrays in turn: W -> R, then T -> D is NOT possible (T needs D): T -> A (global scratch, n >= r rows)
    for (int e = tid; e < n2; e += 256) {
        const int a = e / r, b = e - a * r;
        double sum = 0.0;
        for (int k = 0; k < r; ++k) sum = fma(V[a * r + k] * lam[k], V[b * r + k], sum);
        R[e] = sum;
    }
    __syncthreads();
    for (int e = tid; e < n2; e += 256) {
        const int a = e / r, b = e - a * r;
        double sum = 0.0;
        for (int k = 0; k < r; ++k) sum = fma(D[k * r + a], R[k * r + b], sum);
        V[e] = sum;  // T = Delta^T W
    }
    __syncthreads();
    const double rh = (double)rho[slab];
    const double *Sm = S + (long)slab * n2;
    for (int e = tid; e < n2; e += 256) {
        const int a = e / r, b = e - a * r;
        double sum = 0.0;
        for (int k = 0; k < r; ++k) sum = fma(V[k * r + a], Sm[k * r + b], sum);
        acc_out[(long)slab * (n2 + 1) + e] = rh * sum;
        T[(long)slab * n2 + e] = (float)V[e];
        if (T64 != nullptr) T64[(long)slab * n2 + e] = V[e];
    }
    if (tid == 0) acc_out[(long)slab * (n2 + 1) + n2] = rh;
}

// ---------------------------------------------------------------------------------------------------------
// PARAFAC2 r x r algebra on the fp64 MFMA (one wave per slab), replacing the Jacobi eigen-solver in the common case:
//   G = Delta S Delta^T,  s = tr G,  Newton-Schulz:  Y_0 = G/s, Z_0 = I,  T = (3I - Z Y)/2,  Y <- Y T,  Z <- T Z
//   -> Z = (G/s)^-1/2,  W = Z / sqrt(s),  T_i = Delta^T W,  acc_i = rho_i T_i^T S.
// The D layout of v_mfma_f64_16x16x4_f64 (lane l, reg v: row = (l>>4) + 4v, col = l&15) is directly the B-operand
// layout (B[k = (l>>4) + 4 step][n = l&15], step = v) and, read as an A operand (A[i = l&15][k = (l>>4) + 4 step]),
// supplies the TRANSPOSE: two accumulator-layout matrices M1, M2 give M1^T M2 with no data movement.  The iterates
// are symmetric only up to rounding, and treating them as exactly symmetric destabilises Newton-Schulz for
// cond(G) > ~1e3; so every iterate is carried together with its transpose (Y, Yt, Z, Zt) and both are advanced with
// the products that are available (6 small matmuls per iteration) - stable up to cond(G) ~ 1e11 (tools/ check).
// status[slab] = 1 if the iteration did not converge (rank-deficient / extremely ill-conditioned Y_i Delta^T, or
// J_i < r): those slabs are redone by k_pf2_algebra (Jacobi, pseudo-inverse square root).
// ---------------------------------------------------------------------------------------------------------
template <int NB>
struct SymTiles {
    f64x4 t[NB][NB];
};

// C = A^T B for A and B in D layout; result in D layout
template <int NB>
static __device__ __forceinline__ void mm_t(const SymTiles<NB> &A, const SymTiles<NB> &B, SymTiles<NB> &C) {
#pragma unroll
    for (int a = 0; a < NB; ++a)
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            f64x4 acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int kb = 0; kb < NB; ++kb)
#pragma unroll
                for (int st = 0; st < 4; ++st)
                    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(A.t[kb][a][st], B.t[kb][b][st], acc, 0, 0, 0);
            C.t[a][b] = acc;
        }
}

// At = A^T for a matrix in D layout, through a wave-private LDS area of (16 NB) x (16 NB + 1) doubles (the kernel runs ONE wave
// per workgroup; LDS operations of a wave complete in order, so consecutive transposes need no barrier).  Round 3: the
// Newton-Schulz iteration used to carry every iterate WITH its transpose and advance both by matrix products (6 per step);
// the fp64 matrix pipe is what bounds the kernel (one v_mfma_f64_16x16x4_f64 per 143 cycles and wave, 44 TFLOP/s for the
// whole part: tools/mfma64_rate.hip), so the transposes now cost 8 NB^2 LDS operations instead of 4 NB^3 MFMAs each.
template <int NB>
static __device__ __forceinline__ void tr_lds(const SymTiles<NB> &A, SymTiles<NB> &At, double *W, int q, int c16) {
    constexpr int LD = 16 * NB + 1;
#pragma unroll
    for (int a = 0; a < NB; ++a)
#pragma unroll
        for (int b = 0; b < NB; ++b)
#pragma unroll
            for (int v = 0; v < 4; ++v) W[(16 * a + q + 4 * v) * LD + 16 * b + c16] = A.t[a][b][v];
#pragma unroll
    for (int a = 0; a < NB; ++a)
#pragma unroll
        for (int b = 0; b < NB; ++b)
#pragma unroll
            for (int v = 0; v < 4; ++v) At.t[a][b][v] = W[(16 * b + c16) * LD + 16 * a + q + 4 * v];
}

// TILES: the per-tile statistics of the solve pass (k_rows_solve_stats / k_rows_finish_solve_stats) are summed HERE, in
// k_stats_reduce's order - S_i goes to LDS (and to S for the Jacobi fallback), the L2-ball column sums to colsq - which
// saves the separate reduction launch in front of this kernel in every inner iteration.
struct TileStats {
    const int *slab_tile_ptr;
    const double *stat_gram, *stat_colsq;
    double *colsq;
    int W, n_slabs;
};
// -DMCL_NS_STAMPS (tools/ns_stamps.py; never in the shipped library): s_memtime stamps of the kernel's sections per slab -
// [0] entry, [1] statistics summed, [2] G formed, [3] iteration done, [4] exit, [5] steps - in the scratch of pf2_acc's tail
#ifdef MCL_NS_STAMPS
#define NS_STAMP(i) do { if (lane == 0) stamps[(long)slab * 8 + (i)] = (long long)__builtin_readcyclecounter(); } while (0)
#else
#define NS_STAMP(i) do { } while (0)
#endif
// Slabs per workgroup.  Rank <= 16 (config 4: 1024 slabs = one per SIMD, the kernel lasts as long as its slowest slab): FOUR, one
// wave each.  The waves of a workgroup are placed on the four SIMDs of its CU in turn, whereas the SIMD of a one-wave workgroup is
// the dispatcher's choice - and with 4 such workgroups per CU it put two Newton-Schulz waves on one SIMD for 140 of 1024 slabs
// (in-kernel HW_ID stamps, tools/ns_stamps.py: 70 SIMDs with two waves, 70 idle), where two fp64-MFMA chains run 1.3-1.5 x
// slower each (2520 against 1900 cycles per step; tools/ns_valu_probe.hip: 1355 -> 1980 for the bare step).
template <int NB>
struct NsShape {
    static constexpr int SPW = NB == 1 ? 4 : 1;
};
template <int NB, bool TILES>
__global__ __launch_bounds__(64 * NsShape<NB>::SPW + ((TILES && NB == 1) ? 64 : 0)) __attribute__((amdgpu_waves_per_eu(2))) void k_pf2_algebra_ns(double *__restrict__ S, const float *__restrict__ Delta,
                                                       const float *__restrict__ rho, const int *__restrict__ ext, int r,
                                                       float *__restrict__ T, double *__restrict__ acc_out,
                                                       int *__restrict__ status, TileStats ts, RegSet regs,
                                                       float *__restrict__ xmin_est, int scaled, double *__restrict__ T64) {
    MCL_GATE(regs.gate);
    // S_i while the system is formed (TILES), then the scratch of the LDS transposes (the epilogue re-reads S_i from memory)
    constexpr int SPW = NsShape<NB>::SPW;
    __shared__ double Ssm_w[SPW][(16 * NB) * (16 * NB + 1)];
    __shared__ float Dsm_w[SPW][256 * NB * NB];
    // rank <= 16: the Jacobi route of a slab this iteration cannot handle runs right here (8 KB of LDS; saves the launch of
    // the stand-alone kernel in every inner iteration); rank 32 would need 33 KB and lose a wave per CU, so those slabs are
    // left to k_pf2_algebra (status = 1)
    constexpr bool INK = NB == 1;
    __shared__ double Jsm_w[INK ? SPW : 1][INK ? 4 * 256 + 16 : 1];
    const int wave = SPW == 1 ? 0 : (int)(threadIdx.x >> 6), lane = threadIdx.x & 63;
    // (the column-sum wave has its own slabs below)
    const int slab = SPW == 1 ? (int)blockIdx.x : min((int)blockIdx.x * SPW + (wave < SPW ? wave : 0), ts.n_slabs - 1);
    auto &Ssm = Ssm_w[wave < SPW ? wave : 0];
    // scratch of the LDS transposes.  Rank <= 16: an area of its own, so that S_i stays in LDS for the epilogue's T^T S (its re-read
    // from memory was a round trip at the end of every slab's chain); rank 32 has no LDS to spare (8 workgroups per CU) and uses
    // S_i's area once U1 has consumed it
    __shared__ double Wsm_w[NB == 1 ? SPW : 1][NB == 1 ? 16 * 17 : 1];
    double *Wtr;
    if constexpr (NB == 1) Wtr = Wsm_w[wave < SPW ? wave : 0];
    else Wtr = Ssm;
    auto &Dsm = Dsm_w[wave < SPW ? wave : 0];
    auto &Jsm = Jsm_w[(INK && wave < SPW) ? wave : 0];
    const int q = lane >> 4, c16 = lane & 15;
    const int n2 = r * r;
    const double *Ss = S + (long)slab * n2;
    // The L2-ball column sums of the slab's tiles, in k_stats_reduce's order: two more memory round trips.  Rank <= 16 (one
    // slab per SIMD at config 4: the chain's latency is the kernel's duration): a SECOND wave takes them and is done; rank 32
    // (register-bound at two waves per SIMD: a second wave would halve the resident slabs) keeps them in front of the chain.
    // (round 6: that wave is the FIFTH of the workgroup and takes the column sums of its four slabs, 16 lanes each)
    constexpr bool COLSQ_WAVE = TILES && NB == 1;
    if (TILES && (COLSQ_WAVE ? wave == SPW : true)) {
        const int cslab = COLSQ_WAVE ? blockIdx.x * SPW + (lane >> 4) : slab;
        const bool cs_ok = cslab < ts.n_slabs;
        const int t0 = cs_ok ? ts.slab_tile_ptr[cslab] : 0, t1 = cs_ok ? ts.slab_tile_ptr[cslab + 1] : 0;
        for (int k = 0; k < regs.n; ++k) {
            if (regs.kind[k] != MCL_PEN_L2BALL) continue;
            for (int col = COLSQ_WAVE ? (lane & 15) : lane; col < r; col += (COLSQ_WAVE ? 16 : 64)) {
                double sq = 0.0;
                for (int tb = t0; tb < t1; tb += 8) {  // ascending order, 8 loads in flight
                    double v[8];
#pragma unroll
                    for (int u = 0; u < 8; ++u) v[u] = ts.stat_colsq[((long)min(tb + u, t1 - 1) * MCL_MAX_REGS + k) * r + col];
#pragma unroll
                    for (int u = 0; u < 8; ++u)
                        if (tb + u < t1) sq += v[u];
                }
                if (cs_ok) ts.colsq[((long)k * ts.n_slabs + cslab) * r + col] = sq;
            }
        }
        if (COLSQ_WAVE) return;
    }
    if (SPW > 1 && (int)blockIdx.x * SPW + wave >= ts.n_slabs) return;  // the last workgroup's spare waves (nothing below is a workgroup barrier)
#ifdef MCL_NS_STAMPS
    long long *stamps = reinterpret_cast<long long *>(xmin_est + ts.n_slabs);  // the plan reserves 8 int64 per slab behind pf2_xmin
#endif
    NS_STAMP(0);
#ifdef MCL_NS_STAMPS  // where the wave runs: HW_REG_HW_ID (wave, SIMD, CU, SH, SE) and HW_REG_XCC_ID
    if (lane == 0) {
        stamps[(long)slab * 8 + 6] = (long long)__builtin_amdgcn_s_getreg((31 << 11) | 4);
        stamps[(long)slab * 8 + 7] = (long long)__builtin_amdgcn_s_getreg((31 << 11) | 20);
    }
#endif
    // everything this wave needs besides the statistics is requested up front, so its latency overlaps the tile loop:
    // the slab's extent and weight, and Delta (staged in LDS; every product below reads it from there)
    const int slab_rows = ext[slab + 1] - ext[slab];
    const double rh = (double)rho[slab];
    {
        float dv[4 * NB * NB];
#pragma unroll
        for (int m = 0; m < 4 * NB * NB; ++m) dv[m] = Delta[min(lane + 64 * m, n2 - 1)];
#pragma unroll
        for (int m = 0; m < 4 * NB * NB; ++m)
            if (lane + 64 * m < n2) Dsm[lane + 64 * m] = dv[m];
    }
    if (TILES) {
        const int t0 = ts.slab_tile_ptr[slab], t1 = ts.slab_tile_ptr[slab + 1];
        const long WW = (long)ts.W * ts.W;
        // the order of k_stats_reduce (even tile offsets -> s0, odd -> s1, ascending), tiles fetched TB at a time with
        // independent clamped loads (one memory latency per batch instead of one per tile)
        constexpr int EPL = 4 * NB * NB, TB = NB == 1 ? 16 : 2;  // elements per lane (n2 <= 256 NB^2); register budget
        // (rank <= 16: a slab of <= 1024 rows is ONE batch - one memory round trip instead of two in front of the chain)
        double s0[EPL], s1[EPL];
        long off[EPL];
#pragma unroll
        for (int m = 0; m < EPL; ++m) {
            const int e = min(lane + 64 * m, n2 - 1);
            const int a = e / r, b = e - a * r;
            off[m] = (long)a * ts.W + b;
            s0[m] = 0.0, s1[m] = 0.0;
        }
        for (int tb = t0; tb < t1; tb += TB) {
            double v[TB][EPL];
#pragma unroll
            for (int u = 0; u < TB; ++u)
#pragma unroll
                for (int m = 0; m < EPL; ++m) v[u][m] = ts.stat_gram[min(tb + u, t1 - 1) * WW + off[m]];
#pragma unroll
            for (int u = 0; u < TB; ++u)
                if (tb + u < t1) {
#pragma unroll
                    for (int m = 0; m < EPL; ++m) {
                        if (((tb + u - t0) & 1) == 0) s0[m] += v[u][m];
                        else s1[m] += v[u][m];
                    }
                }
        }
#pragma unroll
        for (int m = 0; m < EPL; ++m) {
            const int e = lane + 64 * m;
            if (e < n2) {
                Ssm[e] = s0[m] + s1[m];
                S[(long)slab * n2 + e] = s0[m] + s1[m];
            }
        }
    }
    if constexpr (SPW == 1) __syncthreads();  // (a one-wave workgroup: the compiler drops the barrier instruction)
    else wave_sync_lds();
    NS_STAMP(1);
    auto Sat = [&](int i, int j) -> double {
        if (TILES) return (i < r && j < r) ? Ssm[i * r + j] : 0.0;
        return (i < r && j < r) ? Ss[i * r + j] : 0.0;
    };
    auto Dat = [&](int i, int j) -> double { return (i < r && j < r) ? (double)Dsm[i * r + j] : 0.0; };
    const double *Sany = TILES ? static_cast<const double *>(Ssm) : Ss;
    if (slab_rows < r) {  // fewer rows than columns: rank-deficient by construction
        if (lane == 0) status[slab] = 1;
        if (INK) pf2_jacobi_slab(Jsm, Sany, Delta, rh, r, slab, lane, T, acc_out, T64);
        return;
    }
    // U1 = S Delta^T   (A = S, symmetric: A[i][k] = S[k][i];  B[k][n] = Delta[n][k])
    SymTiles<NB> U1, G;
#pragma unroll
    for (int a = 0; a < NB; ++a)
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            f64x4 acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int kb = 0; kb < NB; ++kb)
#pragma unroll
                for (int st = 0; st < 4; ++st) {
                    const int k = 16 * kb + q + 4 * st;
                    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(Sat(k, 16 * a + c16), Dat(16 * b + c16, k), acc, 0, 0, 0);
                }
            U1.t[a][b] = acc;
        }
    // G = Delta U1 (A[i][k] = Delta[i][k];  B = U1 in D layout)  and  Gt = G^T = U1^T Delta^T (A = U1 as A-operand,
    // B[k][n] = Delta[n][k])
    SymTiles<NB> Gt;
    double tr = 0.0;
#pragma unroll
    for (int a = 0; a < NB; ++a)
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            f64x4 acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int kb = 0; kb < NB; ++kb)
#pragma unroll
                for (int st = 0; st < 4; ++st) {
                    const int k = 16 * kb + q + 4 * st;
                    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(Dat(16 * a + c16, k), U1.t[kb][b][st], acc, 0, 0, 0);
                }
            G.t[a][b] = acc;
            if (a == b) {
#pragma unroll
                for (int v = 0; v < 4; ++v)
                    if (q + 4 * v == c16 && 16 * a + c16 < r) tr += acc[v];
            }
        }
    tr = wave_sum_d(tr);
    tr_lds<NB>(G, Gt, Wtr, q, c16);  // G^T (S_i has been consumed by U1: its LDS copy is free; the fallbacks below read memory)
    if (!(tr > 0.0)) {
        if (lane == 0) status[slab] = 1;
        if (INK) pf2_jacobi_slab(Jsm, Ss, Delta, rh, r, slab, lane, T, acc_out, T64, status, true);  // may flag the slab (2)
        return;
    }
    NS_STAMP(2);
    // Newton-Schulz for the inverse square root of G / tr (padding rows/cols >= r carry the identity)
    SymTiles<NB> Y, Yt, Z, Zt, P, Pt, Tm, Tmt, N1, N2, N3, N4;
    const double inv_s = 1.0 / tr;
#pragma unroll
    for (int a = 0; a < NB; ++a)
#pragma unroll
        for (int b = 0; b < NB; ++b)
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int row = 16 * a + q + 4 * v, col = 16 * b + c16;
                const double id = (row == col) ? 1.0 : 0.0;
                const bool in = (row < r && col < r);
                Y.t[a][b][v] = in ? G.t[a][b][v] * inv_s : id;
                Yt.t[a][b][v] = in ? Gt.t[a][b][v] * inv_s : id;
                Z.t[a][b][v] = id;
                Zt.t[a][b][v] = id;
            }
    bool converged = false;
    double prev = 1e300;
    int it_used = 0;
    // Scaled iteration: with x = sqrt(eig(Z Y)) in [lo, hi] the step T = a I - b Z Y maps x to x (a - b x^2); (a, b) are
    // the minimax coefficients of that cubic on [lo, hi] (equi-oscillation at lo, sqrt(s/3), hi; (1.5, 0.5) when lo = hi = 1),
    // which roughly doubles the growth of the small eigenvalues per step (2.6 x instead of 1.5 x) and so halves the
    // iteration count.  hi = 1 holds by the trace scaling; lo starts from the estimate 1 / ||Z||_F left by the previous
    // call for this slab (the matrices change slowly between inner iterations; 1e-2 when there is none).  An eigenvalue
    // below the assumed lo still grows by a every step (the cubic is increasing there) and nothing exceeds 1 + e, so a wrong
    // estimate costs iterations, not convergence.
    // Round 3: the interval is PREDICTED ([1 - e, 1 + e] after every step, e from the coefficients) instead of measured: the
    // coefficient chain - three square roots and a division, formerly in fp64 behind the wave reduction of ||I - Z Y||^2,
    // 1.4 k of a step's 3.0 k cycles - is a handful of fp32 instructions that do not depend on this step's product, and
    // the residual is only reduced once the prediction says the end is near (e < 0.01).  Below e = 1e-3 the step is the
    // plain Newton-Schulz one with EXACT coefficients (a - b = 1 is what fixes x = 1; fp32 coefficients would leave the
    // fixed point at 1 + 1e-7), where the minimax scaling has nothing left to gain.
    float flo = 1.f, fhi = 1.f;
    if (scaled) {
        const float est = xmin_est[slab];
        flo = est > 0.f ? fminf(0.5f * est, 1.f) : 1e-2f;
    }
    // (the interval, the residual and everything decided from them are the same in all lanes: kept in scalar registers, so that the
    // branches of a step are scalar branches and not the exec-mask sequences of a divergent one)
    // (rank <= 16 only: the rank-32 kernel sits at its 256-register budget and the extra scalar traffic costs it spills)
    auto uni_f = [](float v) { return NB == 1 ? __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))) : v; };
    flo = uni_f(flo);
    for (int it = 0; it < 100; ++it) {
        it_used = it;
        double ca = 1.5, cb = 0.5;
        const bool watch = !scaled || (1.f - flo) < 1e-2f;  // the end is near: measure the residual from here on
        if (scaled && (1.f - flo) >= 1e-3f) {
            // (the hardware's own square root and reciprocal - one instruction each, 1 ulp - where the library forms spent ~45
            // instructions per step on correct rounding and denormals: these coefficients only steer the speed of convergence)
            // (rank <= 16, where the step's latency is the kernel's; the rank-32 kernel keeps the forms its register allocation was
            // tuned with)
            const float ss = fhi * fhi + fhi * flo + flo * flo;
            const float sq = NB == 1 ? __builtin_amdgcn_sqrtf(ss * (1.f / 3.f)) : __builtin_sqrtf(ss * (1.f / 3.f));
            const float den = (2.f / 3.f) * ss * sq + flo * fhi * (flo + fhi);
            const float fb = NB == 1 ? 2.f * __builtin_amdgcn_rcpf(den) : 2.f / den;
            const float fa = fb * ss;
            const float e = (2.f / 3.f) * fa * sq - 1.f;
            ca = (double)fa, cb = (double)fb;
            flo = uni_f(1.f - e), fhi = uni_f(1.f + e);
        } else if (scaled) {
            const float e = 1.f - flo;
            flo = uni_f(1.f - 1.5f * e * e), fhi = 1.f;  // plain Newton-Schulz: x -> x (3 - x^2) / 2 <= 1, error 1.5 e^2
        }
        mm_t<NB>(Zt, Y, P);             // P  = Z Y
        tr_lds<NB>(P, Pt, Wtr, q, c16);  // Pt = P^T
        double res = 1.0;
        if (watch) {
            res = 0.0;
#pragma unroll
            for (int a = 0; a < NB; ++a)
#pragma unroll
                for (int b = 0; b < NB; ++b)
#pragma unroll
                    for (int v = 0; v < 4; ++v) {
                        const int row = 16 * a + q + 4 * v, col = 16 * b + c16;
                        const double id = (row == col) ? 1.0 : 0.0;
                        const double d = id - P.t[a][b][v];
                        res += d * d;
                    }
            res = wave_sum_d(res);
            if constexpr (NB == 1)
                res = __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(res)), __builtin_amdgcn_readfirstlane(__double2loint(res)));
        }
#pragma unroll
        for (int a = 0; a < NB; ++a)
#pragma unroll
            for (int b = 0; b < NB; ++b)
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    const int row = 16 * a + q + 4 * v, col = 16 * b + c16;
                    const double id = (row == col) ? 1.0 : 0.0;
                    Tm.t[a][b][v] = ca * id - cb * P.t[a][b][v];
                    Tmt.t[a][b][v] = ca * id - cb * Pt.t[a][b][v];
                }
        // converged: ||I - Z Y||_F < 1e-12 sqrt(r), or stagnation at the fp64 round-off floor of an ill-conditioned G
        // (the floor grows with cond(G); 1e-8 in ||I - ZY|| still leaves W accurate far beyond the fp32 data)
        if (watch) {
            if (res < 1e-24 * r || (res < 1e-16 && res > 0.25 * prev)) {
                converged = true;
                break;
            }
            prev = res;
            // a lower bound that was too optimistic (an eigenvalue below the assumed lo): the prediction is ahead of the
            // iterate - fall back to measuring, i.e. keep the predicted interval no tighter than the certified one
            // (|1 - x^2| <= ||I - Z Y||_F for every eigenvalue x^2 of Z Y, so x >= 1 - ||I - Z Y||_F)
            if (scaled) flo = uni_f(fminf(flo, res < 1.0 ? 1.f - (NB == 1 ? __builtin_amdgcn_sqrtf((float)res) : __builtin_sqrtf((float)res)) : 0.1f));
        }
        mm_t<NB>(Yt, Tm, N1);            // Y  <- Y T
        mm_t<NB>(Tmt, Z, N3);            // Z  <- T Z
        tr_lds<NB>(N1, N2, Wtr, q, c16);  // Yt <- Y^T
        tr_lds<NB>(N3, N4, Wtr, q, c16);  // Zt <- Z^T
        Y = N1;
        Yt = N2;
        Z = N3;
        Zt = N4;
    }
    if (!converged) {
        if (lane == 0) status[slab] = 1;
        if (INK) pf2_jacobi_slab(Jsm, Ss, Delta, rh, r, slab, lane, T, acc_out, T64, status, true);  // (the LDS copy of S is gone: from memory); may flag the slab (2)
        return;
    }
    NS_STAMP(3);
#ifdef MCL_NS_STAMPS
    if (lane == 0) stamps[(long)slab * 8 + 5] = it_used;
#endif
    // ||Z||_F^2 = sum_i tr / lambda_i(G): between cond(G) and r^2 cond(G)
    double zn = 0.0;
#pragma unroll
    for (int a = 0; a < NB; ++a)
#pragma unroll
        for (int b = 0; b < NB; ++b)
#pragma unroll
            for (int v = 0; v < 4; ++v) zn += Z.t[a][b][v] * Z.t[a][b][v];
    zn = wave_sum_d(zn);
    // 1 / ||Z||_F <= 1 / ||Z||_2 = sqrt(eig_min(G / tr)): the next call's starting estimate for this slab (read only by the scaled
    // iteration) - and what pf2_ill_conditioned goes by
    if (lane == 0) xmin_est[slab] = (float)(1.0 / sqrt(zn));
    // The iteration also "converges" (by stagnation at its round-off floor) on a Gram matrix far too ill-conditioned for the Gram
    // route: cond(Y Delta^T) = 1e6 and 1e7 in 28 - 33 steps, with eps cond^2 in W - Delta off by 7 - 30 times its fp32 bar
    // (tests/test_gpu_pf2_polar.py) where the QR route that ranks > 32 take for the same slab meets it.  Such a slab is flagged
    // (2) like the ones the Jacobi route flags: k_pf2_polar_qr redoes it where it is launched, and what the epilogue below
    // writes stands where it is not.  Rank <= 16: here; rank 32 (any more code behind the iteration costs that kernel two more
    // spilled registers): k_pf2_algebra, launched behind this kernel, flags it by the estimate above.
    // status <= 0: converged (number of Newton-Schulz iterations, for diagnostics)
    if constexpr (INK) {
        if (lane == 0) status[slab] = pf2_ill_conditioned(zn, r) ? 2 : -it_used;
    } else {
        if (lane == 0) status[slab] = -it_used;
    }
    // S_i for the epilogue: from memory (this wave wrote it above when it summed the tiles; its LDS copy has been the scratch of
    // the transposes since)
    auto Smem = [&](int i, int j) -> double {
        if constexpr (NB == 1 && TILES) return (i < r && j < r) ? Ssm[i * r + j] : 0.0;  // (still in LDS: see Wtr)
        else return (i < r && j < r) ? Ss[i * r + j] : 0.0;
    };
    const double wscale = 1.0 / sqrt(tr);  // W = Z / sqrt(tr)
    // T = Delta^T W  (A[i][k] = Delta[k][i];  B = W in D layout), then acc = rho T^T S (A = T^T: A[i][k] = T[k][i] = D layout of T)
    SymTiles<NB> Tt;
#pragma unroll
    for (int a = 0; a < NB; ++a)
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            f64x4 acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int kb = 0; kb < NB; ++kb)
#pragma unroll
                for (int st = 0; st < 4; ++st)
                    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(Dat(16 * kb + q + 4 * st, 16 * a + c16), Z.t[kb][b][st] * wscale, acc, 0, 0, 0);
            Tt.t[a][b] = acc;
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int row = 16 * a + q + 4 * v, col = 16 * b + c16;
                if (row < r && col < r) {
                    T[(long)slab * n2 + row * r + col] = (float)acc[v];
                    if (T64 != nullptr) T64[(long)slab * n2 + row * r + col] = acc[v];  // fp64 row passes (mcl_rows64)
                }
            }
        }
#pragma unroll
    for (int a = 0; a < NB; ++a)
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            f64x4 acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int kb = 0; kb < NB; ++kb)
#pragma unroll
                for (int st = 0; st < 4; ++st)
                    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(Tt.t[kb][a][st], Smem(16 * kb + q + 4 * st, 16 * b + c16), acc, 0, 0, 0);
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int row = 16 * a + q + 4 * v, col = 16 * b + c16;
                if (row < r && col < r) acc_out[(long)slab * (n2 + 1) + row * r + col] = rh * acc[v];
            }
        }
    if (lane == 0) acc_out[(long)slab * (n2 + 1) + n2] = rh;
    NS_STAMP(4);
}

// red[e] = sum_i acc[i][e]: one workgroup per element, fixed summation order
__global__ __launch_bounds__(256) void k_pf2_sum(const double *__restrict__ acc, int n_slabs, int n_el,
                                                 float *__restrict__ red) {
    __shared__ double sm[4];
    const int e = blockIdx.x;
    double s = 0.0;
    for (int i = threadIdx.x; i < n_slabs; i += 256) s += acc[(long)i * n_el + e];
    s = wave_sum_d(s);
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) red[e] = (float)((sm[0] + sm[1]) + (sm[2] + sm[3]));
}

// k_pf2_sum + k_pf2_delta in one launch (single-process runs: no all-reduce between them).  Workgroup e sums element e
// and the weight total with the same order and roundings as the two kernels.
__global__ __launch_bounds__(256) void k_pf2_sum_delta(const double *__restrict__ acc, int n_slabs, int n2,
                                                       float *__restrict__ red, float *__restrict__ Delta,
                                                       const int *__restrict__ gate) {
    MCL_GATE(gate);
    __shared__ double sm[2][4];
    const int e = blockIdx.x, n_el = n2 + 1;
    double s = 0.0, w = 0.0;
    for (int i = threadIdx.x; i < n_slabs; i += 256) {
        s += acc[(long)i * n_el + e];
        w += acc[(long)i * n_el + n2];
    }
    s = wave_sum_d(s);
    w = wave_sum_d(w);
    if ((threadIdx.x & 63) == 0) sm[0][threadIdx.x >> 6] = s, sm[1][threadIdx.x >> 6] = w;
    __syncthreads();
    if (threadIdx.x == 0) {
        const float re = (float)((sm[0][0] + sm[0][1]) + (sm[0][2] + sm[0][3]));
        const float rw = (float)((sm[1][0] + sm[1][1]) + (sm[1][2] + sm[1][3]));
        red[e] = re;
        if (e == 0) red[n2] = rw;
        Delta[e] = re / rw;
    }
}
__global__ void k_pf2_delta(const float *__restrict__ red, int r, float *__restrict__ Delta, const int *__restrict__ gate) {
    MCL_GATE(gate);
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e < r * r) Delta[e] = red[e] / red[r * r];
}

// =========================================================================================================
// host launchers
// =========================================================================================================
// The per-slab sums of the solve pass's tile statistics are taken by the PARAFAC2 Newton-Schulz kernel itself when
// the B stack has a PARAFAC2 member handled by that kernel (otherwise k_stats_reduce runs after the solve pass).
bool mcl_stats_reduce_in_algebra(const mcl_context *c) {
    if (c->sw.stats_reduce || c->sw.pf2_jacobi || c->NB > 2) return false;
    const RegSet &rs = c->regs[1];
    for (int k = 0; k < rs.n; ++k)
        if (rs.kind[k] == MCL_PEN_PARAFAC2) return true;
    return false;
}

// `jacobi`: k_pf2_algebra takes every slab (use_status: only those the Newton-Schulz kernel left to it); `qr`: k_pf2_polar_qr
// redoes the slabs flagged 2 (too ill-conditioned for the Gram route) from Y Delta^T itself.  F64 / U64 / D64: the fp64 state
// of wide.hip, or NULL (the caller's fp32 buffers).  From rank 46 on the kernels' LDS exceeds the 64 KB a launch may ask for
// without the attribute.
static int pf2_jacobi_qr(mcl_context *c, int k, bool jacobi, int use_status, bool qr, const double *F64, const double *U64,
                         const double *D64) {
    // behind the rank-32 Newton-Schulz kernel: its estimate of this call, by which k_pf2_algebra flags the slabs that converged
    // on a Gram matrix too ill-conditioned - where the QR kernel's work does not count, as for rank <= 16 (mcl_launch_pf2_polar):
    // the large problems of the fast kernels (config 5: most slabs of the early iterations) keep the Newton-Schulz factor
    const float *xmin = (use_status && (c->I <= 64 || c->exact)) ? c->pf2_xmin : nullptr;
    const RegSet &rs = c->regs[1];
    const int r = c->r, n2 = r * r;
    if (jacobi) {
        const size_t sm = sizeof(double) * (size_t)(4 * n2 + r);
        if (sm > 65536)
            MCL_CHECK_HIP(c, hipFuncSetAttribute(reinterpret_cast<const void *>(k_pf2_algebra), hipFuncAttributeMaxDynamicSharedMemorySize, (int)sm));
        hipLaunchKernelGGL(k_pf2_algebra, dim3((unsigned)c->I), dim3(64), sm, c->stream, c->pf2_S, rs.aux2[k], c->rhoB, r, c->pf2_T,
                           c->pf2_acc, c->pf2_status, use_status, c->pf2_T64, c->row_ptr_dev, D64, xmin);
    }
    if (qr) {
        const size_t smq = sizeof(double) * (size_t)(3 * n2 + 4 * 64 + 64);
        if (smq > 65536)
            MCL_CHECK_HIP(c, hipFuncSetAttribute(reinterpret_cast<const void *>(k_pf2_polar_qr), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smq));
        hipLaunchKernelGGL(k_pf2_polar_qr, dim3((unsigned)c->I), dim3(256), smq, c->stream, c->row_ptr_dev, c->B, rs.dual[k], rs.aux2[k],
                           c->rhoB, r, c->pf2_S, c->pf2_status, c->pf2_qr, c->pf2_T, c->pf2_acc, c->pf2_T64, c->gate_active, F64, U64, D64);
    }
    return 0;
}

// S_i = Y_i^T Y_i (unless the solve pass produced it), then T_i and rho_i T_i^T S_i of every slab
int mcl_launch_pf2_polar(mcl_context *c, int k, ProxForm form) {
    const RegSet &rs = c->regs[1];
    const int r = c->r;
    if (form.stats_in_solve) {
        // S_i already produced by k_rows_solve_stats + k_stats_reduce
    } else if (c->NB == 1)
        hipLaunchKernelGGL(k_pf2_gram<1>, dim3((unsigned)c->I), dim3(256), 0, c->stream, c->row_ptr_dev, c->B, rs.dual[k], r, c->pf2_S);
    else if (c->NB == 2)
        hipLaunchKernelGGL(k_pf2_gram<2>, dim3((unsigned)c->I), dim3(256), 0, c->stream, c->row_ptr_dev, c->B, rs.dual[k], r, c->pf2_S);
    else
        hipLaunchKernelGGL(k_pf2_gram<4>, dim3((unsigned)c->I), dim3(256), 0, c->stream, c->row_ptr_dev, c->B, rs.dual[k], r, c->pf2_S);
    const bool ns = c->NB <= 2 && !c->sw.pf2_jacobi;  // Newton-Schulz first
    if (ns) {
        TileStats ts{c->slab_tile_ptr, c->stat_gram, c->stat_colsq, c->colsq, 16 * c->NB, (int)c->I};
        const bool tiles = form.stats_in_solve && mcl_stats_reduce_in_algebra(c);
#define MCL_NS(NB_, TILES_)                                                                                          \
    hipLaunchKernelGGL((k_pf2_algebra_ns<NB_, TILES_>), dim3((unsigned)((c->I + NsShape<NB_>::SPW - 1) / NsShape<NB_>::SPW)),                   \
                       dim3(64 * NsShape<NB_>::SPW + (((TILES_) && (NB_) == 1) ? 64 : 0)), 0, c->stream, c->pf2_S,                  \
                       rs.aux2[k], c->rhoB, c->row_ptr_dev, r, c->pf2_T, c->pf2_acc, c->pf2_status, ts, rs, c->pf2_xmin,     \
                       c->sw.ns_plain ? 0 : 1, c->pf2_T64)
        c->variant[MCL_PROF_PF2] = std::string("k_pf2_algebra_ns<NB=") + std::to_string(c->NB) + (tiles ? ",TILES> (+ k_pf2_sum_delta)" : "> (+ k_pf2_sum_delta)");
        if (c->NB == 1) {
            if (tiles) MCL_NS(1, true);
            else MCL_NS(1, false);
        } else {
            if (tiles) MCL_NS(2, true);
            else MCL_NS(2, false);
        }
#undef MCL_NS
        if (c->cond_monitor)  // (mcl_condition_monitor: a trial / an occasional monitored iteration only)
            if (int rc = mcl_launch_pf2_cond_track(c)) return rc;
    } else {
        c->variant[MCL_PROF_PF2] = "k_pf2_algebra (Jacobi) + k_pf2_polar_qr";
    }
    // rank <= 16: the Newton-Schulz kernel runs the Jacobi route itself and flags the slabs whose Gram matrix is too
    // ill-conditioned (2); the QR kernel that redoes them is launched where its launch does not count - small problems
    // (up to 64 slabs, the exact-products mode): on a large rank <= 16 problem (config 4: 1024 slabs, 5 launches of
    // ~3 us per iteration for slabs that do not occur there) such a slab keeps the Gram-route factor
    const bool ink_qr = ns && c->NB == 1 && (c->I <= 64 || c->exact);
    const bool jacobi = !ns || c->NB != 1;
    return pf2_jacobi_qr(c, k, jacobi, ns ? 1 : 0, jacobi || ink_qr, nullptr, nullptr, nullptr);
}

// sum over the slabs of rho_i T_i^T S_i | rho_i (behind the row pass that applies T_i: rows.hip)
void mcl_launch_pf2_sum(mcl_context *c, int k, ProxForm form) {
    const int n2 = c->r * c->r;
    if (form.pf2_delta_fused)  // single-process inner loop: Delta follows at once, no all-reduce in between
        hipLaunchKernelGGL(k_pf2_sum_delta, dim3((unsigned)n2), dim3(256), 0, c->stream, c->pf2_acc, (int)c->I, n2,
                           c->pf2_red, c->regs[1].aux2[k], c->gate_active);
    else
        hipLaunchKernelGGL(k_pf2_sum, dim3((unsigned)(n2 + 1)), dim3(256), 0, c->stream, c->pf2_acc, (int)c->I,
                           n2 + 1, c->pf2_red);
}

void mcl_launch_pf2_delta(mcl_context *c, int k) {
    const int n2 = c->r * c->r;
    hipLaunchKernelGGL(k_pf2_delta, dim3((unsigned)((n2 + 255) / 256)), dim3(256), 0, c->stream, c->pf2_red, c->r,
                       c->regs[1].aux2[k], c->gate_active);
}

// The polar factors of the PARAFAC2 member from the fp64 state of wide.hip (S_i = Y_i^T Y_i already in pf2_S): the Jacobi route
// for every slab, then the QR route for the slabs it flags (Gram matrix too ill-conditioned) - T_i, T_i in fp64, rho_i T_i^T S_i
int mcl_launch_pf2_jacobi_wide(mcl_context *c, int k, const double *F64, const double *U64, const double *D64) {
    ProfScope prof(c, MCL_PROF_PF2);
    c->variant[MCL_PROF_PF2] = "k_pf2_algebra (Jacobi) + k_pf2_polar_qr on the fp64 state";
    if (int rc = pf2_jacobi_qr(c, k, true, 0, true, F64, U64, D64)) return rc;
    MCL_CHECK_HIP(c, hipGetLastError());
    return 0;
}
