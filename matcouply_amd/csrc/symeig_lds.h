// Symmetric eigen-decomposition of a small matrix held in LDS (cyclic Jacobi), shared by the SVD initialiser (svdinit.hip:
// Rayleigh-Ritz step of the subspace iteration), the pseudo-inverse of a singular r x r Gram matrix (cp_passes.h: the CP
// initialisers and parafac2_als) and parafac2_als's polar step (parafac2als.hip).
#pragma once
#include <hip/hip_runtime.h>

// eigen-decomposition of the symmetric m x m matrix S (LDS) by cyclic Jacobi with round-robin pairs: W <- eigenvectors
// (columns), the diagonal of S <- eigenvalues.  me = m rounded up to even (a dummy player idles).  All NT threads of the
// workgroup call it.
template <int NT>
static __device__ void jacobi_lds_nt(double *S, double *W, double *cs, int m) {
    const int tid = threadIdx.x;
    const int me = (m + 1) & ~1, half = me / 2;
    for (int e = tid; e < m * m; e += NT) W[e] = ((e / m) == (e % m)) ? 1.0 : 0.0;
    __shared__ double off_sh, diag_sh;
    __syncthreads();
    for (int sweep = 0; sweep < 40; ++sweep) {
        if (tid == 0) {
            double off = 0.0, dg = 0.0;
            for (int a = 0; a < m; ++a)
                for (int b = 0; b < m; ++b) (a == b ? dg : off) += S[a * m + b] * S[a * m + b];
            off_sh = off, diag_sh = dg;
        }
        __syncthreads();
        if (!(off_sh > 1e-30 * diag_sh)) break;
        for (int step = 0; step < me - 1; ++step) {
            // pair k of this step: (p, q)
            auto pair_of = [&](int k, int &p, int &q) {
                if (k == 0) p = me - 1, q = step;
                else p = (step + k) % (me - 1), q = (step - k + (me - 1)) % (me - 1);
                if (p > q) { const int t = p; p = q; q = t; }
            };
            if (tid < half) {
                int p, q;
                pair_of(tid, p, q);
                double c = 1.0, s = 0.0;
                if (q < m) {
                    const double apq = S[p * m + q], app = S[p * m + p], aqq = S[q * m + q];
                    if (fabs(apq) > 1e-300 && fabs(apq) > 1e-18 * sqrt(fabs(app * aqq))) {
                        const double tau = (aqq - app) / (2.0 * apq);
                        const double t = (tau >= 0.0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(1.0 + tau * tau));
                        c = 1.0 / sqrt(1.0 + t * t), s = t * c;
                    }
                }
                cs[2 * tid] = c, cs[2 * tid + 1] = s;
            }
            __syncthreads();
            for (int e = tid; e < half * m; e += NT) {  // columns p, q of S and of W, every row i
                const int k = e / m, i = e - k * m;
                int p, q;
                pair_of(k, p, q);
                if (q >= m) continue;
                const double c = cs[2 * k], s = cs[2 * k + 1];
                const double sp = S[i * m + p], sq = S[i * m + q];
                S[i * m + p] = c * sp - s * sq, S[i * m + q] = s * sp + c * sq;
                const double wp = W[i * m + p], wq = W[i * m + q];
                W[i * m + p] = c * wp - s * wq, W[i * m + q] = s * wp + c * wq;
            }
            __syncthreads();
            for (int e = tid; e < half * m; e += NT) {  // rows p, q of S, every column j
                const int k = e / m, j = e - k * m;
                int p, q;
                pair_of(k, p, q);
                if (q >= m) continue;
                const double c = cs[2 * k], s = cs[2 * k + 1];
                const double sp = S[p * m + j], sq = S[q * m + j];
                S[p * m + j] = c * sp - s * sq, S[q * m + j] = s * sp + c * sq;
            }
            __syncthreads();
        }
    }
    __syncthreads();
}
// the same with the 256 threads of the initialisers' workgroups
static __device__ void jacobi_lds(double *S, double *W, double *cs, int m) { jacobi_lds_nt<256>(S, W, cs, m); }
