// fp64 helpers for kernels that run a whole fit in one workgroup of MS_THREADS threads (csrc/multistart.hip,
// csrc/pf2als_multistart.hip).  Every sum has a fixed order that depends on the sizes only; no atomics.
#pragma once
#include <cmath>
#include <cstdint>

#include <hip/hip_runtime.h>

constexpr int MS_THREADS = 256;

// sum of one value per thread, tree order fixed; the total in every thread
static __device__ __forceinline__ double wg_sum(double v, double *red) {
    const int t = threadIdx.x;
    red[t] = v;
    __syncthreads();
    for (int h = MS_THREADS / 2; h > 0; h >>= 1) {
        if (t < h) red[t] += red[t + h];
        __syncthreads();
    }
    const double s = red[0];
    __syncthreads();
    return s;
}

// out[e] = sum_{j < n} f(j, e) for e < P: groups of threads take rows j = g, g + G, ..., the G partials are added in group order
template <class F>
static __device__ __forceinline__ void rows_reduce(int P, int64_t n, double *out, double *red, F f) {
    const int t = threadIdx.x;
    if (P > MS_THREADS / 2) {
        for (int e = t; e < P; e += MS_THREADS) {
            double acc = 0.0;
            for (int64_t j = 0; j < n; ++j) acc += f(j, e);
            out[e] = acc;
        }
        __syncthreads();
        return;
    }
    const int G = MS_THREADS / P, e = t % P, g = t / P;
    double acc = 0.0;
    if (g < G)
        for (int64_t j = g; j < n; j += G) acc += f(j, e);
    red[t] = acc;
    __syncthreads();
    if (t < P) {
        double s = 0.0;
        for (int q = 0; q < G; ++q) s += red[q * P + t];
        out[t] = s;
    }
    __syncthreads();
}

// S (R x R, row-major, SPD) <- S^-1 by Cholesky: S = L L^T, W = L^-1, S^-1 = W^T W.  One thread, LDS.  Returns false when a
// pivot is not positive (S is not positive definite; S then holds no inverse).
template <int R>
static __device__ __forceinline__ bool spd_inverse(double *S, double *W) {
    bool ok = true;
    for (int j = 0; j < R; ++j) {  // L in the lower triangle of S
        double d = S[j * R + j];
        for (int k = 0; k < j; ++k) d -= S[j * R + k] * S[j * R + k];
        ok = ok && d > 0.0;
        const double l = sqrt(d);
        S[j * R + j] = l;
        for (int i = j + 1; i < R; ++i) {
            double v = S[i * R + j];
            for (int k = 0; k < j; ++k) v -= S[i * R + k] * S[j * R + k];
            S[i * R + j] = v / l;
        }
    }
    for (int j = 0; j < R; ++j) {  // W = L^-1, lower
        W[j * R + j] = 1.0 / S[j * R + j];
        for (int i = j + 1; i < R; ++i) {
            double v = 0.0;
            for (int k = j; k < i; ++k) v += S[i * R + k] * W[k * R + j];
            W[i * R + j] = -v / S[i * R + i];
        }
    }
    for (int a = 0; a < R; ++a)
        for (int b = a; b < R; ++b) {
            double v = 0.0;
            for (int k = b; k < R; ++k) v += W[k * R + a] * W[k * R + b];
            S[a * R + b] = v, S[b * R + a] = v;
        }
    return ok;
}

// S (R x R symmetric PSD Gram) <- S^{-1/2} on its range: cyclic Jacobi (the rotation of symeig_lds.h), eigenvalues at or below
// `drop` times the largest dropped.  W: R x R work space.  One thread, LDS.
template <int R>
static __device__ __forceinline__ void gram_inv_sqrt(double *S, double *W, double drop) {
    for (int e = 0; e < R * R; ++e) W[e] = (e / R == e % R) ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 40; ++sweep) {
        double off = 0.0, dg = 0.0;
        for (int a = 0; a < R; ++a)
            for (int b = 0; b < R; ++b) (a == b ? dg : off) += S[a * R + b] * S[a * R + b];
        if (!(off > 1e-30 * dg)) break;
        for (int p = 0; p < R - 1; ++p)
            for (int q = p + 1; q < R; ++q) {
                const double apq = S[p * R + q], app = S[p * R + p], aqq = S[q * R + q];
                if (!(fabs(apq) > 1e-300 && fabs(apq) > 1e-18 * sqrt(fabs(app * aqq)))) continue;
                const double tau = (aqq - app) / (2.0 * apq);
                const double tt = (tau >= 0.0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(1.0 + tau * tau));
                const double c = 1.0 / sqrt(1.0 + tt * tt), s = tt * c;
                for (int i = 0; i < R; ++i) {
                    const double sp = S[i * R + p], sq = S[i * R + q];
                    S[i * R + p] = c * sp - s * sq, S[i * R + q] = s * sp + c * sq;
                    const double wp = W[i * R + p], wq = W[i * R + q];
                    W[i * R + p] = c * wp - s * wq, W[i * R + q] = s * wp + c * wq;
                }
                for (int j = 0; j < R; ++j) {
                    const double sp = S[p * R + j], sq = S[q * R + j];
                    S[p * R + j] = c * sp - s * sq, S[q * R + j] = s * sp + c * sq;
                }
            }
    }
    double lam[R], lmax = 0.0;
    #pragma unroll
    for (int k = 0; k < R; ++k) lam[k] = S[k * R + k], lmax = fmax(lmax, lam[k]);
    #pragma unroll
    for (int k = 0; k < R; ++k) lam[k] = lam[k] > drop * lmax ? 1.0 / sqrt(lam[k]) : 0.0;
    for (int a = 0; a < R; ++a)
        for (int b = a; b < R; ++b) {
            double v = 0.0;
            #pragma unroll
            for (int k = 0; k < R; ++k) v += W[a * R + k] * lam[k] * W[b * R + k];
            S[a * R + b] = v, S[b * R + a] = v;
        }
}
