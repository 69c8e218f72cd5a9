// What the CP initialisers (alsinit.hip) and parafac2_als (parafac2als.hip) share: the two passes over X on the fp32 MFMA, the
// fragment layout of C they multiply with, the r x r algebra of a mode's update, the fixed-order sum of fp64 partials.  The
// layout decisions of both kernel families are here and nowhere else: the LDS swizzle of pass 1, the address of C[k][s] in
// Cfrag, the order of the wave sum of pass 2 and of the partial sums (two runs are bitwise equal because of them), the 1e-12
// eigenvalue cut of the pseudo-inverse.  What differs between the callers comes in as a callable (the weights of pass 2, the
// sink of its sums, the entries of G).  The host tables that drive the passes (segments of CP_SEG rows) are in entry_host.h.
#pragma once
#include <algorithm>
#include <string>
#include <vector>

#include "entry_host.h"
#include "mcl_internal.h"
#include "rows_mfma.h"
#include "symeig_lds.h"
#include "xload.h"

// four consecutive elements of X as fp32, zero past column K (VEC: K % 4 == 0 and an aligned base)
template <class XL, bool VEC>
static __device__ __forceinline__ f32x4 x_ld4(const typename XL::T *p, int col, int K) {
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if constexpr (VEC) {
        if (col < K) v = XL::cvt(XL::template ld4<false>(p));
    } else {
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (col + q < K) v[q] = XL::ld1(p + q);
    }
    return v;
}

// the address of C[k][s] in Cfrag[4H + h][hp][lane][kq] = C[64H + 16h + 4g + kq][16hp + (l & 15)] (NB column blocks hp)
static __device__ __forceinline__ long cfrag_index(int k, int s, int NB) {
    return (((long)(k >> 4) * NB + (s >> 4)) * 64 + ((k >> 2) & 3) * 16 + (s & 15)) * 4 + (k & 3);
}

// ---- pass 1: acc = (X C) of one segment ------------------------------------------------------------------------------------
// One wave per segment (<= 64 rows of one slab; sg = {slab, first packed row, rows, first row within the slab}), walking
// 64-column chunks H and, inside each, its 4 row blocks rb of 16 rows:
//   global -> registers: lane (rr = l >> 4, cc = l & 15), t < 4: X[16 rb + 4 t + rr][64 H + 4 cc .. +3]  (256-B row segments)
//   registers -> LDS   : wave-private 16 x 64 fp32 tile T, 16-B slot index XORed with the row (conflict-free)
//   LDS -> fragments   : lane (row16 = l & 15, g = l >> 4), h < 4: X[16 rb + row16][64 H + 16 h + 4 g .. +3]
//   MFMA on the transposed problem (rows_mfma.h) with the fragments of C (cfrag_index):
//   accumulator (rb, hp), lane l, reg v = XC[16 rb + row16][16 hp + 4 g + v].
// The next step's global loads are in flight while the current tile is multiplied (rows clamped into the segment, columns
// past K zero).  LDS operations of one wave complete in order, so the tile needs no barrier.
template <class XL, int NB, bool VEC>
static __device__ __forceinline__ void xc_segment(const typename XL::T *X, const int4 sg, int K, const float *Cfrag, f32x4 *T,
                                                  f32x4 (&acc)[4][NB]) {
    const int lane = threadIdx.x & 63, row0 = sg.y, n = sg.z;
    const int row16 = lane & 15, g = lane >> 4, rr = lane >> 4, cc = lane & 15;
#pragma unroll
    for (int rb = 0; rb < 4; ++rb)
#pragma unroll
        for (int hp = 0; hp < NB; ++hp) acc[rb][hp] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int KC = (K + 63) >> 6;
    f32x4 xn[4];
    auto load = [&](int H, int rb) {
        const int col = 64 * H + 4 * cc;
#pragma unroll
        for (int t = 0; t < 4; ++t)
            xn[t] = x_ld4<XL, VEC>(X + (long)(row0 + min(16 * rb + 4 * t + rr, n - 1)) * K + col, col, K);
    };
    load(0, 0);
    for (int H = 0; H < KC; ++H) {
        f32x4 cf[4][NB];
#pragma unroll
        for (int h = 0; h < 4; ++h)
#pragma unroll
            for (int hp = 0; hp < NB; ++hp)
                cf[h][hp] = *reinterpret_cast<const f32x4 *>(Cfrag + (((long)(4 * H + h) * NB + hp) * 64 + lane) * 4);
#pragma unroll
        for (int rb = 0; rb < 4; ++rb) {
#pragma unroll
            for (int t = 0; t < 4; ++t) T[(4 * t + rr) * 16 + (cc ^ (4 * t + rr))] = xn[t];
            if (rb < 3) load(H, rb + 1);
            else if (H + 1 < KC) load(H + 1, 0);
            f32x4 x[4];
#pragma unroll
            for (int h = 0; h < 4; ++h) x[h] = T[row16 * 16 + ((4 * h + g) ^ row16)];
#pragma unroll
            for (int h = 0; h < 4; ++h)
#pragma unroll
                for (int hp = 0; hp < NB; ++hp)
#pragma unroll
                    for (int kq = 0; kq < 4; ++kq) acc[rb][hp] = MFMA16(cf[h][hp][kq], x[h][kq], acc[rb][hp]);
        }
    }
}

// ---- pass 2: acc = sum over the rows of the segments [s_beg, s_end) of X^T (weights), 64-column block kb --------------------
// Wave w of the workgroup's four takes the 4-row groups w, w + 4, w + 8, w + 12 of every segment.  Lane (rsub = l >> 4,
// c16 = l & 15) loads X[row0 + 4 gi + rsub][64 kb + 4 c16 .. +3]; MFMA (m, nb): A = component m (output row i = c16 <->
// k = 64 kb + 4 i + m), B = the weight of (row, column 16 nb + c16), reduction index = the 4 rows of the group.
// Accumulator (m, nb), lane l, reg v = R[64 kb + 4 (4 (l >> 4) + v) + m][16 nb + (l & 15)].
// The weights come from the caller: wload(sg, loc) loads the raw values of the rows loc[u] (u < 4, clamped into the segment)
// and columns min(16 nb + c16, r - 1) of segment sg into the caller's registers, wget(u, nb) turns them into the fp32 weight.
// The next segment's X rows and raw weights are in flight while the current one is multiplied (loads unconditional; invalid
// rows and columns get a zero weight here).
template <class XL, int NB, bool VEC, class WLoad, class WGet>
static __device__ __forceinline__ void xtw_segments(const typename XL::T *X, const int4 *segs, int s_beg, int s_end, int K, int r, int kb,
                                                    WLoad &&wload, WGet &&wget, f32x4 (&acc)[4][NB]) {
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int rsub = lane >> 4, c16 = lane & 15, col = 64 * kb + 4 * c16;
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) acc[m][nb] = f32x4{0.f, 0.f, 0.f, 0.f};
    f32x4 xn[4];
    int nn = 0;
    auto load = [&](int s) {
        const int4 sg = segs[s];
        nn = sg.z;
        int loc[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            loc[u] = min(4 * (w + 4 * u) + rsub, nn - 1);
            xn[u] = x_ld4<XL, VEC>(X + (long)(sg.y + loc[u]) * K + col, col, K);
        }
        wload(sg, loc);
    };
    if (s_beg < s_end) load(s_beg);
    for (int s = s_beg; s < s_end; ++s) {
        f32x4 x[4];
        float wv[4][NB];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const bool ok = 4 * (w + 4 * u) + rsub < nn;
            x[u] = xn[u];
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) wv[u][nb] = (ok && 16 * nb + c16 < r) ? wget(u, nb) : 0.f;
        }
        if (s + 1 < s_end) load(s + 1);
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int m = 0; m < 4; ++m)
#pragma unroll
                for (int nb = 0; nb < NB; ++nb) acc[m][nb] = MFMA16(x[u][m], wv[u][nb], acc[m][nb]);
    }
}

// the four waves' accumulators of pass 2 summed in fp64 in a fixed order, (w0 + w1) + (w2 + w3), by wave 0, which hands
// sink(kl, q, sum) the entry R[64 kb + kl][q] (kl < 64, q < 16 NB).  All 256 threads call it; it holds one workgroup barrier.
template <int NB, class Sink>
static __device__ __forceinline__ void xtw_wave_sum(const f32x4 (&acc)[4][NB], float (&red)[3][NB * 16][64], Sink &&sink) {
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (w > 0)
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
            for (int nb = 0; nb < NB; ++nb)
#pragma unroll
                for (int v = 0; v < 4; ++v) red[w - 1][(m * NB + nb) * 4 + v][lane] = acc[m][nb][v];
    __syncthreads();
    if (w > 0) return;
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int nb = 0; nb < NB; ++nb)
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int e = (m * NB + nb) * 4 + v;
                const double s = ((double)acc[m][nb][v] + (double)red[0][e][lane]) + ((double)red[1][e][lane] + (double)red[2][e][lane]);
                sink(4 * (4 * (lane >> 4) + v) + m, 16 * nb + (lane & 15), s);
            }
}

// ---- r x r systems in LDS -------------------------------------------------------------------------------------------------
// S (r x r, LDS) = G on entry; S <- G^-1 by Gauss-Jordan without pivoting (SPD: every pivot is positive), in the first wave
// only: its LDS operations complete in order, so the two phases of a pivot need no workgroup barrier.  When a pivot is not
// positive, S <- the pseudo-inverse G = W diag(lam) W^T, 1 / lam for lam > 1e-12 lam_max, from a Jacobi eigen-decomposition of
// G, whose entry e the callable G(e) forms again (no kernel keeps a copy).  W (r x r), cs (r + 2): Jacobi work space.  All NT
// threads call it.
template <int NT, class Entry>
static __device__ void spd_inverse_lds(double *S, double *W, double *cs, int r, Entry &&G) {
    __shared__ int fail_sh;
    const int tid = threadIdx.x, rr = r * r;
    if (tid == 0) fail_sh = 0;
    __syncthreads();
    if (tid < 64)
        for (int q = 0; q < r; ++q) {
            const double piv = S[q * r + q];
            if (!(piv > 0.0) || !isfinite(piv)) {
                if (tid == 0) fail_sh = 1;
                break;
            }
            const double d = 1.0 / piv;
            for (int e = tid; e < rr; e += 64) {
                const int a = e / r, c = e - a * r;
                if (a != q && c != q) S[e] = fma(-S[a * r + q] * d, S[q * r + c], S[e]);
            }
            __builtin_amdgcn_wave_barrier();
            for (int e = tid; e < 2 * r; e += 64) {
                const int k = e < r ? e : e - r;
                if (k == q) {
                    if (e == q) S[q * r + q] = d;
                } else if (e < r) {
                    S[q * r + k] *= d;
                } else {
                    S[k * r + q] *= -d;
                }
            }
            __builtin_amdgcn_wave_barrier();
        }
    __syncthreads();
    if (!fail_sh) return;
    for (int e = tid; e < rr; e += NT) S[e] = G(e);
    __syncthreads();
    jacobi_lds_nt<NT>(S, W, cs, r);
    if (tid < r) cs[tid] = S[tid * r + tid];  // the eigenvalues; the rest of S is free for the result
    __syncthreads();
    double lmax = 0.0;
    for (int k = 0; k < r; ++k) lmax = fmax(lmax, cs[k]);
    for (int e = tid; e < rr; e += NT) {
        const int a = e / r, c = e - a * r;
        double s = 0.0;
        for (int k = 0; k < r; ++k) {
            const double l = cs[k];
            if (l > 1e-12 * lmax) s += W[a * r + k] * W[c * r + k] / l;
        }
        S[e] = s;
    }
    __syncthreads();
}

// one row f of a factor from its right-hand side m: ALS f = m Gm (Gm = G^-1), HALS one pass over the columns (Gm = G):
// for q = 0..r-1: f[q] <- max(0, f[q] + (m[q] - f Gm[:, q]) / Gm[q][q])  (skipped where Gm[q][q] = 0)
template <int RMAX>
static __device__ __forceinline__ void factor_row_update(const double *m, double *f, const double *Gm, int r, int hals) {
    if (!hals) {  // (f is not read: m and f are two arrays)
#pragma unroll
        for (int q = 0; q < RMAX; ++q) {
            double s = 0.0;
#pragma unroll
            for (int p = 0; p < RMAX; ++p)
                if (p < r && q < r) s = fma(m[p], Gm[p * r + q], s);
            f[q] = s;
        }
        return;
    }
#pragma unroll
    for (int q = 0; q < RMAX; ++q) {
        if (q >= r) continue;
        const double gqq = Gm[q * r + q];
        if (gqq == 0.0) continue;
        double s = m[q];
#pragma unroll
        for (int p = 0; p < RMAX; ++p)
            if (p < r) s = fma(-f[p], Gm[p * r + q], s);
        f[q] = fmax(0.0, f[q] + s / gqq);
    }
}

// out[e] = sum over np parts of part[p * stride + e], e < E; NT threads: quarter u of the threads sums the parts p = u (mod 4) of
// entry e in ascending order, quarters combined as (s0 + s1) + (s2 + s3).  red: NT doubles of LDS.  All NT threads call it.
template <int NT>
static __device__ void fixed_order_sum(const double *part, int np, long stride, int E, double *out, double *red) {
    constexpr int Q = NT / 4;
    const int tid = threadIdx.x, u = tid / Q, l = tid - u * Q;
    for (int e0 = 0; e0 < E; e0 += Q) {
        const int e = e0 + l;
        double s = 0.0;
        if (e < E) {
#pragma unroll 8
            for (int p = u; p < np; p += 4) s += part[(long)p * stride + e];
        }
        red[tid] = s;
        __syncthreads();
        if (u == 0 && e < E) out[e] = (red[l] + red[Q + l]) + (red[2 * Q + l] + red[3 * Q + l]);
        __syncthreads();
    }
}

// the slab of a packed row: ext[i] <= row < ext[i + 1]
static __device__ __forceinline__ int slab_of_row(const int *ext, int I, int row) {
    int lo = 0, hi = I;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (ext[mid] <= row) lo = mid;
        else hi = mid;
    }
    return lo;
}
