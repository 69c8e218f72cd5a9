// init="parafac_als" / "cp_als" and "parafac_hals" / "cp_hals" (decomposition.py:55-75) for data resident in HBM: CP-ALS or
// CP-HALS on the zero-padded tensor X~ [I, Jmax, K] (row j >= J_i of slab i is a zero the model fits), deterministic start.
//
// Factors A [I, r], B [Jmax, r], C [K, r] are kept in fp64; B_i = B[:J_i] is what the caller receives.  Per sweep, modes A, B, C:
//     pass 1 (X):  XC = X C on the fp32 MFMA (C as fp32 fragments); epilogue: M_A partial per segment = sum_rows XC o B[j]
//     A <- update(M_A, G_A = B^T B o C^T C)
//     M_B = sum_i X~_i C diag(a_i) from the XC rows (no X traffic), slab groups then a fixed-order sum
//     B <- update(M_B, G_B = A^T A o C^T C)
//     pass 2 (X):  M_C = sum_i X_i^T (B[:J_i] diag(a_i)) on the fp32 MFMA, fp64 partials per row chunk, fixed-order sum
//     C <- update(M_C, G_C = A^T A o B^T B);  e_t = sqrt(max(0, |X|^2 - 2 <M_C, C> + 1^T (A^T A o B^T B o C^T C) 1)) / |X|
// update: ALS  F = M_F G_F^-1 (in-place Gauss-Jordan of the SPD r x r matrix; not positive definite: the pseudo-inverse from a
//         Jacobi eigen-decomposition, eigenvalues <= 1e-12 lam_max dropped);
//         HALS for q = 0..r-1: F[:,q] <- max(0, F[:,q] + (M_F[:,q] - F G_F[:,q]) / G_F[q,q])  (skipped where G_F[q,q] = 0).
// M_C needs the A and B of the same sweep, so two reads of X per sweep is the floor.  Every reduction has a fixed order and no
// float atomics are used: two runs are bitwise equal.
// The two X passes, the fragment layout of C, the r x r inverse, the row update and the fixed-order sum are cp_passes.h's, shared
// with parafac2als.hip; this file keeps the epilogues, the weights of pass 2 and the sweep.
// Start: C0 = the C of mcl_svd_init (the stack's right singular vectors), B0 = the leading eigenvectors of the padded-row Gram
// matrix sum_i X~_i X~_i^T (Jmax x Jmax, fp64), both with the entry of largest magnitude positive (HALS: clipped at 0); A0 = 1.
#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "cp_passes.h"

namespace {

static ErrorSlot g_als_error{"mcl_als_init: "};
constexpr int ALS_TARGET_WG = 1024;  // workgroups of pass 2 (row chunks x 64-column blocks)
enum { OP_LOAD = 0, OP_ALS = 1, OP_HALS = 2 };

inline int als_nb(int r) { return r <= 16 ? 1 : r <= 32 ? 2 : 4; }

// sum of a double over the 16 lanes of a DPP row (lanes with the same l >> 4); the total in every lane of the row
static __device__ __forceinline__ double row16_sum(double v) {
    v += dpp_mov_f64<0xB1>(v);
    v += dpp_mov_f64<0x4E>(v);
    v += dpp_mov_f64<0x141>(v);
    v += dpp_mov_f64<0x140>(v);
    return v;
}

// ---- pass 1: XC = X C, M_A partials ---------------------------------------------------------------------------------------
// One wave per segment (xc_segment, cp_passes.h); the epilogue stores the X C rows and the segment's partial of M_A.
template <class XL, int NB, bool VEC>
__global__ __launch_bounds__(256) void k_als_xc(const typename XL::T *__restrict__ X, const int4 *__restrict__ segs, int nseg, int K, int r,
                                                const float *__restrict__ Cfrag, const double *__restrict__ B64, float *__restrict__ XC,
                                                double *__restrict__ Pa) {
    __shared__ f32x4 tiles[4][16 * 16];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, seg = blockIdx.x * 4 + w;
    if (seg >= nseg) return;  // whole waves; no barrier below
    const int4 sg = segs[seg];
    const int row0 = sg.y, n = sg.z, j0 = sg.w;
    const int row16 = lane & 15, g = lane >> 4;
    f32x4 acc[4][NB];
    xc_segment<XL, NB, VEC>(X, sg, K, Cfrag, tiles[w], acc);
    double pa[NB][4];
#pragma unroll
    for (int hp = 0; hp < NB; ++hp)
#pragma unroll
        for (int v = 0; v < 4; ++v) pa[hp][v] = 0.0;
#pragma unroll
    for (int rb = 0; rb < 4; ++rb) {
        const int loc = 16 * rb + row16;
        if (loc >= n) continue;
#pragma unroll
        for (int hp = 0; hp < NB; ++hp)
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int q = 16 * hp + 4 * g + v;
                if (q < r) {
                    XC[(long)(row0 + loc) * r + q] = acc[rb][hp][v];
                    pa[hp][v] = fma((double)acc[rb][hp][v], B64[(long)(j0 + loc) * r + q], pa[hp][v]);
                }
            }
    }
#pragma unroll
    for (int hp = 0; hp < NB; ++hp)
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const double s = row16_sum(pa[hp][v]);
            const int q = 16 * hp + 4 * g + v;
            if (row16 == 0 && q < r) Pa[(long)seg * r + q] = s;
        }
}

// ---- pass 2: M_C partials = sum over the rows of a chunk of X^T (B[j] o a_i) ----------------------------------------------------
// Workgroup (chunk c = consecutive segments, 64-column block kb): xtw_segments (cp_passes.h) with the weights B[j][q] a_i[q],
// formed in fp64 and rounded to fp32; the four waves' fixed-order fp64 sum is the chunk's partial Pc[c][k][q].
template <class XL, int NB, bool VEC>
__global__ __launch_bounds__(256) void k_als_xtw(const typename XL::T *__restrict__ X, const int4 *__restrict__ segs,
                                                 const int *__restrict__ chunk_seg, int K, int r, const double *__restrict__ A64,
                                                 const double *__restrict__ B64, double *__restrict__ Pc) {
    __shared__ float red[3][NB * 16][64];
    const int c16 = threadIdx.x & 15, c = blockIdx.x, kb = blockIdx.y;
    f32x4 acc[4][NB];
    double bn[4][NB], an[NB];
    auto wload = [&](const int4 sg, const int(&loc)[4]) {
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
            const int q = min(16 * nb + c16, r - 1);
#pragma unroll
            for (int u = 0; u < 4; ++u) bn[u][nb] = B64[(long)(sg.w + loc[u]) * r + q];
            an[nb] = A64[(long)sg.x * r + q];
        }
    };
    xtw_segments<XL, NB, VEC>(X, segs, chunk_seg[c], chunk_seg[c + 1], K, r, kb, wload,
                              [&](int u, int nb) { return (float)(bn[u][nb] * an[nb]); }, acc);
    xtw_wave_sum<NB>(acc, red, [&](int kl, int q, double s) {
        const int k = 64 * kb + kl;
        if (k < K && q < r) Pc[((long)c * K + k) * r + q] = s;
    });
}

// ---- start: the padded-row Gram matrix P = sum_i X~_i X~_i^T [Jmax, Jmax] (fp64 sums of exact products) ----------------------
// 32 x 32 output tile per workgroup, upper triangle of tiles (mirrored); slabs in ascending order, then columns.
template <class XL>
__global__ __launch_bounds__(256) void k_als_rowgram(const typename XL::T *__restrict__ X, const int *__restrict__ ext, int I, int K, int Jm,
                                                     double *__restrict__ P) {
    if (blockIdx.y < blockIdx.x) return;
    __shared__ float As[32][33], Bs[32][33];
    const int a0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    double acc[2][2] = {{0.0, 0.0}, {0.0, 0.0}};
    for (int i = 0; i < I; ++i) {
        const long s0 = ext[i];
        const int n = ext[i + 1] - ext[i];
        if (n <= a0) continue;  // (c0 >= a0) the slab has no row in the tile's first range
        for (int k0 = 0; k0 < K; k0 += 32) {
            __syncthreads();
            for (int e = threadIdx.x; e < 32 * 32; e += 256) {
                const int jj = e >> 5, kk = e & 31;
                const bool okk = k0 + kk < K;
                As[kk][jj] = (okk && a0 + jj < n) ? XL::ld1(X + (s0 + a0 + jj) * K + k0 + kk) : 0.f;
                Bs[kk][jj] = (okk && c0 + jj < n) ? XL::ld1(X + (s0 + c0 + jj) * K + k0 + kk) : 0.f;
            }
            __syncthreads();
#pragma unroll 8
            for (int kk = 0; kk < 32; ++kk) {
                const double a_0 = (double)As[kk][2 * ty], a_1 = (double)As[kk][2 * ty + 1];
                const double b_0 = (double)Bs[kk][2 * tx], b_1 = (double)Bs[kk][2 * tx + 1];
                acc[0][0] = fma(a_0, b_0, acc[0][0]), acc[0][1] = fma(a_0, b_1, acc[0][1]);
                acc[1][0] = fma(a_1, b_0, acc[1][0]), acc[1][1] = fma(a_1, b_1, acc[1][1]);
            }
        }
    }
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int v = 0; v < 2; ++v) {
            const int a = a0 + 2 * ty + u, c = c0 + 2 * tx + v;
            if (a < Jm && c < Jm) P[(long)a * Jm + c] = acc[u][v], P[(long)c * Jm + a] = acc[u][v];
        }
}

// |X|^2 = trace(P), in row order
__global__ void k_als_trace(const double *__restrict__ P, int Jm, double *__restrict__ nx2) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double s = 0.0;
    for (int j = 0; j < Jm; ++j) s += P[(long)j * Jm + j];
    *nx2 = s;
}

// M_B partials: Pb[g][j][q] = sum over the slabs i of group g (ascending) with J_i > j of a_i[q] XC[row of (i, j)][q]
__global__ __launch_bounds__(256) void k_als_mb(const float *__restrict__ XC, const double *__restrict__ A64, const int *__restrict__ ext,
                                                const int *__restrict__ bgrp, int ngrp, int Jm, int r, double *__restrict__ Pb) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x, E = (long)Jm * r;
    if (e >= E * ngrp) return;
    const int gidx = (int)(e / E);
    const int rem = (int)(e - (long)gidx * E), j = rem / r, q = rem - j * r;
    double s = 0.0;
#pragma unroll 8
    for (int i = bgrp[gidx]; i < bgrp[gidx + 1]; ++i) {  // (rows past J_i: a clamped load, weight 0)
        const int s0 = ext[i], n = ext[i + 1] - s0;
        const double a = n > j ? A64[(long)i * r + q] : 0.0;
        s = fma(a, (double)XC[(n > 0 ? (long)s0 + min(j, n - 1) : 0L) * r + q], s);
    }
    Pb[e] = s;
}

// M_A[i][q] = sum of the partials of the segments of slab i, in segment order
__global__ __launch_bounds__(256) void k_als_segsum(const double *__restrict__ Pa, const int *__restrict__ slab_seg, int I, int r,
                                                    double *__restrict__ Ma) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= I * r) return;
    const int i = e / r, q = e - i * r;
    double s = 0.0;
    for (int g = slab_seg[i]; g < slab_seg[i + 1]; ++g) s += Pa[(long)g * r + q];
    Ma[e] = s;
}

// out[e] = sum_p part[p][e] in the order of fixed_order_sum (cp_passes.h), 64 elements per workgroup
__global__ __launch_bounds__(256) void k_als_reduce(const double *__restrict__ part, int np, long E, double *__restrict__ out) {
    __shared__ double red[256];
    const long e0 = (long)blockIdx.x * 64;
    fixed_order_sum<256>(part + e0, np, E, (int)min(64L, E - e0), out + e0, red);
}

// ---- the row update of one mode (one thread per row of F, 64 rows per workgroup) -------------------------------------------------
// op LOAD: F = the fp32 start (NULL: ones); ALS: F = M Ginv; HALS: one pass over the columns.  Then every workgroup writes its
// partial Gram matrix sum_rows F^T F (fp64, rows in order); mode C also its part of <M_C, C> and the fp32 fragments of C.
struct AlsUpd {
    int mode, op, n, r, NB;
    const double *M;      // [n, r]
    const float *F32;     // LOAD
    const double *Gm;     // [r, r]: G^-1 (ALS) or G (HALS)
    double *F64, *Gp, *Ep;
    float *Cfrag;
};

template <int RMAX>
__global__ __launch_bounds__(64) void k_als_update(AlsUpd u) {
    __shared__ double buf[64 * (RMAX + 1)];  // G (r x r) during the update, then the rows (64 x (RMAX + 1)) for the Gram partial
    __shared__ double ep[64];
    const int tid = threadIdx.x, row = blockIdx.x * 64 + tid, r = u.r;
    const bool ok = row < u.n;
    double *Gs = buf;
    if (u.op != OP_LOAD)
        for (int e = tid; e < r * r; e += 64) Gs[e] = u.Gm[e];
    __syncthreads();
    double m[RMAX], f[RMAX];
#pragma unroll
    for (int q = 0; q < RMAX; ++q) m[q] = 0.0, f[q] = 0.0;
    if (ok && u.op != OP_LOAD)
#pragma unroll
        for (int q = 0; q < RMAX; ++q)
            if (q < r) m[q] = u.M[(long)row * r + q];
    if (ok) {
        if (u.op == OP_LOAD) {
#pragma unroll
            for (int q = 0; q < RMAX; ++q)
                if (q < r) f[q] = u.F32 ? (double)u.F32[(long)row * r + q] : 1.0;
        } else if (u.op == OP_ALS) {
            factor_row_update<RMAX>(m, f, Gs, r, 0);
        } else {
#pragma unroll
            for (int q = 0; q < RMAX; ++q)
                if (q < r) f[q] = u.F64[(long)row * r + q];
            factor_row_update<RMAX>(m, f, Gs, r, 1);
        }
#pragma unroll
        for (int q = 0; q < RMAX; ++q)
            if (q < r) u.F64[(long)row * r + q] = f[q];
        if (u.mode == 2) {
#pragma unroll
            for (int q = 0; q < RMAX; ++q)
                if (q < r) u.Cfrag[cfrag_index(row, q, u.NB)] = (float)f[q];
        }
    }
    __syncthreads();  // (G is no longer read)
    double(*Fs)[RMAX + 1] = reinterpret_cast<double(*)[RMAX + 1]>(buf);
#pragma unroll
    for (int q = 0; q < RMAX; ++q) Fs[tid][q] = f[q];
    if (u.mode == 2) {
        double d = 0.0;
#pragma unroll
        for (int q = 0; q < RMAX; ++q) d = fma(m[q], f[q], d);
        ep[tid] = d;
    }
    __syncthreads();
    if (u.mode == 2 && tid == 0) {
        double d = 0.0;
#pragma unroll 16
        for (int t = 0; t < 64; ++t) d += ep[t];
        u.Ep[blockIdx.x] = d;
    }
    for (int e = tid; e < r * r; e += 64) {
        const int a = e / r, c = e - a * r;
        double s = 0.0;
#pragma unroll 16
        for (int t = 0; t < 64; ++t) s = fma(Fs[t][a], Fs[t][c], s);
        u.Gp[(long)blockIdx.x * r * r + e] = s;
    }
}

// ---- r x r work between the updates (one workgroup) ------------------------------------------------------------------------
// prev >= 0: Gram[prev] = the sum of the partial Gram matrices of the factor just updated.  t >= 0 (after mode C): the error
// e_t.  next >= 0: G_next = the Hadamard product of the other two Gram matrices; ALS: its inverse (pseudo-inverse when it is
// not positive definite: spd_inverse_lds, cp_passes.h), HALS: G itself, into Gm.
struct AlsPrep {
    int prev, nprev, next, method, t, r, nEp;
    const double *Gp;
    double *Gram;  // [3][r * r]
    double *Gm;
    const double *Ep, *nx2;
    double *ews, *errors;
};

__global__ __launch_bounds__(256) void k_als_prep(AlsPrep p) {
    extern __shared__ double sm[];
    const int r = p.r, rr = r * r, tid = threadIdx.x;
    double *S = sm, *W = S + rr, *cs = W + rr;
    if (p.prev >= 0)
        for (int e = tid; e < rr; e += 256) {
            double s = 0.0;
            for (int w = 0; w < p.nprev; ++w) s += p.Gp[(long)w * rr + e];
            p.Gram[p.prev * rr + e] = s;
        }
    __threadfence_block();
    __syncthreads();
    if (p.t >= 0) {  // 1^T (A^T A o B^T B o C^T C) 1 and <M_C, C>: per-thread sums in index order, then a fixed tree
        __shared__ double fit_sh[256], dot_sh[256];
        double fit = 0.0, d = 0.0;
        for (int e = tid; e < rr; e += 256) fit += p.Gram[e] * p.Gram[rr + e] * p.Gram[2 * rr + e];
        for (int w = tid; w < p.nEp; w += 256) d += p.Ep[w];
        fit_sh[tid] = fit, dot_sh[tid] = d;
        __syncthreads();
        for (int o = 128; o > 0; o >>= 1) {
            if (tid < o) fit_sh[tid] += fit_sh[tid + o], dot_sh[tid] += dot_sh[tid + o];
            __syncthreads();
        }
        if (tid == 0) {
            const double nx2 = *p.nx2;
            const double err = nx2 > 0.0 ? sqrt(fmax(0.0, nx2 - 2.0 * dot_sh[0] + fit_sh[0])) / sqrt(nx2) : 0.0;
            p.ews[0] = err;
            if (p.errors) p.errors[p.t] = err;
        }
    }
    if (p.next < 0) return;
    const int o1 = p.next == 0 ? 1 : 0, o2 = p.next == 2 ? 1 : 2;
    auto G = [&](int e) { return p.Gram[o1 * rr + e] * p.Gram[o2 * rr + e]; };
    for (int e = tid; e < rr; e += 256) S[e] = G(e);
    __syncthreads();
    if (p.method == 0) spd_inverse_lds<256>(S, W, cs, r, G);
    for (int e = tid; e < rr; e += 256) p.Gm[e] = S[e];
}

// outputs in fp32: A, B packed along the rows of X (B_i = B[:J_i]), C
__global__ __launch_bounds__(256) void k_als_out(const double *__restrict__ A64, const double *__restrict__ B64, const double *__restrict__ C64,
                                                 const int *__restrict__ ext, int I, int N, int K, int r, float *__restrict__ A,
                                                 float *__restrict__ B, float *__restrict__ C) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (blockIdx.y == 0) {
        if (e >= (long)N * r) return;
        const int row = (int)(e / r), q = (int)(e - (long)row * r);
        B[e] = (float)B64[(long)(row - ext[slab_of_row(ext, I, row)]) * r + q];
    } else if (blockIdx.y == 1) {
        if (e < (long)I * r) A[e] = (float)A64[e];
    } else {
        if (e < (long)K * r) C[e] = (float)C64[e];
    }
}

struct AlsPlan {
    int64_t N, Jm;
    int nseg, nchunk, nkb, ngrp, NB, KH, wgA, wgB, wgC;
    int4 *segs;
    int *slab_seg, *chunk_seg, *ext, *bgrp, *info;
    double *A, *B, *C, *Pa, *Pb, *Mb, *Pc, *Mc, *Ma, *Gp, *Ep, *Gram, *Gm, *small;
    float *Cfrag, *XC;
    char *scratch;
    int64_t svd_ws, gv_ws, total;
};

// workspace NULL: the parts are null and `total` is the size (mcl_als_init_workspace_bytes)
AlsPlan als_plan(void *workspace, const int64_t *row_ptr, int64_t I, int64_t K, int rank) {
    AlsPlan p{};
    p.N = row_ptr[I];
    p.Jm = 0;
    for (int64_t i = 0; i < I; ++i) p.Jm = std::max(p.Jm, row_ptr[i + 1] - row_ptr[i]);
    const int64_t nseg = seg_count(row_ptr, I);
    const int64_t r = rank;
    p.nseg = (int)nseg;
    p.nkb = (int)((K + 63) / 64);
    p.nchunk = (int)std::max<int64_t>(1, std::min<int64_t>(nseg, ALS_TARGET_WG / p.nkb));
    p.ngrp = (int)std::max<int64_t>(1, std::min<int64_t>(I, (262144 + p.Jm * r - 1) / std::max<int64_t>(p.Jm * r, 1)));
    p.NB = als_nb(rank);
    p.KH = 4 * (int)((K + 63) / 64);  // 16-row blocks of the C fragments, whole 64-column chunks (zero past K)
    p.wgA = (int)((I + 63) / 64), p.wgB = (int)((p.Jm + 63) / 64), p.wgC = (int)((K + 63) / 64);
    const int wgmax = std::max(p.wgA, std::max(p.wgB, p.wgC));
    WsCursor ws(workspace);
    p.segs = ws.take<int4>(std::max<int64_t>(nseg, 1) * 16);
    p.slab_seg = ws.take<int>((I + 1) * 4);
    p.chunk_seg = ws.take<int>((int64_t)(p.nchunk + 1) * 4);
    p.ext = ws.take<int>((I + 1) * 4);
    p.bgrp = ws.take<int>((int64_t)(p.ngrp + 1) * 4);
    p.A = ws.take<double>(I * r * 8);
    p.B = ws.take<double>(p.Jm * r * 8);
    p.C = ws.take<double>(K * r * 8);
    p.Cfrag = ws.take<float>((int64_t)p.KH * p.NB * 64 * 4 * 4);
    p.XC = ws.take<float>(p.N * r * 4);
    p.Pa = ws.take<double>(std::max<int64_t>(nseg, 1) * r * 8);
    p.Pb = ws.take<double>((int64_t)p.ngrp * p.Jm * r * 8);
    p.Mb = ws.take<double>(p.Jm * r * 8);
    p.Pc = ws.take<double>((int64_t)p.nchunk * K * r * 8);
    p.Mc = ws.take<double>(K * r * 8);
    p.Ma = ws.take<double>(I * r * 8);
    p.Gp = ws.take<double>((int64_t)3 * wgmax * r * r * 8);
    p.Ep = ws.take<double>((int64_t)p.wgC * 8);
    p.Gram = ws.take<double>(3 * r * r * 8);
    p.Gm = ws.take<double>(r * r * 8);
    p.small = ws.take<double>(4 * 8);  // |X|^2, e_t
    p.info = ws.take<int>((I + 2) * 4);
    // the start: mcl_svd_init's workspace + C0 (fp32), then P [Jmax, Jmax] + the subspace iteration's + B0 (fp32)
    p.svd_ws = (mcl_svd_stack_workspace_bytes(row_ptr, I, K, rank) + 255) & ~int64_t(255);
    p.gv_ws = (mcl_gram_vectors_workspace_bytes(p.Jm, rank) + 255) & ~int64_t(255);
    const int64_t s1 = p.svd_ws + K * r * 4;
    const int64_t s2 = ((p.Jm * p.Jm * 8 + 255) & ~int64_t(255)) + p.gv_ws + p.Jm * r * 4;
    p.scratch = ws.take<char>(std::max(s1, s2));
    p.total = ws.off;
    return p;
}

template <int RMAX>
void launch_update(const AlsUpd &u, hipStream_t s) {
    hipLaunchKernelGGL(k_als_update<RMAX>, dim3((unsigned)((u.n + 63) / 64)), dim3(64), 0, s, u);
}

void update(AlsUpd u, hipStream_t s) {
    if (u.r <= 16) launch_update<16>(u, s);
    else if (u.r <= 32) launch_update<32>(u, s);
    else launch_update<64>(u, s);
}

template <class XL>
int als_init(const typename XL::T *X, int32_t x_type, const int64_t *row_ptr, int64_t I, int64_t K, int32_t rank, int32_t method,
             int32_t n_iter_max, double tol, float *A, float *B, float *C, double *errors, int32_t *info, const AlsPlan &p, hipStream_t s) {
    auto fail = [](const std::string &msg) { return g_als_error.as_is(msg); };  // (a HIP call's or the svd start's message)
    double *nx2 = p.small, *ews = nx2 + 1;
    const int r = rank, Jm = (int)p.Jm, N = (int)p.N;
    const int wgmax = std::max(p.wgA, std::max(p.wgB, p.wgC));
    double *GpM[3] = {p.Gp, p.Gp + (int64_t)wgmax * r * r, p.Gp + (int64_t)2 * wgmax * r * r};
    const int nwg[3] = {p.wgA, p.wgB, p.wgC};

    // host-built tables: segments, per-slab segment ranges, row chunks of pass 2, slab groups of M_B
    SegTables h = seg_tables(row_ptr, I);
    std::vector<int> h_chunk((size_t)p.nchunk + 1), h_bgrp((size_t)p.ngrp + 1);
    if (h.segs.empty()) h.segs.push_back(int4{0, 0, 0, 0});
    for (int c = 0; c <= p.nchunk; ++c) h_chunk[(size_t)c] = (int)((int64_t)p.nseg * c / p.nchunk);
    for (int g = 0; g <= p.ngrp; ++g) h_bgrp[(size_t)g] = (int)(I * g / p.ngrp);
    CP_HIP(upload_tables(h, p.segs, p.slab_seg, p.ext, s));
    CP_HIP(upload(p.chunk_seg, h_chunk, s));
    CP_HIP(upload(p.bgrp, h_bgrp, s));
    CP_HIP(hipMemsetAsync(p.Cfrag, 0, (size_t)p.KH * p.NB * 64 * 4 * 4, s));
    CP_HIP(hipStreamSynchronize(s));  // (the tables are locals)

    const int hals = method == MCL_ALS_CP_HALS;
    // ---- start.  C0: the C of mcl_svd_init
    float *C32 = reinterpret_cast<float *>(p.scratch + p.svd_ws);
    std::string err;
    if (mcl_svd_stack_right(X, x_type, row_ptr, I, K, rank, hals, C32, p.scratch, p.svd_ws, p.info, s, err)) return fail(err);
    AlsUpd u{};
    u.r = r, u.NB = p.NB, u.op = OP_LOAD;
    u.mode = 2, u.n = (int)K, u.F32 = C32, u.F64 = p.C, u.Gp = GpM[2], u.Ep = p.Ep, u.Cfrag = p.Cfrag;
    update(u, s);
    // B0: the leading eigenvectors of the padded-row Gram matrix
    double *P = reinterpret_cast<double *>(p.scratch);
    char *gv = p.scratch + ((p.Jm * p.Jm * 8 + 255) & ~int64_t(255));
    float *B32 = reinterpret_cast<float *>(gv + p.gv_ws);
    const unsigned tj = (unsigned)((Jm + 31) / 32);
    hipLaunchKernelGGL(k_als_rowgram<XL>, dim3(tj, tj), dim3(256), 0, s, X, (const int *)p.ext, (int)I, (int)K, Jm, P);
    hipLaunchKernelGGL(k_als_trace, dim3(1), dim3(64), 0, s, (const double *)P, Jm, nx2);
    if (mcl_gram_vectors(P, p.Jm, rank, hals, B32, gv, p.info, (int)I + 1, s, err)) return fail(err);
    u.mode = 1, u.n = Jm, u.F32 = B32, u.F64 = p.B, u.Gp = GpM[1];
    update(u, s);
    u.mode = 0, u.n = (int)I, u.F32 = nullptr, u.F64 = p.A, u.Gp = GpM[0];  // A0 = 1
    update(u, s);

    const int rr = r * r;
    const size_t psm = sizeof(double) * (size_t)(2 * rr + 2 * (r / 2 + 2)) + 64;
    CP_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(k_als_prep), hipFuncAttributeMaxDynamicSharedMemorySize, (int)psm));
    auto prep = [&](int prev, int next, int t) {
        AlsPrep q{};
        q.prev = prev, q.nprev = prev >= 0 ? nwg[prev] : 0, q.next = next, q.method = hals, q.t = t, q.r = r, q.nEp = p.wgC;
        q.Gp = prev >= 0 ? GpM[prev] : nullptr, q.Gram = p.Gram, q.Gm = p.Gm, q.Ep = p.Ep, q.nx2 = nx2, q.ews = ews, q.errors = errors;
        hipLaunchKernelGGL(k_als_prep, dim3(1), dim3(256), psm, s, q);
    };
    prep(1, -1, -1);
    prep(0, -1, -1);
    prep(2, 0, -1);
    CP_HIP(hipGetLastError());

    const bool vec = K % 4 == 0 && mcl_x_vec_aligned(X, x_type);
    auto pass_nb = [&](bool second, auto nb) {  // XC and the M_A partials, or the M_C partials
        vec_dispatch(vec, [&](auto v) {
            constexpr int NB = decltype(nb)::value;
            constexpr bool VEC = decltype(v)::value;
            if (!second)
                hipLaunchKernelGGL((k_als_xc<XL, NB, VEC>), dim3((unsigned)((p.nseg + 3) / 4)), dim3(256), 0, s, X, (const int4 *)p.segs, p.nseg,
                                   (int)K, r, (const float *)p.Cfrag, (const double *)p.B, p.XC, p.Pa);
            else
                hipLaunchKernelGGL((k_als_xtw<XL, NB, VEC>), dim3((unsigned)p.nchunk, (unsigned)p.nkb), dim3(256), 0, s, X, (const int4 *)p.segs,
                                   (const int *)p.chunk_seg, (int)K, r, (const double *)p.A, (const double *)p.B, p.Pc);
        });
    };
    auto pass = [&](bool second) {
        if (p.NB == 1) pass_nb(second, std::integral_constant<int, 1>{});
        else if (p.NB == 2) pass_nb(second, std::integral_constant<int, 2>{});
        else pass_nb(second, std::integral_constant<int, 4>{});
    };
    const int op = hals ? OP_HALS : OP_ALS;
    double e_prev = 0.0;
    int used = 0;
    for (int t = 0; t < n_iter_max; ++t) {
        pass(false);
        u = AlsUpd{};
        u.r = r, u.NB = p.NB, u.op = op, u.Gm = p.Gm, u.Ep = p.Ep, u.Cfrag = p.Cfrag;
        hipLaunchKernelGGL(k_als_segsum, dim3((unsigned)((I * r + 255) / 256)), dim3(256), 0, s, (const double *)p.Pa, (const int *)p.slab_seg,
                           (int)I, r, p.Ma);
        u.mode = 0, u.n = (int)I, u.M = p.Ma, u.F64 = p.A, u.Gp = GpM[0];
        update(u, s);
        const long EB = (long)Jm * r;
        hipLaunchKernelGGL(k_als_mb, dim3((unsigned)((EB * p.ngrp + 255) / 256)), dim3(256), 0, s, (const float *)p.XC, (const double *)p.A,
                           (const int *)p.ext, (const int *)p.bgrp, p.ngrp, Jm, r, p.Pb);
        hipLaunchKernelGGL(k_als_reduce, dim3((unsigned)((EB + 63) / 64)), dim3(256), 0, s, (const double *)p.Pb, p.ngrp, EB, p.Mb);
        prep(0, 1, -1);
        u.mode = 1, u.n = Jm, u.M = p.Mb, u.F64 = p.B, u.Gp = GpM[1];
        update(u, s);
        prep(1, 2, -1);
        pass(true);
        const long EC = (long)K * r;
        hipLaunchKernelGGL(k_als_reduce, dim3((unsigned)((EC + 63) / 64)), dim3(256), 0, s, (const double *)p.Pc, p.nchunk, EC, p.Mc);
        u.mode = 2, u.n = (int)K, u.M = p.Mc, u.F64 = p.C, u.Gp = GpM[2];
        update(u, s);
        prep(2, 0, t);
        CP_HIP(hipGetLastError());
        used = t + 1;
        if (tol > 0.0) {  // TensorLy's abs_rec_error rule: one 8-byte read per sweep
            double e_t = 0.0;
            CP_HIP(hipMemcpyAsync(&e_t, ews, sizeof(double), hipMemcpyDeviceToHost, s));
            CP_HIP(hipStreamSynchronize(s));
            if (t >= 1 && std::fabs(e_prev - e_t) < tol) break;
            e_prev = e_t;
        }
    }
    const long big = std::max<long>((long)N, std::max<long>((long)I, (long)K)) * r;
    hipLaunchKernelGGL(k_als_out, dim3((unsigned)((big + 255) / 256), 3), dim3(256), 0, s, (const double *)p.A, (const double *)p.B,
                       (const double *)p.C, (const int *)p.ext, (int)I, N, (int)K, r, A, B, C);
    CP_HIP(hipGetLastError());
    CP_HIP(hipMemcpyAsync(info, &used, sizeof(int32_t), hipMemcpyHostToDevice, s));
    CP_HIP(hipStreamSynchronize(s));  // (`used` is a local)
    return 0;
}

// (a matrix may have fewer rows than the rank: the padded tensor has Jmax rows in every slab)
std::string check_args(const int64_t *row_ptr, int64_t I, int64_t K, int32_t rank) {
    const std::string bad = packed_args_error(row_ptr, I, K, rank, MCL_MAX_RANK);
    if (!bad.empty()) return bad;
    if (row_ptr[0] != 0) return "row_ptr[0] must be 0";
    int64_t Jm = 0;
    for (int64_t i = 0; i < I; ++i) {
        if (row_ptr[i + 1] < row_ptr[i]) return "row_ptr must be non-decreasing";
        Jm = std::max(Jm, row_ptr[i + 1] - row_ptr[i]);
    }
    if (K > 2048 || Jm > 2048) return "K and the longest matrix must be at most 2048 (the start's Gram matrices)";
    if (rank > K || rank > Jm) return "rank exceeds min(longest matrix, K)";
    if (row_ptr[I] >= (int64_t(1) << 31)) return "more than 2^31 packed rows are not supported";
    return "";
}

}  // namespace

extern "C" {

const char *mcl_als_init_last_error(void) { return g_als_error.c_str(); }

int64_t mcl_als_init_workspace_bytes(const int64_t *row_ptr, int64_t I, int64_t K, int32_t rank) {
    if (!check_args(row_ptr, I, K, rank).empty()) return -1;
    return als_plan(nullptr, row_ptr, I, K, rank).total;
}

int mcl_als_init_typed(const void *X, int32_t x_type, const int64_t *row_ptr, int64_t I, int64_t K, int32_t rank, int32_t method,
                       int32_t n_iter_max, double tol, float *A, float *B, float *C, double *errors, int32_t *info, void *workspace,
                       int64_t workspace_bytes, void *hip_stream) {
    ErrorSlot &fail = g_als_error;
    const std::string bad = check_args(row_ptr, I, K, rank);
    if (!bad.empty()) return fail(bad);
    if (!X || !A || !B || !C || !info || !workspace) return fail("NULL argument");
    if (!x_type_error(x_type).empty()) return fail(x_type_error(x_type));
    if (method != MCL_ALS_CP && method != MCL_ALS_CP_HALS)
        return fail("unknown method " + std::to_string(method) + " (MCL_ALS_CP = 0, MCL_ALS_CP_HALS = 1)");
    if (n_iter_max < 0 || !(tol >= 0.0)) return fail("need n_iter_max >= 0 and tol >= 0");
    const AlsPlan p = als_plan(workspace, row_ptr, I, K, rank);
    if (workspace_refused(fail, workspace, workspace_bytes, p.total, "mcl_als_init_workspace_bytes")) return 1;
    hipStream_t s = reinterpret_cast<hipStream_t>(hip_stream);
    return mcl_x_dispatch(x_type, [&](auto xl) {
        using XL = decltype(xl);
        return als_init<XL>(static_cast<const typename XL::T *>(X), x_type, row_ptr, I, K, rank, method, n_iter_max, tol, A, B, C, errors, info,
                            p, s);
    });
}

}  // extern "C"
