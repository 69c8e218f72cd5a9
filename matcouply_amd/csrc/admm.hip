// ADMM-side kernels of the AO-ADMM engine (gfx950): rank x rank normal-equation algebra (fp64, in LDS),
// the B-phase systems, the exact fp64 solves, the fused inner ADMM loop for row-separable penalties and the C-phase
// finish built on it.  (The A-phase finish: afinish.h, included at the end; diagnostics and the stopping rule: diag.hip.)
//
// Reference sites: B1/B3-B5 (decomposition.py:240-256), B6-B9 (:259-285), C2-C3 (:319-338),
// prox: penalties.py:503-586.
#include <cstdlib>
#include <type_traits>

#include "mcl_internal.h"
#include "xload.h"
#include "gj_inverse.h"

// ---------------------------------------------------------------------------------------------------------
// CtC = C^T C  (fp64 accumulation, one workgroup; C staged through LDS in row chunks)
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_ctc(const float *__restrict__ C, int K, int r, int RP,
                                               float *__restrict__ CtC, double *__restrict__ CtC64) {
    // block a computes row a of CtC; thread (b = t % RP, ks = t / RP) strides over k
    __shared__ double sm[256];
    const int a = blockIdx.x;
    const int b = threadIdx.x % RP, ks = threadIdx.x / RP, nks = 256 / RP;
    double acc = 0.0;
    if (b < r)
        for (int k = ks; k < K; k += nks) acc += (double)C[(long)k * r + a] * (double)C[(long)k * r + b];
    sm[threadIdx.x] = acc;
    __syncthreads();
    if ((int)threadIdx.x < RP && b < r) {
        double t = 0.0;
        for (int q = 0; q < nks; ++q) t += sm[q * RP + b];
        CtC[a * r + b] = (float)t;
        CtC64[a * r + b] = t;
    }
}

// ---------------------------------------------------------------------------------------------------------
// B-phase systems: rho_i = 1/2 tr(CtC o a_i a_i^T) * scale ; L_i = CtC o a_i a_i^T + (rho_i n + l2) I ; L_i^-1
// ---------------------------------------------------------------------------------------------------------
__global__ void k_B_rho(const double *__restrict__ CtC, const float *__restrict__ A, int I, int r, float scale,
                        float *__restrict__ rhoB, float *__restrict__ rho_max) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= I) return;
    double s = 0.0;
    for (int c = 0; c < r; ++c) {
        const double a = A[(long)i * r + c];
        s += CtC[c * r + c] * a * a;
    }
    const float rho = rho_of_trace(s, scale);
    rhoB[i] = rho;
    atomicMax(reinterpret_cast<int *>(rho_max), __float_as_int(rho));  // rho >= 0: int order == float order
}

template <int RP>
__global__ __launch_bounds__(256) void k_B_systems(const double *__restrict__ CtC, const float *__restrict__ A, int I,
                                                   int r, float scale, float l2, int n_regs, int constant,
                                                   const float *__restrict__ rho_max, float *__restrict__ rhoB,
                                                   float *__restrict__ Linv, double *__restrict__ Linv64) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);  // one wave per slab
    if (i >= I) return;
    const float *a = A + (long)i * r;
    double tr = 0.0;
    for (int c = 0; c < r; ++c) tr += CtC[c * r + c] * (double)a[c] * (double)a[c];
    float rho = rho_of_trace(tr, scale);
    if (constant) rho = rho_max[0];
    const double shift = (double)rho * n_regs + (double)l2;
    const bool act = lane < r;
    const double ac = act ? (double)a[lane] : 0.0;
    double col[RP];
#pragma unroll
    for (int d = 0; d < RP; ++d) {
        double v = (d == lane) ? 1.0 : 0.0;
        if (act && d < r) v = CtC[d * r + lane] * (double)a[d] * ac + (d == lane ? shift : 0.0);
        col[d] = v;
    }
    gj_inverse_reg<RP>(col, r, lane);
#pragma unroll
    for (int d = 0; d < RP; ++d)
        if (act && d < r) {
            Linv[((long)i * r + d) * r + lane] = (float)col[d];
            if (Linv64 != nullptr) Linv64[((long)i * r + d) * r + lane] = col[d];
        }
    if (lane == 0) rhoB[i] = rho;
}

// Penalty-free B (decomposition.py:266-273 with an empty penalty list): B_i = ((X_i C) o a_i) L_i^-1 with un-shifted (or
// only l2-shifted) systems - the product runs in fp64 with the fp64 inverse, one wave per tile of <= 64 rows, lane c
// owning column c of L_i^-1; the row's right-hand side entries are fetched with v_readlane.
// X C in fp64 for that solve: the un-shifted systems would amplify the rounding of an fp32 contraction (1e-7 over a
// K-long chain) by their condition number - the products of fp32 values are exact in fp64, so XC64 carries only the
// final fp64 roundings.  A wave owns 16 packed rows; per 16 columns of K: lane (i = l & 15, kk = l >> 4) holds
// X[row0 + i][k0 + 4 kk .. + 3], step s of the fp64 MFMA pairs it with C[k0 + 4 kk + s][16 nb + (l & 15)]
// (D: row = (l >> 4) + 4 reg, col = l & 15).  Only used when mode 1 has no penalty: a rare, accuracy-first path.
template <class XL, int NB>
static __device__ __forceinline__ void k_contract_xc_f64_body(const typename XL::T *X, const float *C, long N, int K, int r, double *XC64, float *XC32) {
    typedef double f64x4 __attribute__((ext_vector_type(4)));
    const int lane = threadIdx.x & 63;
    const long row0 = ((long)blockIdx.x * 4 + (threadIdx.x >> 6)) * 16;
    if (row0 >= N) return;
    const int i = lane & 15, kk = lane >> 4;
    const long jx = min(row0 + i, N - 1);
    f64x4 acc[NB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) acc[nb] = f64x4{0.0, 0.0, 0.0, 0.0};
    for (int k0 = 0; k0 < K; k0 += 32) {  // two 16-column steps per trip: their loads are independent and issued together
        float xv[2][4], cv[2][NB][4];
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const int k = k0 + 16 * h + 4 * kk + s;
                const int kc = min(k, K - 1);  // unconditional loads at clamped indices, masked by a multiplication (no branch per load)
                xv[h][s] = XL::ld1(X + jx * K + kc) * ((k < K) ? 1.f : 0.f);
#pragma unroll
                for (int nb = 0; nb < NB; ++nb) {
                    const int col = 16 * nb + i;
                    cv[h][nb][s] = C[(long)kc * r + min(col, r - 1)] * ((k < K && col < r) ? 1.f : 0.f);
                }
            }
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int s = 0; s < 4; ++s)
#pragma unroll
                for (int nb = 0; nb < NB; ++nb)
                    acc[nb] = __builtin_amdgcn_mfma_f64_16x16x4f64((double)xv[h][s], (double)cv[h][nb][s], acc[nb], 0, 0, 0);
    }
#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const long j = row0 + kk + 4 * v;
            const int col = 16 * nb + i;
            if (j < N && col < r) {
                XC64[j * r + col] = acc[nb][v];
                if (XC32 != nullptr) XC32[j * r + col] = (float)acc[nb][v];  // exact-products mode: the image the row kernels read
            }
        }
}
template <int NB>
__global__ __launch_bounds__(256) void k_contract_xc_f64(const float *__restrict__ X, const float *__restrict__ C, long N,
                                                         int K, int r, double *__restrict__ XC64,
                                                         float *__restrict__ XC32 = nullptr) {
    k_contract_xc_f64_body<XF32, NB>(X, C, N, K, r, XC64, XC32);
}
// the 16-bit twin (xload.h): the same template arguments after the element type
template <class XL, int NB>
__global__ __launch_bounds__(256) void k_contract_xc_f64_h(const typename XL::T *__restrict__ X, const float *__restrict__ C, long N,
                                                         int K, int r, double *__restrict__ XC64,
                                                         float *__restrict__ XC32 = nullptr) {
    k_contract_xc_f64_body<XL, NB>(X, C, N, K, r, XC64, XC32);
}

template <int RP>
__global__ __launch_bounds__(256) void k_B_solve_f64(const int *__restrict__ tile_slab, const int *__restrict__ tile_row0,
                                                     const int *__restrict__ tile_nrows, int n_tiles,
                                                     const double *__restrict__ XC, const float *__restrict__ A,
                                                     const double *__restrict__ Linv64, int r, float *__restrict__ B,
                                                     const int *__restrict__ gate) {
    MCL_GATE(gate);
    const int lane = threadIdx.x & 63;
    const int tile = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (tile >= n_tiles) return;
    const int slab = __builtin_amdgcn_readfirstlane(tile_slab[tile]);
    const long row0 = __builtin_amdgcn_readfirstlane(tile_row0[tile]);
    const int nrows = __builtin_amdgcn_readfirstlane(tile_nrows[tile]);
    const bool act = lane < r;
    const int c = act ? lane : 0;
    double col[RP];
#pragma unroll
    for (int d = 0; d < RP; ++d) col[d] = (act && d < r) ? Linv64[((long)slab * r + d) * r + c] : 0.0;
    const double a = act ? (double)A[(long)slab * r + c] : 0.0;
    for (int j = 0; j < nrows; ++j) {
        const double t = act ? XC[(row0 + j) * r + c] * a : 0.0;
        double acc = 0.0;
#pragma unroll
        for (int d = 0; d < RP; ++d)
            if (d < r) acc = fma(readlane_f64_u(t, d), col[d], acc);
        if (act) B[(row0 + j) * r + c] = (float)acc;
    }
}

// C-phase system from the (all-reduced) fp64 normal equations [G | R]: block 0 builds and inverts G + (rho n + l2) I
// (fp32 and fp64 copies of the inverse), the other blocks round R to the fp32 image the fp32 row kernels read.
template <int RP>
__global__ __launch_bounds__(64) void k_C_prepare(const double *__restrict__ GR, int r, int K, float scale, float l2,
                                                  int n_regs, float *__restrict__ rhoC, float *__restrict__ LinvC,
                                                  double *__restrict__ LinvC64, float *__restrict__ Rf) {
    const int lane = threadIdx.x;
    if (blockIdx.x > 0) {
        const long e = (long)(blockIdx.x - 1) * 64 + lane;
        if (e < (long)K * r) Rf[e] = (float)GR[(long)r * r + e];
        return;
    }
    double tr = 0.0;
    for (int c = 0; c < r; ++c) tr += GR[c * r + c];
    const float rho = rho_of_trace(tr, scale);
    const double shift = (double)rho * n_regs + (double)l2;
    const bool act = lane < r;
    double col[RP];
#pragma unroll
    for (int d = 0; d < RP; ++d) {
        double v = (d == lane) ? 1.0 : 0.0;
        if (act && d < r) v = GR[d * r + lane] + (d == lane ? shift : 0.0);
        col[d] = v;
    }
    gj_inverse_reg<RP>(col, r, lane);
#pragma unroll
    for (int d = 0; d < RP; ++d)
        if (act && d < r) {
            LinvC[d * r + lane] = (float)col[d];
            LinvC64[d * r + lane] = col[d];
        }
    if (lane == 0) rhoC[0] = rho;
}

// Penalty-free C (decomposition.py:328-331 with an empty penalty list): C = R G^-1 is a plain least-squares solve whose
// normal equations are not shifted, so the product is taken in fp64 from the fp64 [G | R] and rounded once.
__global__ __launch_bounds__(256) void k_C_solve_f64(const double *__restrict__ R, const double *__restrict__ Linv, int K,
                                                     int r, float *__restrict__ C, const int *__restrict__ gate) {
    MCL_GATE(gate);
    extern __shared__ double Ls[];
    for (int e = threadIdx.x; e < r * r; e += 256) Ls[e] = Linv[e];
    __syncthreads();
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long)K * r) return;
    const int k = (int)(e / r), c = (int)(e - (long)k * r);
    double acc = 0.0;
    for (int d = 0; d < r; ++d) acc = fma(R[(long)k * r + d], Ls[d * r + c], acc);
    C[e] = (float)acc;
}

// ---------------------------------------------------------------------------------------------------------
// Fused inner ADMM loop for row-separable penalties (NN / Box / L1), `inner` iterations in registers:
//   t   = rhs + rho * sum_k (z_k - u_k)            decomposition.py:269-273 / 328-331
//   f   = t L^-1                                   as v_mfma_f32_16x16x4_f32 on the TRANSPOSED problem
//   z_k = prox_k(f + u_k, rho) ; u_k = f - (z_k - u_k)     decomposition.py:278-285 / 337-338
// A wave owns a tile of <= 64 rows of one slab = 4 blocks of 16 rows.  Lane l = (row = l&15, g = l>>4) holds,
// for every 16-column block h, the 4 consecutive columns 16h + 4g .. +3 of its row (one 16-B load; the 64
// lanes of a wave cover 16 full rows = one contiguous 1 KB region when r = 16).
// MFMA (h', h, kq):  D[c'][row] += A[c'][kk] * B[kk][row]  with  kk = g,  k = 16h + 4g + kq:
//     A (lane (c' = l&15, g)) = L^-1[k][16h' + c']        B (lane (row = l&15, g)) = t[row][k]
//     D (lane l, reg v)       = f[row = l&15][16h' + 4g + v]
// i.e. the k-permutation is chosen so that the INPUT fragment layout equals the OUTPUT layout: the inner
// iterations need no cross-lane data movement at all.
// Per-tile diagnostics (fp64): ||f||^2, sum|f|, ||z_k - f||^2.
// ---------------------------------------------------------------------------------------------------------

// One block of 16 rows of the fused inner loop in a wave's registers: rhs (already rounded to fp32), aux and dual.
// All loads are unconditional (padding lanes re-read a valid address of the same row: their values only ever meet the
// zero entries of the L^-1 fragments and are never stored), so they leave back to back and a caller can issue them
// long before the values are needed (k_C_finish_fused: under the Gauss-Jordan of wave 0).
template <int NBR, int NREG, bool VEC>
struct RowBlock {
    static constexpr int NR = NREG > 0 ? NREG : 1;
    f32x4 rhs[NBR], z[NR][NBR], u[NR][NBR];

    static __device__ __forceinline__ f32x4 ld4(const float *__restrict__ base, long j, int col, int r) {
        if (VEC) return *reinterpret_cast<const f32x4 *>(base + j * r + (col < r ? col : 0));
        f32x4 v;
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] = base[j * r + min(col + q, r - 1)];
        return v;
    }
    // j: a VALID row for every lane (lanes past the tile's end pass the tile's first row)
    __device__ __forceinline__ void load(int lane, long j, int r, const float *__restrict__ rhs_src,
                                         const double *__restrict__ rhs64, const RegSet &regs) {
        const int g = lane >> 4;
#pragma unroll
        for (int h = 0; h < NBR; ++h) {
            const int col = 16 * h + 4 * g;
            if (rhs64 != nullptr) {  // fp64 [G | R] of the C-phase, rounded on load
                if (VEC) {
                    const double *src = rhs64 + j * r + (col < r ? col : 0);
#pragma unroll
                    for (int v = 0; v < 4; ++v) rhs[h][v] = (float)src[v];
                } else {
#pragma unroll
                    for (int v = 0; v < 4; ++v) rhs[h][v] = (float)rhs64[j * r + min(col + v, r - 1)];
                }
            } else {
                rhs[h] = ld4(rhs_src, j, col, r);
            }
#pragma unroll
            for (int k = 0; k < NREG; ++k) {
                z[k][h] = ld4(regs.aux[k], j, col, r);
                u[k][h] = ld4(regs.dual[k], j, col, r);
            }
        }
    }
};

// One wave's share of the fused inner loop: a tile of <= 64 rows [row0, row0 + nrows) of one slab.
// Li: the slab's L^-1 (global or LDS), Arow: the slab's a_i or nullptr, Fcopy: optional second destination (LDS).
// pre: the tile's first row block, loaded by the caller (or nullptr).
// Returns the tile's diagnostic sums (already reduced over the wave) in dg[0..1+NREG].
template <int NBR, int NREG, bool VEC>
static __device__ __forceinline__ void rows_fused_tile(int lane, long row0, int nrows, float rho, const float *Li,
                                                       const float *Arow, const float *__restrict__ rhs_src,
                                                       float *__restrict__ F, float *Fcopy, const RegSet &regs, int r,
                                                       int inner, double *dg, const double *__restrict__ rhs64 = nullptr,
                                                       const RowBlock<NBR, NREG, VEC> *pre = nullptr) {
    const int row16 = lane & 15, g = lane >> 4;
    constexpr int NR = NREG > 0 ? NREG : 1;

    // A-operand fragments of (L^-1)^T (clamped addresses, masked values: the reads leave together)
    float LT[NBR][NBR][4];
#pragma unroll
    for (int hp = 0; hp < NBR; ++hp)
#pragma unroll
        for (int h = 0; h < NBR; ++h)
#pragma unroll
            for (int kq = 0; kq < 4; ++kq) {
                const int k = 16 * h + 4 * g + kq, c = 16 * hp + row16;
                const float v = Li[min(k, r - 1) * r + min(c, r - 1)];
                LT[hp][h][kq] = (k < r && c < r) ? v : 0.f;
            }
    float av[NBR][4];
#pragma unroll
    for (int h = 0; h < NBR; ++h)
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const int col = 16 * h + 4 * g + v;
            av[h][v] = (Arow != nullptr && col < r) ? Arow[col] : 1.f;
        }
    ProxClamp prox[NR];  // branch-free prox of the row-separable penalties (penalties.py:503-586)
#pragma unroll
    for (int k = 0; k < NR; ++k) {
        if (k < NREG) prox[k].set(regs.kind[k], regs.nonneg[k], regs.p0[k], regs.p1[k], regs.p0[k] / rho);
        else prox[k].set(0, 0, 0.f, 0.f, 0.f);
    }

    double nf = 0.0, na = 0.0, gap[NR];
#pragma unroll
    for (int k = 0; k < NR; ++k) gap[k] = 0.0;

    auto st4 = [&](float *__restrict__ base, long j, int col, bool ok, f32x4 v) {
        if (VEC) {
            if (ok && col < r) *reinterpret_cast<f32x4 *>(base + j * r + col) = v;
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (ok && col + q < r) base[j * r + col + q] = v[q];
        }
    };

    const int n_it = (NREG == 0 && inner > 1) ? 1 : inner;  // without penalties every inner solve is identical
#pragma unroll
    for (int rb = 0; rb < 4; ++rb) {
        if (16 * rb >= nrows) break;  // wave-uniform
        const bool ok = 16 * rb + row16 < nrows;
        const long j = (long)row0 + 16 * rb + (ok ? row16 : 0);
        RowBlock<NBR, NREG, VEC> blk;
        if (rb == 0 && pre != nullptr)
            blk = *pre;
        else
            blk.load(lane, j, r, rhs_src, rhs64, regs);
        f32x4(&rhs)[NBR] = blk.rhs;
        f32x4(&z)[NR][NBR] = blk.z;
        f32x4(&u)[NR][NBR] = blk.u;
        f32x4 f[NBR];
#pragma unroll
        for (int h = 0; h < NBR; ++h) {
#pragma unroll
            for (int v = 0; v < 4; ++v) rhs[h][v] *= av[h][v];
            f[h] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
        for (int it = 0; it < n_it; ++it) {
            f32x4 t[NBR];
#pragma unroll
            for (int h = 0; h < NBR; ++h) {
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    float s = 0.f;
#pragma unroll
                    for (int k = 0; k < NREG; ++k) s += z[k][h][v] - u[k][h][v];
                    t[h][v] = (NREG > 0) ? fmaf(rho, s, rhs[h][v]) : rhs[h][v];
                }
            }
#pragma unroll
            for (int hp = 0; hp < NBR; ++hp) {
                f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int h = 0; h < NBR; ++h)
#pragma unroll
                    for (int kq = 0; kq < 4; ++kq) acc = MFMA16(LT[hp][h][kq], t[h][kq], acc);
                f[hp] = acc;
            }
#pragma unroll
            for (int k = 0; k < NREG; ++k) {
#pragma unroll
                for (int h = 0; h < NBR; ++h)
#pragma unroll
                    for (int v = 0; v < 4; ++v) {
                        const float y = f[h][v] + u[k][h][v];
                        const float zn = prox[k](y);
                        u[k][h][v] = f[h][v] - (zn - u[k][h][v]);
                        z[k][h][v] = zn;
                    }
            }
        }
#pragma unroll
        for (int h = 0; h < NBR; ++h) {
            const int col = 16 * h + 4 * g;
            st4(F, j, col, ok, f[h]);
            if (Fcopy != nullptr) st4(Fcopy, j, col, ok, f[h]);
#pragma unroll
            for (int k = 0; k < NREG; ++k) {
                st4(regs.aux[k], j, col, ok, z[k][h]);
                st4(regs.dual[k], j, col, ok, u[k][h]);
            }
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                if (ok && col + v < r) {
                    const double fv = (double)f[h][v];
                    nf += fv * fv;
                    na += fabs(fv);
#pragma unroll
                    for (int k = 0; k < NREG; ++k) {
                        const double dlt = (double)z[k][h][v] - fv;
                        gap[k] += dlt * dlt;
                    }
                }
            }
        }
    }
    dg[0] = wave_sum(nf);
    dg[1] = wave_sum(na);
#pragma unroll
    for (int k = 0; k < NREG; ++k) dg[2 + k] = wave_sum(gap[k]);
}

template <int NBR, int NREG, bool VEC>
__global__ __launch_bounds__(256) void k_rows_fused(const int *__restrict__ tile_slab, const int *__restrict__ tile_row0,
                                                    const int *__restrict__ tile_nrows, int n_tiles,
                                                    const float *__restrict__ rhs_src, const float *__restrict__ Arows,
                                                    const float *__restrict__ rho_arr, const float *__restrict__ Linv,
                                                    float *__restrict__ F, RegSet regs, int r, int inner,
                                                    double *__restrict__ diag_tile) {
    MCL_GATE(regs.gate);
    __shared__ double dsm[4][DIAG_COLS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int tile_raw = blockIdx.x * 4 + wave;
    const bool live = tile_raw < n_tiles;       // wave-uniform; dead waves do no memory traffic (nrows = 0)
    const int tile = live ? tile_raw : n_tiles - 1;
    const int slab = __builtin_amdgcn_readfirstlane(tile_slab[tile]);
    const int row0 = __builtin_amdgcn_readfirstlane(tile_row0[tile]);
    const int nrows = live ? __builtin_amdgcn_readfirstlane(tile_nrows[tile]) : 0;
    double dg[DIAG_COLS];
    rows_fused_tile<NBR, NREG, VEC>(lane, row0, nrows, rho_arr[slab], Linv + (long)slab * r * r,
                                    Arows ? Arows + (long)slab * r : nullptr, rhs_src, F, nullptr, regs, r, inner, dg);
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 2 + NREG; ++k) dsm[wave][k] = dg[k];
    }
    __syncthreads();
    if (threadIdx.x < 2 + NREG)  // one diagnostics row per BLOCK (4 tiles), fixed summation order
        diag_tile[(long)blockIdx.x * DIAG_COLS + threadIdx.x] =
            (dsm[0][threadIdx.x] + dsm[1][threadIdx.x]) + (dsm[2][threadIdx.x] + dsm[3][threadIdx.x]);
}

// ---------------------------------------------------------------------------------------------------------
// The two parts the C-side finish kernels (k_C_finish_fused, k_C_finish_multi) share.
// ---------------------------------------------------------------------------------------------------------
// One wave: the C-phase system G + (rho n + l2) I from the all-reduced fp64 [G | R], inverted in the row-split layout of
// GJRows<RP> (lane = g * RP + c holds rows g * RL + j of column c): all loads in flight at once (clamped indices, masked at
// use), all 64 lanes busy in the Gauss-Jordan.  The inverse goes to LDS (Ls; Ls64 for the penalty-free fp64 solve) and rho to
// *rho_s; to_global: also to LinvC / rhoC.
template <int RP, int NREG>
static __device__ __forceinline__ void c_finish_system(const double *GR, int r, float scale, float l2, int lane, float *Ls,
                                                       double *Ls64, float *rho_s, bool to_global, float *LinvC,
                                                       float *rhoC) {
    constexpr int RL = GJRows<RP>::RL;
    const int cc = lane % RP, g = lane / RP;
    const bool act = cc < r;
    const int cl = act ? cc : 0;
    double gv[RL];
    double tr = 0.0;
#pragma unroll
    for (int j = 0; j < RL; ++j) {
        const int d = g * RL + j;
        gv[j] = GR[(d < r ? d : r - 1) * r + cl];
    }
#pragma unroll
    for (int j = 0; j < RL; ++j)
        if (act && g * RL + j == cc) tr = gv[j];
    tr = wave_sum(tr);
    const float rho = rho_of_trace(tr, scale);
    const double shift = (double)rho * NREG + (double)l2;
    double col[RL];
#pragma unroll
    for (int j = 0; j < RL; ++j) {
        const int d = g * RL + j;
        double v = (d == cc) ? 1.0 : 0.0;
        if (act && d < r) v = gv[j] + (d == cc ? shift : 0.0);
        col[j] = v;
    }
    gj_inverse_rows<RP>(col, r, lane);
#pragma unroll
    for (int j = 0; j < RL; ++j) {
        const int d = g * RL + j;
        if (act && d < r) {
            Ls[d * r + cc] = (float)col[j];
            if (NREG == 0) Ls64[d * r + cc] = col[j];
            if (to_global) LinvC[d * r + cc] = (float)col[j];
        }
    }
    if (lane == 0) {
        *rho_s = rho;
        if (to_global) rhoC[0] = rho;
    }
}

// One wave's rows [row0, row0 + nrows) of the penalty-free C = R G^-1 in fp64 (un-shifted normal equations: every rounding of
// the product is amplified by cond(G)), to C and its LDS copy Cs (both indexed by the global row); dg[0..1]: ||C||^2, sum|C|.
static __device__ __forceinline__ void c_solve_plain_f64(const double *R, const double *Ls64, int lane, long row0, int nrows,
                                                         int r, int inner, float *C, float *Cs, double *dg) {
    double nf = 0.0, na = 0.0;
    if (inner > 0)
        for (int e = lane; e < nrows * r; e += 64) {
            const int rl = e / r, cidx = e - rl * r;
            const long j = row0 + rl;
            double acc = 0.0;
            for (int d = 0; d < r; ++d) acc = fma(R[j * r + d], Ls64[d * r + cidx], acc);
            const float f = (float)acc;
            C[j * r + cidx] = f;
            Cs[j * r + cidx] = f;
            nf += (double)f * (double)f;
            na += fabs((double)f);
        }
    dg[0] = wave_sum(nf);
    dg[1] = wave_sum(na);
}

// ---------------------------------------------------------------------------------------------------------
// Whole C-side finish in ONE workgroup (K <= 1024 rows): system from the all-reduced [G | R] (decomposition.py:319-321)
// -> fused inner loop on the rows of C (:325-338) -> CtC = C^T C (fp64) and the MFMA-fragment image of C for the
// next X C pass.  Replaces four dependent launches (k_C_prepare, k_rows_fused, k_ctc, k_build_cfrag).
// LDS: L^-1 [r*r] | C [K*r] (fp32).
// ---------------------------------------------------------------------------------------------------------
template <int NBR, int NREG, bool VEC>
__global__ __launch_bounds__(1024) void k_C_finish_fused(const double *__restrict__ GR, int K, int r, float scale, float l2,
                                                         float *__restrict__ rhoC, float *__restrict__ LinvC,
                                                         float *__restrict__ C, RegSet regs, int inner,
                                                         float *__restrict__ CtC, double *__restrict__ CtC64,
                                                         float *__restrict__ Cfrag, int KC, int NBc,
                                                         double *__restrict__ diag_row, int rows_per_wave) {
    MCL_GATE(regs.gate);
    extern __shared__ float smc[];
    __shared__ double dsm[16][DIAG_COLS];
    __shared__ float rho_s;
    __shared__ double Ls64[NREG == 0 ? 256 * NBR * NBR : 1];  // penalty-free C: the solve itself runs in fp64
    float *Ls = smc, *Cs = smc + r * r;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n_waves = blockDim.x >> 6;
    constexpr int RP = 16 * NBR;
    // up to 16 waves, 16 / 32 / 64 rows each: short tiles keep the serial 5-iteration chain per wave short
    const long row0 = (long)rows_per_wave * wave;
    const int nrows = max(0, min(rows_per_wave, K - rows_per_wave * wave));
    // every wave's first row block (R rows from the fp64 [G | R], aux, dual) is requested BEFORE the system is built:
    // the round trips run under wave 0's Gauss-Jordan instead of after the barrier
    RowBlock<NBR, NREG, VEC> pre;
    if (NREG > 0 && nrows > 0)
        pre.load(lane, row0 + ((lane & 15) < nrows ? (lane & 15) : 0), r, nullptr, GR + (long)r * r, regs);
    if (wave == 0) c_finish_system<RP, NREG>(GR, r, scale, l2, lane, Ls, Ls64, &rho_s, true, LinvC, rhoC);
    __syncthreads();
    double dg[DIAG_COLS];
    if (NREG == 0) {
        c_solve_plain_f64(GR + (long)r * r, Ls64, lane, row0, nrows, r, inner, C, Cs, dg);
    } else {
        rows_fused_tile<NBR, NREG, VEC>(lane, row0, nrows, rho_s, Ls, nullptr, nullptr, C, Cs, regs, r, inner, dg,
                                        GR + (long)r * r, &pre);
    }
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 2 + NREG; ++k) dsm[wave][k] = dg[k];
    }
    __syncthreads();
    if (threadIdx.x < 2 + NREG) {
        double t = 0.0;
        for (int wv = 0; wv < n_waves; ++wv) t += dsm[wv][threadIdx.x];
        diag_row[threadIdx.x] = t;
    }
    // CtC = C^T C from the LDS copy of the new C on the fp64 MFMA (fp32 x fp32 products are exact in fp64): lane
    // (rsub = l>>4, c16 = l&15) feeds C[4g + rsub][16nb + c16]; every wave takes every n_waves-th group of 4 rows;
    // the per-wave accumulators (D layout: row = (l>>4) + 4 reg, col = l&15) are summed through LDS in fixed order.
    {
        typedef double f64x4 __attribute__((ext_vector_type(4)));
        __shared__ double csm[16 * NBR][16 * NBR];
        const int rsub = lane >> 4, c16 = lane & 15;
        f64x4 acc[NBR][NBR];
#pragma unroll
        for (int a = 0; a < NBR; ++a)
#pragma unroll
            for (int b = 0; b < NBR; ++b) acc[a][b] = f64x4{0.0, 0.0, 0.0, 0.0};
        const int n_groups = (K + 3) >> 2;
        for (int gq = wave; gq < n_groups; gq += n_waves) {
            const int row = 4 * gq + rsub;
            double y[NBR];
#pragma unroll
            for (int nb = 0; nb < NBR; ++nb) {
                const int col = 16 * nb + c16;
                y[nb] = (row < K && col < r) ? (double)Cs[row * r + col] : 0.0;
            }
#pragma unroll
            for (int a = 0; a < NBR; ++a)
#pragma unroll
                for (int b = 0; b < NBR; ++b) acc[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(y[a], y[b], acc[a][b], 0, 0, 0);
        }
        if (NBR == 1) {
            // every wave parks its accumulators in its own LDS slot (behind the C image), then one pass sums the slots
            // in wave order: 2 barriers instead of n_waves
            double *slots = reinterpret_cast<double *>(smc + ((r * r + K * r + 1) & ~1));
#pragma unroll
            for (int v = 0; v < 4; ++v) slots[wave * 256 + (rsub + 4 * v) * 16 + c16] = acc[0][0][v];
            __syncthreads();
            for (int e = threadIdx.x; e < 256; e += blockDim.x) {
                double t = 0.0;
                for (int wv = 0; wv < n_waves; ++wv) t += slots[wv * 256 + e];  // fixed order
                csm[e >> 4][e & 15] = t;
            }
            __syncthreads();
        } else {
            for (int wv = 0; wv < n_waves; ++wv) {  // fixed summation order
                if (wave == wv) {
#pragma unroll
                    for (int a = 0; a < NBR; ++a)
#pragma unroll
                        for (int b = 0; b < NBR; ++b)
#pragma unroll
                            for (int v = 0; v < 4; ++v) {
                                double &dst = csm[16 * a + rsub + 4 * v][16 * b + c16];
                                dst = (wv == 0) ? acc[a][b][v] : dst + acc[a][b][v];
                            }
                }
                __syncthreads();
            }
        }
        for (int pr = threadIdx.x; pr < r * r; pr += blockDim.x) {
            const int a = pr / r, b = pr - a * r;
            CtC[pr] = (float)csm[a][b];
            CtC64[pr] = csm[a][b];
        }
    }
    // fragment image of C for the X C kernels (see k_build_cfrag)
    const long total = (long)KC * 4 * NBc * 256;
    for (long idx = threadIdx.x; idx < total; idx += blockDim.x) {
        const int m = idx & 3, ln = (idx >> 2) & 63;
        long t = idx >> 8;
        const int nb = t % NBc;
        t /= NBc;
        const int kq = t & 3, kc = t >> 2;
        const int k = 64 * kc + 16 * kq + 4 * (ln >> 4) + m, col = 16 * nb + (ln & 15);
        Cfrag[idx] = (k < K && col < r) ? Cs[(long)k * r + col] : 0.f;
    }
}

// =========================================================================================================
// host launchers
// =========================================================================================================
bool mcl_mode_is_row_separable(const mcl_context *c, int mode) {
    const RegSet &rs = c->regs[mode];
    for (int k = 0; k < rs.n; ++k)
        if (rs.kind[k] != MCL_PEN_NN && rs.kind[k] != MCL_PEN_BOX && rs.kind[k] != MCL_PEN_L1) return false;
    return true;
}

#define DISPATCH_RP_T(c, KERNEL, grid, block, ...)                                                       \
    switch ((c)->RP) {                                                                                   \
        case 4: hipLaunchKernelGGL((KERNEL<4>), grid, block, 0, (c)->stream, __VA_ARGS__); break;         \
        case 8: hipLaunchKernelGGL((KERNEL<8>), grid, block, 0, (c)->stream, __VA_ARGS__); break;         \
        case 16: hipLaunchKernelGGL((KERNEL<16>), grid, block, 0, (c)->stream, __VA_ARGS__); break;       \
        case 32: hipLaunchKernelGGL((KERNEL<32>), grid, block, 0, (c)->stream, __VA_ARGS__); break;       \
        default: hipLaunchKernelGGL((KERNEL<64>), grid, block, 0, (c)->stream, __VA_ARGS__); break;       \
    }

int mcl_launch_ctc(mcl_context *c) {
    ProfScope prof_(c, MCL_PROF_OTHER);
    const int RPc = c->RP < 4 ? 4 : c->RP;
    hipLaunchKernelGGL(k_ctc, dim3((unsigned)c->r), dim3(256), 0, c->stream, c->C, (int)c->K, c->r, RPc, c->CtC, c->CtC64);
    MCL_CHECK_HIP(c, hipGetLastError());
    return 0;
}

int mcl_launch_B_rho(mcl_context *c) {
    ProfScope prof_(c, MCL_PROF_OTHER);
    MCL_CHECK_HIP(c, hipMemsetAsync(c->rho_max, 0, sizeof(float), c->stream));
    if (c->I == 0) return 0;
    hipLaunchKernelGGL(k_B_rho, dim3((unsigned)((c->I + 255) / 256)), dim3(256), 0, c->stream, c->CtC64, c->A, (int)c->I,
                       c->r, (float)c->opt.feasibility_penalty_scale, c->rhoB, c->rho_max);
    MCL_CHECK_HIP(c, hipGetLastError());
    return 0;
}

int mcl_launch_B_systems(mcl_context *c) {
    ProfScope prof_(c, MCL_PROF_OTHER);
    if (c->I == 0) return 0;
    dim3 grid((unsigned)((c->I + 3) / 4)), block(256);
    DISPATCH_RP_T(c, k_B_systems, grid, block, c->CtC64, c->A, (int)c->I, c->r, (float)c->opt.feasibility_penalty_scale,
                  (float)c->opt.l2_penalty[1], c->regs[1].n, c->opt.constant_B, c->rho_max, c->rhoB, c->LinvB, c->LinvB64);
    MCL_CHECK_HIP(c, hipGetLastError());
    return 0;
}

// exact-products mode (mcl_exact_mode): X C as fp64 sums of exact products, with its once-rounded fp32 image
int mcl_launch_exact_xc(mcl_context *c) {
    ProfScope prof_(c, MCL_PROF_XC);
    if (c->N == 0) {
        c->variant[MCL_PROF_XC] = "k_contract_xc_f64";
        return 0;
    }
    const dim3 g((unsigned)(((c->N + 15) / 16 + 3) / 4));
    return mcl_x_dispatch(c->x_type, [&](auto xl) {
    using XL = decltype(xl);
    const typename XL::T *X = mcl_x<XL>(c);
    c->variant[MCL_PROF_XC] = std::string("k_contract_xc_f64") + mcl_x_kname<XL>() + (std::is_same_v<XL, XF32> ? "" : std::string("<") + XL::name + ">");
    if (c->NB == 1)
        hipLaunchKernelGGL((MCL_XKERNEL(k_contract_xc_f64, 1)), g, dim3(256), 0, c->stream, X, c->C, (long)c->N, (int)c->K, c->r, c->XC64, c->XC);
    else if (c->NB == 2)
        hipLaunchKernelGGL((MCL_XKERNEL(k_contract_xc_f64, 2)), g, dim3(256), 0, c->stream, X, c->C, (long)c->N, (int)c->K, c->r, c->XC64, c->XC);
    else
        hipLaunchKernelGGL((MCL_XKERNEL(k_contract_xc_f64, 4)), g, dim3(256), 0, c->stream, X, c->C, (long)c->N, (int)c->K, c->r, c->XC64, c->XC);
    MCL_CHECK_HIP(c, hipGetLastError());
    return 0;
    });
}

int mcl_launch_B_solve_f64(mcl_context *c) {
    ProfScope prof_(c, MCL_PROF_ROWS_FUSED);
    c->variant[MCL_PROF_ROWS_FUSED] = "k_contract_xc_f64 + k_B_solve_f64";
    if (c->tilesB.n_tiles == 0) return 0;
    mcl_x_dispatch(c->x_type, [&](auto xl) {  // X C in fp64 (one inner iteration per phase for a penalty-free mode: computed right here)
        using XL = decltype(xl);
        const typename XL::T *X = mcl_x<XL>(c);
        const dim3 g((unsigned)(((c->N + 15) / 16 + 3) / 4));
        if (c->NB == 1)
            hipLaunchKernelGGL((MCL_XKERNEL(k_contract_xc_f64, 1)), g, dim3(256), 0, c->stream, X, c->C, (long)c->N, (int)c->K, c->r, c->XC64, nullptr);
        else if (c->NB == 2)
            hipLaunchKernelGGL((MCL_XKERNEL(k_contract_xc_f64, 2)), g, dim3(256), 0, c->stream, X, c->C, (long)c->N, (int)c->K, c->r, c->XC64, nullptr);
        else
            hipLaunchKernelGGL((MCL_XKERNEL(k_contract_xc_f64, 4)), g, dim3(256), 0, c->stream, X, c->C, (long)c->N, (int)c->K, c->r, c->XC64, nullptr);
        return 0;
    });
    dim3 grid((unsigned)((c->tilesB.n_tiles + 3) / 4)), block(256);
    DISPATCH_RP_T(c, k_B_solve_f64, grid, block, c->tilesB.slab, c->tilesB.row0, c->tilesB.nrows, c->tilesB.n_tiles, c->XC64,
                  c->A, c->LinvB64, c->r, c->B, c->gate_active);
    MCL_CHECK_HIP(c, hipGetLastError());
    return 0;
}

int mcl_launch_C_prepare(mcl_context *c) {
    dim3 grid((unsigned)(1 + (c->K * c->r + 63) / 64)), block(64);
    DISPATCH_RP_T(c, k_C_prepare, grid, block, c->GR, c->r, (int)c->K, (float)c->opt.feasibility_penalty_scale,
                  (float)c->opt.l2_penalty[2], c->regs[2].n, c->rhoC, c->LinvC, c->LinvC64, c->GRf + (long)c->r * c->r);
    MCL_CHECK_HIP(c, hipGetLastError());
    return 0;
}

int mcl_launch_C_solve_f64(mcl_context *c) {
    const long n = (long)c->K * c->r;
    hipLaunchKernelGGL(k_C_solve_f64, dim3((unsigned)((n + 255) / 256)), dim3(256), sizeof(double) * c->r * c->r, c->stream,
                       c->GR + (long)c->r * c->r, c->LinvC64, (int)c->K, c->r, c->C, c->gate_active);
    MCL_CHECK_HIP(c, hipGetLastError());
    return 0;
}

template <int NBR, int NREG>
static void launch_rows_fused_t(mcl_context *c, const TileMap &tm, const float *rhs, const float *Arows,
                                const float *rho, const float *Linv, float *F, const RegSet &rs, double *diag) {
    const bool vec = mcl_rows_vec_ok(c->r, rs, F, rhs);
    dim3 grid((unsigned)((tm.n_tiles + 3) / 4)), block(256);
    if (vec)
        hipLaunchKernelGGL((k_rows_fused<NBR, NREG, true>), grid, block, 0, c->stream, tm.slab, tm.row0, tm.nrows,
                           tm.n_tiles, rhs, Arows, rho, Linv, F, rs, c->r, c->opt.inner_n_iter_max, diag);
    else
        hipLaunchKernelGGL((k_rows_fused<NBR, NREG, false>), grid, block, 0, c->stream, tm.slab, tm.row0, tm.nrows,
                           tm.n_tiles, rhs, Arows, rho, Linv, F, rs, c->r, c->opt.inner_n_iter_max, diag);
}

template <int NBR>
static int launch_rows_fused_n(mcl_context *c, const TileMap &tm, const float *rhs, const float *Arows,
                               const float *rho, const float *Linv, float *F, const RegSet &rs, double *diag) {
    switch (rs.n) {
        case 0: launch_rows_fused_t<NBR, 0>(c, tm, rhs, Arows, rho, Linv, F, rs, diag); return 0;
        case 1: launch_rows_fused_t<NBR, 1>(c, tm, rhs, Arows, rho, Linv, F, rs, diag); return 0;
        case 2: launch_rows_fused_t<NBR, 2>(c, tm, rhs, Arows, rho, Linv, F, rs, diag); return 0;
        case 3:
            if (NBR == 1) {
                launch_rows_fused_t<1, 3>(c, tm, rhs, Arows, rho, Linv, F, rs, diag);
                return 0;
            }
            return -1;
        default: return -1;
    }
}

// returns -1 when the (rank, #penalties) combination has no fused instantiation (caller uses the generic path)
int mcl_rows_fused_dispatch(mcl_context *c, int mode, double *diag) {
    const RegSet &rs = c->regs[mode];
    const TileMap &tm = (mode == 1) ? c->tilesB : c->tilesC;
    if (tm.n_tiles == 0) return 0;
    const float *rhs = (mode == 1) ? c->XC : c->GRf + (long)c->r * c->r;  // fp32 image of R (k_C_prepare)
    const float *Arows = (mode == 1) ? c->A : nullptr;
    const float *rho = (mode == 1) ? c->rhoB : c->rhoC;
    const float *Linv = (mode == 1) ? c->LinvB : c->LinvC;
    float *F = (mode == 1) ? c->B : c->C;
    if (c->r <= 16) return launch_rows_fused_n<1>(c, tm, rhs, Arows, rho, Linv, F, rs, diag);
    if (c->r <= 32) return launch_rows_fused_n<2>(c, tm, rhs, Arows, rho, Linv, F, rs, diag);
    if (rs.n <= 1) return launch_rows_fused_n<4>(c, tm, rhs, Arows, rho, Linv, F, rs, diag);
    return -1;
}

int mcl_launch_rows_fused(mcl_context *c, int mode) {
    double *diag = (mode == 1) ? c->diagB_tile : c->diagC_tile;
    int rc;
    if (mode == 1) {
        ProfScope prof(c, MCL_PROF_ROWS_FUSED);
        rc = mcl_rows_fused_dispatch(c, mode, diag);
        char buf[64];
        snprintf(buf, sizeof buf, "k_rows_fused<NBR=%d,NREG=%d>", c->r <= 16 ? 1 : (c->r <= 32 ? 2 : 4), c->regs[1].n);
        c->variant[MCL_PROF_ROWS_FUSED] = buf;
    } else {
        rc = mcl_rows_fused_dispatch(c, mode, diag);
    }
    if (rc < 0) return rc;
    c->bp.diag_rows[mode] = (((mode == 1) ? c->tilesB.n_tiles : c->tilesC.n_tiles) + 3) / 4;  // one row per block
    MCL_CHECK_HIP(c, hipGetLastError());
    return 0;
}

template <int NBR, int NREG>
static int launch_C_fused_t(mcl_context *c) {
    const RegSet &rs = c->regs[2];
    const bool vec = mcl_rows_vec_ok(c->r, rs, c->C) && ((c->r * c->r) % 4 == 0);
    const int rpw = c->K <= 256 ? 16 : (c->K <= 512 ? 32 : 64);
    const int n_waves = (int)((c->K + rpw - 1) / rpw);
    size_t sm = sizeof(float) * (size_t)(c->r * c->r + c->K * c->r);
    if (NBR == 1) sm = ((sm + 7) & ~size_t(7)) + sizeof(double) * 256 * (size_t)n_waves;  // per-wave CtC slots
    int kct = 0;
    const int KC = mcl_xc_chunks(c, &kct);
#define MCL_CF(VEC_)                                                                                                  \
    do {                                                                                                              \
        if (sm > 65536)                                                                                               \
            MCL_CHECK_HIP(c, hipFuncSetAttribute(reinterpret_cast<const void *>(k_C_finish_fused<NBR, NREG, VEC_>),   \
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)sm));               \
        hipLaunchKernelGGL((k_C_finish_fused<NBR, NREG, VEC_>), dim3(1), dim3(64 * n_waves), sm, c->stream, c->GR,    \
                           (int)c->K, c->r, (float)c->opt.feasibility_penalty_scale, (float)c->opt.l2_penalty[2],     \
                           c->rhoC, c->LinvC, c->C, rs, c->opt.inner_n_iter_max, c->CtC, c->CtC64, c->Cfrag, mcl_cfrag_chunks(c), c->NB, \
                           c->diagC_tile, rpw);                                                                       \
    } while (0)
    if (vec) MCL_CF(true);
    else MCL_CF(false);
#undef MCL_CF
    MCL_CHECK_HIP(c, hipGetLastError());
    c->variant[MCL_PROF_C_FINISH] = "k_C_finish_fused<NBR=" + std::to_string(NBR) + ",NREG=" + std::to_string(NREG) + ">";
    c->bp.diag_rows[2] = 1;
    return 0;
}

// ---------------------------------------------------------------------------------------------------------
// The C-side finish over ceil(K / 64) workgroups (rank <= 16, K >= 128).  In the single workgroup of
// k_C_finish_fused the 16-row tiles of C queue four deep on every SIMD (9 k of its 23.5 k cycles at K = 256) and C^T C, the
// fragment image and the barriers see all K rows; here a workgroup owns 64 rows = one 16-row tile per wave = one 64-column
// chunk of the fragment image.  Every workgroup builds and inverts the (identical) r x r system itself - same inputs,
// same instructions, same bits - so nothing crosses workgroups inside the launch: C^T C leaves as one partial 16 x 16
// fp64 block per workgroup, which the A-phase finish sums in fixed order (AFuse::ctc_parts; ensure_ctc folds them for
// any other consumer).
// ---------------------------------------------------------------------------------------------------------
template <int NREG, bool VEC>
__global__ __launch_bounds__(256) void k_C_finish_multi(const double *__restrict__ GR, int K, int r, float scale, float l2,
                                                        float *__restrict__ rhoC, float *__restrict__ LinvC,
                                                        float *__restrict__ C, RegSet regs, int inner,
                                                        double *__restrict__ CtCpart, float *__restrict__ Cfrag, int KC,
                                                        double *__restrict__ diag_row) {
    MCL_GATE(regs.gate);
    __shared__ float Ls[256];
    __shared__ float Cs[64 * 16];
    __shared__ double dsm[4][DIAG_COLS];
    __shared__ double slots[4][256];
    __shared__ float rho_s;
    __shared__ double Ls64[NREG == 0 ? 256 : 1];  // penalty-free C: the solve itself runs in fp64 (as in k_C_finish_fused)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b0 = 64 * blockIdx.x;
    const long row0 = b0 + 16 * wave;
    const int nrows = max(0, min(16, K - (int)row0));
    RowBlock<1, NREG, VEC> pre;
    if (NREG > 0 && nrows > 0)
        pre.load(lane, row0 + ((lane & 15) < nrows ? (lane & 15) : 0), r, nullptr, GR + (long)r * r, regs);
    // every workgroup builds the system; the first one stores it
    if (wave == 0) c_finish_system<16, NREG>(GR, r, scale, l2, lane, Ls, Ls64, &rho_s, blockIdx.x == 0, LinvC, rhoC);
    __syncthreads();
    double dg[DIAG_COLS];
    // (the LDS copy is indexed by the GLOBAL row like C itself: its base is shifted back by the workgroup's first row)
    float *Csg = Cs - (long)b0 * r;
    if (NREG == 0) {
        c_solve_plain_f64(GR + (long)r * r, Ls64, lane, row0, nrows, r, inner, C, Csg, dg);
    } else {
        rows_fused_tile<1, NREG, VEC>(lane, row0, nrows, rho_s, Ls, nullptr, nullptr, C, Csg, regs, r, inner, dg,
                                      GR + (long)r * r, &pre);
    }
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 2 + NREG; ++k) dsm[wave][k] = dg[k];
    }
    __syncthreads();
    if (threadIdx.x < 2 + NREG)  // one diagnostics row per workgroup
        diag_row[(long)blockIdx.x * DIAG_COLS + threadIdx.x] =
            (dsm[0][threadIdx.x] + dsm[1][threadIdx.x]) + (dsm[2][threadIdx.x] + dsm[3][threadIdx.x]);
    // partial C^T C of the workgroup's rows on the fp64 MFMA (fp32 x fp32 products are exact in fp64)
    {
        typedef double f64x4 __attribute__((ext_vector_type(4)));
        const int rsub = lane >> 4, c16 = lane & 15;
        f64x4 acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int gq = 0; gq < 4; ++gq) {
            const int rl = 4 * (4 * gq + wave) + rsub;  // groups of 4 rows, interleaved over the waves
            const double y = (b0 + rl < K && c16 < r) ? (double)Cs[rl * r + c16] : 0.0;
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(y, y, acc, 0, 0, 0);
        }
#pragma unroll
        for (int v = 0; v < 4; ++v) slots[wave][(rsub + 4 * v) * 16 + c16] = acc[v];
        __syncthreads();
        const int e = threadIdx.x;
        CtCpart[(long)blockIdx.x * 256 + e] = (slots[0][e] + slots[1][e]) + (slots[2][e] + slots[3][e]);
    }
    // the workgroup's chunk of the fragment image of C (see k_build_cfrag; NB = 1): 1024 floats; the last workgroup also
    // clears the chunks past K
    for (int idx = threadIdx.x; idx < 1024; idx += 256) {
        const int m = idx & 3, ln = (idx >> 2) & 63, kq = idx >> 8;
        const int kl = 16 * kq + 4 * (ln >> 4) + m, col = ln & 15;
        Cfrag[(long)blockIdx.x * 1024 + idx] = (b0 + kl < K && col < r) ? Cs[kl * r + col] : 0.f;
    }
    if (blockIdx.x == gridDim.x - 1)
        for (long idx = (long)gridDim.x * 1024 + threadIdx.x; idx < (long)KC * 1024; idx += 256) Cfrag[idx] = 0.f;
}

// C^T C from the partial blocks of k_C_finish_multi, for the consumers other than the A-phase finish
__global__ __launch_bounds__(256) void k_ctc_fold(const double *__restrict__ CtCpart, int parts, int r, float *__restrict__ CtC,
                                                  double *__restrict__ CtC64) {
    const int e = threadIdx.x, a = e >> 4, b = e & 15;
    double t = 0.0;
    for (int p = 0; p < parts; ++p) t = (p == 0) ? CtCpart[e] : t + CtCpart[(long)p * 256 + e];
    if (a < r && b < r) {
        CtC64[a * r + b] = t;
        CtC[a * r + b] = (float)t;
    }
}

int mcl_launch_ctc_fold(mcl_context *c) {
    ProfScope prof_(c, MCL_PROF_OTHER);
    hipLaunchKernelGGL(k_ctc_fold, dim3(1), dim3(256), 0, c->stream, c->CtCpart, c->bp.ctc_parts, c->r, c->CtC, c->CtC64);
    MCL_CHECK_HIP(c, hipGetLastError());
    c->bp.ctc_parts = 0;
    return 0;
}

template <int NREG>
static int launch_C_multi_t(mcl_context *c) {
    const RegSet &rs = c->regs[2];
    const bool vec = mcl_rows_vec_ok(c->r, rs, c->C) && ((c->r * c->r) % 4 == 0);
    const int nblk = (int)((c->K + 63) / 64);
#define MCL_CM(VEC_)                                                                                                   \
    hipLaunchKernelGGL((k_C_finish_multi<NREG, VEC_>), dim3(nblk), dim3(256), 0, c->stream, c->GR, (int)c->K, c->r,       \
                       (float)c->opt.feasibility_penalty_scale, (float)c->opt.l2_penalty[2], c->rhoC, c->LinvC, c->C, rs, \
                       c->opt.inner_n_iter_max, c->CtCpart, c->Cfrag, mcl_cfrag_chunks(c), c->diagC_tile)
    if (vec) MCL_CM(true);
    else MCL_CM(false);
#undef MCL_CM
    MCL_CHECK_HIP(c, hipGetLastError());
    c->variant[MCL_PROF_C_FINISH] = "k_C_finish_multi<NREG=" + std::to_string(NREG) + ">";
    c->bp.diag_rows[2] = nblk;
    c->bp.ctc_parts = nblk;
    return 0;
}

// Single-workgroup C-side finish; returns -1 if the shape has no instantiation (caller uses the separate kernels)
int mcl_launch_C_finish_fused(mcl_context *c) {
    if (c->K > 1024 || c->sw.no_fused_c) return -1;
    if ((size_t)(c->r * c->r + c->K * c->r) * sizeof(float) > 150 * 1024) return -1;
    const int n = c->regs[2].n;
    c->bp.ctc_parts = 0;
    // rank <= 16 and at least two 64-row chunks: one workgroup per chunk (k_C_finish_multi); the
    // fragment image is then the one of the sweep / X C kernels with NB = 1
    if (c->r <= 16 && n <= 2 && c->K >= 128 && c->NB == 1 && !c->sw.no_multi_c &&
        mcl_cfrag_chunks(c) >= (int)((c->K + 63) / 64))
        return n == 0 ? launch_C_multi_t<0>(c) : (n == 1 ? launch_C_multi_t<1>(c) : launch_C_multi_t<2>(c));
    if (c->r <= 16) {
        switch (n) {
            case 0: return launch_C_fused_t<1, 0>(c);
            case 1: return launch_C_fused_t<1, 1>(c);
            case 2: return launch_C_fused_t<1, 2>(c);
            default: return -1;
        }
    }
    if (c->r <= 32) {
        switch (n) {
            case 0: return launch_C_fused_t<2, 0>(c);
            case 1: return launch_C_fused_t<2, 1>(c);
            default: return -1;
        }
    }
    return -1;
}

#include "afinish.h"  // the A-phase finish: kernels and launchers, in this code object
