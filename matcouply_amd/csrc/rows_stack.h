// The arithmetic of the B-mode row pass of a fused penalty stack, written ONCE.
//
// Seven kernels run it: k_rows_solve, k_rows_solve_stats, k_rows_finish_fused and k_rows_finish_solve_stats of rows.hip, and
// their software-pipelined forms k_rows_chain_first / _mid / _last of rowchain.hip.  The kernels own what differs between them:
// how rows are loaded, masked and stored (masked row_ld4 / row_st4 in rows.hip; unconditional loads at clamped addresses,
// masks at use and sink stores in rowchain.hip) and whether the class of a penalty is a run-time or a compile-time value.  The
// parts below take rows that are already loaded and masked (zeros for padding rows / columns) as f32x4[NBR] in the fragment
// layout of rows_mfma.h and return rows to store; the only global memory they touch themselves are the r x r matrices of the
// prologue and the per-tile statistics / diagnostics tables of the epilogue.  Every function is forced inline: `cls`, `k` and
// the flags fold where the kernel passes constants.  Reference: the inner loop of admm_update_B, decomposition.py:259-285.
#pragma once
#include <type_traits>

#include "mcl_internal.h"
#include "rows_mfma.h"

// for the lambdas a kernel hands to stack_prox: inlined like everything else here
#define ROWS_INLINE __attribute__((always_inline))

// What a penalty asks of the row pass
enum { CLS_ROWSEP = 0, CLS_PF2 = 1, CLS_UNI = 2, CLS_L2 = 3 };
constexpr int class_of(int kind) {
    return kind == MCL_PEN_PARAFAC2 ? CLS_PF2 : (kind == MCL_PEN_UNIMODAL ? CLS_UNI : (kind == MCL_PEN_L2BALL ? CLS_L2 : CLS_ROWSEP));
}

// The wave's tile: gate, lane / tile, the wave-uniform slab, first row and row count, the lane's (row16, g) of rows_mfma.h
#define ROW_TILE_PROLOGUE()                                                                                  \
    MCL_GATE(mv.gate);                                                                                       \
    const int lane = threadIdx.x & 63;                                                                       \
    const int tile = blockIdx.x * 4 + (threadIdx.x >> 6);                                                    \
    if (tile >= mv.n_tiles) return;                                                                          \
    const int slab = __builtin_amdgcn_readfirstlane(mv.tile_slab[tile]);                                     \
    const long row0 = __builtin_amdgcn_readfirstlane(mv.tile_row0[tile]);                                    \
    const int nrows = __builtin_amdgcn_readfirstlane(mv.tile_nrows[tile]);                                   \
    const int row16 = lane & 15, g = lane >> 4;                                                              \
    (void)slab; (void)row16; (void)g

// index of the stack's last penalty of `kind`, -1 without one (run-time stacks; rowchain.hip reads it off its signature)
static __device__ __forceinline__ int last_of_kind(const RegSet &regs, int kind) {
    int found = -1;
    for (int k = 0; k < regs.n; ++k)
        if (regs.kind[k] == kind) found = k;
    return found;
}

// the slab's r x r matrix (L_i^-1, T_i) in the arithmetic of the kernel: R64 reads the fp64 copy
template <bool R64, typename MAT>
static __device__ __forceinline__ void load_slab_mat(MAT &M, const float *__restrict__ M32, const double *__restrict__ M64, int slab,
                                                     int r, int lane) {
    if constexpr (R64) M.load(M64 + (long)slab * r * r, r, lane);
    else M.load(M32 + (long)slab * r * r, r, lane);
}

// column scale of the right-hand side: row `slab` of A (mode 1), ones without it
template <int NBR>
static __device__ __forceinline__ void a_col_scale(const float *__restrict__ Arows, int slab, int r, int g, float (&av)[NBR][4]) {
#pragma unroll
    for (int h = 0; h < NBR; ++h)
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const int col = 16 * h + 4 * g + v;
            av[h][v] = (Arows != nullptr && col < r) ? Arows[(long)slab * r + col] : 1.f;
        }
}

// L2 ball k: bound / max(||column||, bound) from the per-slab column sums of squares
static __device__ __forceinline__ float l2_ball_scale(const RegSet &regs, int k, const double *__restrict__ colsq, int n_slabs, int slab,
                                                      int r, int col) {
    const float bound = regs.p0[k];
    const float nrm = (col < r) ? (float)sqrt(colsq[((long)k * n_slabs + slab) * r + col]) : 1.f;
    return bound / fmaxf(nrm, bound);
}
// ... of the lane's columns, once per tile; ones for k < 0 (no ball)
template <int NBR>
static __device__ __forceinline__ void l2_ball_scales(const RegSet &regs, int k, const double *__restrict__ colsq, int n_slabs,
                                                      int slab, int r, int g, float (&s)[NBR][4]) {
#pragma unroll
    for (int h = 0; h < NBR; ++h)
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            s[h][v] = 1.f;
            if (k >= 0) s[h][v] = l2_ball_scale(regs, k, colsq, n_slabs, slab, r, 16 * h + 4 * g + v);
        }
}

// the stored aux rows of PARAFAC2 are P, its Z is P Delta
template <int NBR, typename MAT>
static __device__ __forceinline__ void times_delta(const MAT &D, f32x4 (&z)[NBR]) {
    f32x4 pz[NBR];
    D.apply(z, pz);
#pragma unroll
    for (int h = 0; h < NBR; ++h) z[h] = pz[h];
}

// t += rho (Z_k - U_k)
template <int NBR>
static __device__ __forceinline__ void rhs_add(float rho, const f32x4 (&z)[NBR], const f32x4 (&u)[NBR], f32x4 (&t)[NBR]) {
#pragma unroll
    for (int h = 0; h < NBR; ++h)
#pragma unroll
        for (int v = 0; v < 4; ++v) t[h][v] = fmaf(rho, z[h][v] - u[h][v], t[h][v]);
}

// prox of penalty k at F + U_k.  z: what is stored as its aux rows; zg: what the dual and the feasibility gap are measured
// against (P Delta for PARAFAC2, else z).  Ts / D: T_i and Delta (read for CLS_PF2 only).  The two callables are the kernel's:
// aux_rows(h) returns the masked aux row block the column regressions wrote (called for CLS_UNI only), l2_scale(h, v) the
// factor of l2_ball_scale for the lane's column (CLS_L2 only) - a table filled once per tile, or the function itself.
// They are callables, not arrays, so that a kernel with run-time classes loads the aux rows and forms the scales INSIDE the
// branch of the class, as the hand-written kernels did.  zg is formed by one select after the branches and not by a store in
// each: stores of whole f32x4 into zg[h] from several run-time branches get merged into one store at a variable index, which
// puts zg in scratch (48 B in k_rows_finish_fused / k_rows_finish_solve_stats at NBR = 2 when it was tried).
template <typename RA, int NBR, typename AUX, typename SCALE>
static __device__ __forceinline__ void stack_prox(int cls, const RegSet &regs, int k, float rho,
                                                  const typename RA::template Mat<NBR> &Ts, const typename RA::template Mat<NBR> &D,
                                                  const f32x4 (&f)[NBR], const f32x4 (&u)[NBR], AUX aux_rows, SCALE l2_scale,
                                                  f32x4 (&z)[NBR], f32x4 (&zg)[NBR]) {
    f32x4 pd[NBR];
    if (cls == CLS_PF2) {
        typename RA::Y y[NBR], pw[NBR];
#pragma unroll
        for (int h = 0; h < NBR; ++h) y[h] = RA::ysum(f[h], u[h]);
        Ts.apply(y, pw);   // P = Y T_i      (the aux variable)
        D.apply(pw, pd);   // P Delta        (what the dual is measured against)
#pragma unroll
        for (int h = 0; h < NBR; ++h) z[h] = RA::narrow(pw[h]);
    } else if (cls == CLS_UNI) {
#pragma unroll
        for (int h = 0; h < NBR; ++h) z[h] = aux_rows(h);
    } else if (cls == CLS_L2) {
#pragma unroll
        for (int h = 0; h < NBR; ++h)
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                float y = f[h][v] + u[h][v];
                if (regs.nonneg[k]) y = fmaxf(y, 0.f);
                z[h][v] = l2_scaled(y, l2_scale(h, v));
            }
    } else {
        const float thr = regs.p0[k] / rho;
#pragma unroll
        for (int h = 0; h < NBR; ++h)
#pragma unroll
            for (int v = 0; v < 4; ++v) z[h][v] = prox_elem(regs.kind[k], regs.nonneg[k], regs.p0[k], regs.p1[k], thr, f[h][v] + u[h][v]);
    }
#pragma unroll
    for (int h = 0; h < NBR; ++h) zg[h] = (cls == CLS_PF2) ? pd[h] : z[h];
}

// U_k = F - (Z_k - U_k)
template <int NBR>
static __device__ __forceinline__ void dual_step(const f32x4 (&f)[NBR], const f32x4 (&zg)[NBR], f32x4 (&u)[NBR]) {
#pragma unroll
    for (int h = 0; h < NBR; ++h)
#pragma unroll
        for (int v = 0; v < 4; ++v) u[h][v] = f[h][v] - (zg[h][v] - u[h][v]);
}

// PARAFAC2: the tile's Gram Y^T Y, Y = F + U, in fp64.  The new rows go ROW -> COL layout through 4 selector MFMAs (exact; COL
// layout: lane (q, i16) reg w = Y[4q + w][16nb + i16]), then the fp64 MFMA accumulates exact fp32 x fp32 products exactly like
// k_pf2_gram.  R64: Y is the exact fp64 sum of the two stored values and is transposed through the wave's padded 16 x 16 LDS
// tile instead (lane (q, i16) reg w = Y[q + 4w][16nb + i16]; the fp64 matrix pipe is the scarce unit of these passes: 44 TFLOP/s
// at best, tools/mfma64_rate.hip).  Padding rows contribute zeros (`ok`), padding columns are zero in F and U.
template <int NBR, bool R64>
struct YGram {
    typedef double f64x4s __attribute__((ext_vector_type(4)));
    static constexpr int LDS_DOUBLES = R64 ? 4 * 16 * 17 : 1;  // __shared__ double ytile[LDS_DOUBLES] of the kernel's workgroup
    f64x4s acc[NBR][NBR];
    typename std::conditional<R64, double, float>::type bsel[4];
    __device__ __forceinline__ void clear(int row16, int g) {
#pragma unroll
        for (int v = 0; v < 4; ++v) bsel[v] = (row16 == 4 * g + v) ? 1.f : 0.f;
#pragma unroll
        for (int a = 0; a < NBR; ++a)
#pragma unroll
            for (int b = 0; b < NBR; ++b) acc[a][b] = f64x4s{0.0, 0.0, 0.0, 0.0};
    }
    __device__ __forceinline__ void add(const f32x4 (&fn)[NBR], const f32x4 (&u)[NBR], bool ok, double *ytile, int row16, int g) {
        double yt[NBR][4];
#pragma unroll
        for (int nb = 0; nb < NBR; ++nb) {
            if constexpr (R64) {
                double *yl = ytile + (threadIdx.x >> 6) * (16 * 17);
#pragma unroll
                for (int v = 0; v < 4; ++v) yl[row16 * 17 + 4 * g + v] = ok ? (double)fn[nb][v] + (double)u[nb][v] : 0.0;
#pragma unroll
                for (int w = 0; w < 4; ++w) yt[nb][w] = yl[(g + 4 * w) * 17 + row16];
            } else {
                f32x4 tr = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    const float y = ok ? fn[nb][v] + u[nb][v] : 0.f;
                    tr = MFMA16(y, bsel[v], tr);
                }
#pragma unroll
                for (int w = 0; w < 4; ++w) yt[nb][w] = (double)tr[w];
            }
        }
#pragma unroll
        for (int w = 0; w < 4; ++w)
#pragma unroll
            for (int a = 0; a < NBR; ++a)
#pragma unroll
                for (int b = 0; b < NBR; ++b) acc[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(yt[a][w], yt[b][w], acc[a][b], 0, 0, 0);
    }
    // D layout of the f64 MFMA: col = l & 15, row = (l >> 4) + 4 reg
    __device__ __forceinline__ void store(double *__restrict__ stat_gram, int tile, int row16, int g) const {
        constexpr int W = 16 * NBR;
        double *out = stat_gram + (long)tile * W * W;
#pragma unroll
        for (int a = 0; a < NBR; ++a)
#pragma unroll
            for (int b = 0; b < NBR; ++b)
#pragma unroll
                for (int v = 0; v < 4; ++v) out[(16 * a + g + 4 * v) * W + 16 * b + row16] = acc[a][b][v];
    }
};

// L2 ball: the tile's column sums of squares of Y = F + U (clamped at 0 for a non-negative ball), fp64
template <int NBR>
struct ColSq {
    double s[NBR][4];
    __device__ __forceinline__ void clear() {
#pragma unroll
        for (int h = 0; h < NBR; ++h)
#pragma unroll
            for (int v = 0; v < 4; ++v) s[h][v] = 0.0;
    }
    __device__ __forceinline__ void add(const f32x4 (&fn)[NBR], const f32x4 (&u)[NBR], int nonneg, bool ok) {
#pragma unroll
        for (int h = 0; h < NBR; ++h)
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                float y = fn[h][v] + u[h][v];
                if (nonneg) y = fmaxf(y, 0.f);
                if (ok) s[h][v] += (double)y * (double)y;
            }
    }
    // sum over the 16 rows of the four blocks (lanes of equal g), then one store per column: stat_colsq[tile][k][col]
    __device__ __forceinline__ void reduce_store(double *__restrict__ stat_colsq, int tile, int k, int r, int row16, int g) const {
#pragma unroll
        for (int h = 0; h < NBR; ++h)
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                double sq = s[h][v];
                sq += __shfl_xor(sq, 1);
                sq += __shfl_xor(sq, 2);
                sq += __shfl_xor(sq, 4);
                sq += __shfl_xor(sq, 8);
                const int col = 16 * h + 4 * g + v;
                if (row16 == 0 && col < r) stat_colsq[((long)tile * MCL_MAX_REGS + k) * r + col] = sq;
            }
    }
};

// The mode's per-tile diagnostics: ||F||^2, sum |F|, ||Z_k - F||^2 of every penalty (the same sums as k_rows_diag)
struct TileDiag {
    double nf, na, gap[MCL_MAX_REGS];
    __device__ __forceinline__ void clear() {
        nf = 0.0, na = 0.0;
#pragma unroll
        for (int k = 0; k < MCL_MAX_REGS; ++k) gap[k] = 0.0;
    }
    template <int NBR>
    __device__ __forceinline__ void add_f(const f32x4 (&f)[NBR]) {
#pragma unroll
        for (int h = 0; h < NBR; ++h)
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                nf += (double)f[h][v] * (double)f[h][v];
                na += fabs((double)f[h][v]);
            }
    }
    template <int NBR>
    __device__ __forceinline__ void add_gap(int k, const f32x4 (&zg)[NBR], const f32x4 (&f)[NBR], bool ok, int r, int g) {
#pragma unroll
        for (int h = 0; h < NBR; ++h)
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const bool valid = ok && (16 * h + 4 * g + v < r);
                const double dlt = valid ? (double)zg[h][v] - (double)f[h][v] : 0.0;
                gap[k] += dlt * dlt;
            }
    }
    __device__ __forceinline__ void store(double *__restrict__ diag_tile, int tile, int lane) {
        nf = wave_sum(nf);
        na = wave_sum(na);
#pragma unroll
        for (int k = 0; k < MCL_MAX_REGS; ++k) gap[k] = wave_sum(gap[k]);
        if (lane == 0) {
            double *o = diag_tile + (long)tile * DIAG_COLS;
            o[0] = nf;
            o[1] = na;
#pragma unroll
            for (int k = 0; k < MCL_MAX_REGS; ++k) o[2 + k] = gap[k];
        }
    }
};
