// The row passes of the un-fused inner ADMM loop (one kernel per step), for the penalty stacks the fused kernels of admm.hip do
// not take: those with a member that couples the rows of a slab or the slabs
//   L2Ball, TotalVariation, GeneralizedL2Penalty, UnitSimplex   slabprox.hip
//   Unimodality                                                 unimodal.hip
//   Parafac2                                                    pf2polar.hip (polar factors per slab + cross-slab coordinate matrix)
// plus the row-separable ones when they share a mode with the above.  A pass handles whatever is separable by rows - solve, the
// elementwise proxes, the dual steps, applying T_i - with the arithmetic of rows_stack.h; rowchain.hip holds the software-pipelined
// twins of the three chained passes.  mcl_launch_generic_prox_local / _finish dispatch a penalty's prox on its kind.
#include "rows_launch.h"

// solve:  F = (rhs (o a) + rho sum_k (Z_k - U_k)) L^-1   (decomposition.py:266-273 / 328-331)
template <int NBR, bool VEC>
__global__ __launch_bounds__(256) void k_rows_solve(ModeView mv, const float *__restrict__ rhs_src,
                                                    const float *__restrict__ Arows, const float *__restrict__ Linv,
                                                    RegSet regs, int r, double *__restrict__ change_part) {
    // change_part != nullptr: per tile ||f_new - f_old||^2 (the inner stopping test, decomposition.py:100-107)
    ROW_TILE_PROLOGUE();
    double chg = 0.0;
    const float rho = mv.rho[slab];
    RowMat<NBR> L, D;
    L.load(Linv + (long)slab * r * r, r, lane);
    const int kpf2 = last_of_kind(regs, MCL_PEN_PARAFAC2);
    if (kpf2 >= 0) D.load(regs.aux2[kpf2], r, lane);
    float av[NBR][4];
    a_col_scale(Arows, slab, r, g, av);
    FOR_ROW_BLOCKS() {
        const bool ok = 16 * rb + row16 < nrows;
        const long j = row0 + 16 * rb + (ok ? row16 : 0);
        f32x4 t[NBR], f[NBR];
#pragma unroll
        for (int h = 0; h < NBR; ++h) {
            t[h] = row_ld4<VEC>(rhs_src, j, 16 * h + 4 * g, ok, r);
#pragma unroll
            for (int v = 0; v < 4; ++v) t[h][v] *= av[h][v];
        }
        for (int k = 0; k < regs.n; ++k) {
            f32x4 z[NBR], u[NBR];
#pragma unroll
            for (int h = 0; h < NBR; ++h) z[h] = row_ld4<VEC>(regs.aux[k], j, 16 * h + 4 * g, ok, r);
            if (k == kpf2) times_delta(D, z);
#pragma unroll
            for (int h = 0; h < NBR; ++h) u[h] = row_ld4<VEC>(regs.dual[k], j, 16 * h + 4 * g, ok, r);
            rhs_add(rho, z, u, t);
        }
        L.apply(t, f);
        if (change_part != nullptr) {
#pragma unroll
            for (int h = 0; h < NBR; ++h) {
                const f32x4 fo = row_ld4<VEC>((const float *)mv.F, j, 16 * h + 4 * g, ok, r);
#pragma unroll
                for (int v = 0; v < 4; ++v)
                    if (ok && 16 * h + 4 * g + v < r) {
                        const double d = (double)f[h][v] - (double)fo[v];
                        chg = fma(d, d, chg);
                    }
            }
        }
#pragma unroll
        for (int h = 0; h < NBR; ++h) row_st4<VEC>(mv.F, j, 16 * h + 4 * g, ok, r, f[h]);
    }
    if (change_part != nullptr) {
        chg = wave_sum_d(chg);
        if (lane == 0) change_part[tile] = chg;
    }
}

// The same solve with the per-slab statistics of the slab-wise penalties riding in its epilogue (mode 1, fused stacks):
//   PARAFAC2:  per-tile Gram Y^T Y, Y = F + U   - B_new rows go ROW -> COL layout through 4 selector MFMAs (exact), then
//              the fp64 MFMA accumulates exact fp32 x fp32 products exactly like k_pf2_gram
//   L2 ball :  per-tile column sums of squares of (F + U) (optionally clamped at 0), fp64
// k_stats_reduce sums the tiles of every slab in fixed order.  Saves the two extra reads of F and the duals that
// k_pf2_gram and k_slab_colsq need.
// R64 (rank <= 16 with a PARAFAC2 member, see mcl_rows64): the same pass with every product and sum in fp64 registers
// around the fp32 loads and stores - L^-1 from its fp64 copy, the statistics of Y = F + U from the exact fp64 sum of the
// two STORED (fp32) values.  tools/pf2_rounding_study.py: the fp32 accumulation chains of the r x r products, the fp32
// image of T_i and the rounded sum F + U carry two thirds of the B-phase error of BASELINE config 4 against the fp64
// reference (7e-7 per phase, amplified to 1e-5 in A by the penalty-free A / C systems of that configuration).
template <int NBR, bool VEC, bool R64 = false>
__global__ __launch_bounds__(256) void k_rows_solve_stats(ModeView mv, const float *__restrict__ rhs_src,
                                                          const float *__restrict__ Arows, const float *__restrict__ Linv,
                                                          RegSet regs, int r, double *__restrict__ stat_gram,
                                                          double *__restrict__ stat_colsq,
                                                          const double *__restrict__ Linv64 = nullptr) {
    typedef RowArith<R64> RA;
    __shared__ double ytile[YGram<NBR, R64>::LDS_DOUBLES];  // R64: one padded 16 x 16 fp64 tile per wave (row -> column layout of Y)
    ROW_TILE_PROLOGUE();
    const float rho = mv.rho[slab];
    typename RA::template Mat<NBR> L, D;
    load_slab_mat<R64>(L, Linv, Linv64, slab, r, lane);
    const int kpf2 = last_of_kind(regs, MCL_PEN_PARAFAC2);
    if (kpf2 >= 0) D.load(regs.aux2[kpf2], r, lane);
    float av[NBR][4];
    a_col_scale(Arows, slab, r, g, av);
    YGram<NBR, R64> gram;
    gram.clear(row16, g);
    ColSq<NBR> csq[MCL_MAX_REGS];
#pragma unroll
    for (int k = 0; k < MCL_MAX_REGS; ++k) csq[k].clear();
    FOR_ROW_BLOCKS() {
        const bool ok = 16 * rb + row16 < nrows;
        const long j = row0 + 16 * rb + (ok ? row16 : 0);
        f32x4 t[NBR], f[NBR], ukeep[MCL_MAX_REGS][NBR];
#pragma unroll
        for (int h = 0; h < NBR; ++h) {
            t[h] = (row_ld4<VEC>(rhs_src, j, 16 * h + 4 * g, ok, r));
#pragma unroll
            for (int v = 0; v < 4; ++v) t[h][v] *= av[h][v];
        }
#pragma unroll
        for (int k = 0; k < MCL_MAX_REGS; ++k) {
            if (k < regs.n) {
                f32x4 z[NBR];
#pragma unroll
                for (int h = 0; h < NBR; ++h) z[h] = (row_ld4<VEC>(regs.aux[k], j, 16 * h + 4 * g, ok, r));
                if (k == kpf2) times_delta(D, z);
#pragma unroll
                for (int h = 0; h < NBR; ++h) ukeep[k][h] = (row_ld4<VEC>(regs.dual[k], j, 16 * h + 4 * g, ok, r));
                rhs_add(rho, z, ukeep[k], t);
            }
        }
        L.apply(t, f);
#pragma unroll
        for (int h = 0; h < NBR; ++h) row_st4<VEC>(mv.F, j, 16 * h + 4 * g, ok, r, f[h]);
        // ---- statistics of the new rows (padding rows / columns contribute zeros: row_ld4 returned zeros for them and
        //      L.apply leaves padding columns at zero)
#pragma unroll
        for (int k = 0; k < MCL_MAX_REGS; ++k) {
            if (k < regs.n) {
                if (regs.kind[k] == MCL_PEN_L2BALL) csq[k].add(f, ukeep[k], regs.nonneg[k], ok);
                else if (k == kpf2) gram.add(f, ukeep[k], ok, ytile, row16, g);
            }
        }
    }
    if (kpf2 >= 0) gram.store(stat_gram, tile, row16, g);
#pragma unroll
    for (int k = 0; k < MCL_MAX_REGS; ++k)
        if (k < regs.n && regs.kind[k] == MCL_PEN_L2BALL) csq[k].reduce_store(stat_colsq, tile, k, r, row16, g);
}

// per-slab sums of the per-tile statistics, fixed order: S[slab] (natural r x r layout) and colsq[k][slab]
__global__ __launch_bounds__(256) void k_stats_reduce(const int *__restrict__ slab_tile_ptr, const double *__restrict__ stat_gram,
                                                      const double *__restrict__ stat_colsq, RegSet regs, int r, int W,
                                                      int n_slabs, double *__restrict__ S, double *__restrict__ colsq) {
    MCL_GATE(regs.gate);
    const int slab = blockIdx.x;
    const int t0 = slab_tile_ptr[slab], t1 = slab_tile_ptr[slab + 1];
    int kpf2 = -1;
    for (int k = 0; k < regs.n; ++k)
        if (regs.kind[k] == MCL_PEN_PARAFAC2) kpf2 = k;
    if (kpf2 >= 0) {
        for (int e = threadIdx.x; e < r * r; e += 256) {
            const int a = e / r, b = e - a * r;
            double s0 = 0.0, s1 = 0.0;
            int t = t0;
            for (; t + 1 < t1; t += 2) {
                s0 += stat_gram[(long)t * W * W + a * W + b];
                s1 += stat_gram[(long)(t + 1) * W * W + a * W + b];
            }
            if (t < t1) s0 += stat_gram[(long)t * W * W + a * W + b];
            S[((long)slab * r + a) * r + b] = s0 + s1;
        }
    }
    for (int k = 0; k < regs.n; ++k) {
        if (regs.kind[k] != MCL_PEN_L2BALL) continue;
        for (int col = threadIdx.x; col < r; col += 256) {
            double s = 0.0;
            for (int t = t0; t < t1; ++t) s += stat_colsq[((long)t * MCL_MAX_REGS + k) * r + col];
            colsq[((long)k * n_slabs + slab) * r + col] = s;
        }
    }
}

// mode 0: every row has its own system (decomposition.py:184-195); one wave per row
__global__ __launch_bounds__(64) void k_A_rows_solve(const float *__restrict__ rhsA, const float *__restrict__ rhoA,
                                                     const float *__restrict__ LinvA, float *__restrict__ A,
                                                     RegSet regs, int r, double *__restrict__ change_part) {
    MCL_GATE(regs.gate);
    __shared__ float tS[MCL_MAX_RANK];
    const int i = blockIdx.x, lane = threadIdx.x;
    const bool act = lane < r;
    const int c = act ? lane : 0;
    const float rho = rhoA[i];
    float t = rhsA[(long)i * r + c];
    for (int k = 0; k < regs.n; ++k) t = fmaf(rho, regs.aux[k][(long)i * r + c] - regs.dual[k][(long)i * r + c], t);
    if (act) tS[c] = t;
    __syncthreads();
    float a = 0.f;
    for (int d = 0; d < r; ++d) a = fmaf(tS[d], LinvA[((long)i * r + d) * r + c], a);
    if (change_part != nullptr) {  // ||a_new - a_old||^2 of the row (the inner stopping test)
        const double d = act ? (double)a - (double)A[(long)i * r + c] : 0.0;
        const double s = wave_sum_d(d * d);
        if (lane == 0) change_part[i] = s;
    }
    if (act) A[(long)i * r + c] = a;
}

// row-separable prox + dual step of penalty k on the rows of A when every row has ITS OWN feasibility penalty rho_i
// (decomposition.py:197-213 with factor_matrix_row_update): the threshold of an L1 penalty is reg_strength / rho_i
__global__ __launch_bounds__(256) void k_A_rows_prox(const float *__restrict__ rhoA, float *__restrict__ A, RegSet regs, int k, int I,
                                                     int r) {
    MCL_GATE(regs.gate);
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long)I * r) return;
    const float rho = rhoA[e / r];
    const float f = A[e], u = regs.dual[k][e];
    const float z = prox_elem(regs.kind[k], regs.nonneg[k], regs.p0[k], regs.p1[k], regs.p0[k] / rho, f + u);
    regs.aux[k][e] = z;
    regs.dual[k][e] = f - (z - u);
}

// The inner stopping test of a phase (decomposition.py:90-117) on the device.  begin: flag <- the run's stop flag (a gated run
// that has stopped stays stopped).  Otherwise: change = sum of the solve pass's per-tile ||x - x_old||^2, norm and gaps from the
// per-tile diagnostics table (column 0: ||x||^2, columns 2 + k: ||aux_k - x||^2); converged = change <= tol * norm and
// every gap < tol (all on square roots, as the reference compares norms) -> flag = 1.  One workgroup, fixed summation order.
__global__ __launch_bounds__(256) void k_inner_check(int begin, const int *__restrict__ run_gate, int *__restrict__ flag,
                                                     const double *__restrict__ change_part, int n_change,
                                                     const double *__restrict__ diag_tab, int n_rows, int n_regs, double tol) {
    __shared__ double sm[256];
    if (begin) {
        if (threadIdx.x == 0) flag[0] = (run_gate != nullptr) ? run_gate[0] : 0;
        return;
    }
    if (flag[0] != 0) return;
    auto block_sum = [&](double v) {
        sm[threadIdx.x] = v;
        __syncthreads();
        for (int o = 128; o > 0; o >>= 1) {
            if ((int)threadIdx.x < o) sm[threadIdx.x] += sm[threadIdx.x + o];
            __syncthreads();
        }
        const double t = sm[0];
        __syncthreads();
        return t;
    };
    double v = 0.0;
    for (int e = threadIdx.x; e < n_change; e += 256) v += change_part[e];
    const double change = block_sum(v);
    v = 0.0;
    for (int e = threadIdx.x; e < n_rows; e += 256) v += diag_tab[(long)e * DIAG_COLS];
    const double norm = block_sum(v);
    bool ok = !(sqrt(change) > tol * sqrt(norm));
    for (int k = 0; k < n_regs; ++k) {
        v = 0.0;
        for (int e = threadIdx.x; e < n_rows; e += 256) v += diag_tab[(long)e * DIAG_COLS + 2 + k];
        const double gap = sqrt(block_sum(v)) / sqrt(norm);
        ok = ok && (gap < tol);
    }
    if (threadIdx.x == 0 && ok) flag[0] = 1;
}

// row-separable prox + dual update of penalty k (generic path)
template <int NBR, bool VEC>
__global__ __launch_bounds__(256) void k_rows_prox_rowsep(ModeView mv, RegSet regs, int k, int r) {
    ROW_TILE_PROLOGUE();
    const float rho = mv.rho[slab];
    const float thr = regs.p0[k] / rho;
    FOR_ROW_BLOCKS() {
        const bool ok = 16 * rb + row16 < nrows;
        const long j = row0 + 16 * rb + (ok ? row16 : 0);
#pragma unroll
        for (int h = 0; h < NBR; ++h) {
            const int col = 16 * h + 4 * g;
            const f32x4 f = row_ld4<VEC>(mv.F, j, col, ok, r);
            f32x4 u = row_ld4<VEC>(regs.dual[k], j, col, ok, r), z;
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                z[v] = prox_elem(regs.kind[k], regs.nonneg[k], regs.p0[k], regs.p1[k], thr, f[v] + u[v]);
                u[v] = f[v] - (z[v] - u[v]);
            }
            row_st4<VEC>(regs.aux[k], j, col, ok, r, z);
            row_st4<VEC>(regs.dual[k], j, col, ok, r, u);
        }
    }
}

// P = Y T_slab
template <int NBR, bool VEC>
__global__ __launch_bounds__(256) void k_pf2_apply(ModeView mv, const float *__restrict__ U, const float *__restrict__ T,
                                                   float *__restrict__ P, int r) {
    ROW_TILE_PROLOGUE();
    RowMat<NBR> Ts;
    Ts.load(T + (long)slab * r * r, r, lane);
    FOR_ROW_BLOCKS() {
        const bool ok = 16 * rb + row16 < nrows;
        const long j = row0 + 16 * rb + (ok ? row16 : 0);
        // Y = F + U as an unevaluated sum y + yl of two floats (Knuth's two-sum: exact), P = y T + yl T: the polar factor of the
        // SAME matrix whose Gram k_pf2_gram formed, not of its fp32 rounding
        f32x4 y[NBR], yl[NBR], p[NBR], pl[NBR];
#pragma unroll
        for (int h = 0; h < NBR; ++h) {
            const f32x4 f = row_ld4<VEC>(mv.F, j, 16 * h + 4 * g, ok, r);
            const f32x4 u = row_ld4<VEC>(U, j, 16 * h + 4 * g, ok, r);
            y[h] = f + u;
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const float bb = y[h][v] - f[v];
                yl[h][v] = (f[v] - (y[h][v] - bb)) + (u[v] - bb);
            }
        }
        Ts.apply(y, p);
        Ts.apply(yl, pl);
#pragma unroll
        for (int h = 0; h < NBR; ++h) row_st4<VEC>(P, j, 16 * h + 4 * g, ok, r, p[h] + pl[h]);
    }
}

// dual update of the PARAFAC2 penalty: U = F - (P Delta - U)
template <int NBR, bool VEC>
__global__ __launch_bounds__(256) void k_rows_pf2_dual(ModeView mv, RegSet regs, int k, int r) {
    ROW_TILE_PROLOGUE();
    RowMat<NBR> D;
    D.load(regs.aux2[k], r, lane);
    FOR_ROW_BLOCKS() {
        const bool ok = 16 * rb + row16 < nrows;
        const long j = row0 + 16 * rb + (ok ? row16 : 0);
        f32x4 p[NBR], z[NBR];
#pragma unroll
        for (int h = 0; h < NBR; ++h) p[h] = row_ld4<VEC>(regs.aux[k], j, 16 * h + 4 * g, ok, r);
        D.apply(p, z);
#pragma unroll
        for (int h = 0; h < NBR; ++h) {
            const int col = 16 * h + 4 * g;
            const f32x4 f = row_ld4<VEC>(mv.F, j, col, ok, r);
            f32x4 u = row_ld4<VEC>(regs.dual[k], j, col, ok, r);
#pragma unroll
            for (int v = 0; v < 4; ++v) u[v] = f[v] - (z[h][v] - u[v]);
            row_st4<VEC>(regs.dual[k], j, col, ok, r, u);
        }
    }
}

// plain dual update of penalty k: U = F - (Z - U)   (decomposition.py:282-285)
template <int NBR, bool VEC>
__global__ __launch_bounds__(256) void k_rows_dual(ModeView mv, RegSet regs, int k, int r) {
    ROW_TILE_PROLOGUE();
    FOR_ROW_BLOCKS() {
        const bool ok = 16 * rb + row16 < nrows;
        const long j = row0 + 16 * rb + (ok ? row16 : 0);
#pragma unroll
        for (int h = 0; h < NBR; ++h) {
            const int col = 16 * h + 4 * g;
            const f32x4 f = row_ld4<VEC>(mv.F, j, col, ok, r);
            const f32x4 z = row_ld4<VEC>(regs.aux[k], j, col, ok, r);
            f32x4 u = row_ld4<VEC>(regs.dual[k], j, col, ok, r);
#pragma unroll
            for (int v = 0; v < 4; ++v) u[v] = f[v] - (z[v] - u[v]);
            row_st4<VEC>(regs.dual[k], j, col, ok, r, u);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------
// ONE row pass for the prox + dual steps of a whole penalty stack made of row-separable kinds, L2 balls and PARAFAC2,
// once the per-slab statistics are known (column norms -> colsq; polar factor T_i and the new Delta): F is read once,
// P = (F + U) T_i stays in registers for its dual update.  Replaces k_pf2_apply + k_rows_pf2_dual + k_rows_l2ball
// (+ k_rows_prox_rowsep), i.e. three to four passes over the B-sized arrays per inner iteration.
// ---------------------------------------------------------------------------------------------------------
template <int NBR, bool VEC, bool R64 = false>
__global__ __launch_bounds__(256) void k_rows_finish_fused(ModeView mv, RegSet regs, int r, const float *__restrict__ T,
                                                           const double *__restrict__ colsq,
                                                           double *__restrict__ diag_tile, int want_diag,
                                                           const double *__restrict__ T64 = nullptr) {
    typedef RowArith<R64> RA;  // R64: the r x r products on the fp64 MFMA, exact Y = F + U (see k_rows_solve_stats)
    ROW_TILE_PROLOGUE();
    TileDiag diag;
    diag.clear();
    const float rho = mv.rho[slab];
    const int kpf2 = last_of_kind(regs, MCL_PEN_PARAFAC2);
    typename RA::template Mat<NBR> Ts, D;
    if (kpf2 >= 0) {
        load_slab_mat<R64>(Ts, T, T64, slab, r, lane);
        D.load(regs.aux2[kpf2], r, lane);
    }
    FOR_ROW_BLOCKS() {
        const bool ok = 16 * rb + row16 < nrows;
        const long j = row0 + 16 * rb + (ok ? row16 : 0);
        f32x4 f[NBR];
#pragma unroll
        for (int h = 0; h < NBR; ++h) f[h] = (row_ld4<VEC>(mv.F, j, 16 * h + 4 * g, ok, r));  // zeros for padding rows / columns
        if (want_diag) diag.add_f(f);
#pragma unroll
        for (int k = 0; k < MCL_MAX_REGS; ++k) {
            if (k >= regs.n) continue;
            const int cls = class_of(regs.kind[k]);
            f32x4 u[NBR], z[NBR], zg[NBR];
#pragma unroll
            for (int h = 0; h < NBR; ++h) u[h] = (row_ld4<VEC>(regs.dual[k], j, 16 * h + 4 * g, ok, r));
            // any number of L2 balls here, so a ball's scales are formed per element (the chained kernels hoist their one ball's)
            const auto aux_rows = [&](int h) ROWS_INLINE { return row_ld4<VEC>(regs.aux[k], j, 16 * h + 4 * g, ok, r); };
            const auto l2_scale = [&](int h, int v) ROWS_INLINE {
                return l2_ball_scale(regs, k, colsq, mv.n_slabs, slab, r, 16 * h + 4 * g + v);
            };
            stack_prox<RA, NBR>(cls, regs, k, rho, Ts, D, f, u, aux_rows, l2_scale, z, zg);
            dual_step(f, zg, u);
#pragma unroll
            for (int h = 0; h < NBR; ++h) {
                if (cls != CLS_UNI) row_st4<VEC>(regs.aux[k], j, 16 * h + 4 * g, ok, r, z[h]);
                row_st4<VEC>(regs.dual[k], j, 16 * h + 4 * g, ok, r, u[h]);
            }
            if (want_diag) diag.add_gap(k, zg, f, ok, r, g);
        }
    }
    if (want_diag) diag.store(diag_tile, tile, lane);
}

// ---------------------------------------------------------------------------------------------------------
// Inner iteration t -> t+1 of a fused stack in ONE row pass (mode 1, single process): the prox + dual steps of
// iteration t (k_rows_finish_fused) followed, on the same registers, by the solve of iteration t+1 and the statistics
// of its new rows (k_rows_solve_stats).  Z_k - U_k of every penalty stays in registers, so between two inner iterations
// the pass reads F, the duals, rhs (+ the aux rows the column regressions wrote) and writes F and the duals:
// (2 + 2n + 1) S_B instead of (2 + 2n) + (1 + 4n) S_B for the two separate passes.  The aux rows are not written here -
// no later step of the inner loop reads them (PARAFAC2's Delta and T_i carry its state); the LAST inner iteration ends
// with the plain k_rows_finish_fused, which writes them and the diagnostics.
// ---------------------------------------------------------------------------------------------------------
template <int NBR, bool VEC, bool R64 = false>
__global__ __launch_bounds__(256) void k_rows_finish_solve_stats(ModeView mv, const float *__restrict__ rhs_src,
                                                                 const float *__restrict__ Arows,
                                                                 const float *__restrict__ Linv, RegSet regs, int r,
                                                                 const float *__restrict__ T,
                                                                 const double *__restrict__ colsq,
                                                                 double *__restrict__ stat_gram,
                                                                 double *__restrict__ stat_colsq,
                                                                 const double *__restrict__ Linv64 = nullptr,
                                                                 const double *__restrict__ T64 = nullptr) {
    typedef RowArith<R64> RA;  // R64: the r x r products on the fp64 MFMA, exact Y = F + U (see k_rows_solve_stats)
    __shared__ double ytile[YGram<NBR, R64>::LDS_DOUBLES];  // R64: one padded 16 x 16 fp64 tile per wave (row -> column layout of Y)
    ROW_TILE_PROLOGUE();
    const float rho = mv.rho[slab];
    const int kpf2 = last_of_kind(regs, MCL_PEN_PARAFAC2);
    typename RA::template Mat<NBR> L, Ts, D;
    load_slab_mat<R64>(L, Linv, Linv64, slab, r, lane);
    if (kpf2 >= 0) {
        load_slab_mat<R64>(Ts, T, T64, slab, r, lane);
        D.load(regs.aux2[kpf2], r, lane);
    }
    float av[NBR][4], l2s[NBR][4];
    a_col_scale(Arows, slab, r, g, av);
    // L2-ball scale factors of iteration t (from the per-slab column norms); the host chains stacks with at most ONE
    // L2 ball (register budget: two waves per SIMD at rank 32)
    const int kl2 = last_of_kind(regs, MCL_PEN_L2BALL);
    l2_ball_scales(regs, kl2, colsq, mv.n_slabs, slab, r, g, l2s);
    YGram<NBR, R64> gram;
    gram.clear(row16, g);
    ColSq<NBR> csq;
    csq.clear();
    FOR_ROW_BLOCKS() {
        const bool ok = 16 * rb + row16 < nrows;
        const long j = row0 + 16 * rb + (ok ? row16 : 0);
        f32x4 f[NBR], t[NBR], upf[NBR], ul2[NBR];  // new duals of the PARAFAC2 / L2-ball penalty (statistics below)
#pragma unroll
        for (int h = 0; h < NBR; ++h) {
            f[h] = (row_ld4<VEC>(mv.F, j, 16 * h + 4 * g, ok, r));  // zeros for padding rows / columns
            t[h] = (row_ld4<VEC>(rhs_src, j, 16 * h + 4 * g, ok, r));
#pragma unroll
            for (int v = 0; v < 4; ++v) t[h][v] *= av[h][v];
        }
        // ---- iteration t: prox + dual of every penalty
#pragma unroll
        for (int k = 0; k < MCL_MAX_REGS; ++k) {
            if (k >= regs.n) continue;
            const int cls = class_of(regs.kind[k]);
            f32x4 u[NBR], z[NBR], zg[NBR];
#pragma unroll
            for (int h = 0; h < NBR; ++h) u[h] = (row_ld4<VEC>(regs.dual[k], j, 16 * h + 4 * g, ok, r));
            const auto aux_rows = [&](int h) ROWS_INLINE { return row_ld4<VEC>(regs.aux[k], j, 16 * h + 4 * g, ok, r); };
            const auto l2_scale = [&](int h, int v) ROWS_INLINE { return l2s[h][v]; };
            stack_prox<RA, NBR>(cls, regs, k, rho, Ts, D, f, u, aux_rows, l2_scale, z, zg);
            dual_step(f, zg, u);
            rhs_add(rho, zg, u, t);
#pragma unroll
            for (int h = 0; h < NBR; ++h) {
                row_st4<VEC>(regs.dual[k], j, 16 * h + 4 * g, ok, r, u[h]);
                if (k == kpf2) upf[h] = u[h];
                if (k == kl2) ul2[h] = u[h];
            }
        }
        // ---- iteration t + 1: solve, store, statistics of the new rows
        f32x4 fn[NBR];
        L.apply(t, fn);
#pragma unroll
        for (int h = 0; h < NBR; ++h) row_st4<VEC>(mv.F, j, 16 * h + 4 * g, ok, r, fn[h]);
        if (kl2 >= 0) csq.add(fn, ul2, regs.nonneg[kl2], ok);
        if (kpf2 >= 0) gram.add(fn, upf, ok, ytile, row16, g);
    }
    if (kpf2 >= 0) gram.store(stat_gram, tile, row16, g);
    if (kl2 >= 0) csq.reduce_store(stat_colsq, tile, kl2, r, row16, g);
}

// =========================================================================================================
// host launchers
// =========================================================================================================
// fp64 row algebra for the B-mode passes of a fused stack with a PARAFAC2 member, rank <= 16 (the kernels above with
// R64 = true): decided by the plan (it owns the fp64 copies of L_i^-1 and T_i); see k_rows_solve_stats
bool mcl_rows64(const mcl_context *c) { return c->rows64 && c->LinvB64 != nullptr && c->pf2_T64 != nullptr; }

// DISPATCH_ROWS for the <NBR, VEC, R64> kernels of the chained B passes (rank <= 32): fp64 algebra at rank <= 16, else fp32
#define DISPATCH_ROWS_R64(c, vec, r64, KERNEL, grid, block, ...)                                              \
    do {                                                                                                      \
        if (r64) {                                                                                            \
            if (vec) hipLaunchKernelGGL((KERNEL<1, true, true>), grid, block, 0, (c)->stream, __VA_ARGS__);   \
            else hipLaunchKernelGGL((KERNEL<1, false, true>), grid, block, 0, (c)->stream, __VA_ARGS__);      \
        } else if ((c)->NB == 1) {                                                                            \
            if (vec) hipLaunchKernelGGL((KERNEL<1, true, false>), grid, block, 0, (c)->stream, __VA_ARGS__);  \
            else hipLaunchKernelGGL((KERNEL<1, false, false>), grid, block, 0, (c)->stream, __VA_ARGS__);     \
        } else {                                                                                              \
            if (vec) hipLaunchKernelGGL((KERNEL<2, true, false>), grid, block, 0, (c)->stream, __VA_ARGS__);  \
            else hipLaunchKernelGGL((KERNEL<2, false, false>), grid, block, 0, (c)->stream, __VA_ARGS__);     \
        }                                                                                                     \
    } while (0)

int mcl_launch_inner_check_raw(mcl_context *c, bool begin, const double *change_part, int n_change, const double *tab, int n_rows,
                               int n_regs) {
    ProfScope prof(c, MCL_PROF_OTHER);
    hipLaunchKernelGGL(k_inner_check, dim3(1), dim3(256), 0, c->stream, begin ? 1 : 0, begin ? c->gate_active : nullptr, c->inner_gate,
                       change_part, n_change, tab, n_rows, n_regs, c->opt.inner_tol);
    MCL_CHECK_HIP(c, hipGetLastError());
    return 0;
}

int mcl_launch_inner_check(mcl_context *c, int mode, bool begin) {
    const int n_change = (mode == 0) ? (int)c->I : mcl_tiles(c, mode).n_tiles;
    return mcl_launch_inner_check_raw(c, begin, c->inner_part, n_change, mcl_diag_tile(c, mode), c->bp.diag_rows[mode], c->regs[mode].n);
}

int mcl_launch_rows_solve(mcl_context *c, int mode, double *change_part) {
    ModeView mv = view_of(c, mode);
    if (mv.n_tiles == 0) return 0;
    const float *rhs = (mode == 1) ? c->XC : c->GRf + (long)c->r * c->r;  // fp32 image of R (k_C_prepare)
    const float *Arows = (mode == 1) ? c->A : nullptr;
    const float *Linv = (mode == 1) ? c->LinvB : c->LinvC;
    dim3 grid((unsigned)((mv.n_tiles + 3) / 4)), block(256);
    const bool vec = mcl_rows_vec_ok(c->r, c->regs[mode], mv.F, rhs);
    ProfScope prof(c, mode == 1 ? MCL_PROF_ROWS_CHAIN : MCL_PROF_OTHER);
    if (mode == 1) c->variant[MCL_PROF_ROWS_CHAIN] = "k_rows_solve";
    DISPATCH_ROWS(c, vec, k_rows_solve, grid, block, mv, rhs, Arows, Linv, c->regs[mode], c->r, change_part);
    MCL_CHECK_HIP(c, hipGetLastError());
    return 0;
}

int mcl_launch_A_rows_solve(mcl_context *c, double *change_part) {
    if (c->I == 0) return 0;
    hipLaunchKernelGGL(k_A_rows_solve, dim3((unsigned)c->I), dim3(64), 0, c->stream, c->rhsA, c->rhoA, c->LinvA, c->A,
                       c->regs[0], c->r, change_part);
    MCL_CHECK_HIP(c, hipGetLastError());
    return 0;
}

// The local part of the prox of penalty k.  A kind that needs more than a row pass calls into the file that owns it; what is
// enqueued here keeps the order of the steps on the stream.
int mcl_launch_generic_prox_local(mcl_context *c, int mode, int k, ProxForm form) {
    ModeView mv = view_of(c, mode);
    if (mv.n_tiles == 0) return 0;
    const RegSet &rs = c->regs[mode];
    dim3 grid((unsigned)((mv.n_tiles + 3) / 4)), block(256);
    const bool vec = mcl_rows_vec_ok(c->r, rs, mv.F);
    const int kind_k = rs.kind[k];
    ProfScope prof(c, kind_k == MCL_PEN_PARAFAC2 ? MCL_PROF_PF2 : (kind_k == MCL_PEN_UNIMODAL ? MCL_PROF_UNIMODAL : MCL_PROF_OTHER));
    switch (kind_k) {
        case MCL_PEN_NN:
        case MCL_PEN_BOX:
        case MCL_PEN_L1:
            if (form.stack_fused) break;  // no statistics; the fused finish pass does the prox
            if (mode == 0 && !c->opt.constant_A) {  // per-row feasibility penalties (the un-fused A loop of the inner stopping test)
                hipLaunchKernelGGL(k_A_rows_prox, dim3((unsigned)((c->I * c->r + 255) / 256)), dim3(256), 0, c->stream,
                                   (const float *)c->rhoA, c->A, rs, k, (int)c->I, c->r);
                break;
            }
            DISPATCH_ROWS(c, vec, k_rows_prox_rowsep, grid, block, mv, rs, k, c->r);
            break;
        case MCL_PEN_L2BALL:
            mcl_launch_prox_l2ball(c, mv, rs, k, vec, form);
            break;
        case MCL_PEN_UNIMODAL:
            if (int rc = mcl_launch_unimodal(c, mv.ext, mv.n_slabs, mv.F, rs, mode, k)) return rc;  // unimodal.hip
            if (!form.stack_fused)  // the fused finish pass updates the dual
                DISPATCH_ROWS(c, vec, k_rows_dual, grid, block, mv, rs, k, c->r);
            break;
        case MCL_PEN_TV:
            mcl_launch_prox_tv(c, mv, rs, k);
            DISPATCH_ROWS(c, vec, k_rows_dual, grid, block, mv, rs, k, c->r);
            break;
        case MCL_PEN_PARAFAC2:
            if (mode != 1) {
                c->err = "PARAFAC2 constraint can only be imposed with mode=1";
                return 1;
            }
            if (int rc = mcl_launch_pf2_polar(c, k, form)) return rc;
            if (!form.stack_fused)  // the fused finish pass applies T_i itself
                DISPATCH_ROWS(c, vec, k_pf2_apply, grid, block, mv, (const float *)rs.dual[k], (const float *)c->pf2_T, rs.aux[k], c->r);
            mcl_launch_pf2_sum(c, k, form);
            break;
        case MCL_PEN_GL2:
            mcl_launch_prox_gl2(c, mv, rs, k);
            break;
        case MCL_PEN_SIMPLEX:
            mcl_launch_prox_simplex(c, mv, rs, k);
            DISPATCH_ROWS(c, vec, k_rows_dual, grid, block, mv, rs, k, c->r);
            break;
        default:
            c->err = "penalty kind has no native prox (EXTERNAL penalties are evaluated by the host)";
            return 1;
    }
    MCL_CHECK_HIP(c, hipGetLastError());
    return 0;
}

int mcl_launch_generic_prox_finish(mcl_context *c, int mode, int k, ProxForm form) {
    const RegSet &rs = c->regs[mode];
    if (rs.kind[k] != MCL_PEN_PARAFAC2) return 0;  // dual update already fused into the local step
    ModeView mv = view_of(c, mode);
    if (mv.n_tiles == 0) return 0;
    if (!form.pf2_delta_fused) mcl_launch_pf2_delta(c, k);
    if (!form.stack_fused) {  // (the dual update of a fused stack rides in its finish pass)
        dim3 grid((unsigned)((mv.n_tiles + 3) / 4)), block(256);
        const bool vec = mcl_rows_vec_ok(c->r, rs, mv.F);
        DISPATCH_ROWS(c, vec, k_rows_pf2_dual, grid, block, mv, rs, k, c->r);
    }
    MCL_CHECK_HIP(c, hipGetLastError());
    return 0;
}

// A penalty stack of row-separable kinds, L2 balls, unimodality and PARAFAC2 (at least one of the latter three, no
// host-evaluated member) can take ONE row pass for all prox + dual steps after the per-slab work (statistics; for
// unimodality the column regressions themselves, which write the aux rows - the pass then only updates their dual).
bool mcl_stack_can_fuse(const mcl_context *c, int mode) {
    if (c->sw.no_stack_fusion) return false;
    const RegSet &rs = c->regs[mode];
    bool slabwise = false;
    for (int k = 0; k < rs.n; ++k) {
        const int kind = rs.kind[k];
        if (kind == MCL_PEN_L2BALL || kind == MCL_PEN_PARAFAC2 || kind == MCL_PEN_UNIMODAL) slabwise = true;
        else if (kind != MCL_PEN_NN && kind != MCL_PEN_BOX && kind != MCL_PEN_L1) return false;
    }
    return slabwise && mode != 0;
}

int mcl_launch_rows_finish_fused(mcl_context *c, int mode, bool want_diag) {
    ModeView mv = view_of(c, mode);
    if (mv.n_tiles == 0) return 0;
    const RegSet &rs = c->regs[mode];
    dim3 grid((unsigned)((mv.n_tiles + 3) / 4)), block(256);
    const bool vec = mcl_rows_vec_ok(c->r, rs, mv.F);
    double *diag = (mode == 1) ? c->diagB_tile : c->diagC_tile;
    ProfScope prof(c, mode == 1 ? MCL_PROF_ROWS_CHAIN : MCL_PROF_OTHER);
    if (mode == 1) c->variant[MCL_PROF_ROWS_CHAIN] = mcl_rows64(c) ? "k_rows_finish_solve_stats<R64> chain (solve_stats -> finish_solve_stats x (n-1) -> finish_fused)" : "k_rows_finish_solve_stats chain (solve_stats -> finish_solve_stats x (n-1) -> finish_fused)";
    if (mode == 1 && mcl_try_rows_chain_last(c, mv, vec, mcl_rows64(c), diag, want_diag ? 1 : 0)) {
        // (rowchain.hip: software-pipelined form)
        c->variant[MCL_PROF_ROWS_CHAIN] = mcl_rows64(c) ? "k_rows_chain_first<R64> -> k_rows_chain_mid x (n-1) -> k_rows_chain_last (software-pipelined chain)"
                                                         : "k_rows_chain_first -> k_rows_chain_mid x (n-1) -> k_rows_chain_last (software-pipelined chain)";
    } else if (mode == 1 && mcl_rows64(c)) {  // rank <= 16 with a PARAFAC2 member: fp64 row algebra
        DISPATCH_ROWS_R64(c, vec, true, k_rows_finish_fused, grid, block, mv, rs, c->r, (const float *)c->pf2_T, (const double *)c->colsq,
                          diag, want_diag ? 1 : 0, (const double *)c->pf2_T64);
    } else {
        DISPATCH_ROWS(c, vec, k_rows_finish_fused, grid, block, mv, rs, c->r, (const float *)c->pf2_T, (const double *)c->colsq,
                      diag, want_diag ? 1 : 0, (const double *)nullptr);
    }
    MCL_CHECK_HIP(c, hipGetLastError());
    if (want_diag) c->bp.diag_rows[mode] = mv.n_tiles;  // one row per tile, as k_rows_diag writes them
    return 0;
}

// mode 1 only (that is where the passes are big); needs the per-tile tables of the plan
bool mcl_stats_can_ride_in_solve(const mcl_context *c, int mode) {
    if (mode != 1 || c->sw.no_solve_stats) return false;
    const RegSet &rs = c->regs[1];
    for (int k = 0; k < rs.n; ++k) {
        if (rs.kind[k] == MCL_PEN_PARAFAC2 && !c->stat_gram) return false;
        if (rs.kind[k] == MCL_PEN_L2BALL && !c->stat_colsq) return false;
    }
    return c->NB <= 2;  // fp64 accumulators: (16 NB)^2 / 64 doubles per lane
}

// What the two B passes that leave per-tile statistics share: the view, the launch shape, `pass` (the row kernel, or its
// pipelined form of rowchain.hip) and, unless the Newton-Schulz kernel sums the tiles itself, k_stats_reduce behind it
template <typename PASS>
static int rows_stats_pass(mcl_context *c, PASS pass) {
    ModeView mv = view_of(c, 1);
    if (mv.n_tiles == 0) return 0;
    const float *rhs = c->XC;
    dim3 grid((unsigned)((mv.n_tiles + 3) / 4)), block(256);
    const bool vec = mcl_rows_vec_ok(c->r, c->regs[1], mv.F, rhs);
    {
        ProfScope prof(c, MCL_PROF_ROWS_CHAIN);
        pass(mv, rhs, grid, block, vec);
    }
    ProfScope prof2(c, MCL_PROF_OTHER);
    if (!mcl_stats_reduce_in_algebra(c))
        hipLaunchKernelGGL(k_stats_reduce, dim3((unsigned)c->I), dim3(256), 0, c->stream, (const int *)c->slab_tile_ptr,
                           (const double *)c->stat_gram, (const double *)c->stat_colsq, c->regs[1], c->r, 16 * c->NB,
                           (int)c->I, c->pf2_S, c->colsq);
    MCL_CHECK_HIP(c, hipGetLastError());
    return 0;
}

// finish of inner iteration t + solve / statistics of iteration t + 1 in one pass (see k_rows_finish_solve_stats)
int mcl_launch_rows_finish_solve_stats(mcl_context *c) {
    return rows_stats_pass(c, [c](const ModeView &mv, const float *rhs, dim3 grid, dim3 block, bool vec) {
        // (rowchain.hip: the same pass with its loads software-pipelined, for the stacks it is instantiated for)
        if (mcl_try_rows_chain_mid(c, mv, rhs, vec, mcl_rows64(c))) return;
        DISPATCH_ROWS_R64(c, vec, mcl_rows64(c), k_rows_finish_solve_stats, grid, block, mv, rhs, (const float *)c->A,
                          (const float *)c->LinvB, c->regs[1], c->r, (const float *)c->pf2_T, (const double *)c->colsq, c->stat_gram,
                          c->stat_colsq, (const double *)c->LinvB64, (const double *)c->pf2_T64);
    });
}

int mcl_launch_rows_solve_stats(mcl_context *c) {
    return rows_stats_pass(c, [c](const ModeView &mv, const float *rhs, dim3 grid, dim3 block, bool vec) {
        if (mcl_try_rows_chain_first(c, mv, rhs, vec, mcl_rows64(c))) return;  // (rowchain.hip: software-pipelined form)
        DISPATCH_ROWS_R64(c, vec, mcl_rows64(c), k_rows_solve_stats, grid, block, mv, rhs, (const float *)c->A, (const float *)c->LinvB,
                          c->regs[1], c->r, c->stat_gram, c->stat_colsq, (const double *)c->LinvB64);
    });
}
