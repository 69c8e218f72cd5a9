// Diagnostics of the AO-ADMM engine (gfx950): the reduction of the per-tile / per-slab tables into the MCL_DIAG_LEN vector,
// the device-side stopping rule of mcl_run on that vector, and the per-tile sums of a factor read back from memory.
//
// Reference sites: E1-E3 (decomposition.py:404-417, 445-452, 916-921), the outer loop's test (:990-1053).
#include <algorithm>

#include "mcl_internal.h"
#include "xload.h"
#include "rows_mfma.h"

// ---------------------------------------------------------------------------------------------------------
// diagnostics: ||X||^2 (once) and ONE launch that reduces every per-tile / per-slab table and assembles the
// MCL_DIAG_LEN vector.  Block b < 3*DIAG_COLS reduces column (b % DIAG_COLS) of table (b / DIAG_COLS) in
// {A rows, B tiles, C tiles}; the next two blocks reduce the e1 columns; the last block writes the constants.
// Every output entry is written by exactly one block (fixed summation order: deterministic).
// ---------------------------------------------------------------------------------------------------------
template <class XL>
static __device__ __forceinline__ void k_sumsq_partial_body(const typename XL::T *X, long n, double *part) {
    __shared__ double sm[4];
    double s = 0.0;
    const long stride = (long)gridDim.x * 256 * 4;
    for (long e = ((long)blockIdx.x * 256 + threadIdx.x) * 4; e < n; e += stride) {
        if (e + 3 < n) {
            const mcl_xf32x4 v = XL::cvt(XL::template ld4<false>(X + e));
            s += (double)v.x * v.x + (double)v.y * v.y + (double)v.z * v.z + (double)v.w * v.w;
        } else {
            for (long t = e; t < n; ++t) s += (double)XL::ld1(X + t) * (double)XL::ld1(X + t);
        }
    }
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = (sm[0] + sm[1]) + (sm[2] + sm[3]);
}
__global__ __launch_bounds__(256) void k_sumsq_partial(const float *__restrict__ X, long n, double *__restrict__ part) {
    k_sumsq_partial_body<XF32>(X, n, part);
}
// the 16-bit twin (xload.h): the same template arguments after the element type
template <class XL>
__global__ __launch_bounds__(256) void k_sumsq_partial_h(const typename XL::T *__restrict__ X, long n, double *__restrict__ part) {
    k_sumsq_partial_body<XL>(X, n, part);
}

__global__ __launch_bounds__(256) void k_sum_doubles(const double *__restrict__ part, int n, double *__restrict__ out) {
    __shared__ double sm[4];
    double s = 0.0;
    for (int e = threadIdx.x; e < n; e += 256) s += part[e];
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) out[0] = (sm[0] + sm[1]) + (sm[2] + sm[3]);
}


// column sum of a [n_rows, ncols] fp64 table by one workgroup of 256 or 1024 threads (fixed order for a given block size: the
// launchers pick the size from the table lengths alone, so it is the same on every rank and in every iteration)
static __device__ double block_colsum(const double *__restrict__ tab, int n_rows, int ncols, int col, double *sm) {
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    const int nt = blockDim.x;
    int e = threadIdx.x;
    for (; e + 3 * nt < n_rows; e += 4 * nt) {
        s0 += tab[(long)e * ncols + col];
        s1 += tab[(long)(e + nt) * ncols + col];
        s2 += tab[(long)(e + 2 * nt) * ncols + col];
        s3 += tab[(long)(e + 3 * nt) * ncols + col];
    }
    for (; e < n_rows; e += nt) s0 += tab[(long)e * ncols + col];
    double s = wave_sum((s0 + s1) + (s2 + s3));
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = s;
    __syncthreads();
    double t = 0.0;
    for (int w = 0; w < (nt >> 6); w += 4) t += (sm[w] + sm[w + 1]) + (sm[w + 2] + sm[w + 3]);
    return t;
}

__global__ __launch_bounds__(1024) void k_diag_final(DiagTables T, int include_replicated, double *__restrict__ out) {
    __shared__ double sm[16];
    const int b = blockIdx.x;
    if (b < 3 * DIAG_COLS) {
        const int t = b / DIAG_COLS, col = b - t * DIAG_COLS;
        const bool live = (t < 2) || include_replicated;
        const double s = (live && T.rows[t] > 0) ? block_colsum(T.tab[t], T.rows[t], DIAG_COLS, col, sm) : 0.0;
        if (threadIdx.x == 0) {
            if (col == 0) {
                out[MCL_DIAG_NORM_SQ + t] = s;
            } else if (col == 1) {
                for (int k = 0; k < MCL_MAX_REGS; ++k)
                    out[MCL_DIAG_REG + (t * MCL_MAX_REGS + k) * 2 + 1] = (k < T.nreg[t]) ? s : 0.0;
            } else {
                const int k = col - 2;
                out[MCL_DIAG_REG + (t * MCL_MAX_REGS + k) * 2] = (k < T.nreg[t]) ? s : 0.0;
            }
        }
    } else if (b < 3 * DIAG_COLS + 2) {
        const int col = b - 3 * DIAG_COLS;
        const double s = (T.I > 0) ? block_colsum(T.e1, T.I, 2, col, sm) : 0.0;
        if (threadIdx.x == 0) out[col == 0 ? MCL_DIAG_INNER : MCL_DIAG_MODEL_SQ] = s;
    } else if (threadIdx.x == 0) {
        out[MCL_DIAG_X_SQ] = T.xsq[0];
        out[6] = 0.0;
        out[7] = 0.0;
    }
}

// ---- device-side stopping rule (mcl_run) ---------------------------------------------------------------------------
// The reduction of the diagnostics tables of k_diag_final, and in the LAST block to finish (ticket) the stopping test of
// the reference's outer loop (decomposition.py:990-1053) on the reduced vector: feasibility gaps (:404-417, :996),
// relative reconstruction error (:1013-1014), regularised loss (:1016-1023), relative / absolute loss criterion
// (:1037-1053) with the quirks kept (Q8: the absolute criterion only counts when `tol` is set; Q9: it tests the newest
// loss; Q10: no loss on an infeasible iterate unless the caller records errors, so "previous loss" means the previous
// COMPUTED one).  A hit sets the gate flag every state-writing kernel of the iterations enqueued behind this one tests
// (MCL_GATE), and is reported - like every iteration's progress - through four int32 in pinned host memory.
struct StopRuleDev {
    double tol, abs_tol, feas_tol;
    double l2[3];
    double w[3][MCL_MAX_REGS];
    int has_tol, has_feas, loss_always, it;
};

// one thread: the stopping test on a complete diagnostics vector (read with device-scope loads: other workgroups wrote it)
static __device__ void verdict_eval(const double *out, const int *nreg, const StopRuleDev &R, int *gate, double *state,
                                    double *verdict_row, int *status_host) {
    auto ld = [&](int i) { return __hip_atomic_load(out + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); };
    // feasibility gaps ||aux - factor|| / ||factor||, worst over all penalties of all modes (vacuously feasible without any)
    double worst = -__builtin_inf();
    for (int m = 0; m < 3; ++m) {
        const double fn = sqrt(ld(MCL_DIAG_NORM_SQ + m));
        for (int k = 0; k < nreg[m]; ++k) {
            const double gap = sqrt(ld(MCL_DIAG_REG + (m * MCL_MAX_REGS + k) * 2)) / fn;
            worst = (gap > worst || gap != gap) ? gap : worst;  // a NaN gap is never feasible
        }
    }
    const bool feasible = R.has_feas && (worst < R.feas_tol);
    int code = 0, computed = 0;
    double rec = 0.0, loss = 0.0;
    if (feasible || R.loss_always) {
        const double xsq = ld(MCL_DIAG_X_SQ), inner = ld(MCL_DIAG_INNER), model = ld(MCL_DIAG_MODEL_SQ);
        rec = sqrt(fmax(0.0, xsq - 2.0 * inner + model)) / sqrt(xsq);
        double reg = 0.0;
        for (int m = 0; m < 3; ++m) {
            for (int k = 0; k < nreg[m]; ++k)
                if (R.w[m][k] != 0.0) reg += R.w[m][k] * ld(MCL_DIAG_REG + (m * MCL_MAX_REGS + k) * 2 + 1);
            if (R.l2[m] != 0.0) reg += 0.5 * R.l2[m] * ld(MCL_DIAG_NORM_SQ + m);
        }
        loss = 0.5 * (rec * rec) + reg;
        computed = 1;
        if (R.has_tol) {
            const double prev = state[0];
            const bool rel = fabs(prev - loss) < R.tol * prev;
            const bool absc = loss < R.abs_tol;
            if (feasible && rel) code = 1;
            else if (feasible && absc) code = 2;
        }
        state[0] = loss;
    }
    verdict_row[0] = rec, verdict_row[1] = loss, verdict_row[2] = worst;
    verdict_row[3] = (double)((feasible ? 1 : 0) | (computed << 1) | (code << 2));
    if (code) {
        gate[1] = R.it, gate[2] = code;
        __threadfence();
        gate[0] = 1;
        status_host[1] = R.it, status_host[2] = code;
        __threadfence_system();
        status_host[0] = 1;
    }
    status_host[3] = R.it + 1;  // progress: the host keeps its run-ahead bounded by this
    __threadfence_system();
}

__global__ __launch_bounds__(1024) void k_diag_verdict(DiagTables T, double *__restrict__ out, StopRuleDev R,
                                                       int *__restrict__ gate, double *__restrict__ state,
                                                       double *__restrict__ verdict_row, int *__restrict__ status_host) {
    __shared__ double sm[16];
    __shared__ int last;
    if (*gate != 0) return;  // an earlier iteration has stopped the run: nothing is evaluated any more
    const int b = blockIdx.x;
    if (b < 3 * DIAG_COLS) {
        const int t = b / DIAG_COLS, col = b - t * DIAG_COLS;
        const double s = (T.rows[t] > 0) ? block_colsum(T.tab[t], T.rows[t], DIAG_COLS, col, sm) : 0.0;
        if (threadIdx.x == 0) {
            if (col == 0) {
                out[MCL_DIAG_NORM_SQ + t] = s;
            } else if (col == 1) {
                for (int k = 0; k < MCL_MAX_REGS; ++k)
                    out[MCL_DIAG_REG + (t * MCL_MAX_REGS + k) * 2 + 1] = (k < T.nreg[t]) ? s : 0.0;
            } else {
                const int k = col - 2;
                out[MCL_DIAG_REG + (t * MCL_MAX_REGS + k) * 2] = (k < T.nreg[t]) ? s : 0.0;
            }
        }
    } else if (b < 3 * DIAG_COLS + 2) {
        const int col = b - 3 * DIAG_COLS;
        const double s = (T.I > 0) ? block_colsum(T.e1, T.I, 2, col, sm) : 0.0;
        if (threadIdx.x == 0) out[col == 0 ? MCL_DIAG_INNER : MCL_DIAG_MODEL_SQ] = s;
    } else if (threadIdx.x == 0) {
        out[MCL_DIAG_X_SQ] = T.xsq[0];
        out[6] = 0.0;
        out[7] = 0.0;
    }
    if (threadIdx.x == 0) {
        __threadfence();  // this block's entries of `out` are visible device-wide before its ticket
        const int ticket = atomicAdd(gate + 3, 1);
        last = ticket == (int)gridDim.x - 1;
    }
    __syncthreads();
    if (!last || threadIdx.x != 0) return;
    __threadfence();
    gate[3] = 0;  // ticket counter ready for the next launch (stream order)
    verdict_eval(out, T.nreg, R, gate, state, verdict_row, status_host);
}

// The same test on a vector that is already complete - the sharded loop: every rank reduces its tables (mcl_diagnostics),
// the host all-reduces the vectors, then every rank evaluates the rule on the SAME bits and reaches the same verdict.
__global__ __launch_bounds__(64) void k_verdict(const double *__restrict__ vec, StopRuleDev R, int n0, int n1, int n2,
                                                int *__restrict__ gate, double *__restrict__ state,
                                                double *__restrict__ verdict_row, int *__restrict__ status_host) {
    if (*gate != 0 || threadIdx.x != 0) return;
    const int nreg[3] = {n0, n1, n2};
    verdict_eval(vec, nreg, R, gate, state, verdict_row, status_host);
}

// Per-tile diagnostics of a packed factor from memory (generic path / initial state):
// ||F||^2, sum|F|, ||Z_k - F||^2 with Z_k = aux_k or P Delta (PARAFAC2; product on the MFMA).  Tile layout of rows_mfma.h.
template <int NBR, bool VEC>
__global__ __launch_bounds__(256) void k_rows_diag(const int *__restrict__ tile_row0, const int *__restrict__ tile_nrows,
                                                   int n_tiles, const float *__restrict__ F, RegSet regs, int r,
                                                   double *__restrict__ diag_tile) {
    MCL_GATE(regs.gate);
    const int lane = threadIdx.x & 63;
    const int tile = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (tile >= n_tiles) return;
    const long row0 = __builtin_amdgcn_readfirstlane(tile_row0[tile]);
    const int nrows = __builtin_amdgcn_readfirstlane(tile_nrows[tile]);
    const int row16 = lane & 15, g = lane >> 4;
    int kpf2 = -1;
    for (int k = 0; k < regs.n; ++k)
        if (regs.kind[k] == MCL_PEN_PARAFAC2) kpf2 = k;
    RowMat<NBR> D;
    if (kpf2 >= 0) D.load(regs.aux2[kpf2], r, lane);
    double nf = 0.0, na = 0.0, gap[MCL_MAX_REGS];
#pragma unroll
    for (int k = 0; k < MCL_MAX_REGS; ++k) gap[k] = 0.0;
#pragma unroll
    for (int rb = 0; rb < 4; ++rb) {
        if (16 * rb >= nrows) break;
        const bool ok = 16 * rb + row16 < nrows;
        const long j = row0 + 16 * rb + (ok ? row16 : 0);
        f32x4 f[NBR];
#pragma unroll
        for (int h = 0; h < NBR; ++h) {
            f[h] = row_ld4<VEC>(F, j, 16 * h + 4 * g, ok, r);
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                nf += (double)f[h][v] * (double)f[h][v];
                na += fabs((double)f[h][v]);
            }
        }
#pragma unroll
        for (int k = 0; k < MCL_MAX_REGS; ++k) {
            if (k < regs.n) {
                f32x4 z[NBR];
#pragma unroll
                for (int h = 0; h < NBR; ++h) z[h] = row_ld4<VEC>(regs.aux[k], j, 16 * h + 4 * g, ok, r);
                if (k == kpf2) {
                    f32x4 pz[NBR];
                    D.apply(z, pz);
#pragma unroll
                    for (int h = 0; h < NBR; ++h) z[h] = pz[h];
                }
#pragma unroll
                for (int h = 0; h < NBR; ++h)
#pragma unroll
                    for (int v = 0; v < 4; ++v) {
                        const double dlt = (double)z[h][v] - (double)f[h][v];  // padded / invalid entries are 0 - 0
                        gap[k] += dlt * dlt;
                    }
            }
        }
    }
    nf = wave_sum(nf);
    na = wave_sum(na);
#pragma unroll
    for (int k = 0; k < MCL_MAX_REGS; ++k) gap[k] = wave_sum(gap[k]);
    if (lane == 0) diag_row_store(diag_tile + (long)tile * DIAG_COLS, nf, na, gap);
}

// =========================================================================================================
// host launchers
// =========================================================================================================
int mcl_launch_rows_diag(mcl_context *c, int mode) {
    ProfScope prof_(c, MCL_PROF_DIAG);
    c->variant[MCL_PROF_DIAG] = "k_diag_final";
    const TileMap &tm = mcl_tiles(c, mode);
    if (tm.n_tiles == 0) return 0;
    const float *F = (mode == 1) ? c->B : (mode == 2 ? c->C : c->A);
    double *diag = mcl_diag_tile(c, mode);
    bool vec = (c->r % 4 == 0) && ((reinterpret_cast<uintptr_t>(F) & 15) == 0);
    for (int k = 0; k < c->regs[mode].n; ++k) vec = vec && ((reinterpret_cast<uintptr_t>(c->regs[mode].aux[k]) & 15) == 0);
    dim3 grid((unsigned)((tm.n_tiles + 3) / 4)), block(256);
#define MCL_RD(NBR_, VEC_)                                                                                       \
    hipLaunchKernelGGL((k_rows_diag<NBR_, VEC_>), grid, block, 0, c->stream, tm.row0, tm.nrows, tm.n_tiles, F,   \
                       c->regs[mode], c->r, diag)
    const int nbr = c->r <= 16 ? 1 : (c->r <= 32 ? 2 : 4);
    if (vec) {
        if (nbr == 1) MCL_RD(1, true);
        else if (nbr == 2) MCL_RD(2, true);
        else MCL_RD(4, true);
    } else {
        if (nbr == 1) MCL_RD(1, false);
        else if (nbr == 2) MCL_RD(2, false);
        else MCL_RD(4, false);
    }
#undef MCL_RD
    c->bp.diag_rows[mode] = tm.n_tiles;  // one row per tile
    MCL_CHECK_HIP(c, hipGetLastError());
    return 0;
}

int mcl_launch_x_sq(mcl_context *c) {
    ProfScope prof_(c, MCL_PROF_OTHER);
    const long n = (long)c->N * c->K;
    const int nb = 1024;
    mcl_x_dispatch(c->x_type, [&](auto xl) {
        using XL = decltype(xl);
        hipLaunchKernelGGL((MCL_XKERNEL0(k_sumsq_partial)), dim3(nb), dim3(256), 0, c->stream, mcl_x<XL>(c), n, c->xsq_part);
        return 0;
    });
    hipLaunchKernelGGL(k_sum_doubles, dim3(1), dim3(256), 0, c->stream, c->xsq_part, nb, c->x_sq);
    MCL_CHECK_HIP(c, hipGetLastError());
    return 0;
}

DiagTables mcl_diag_tables(const mcl_context *c, bool a_from_rows) {
    DiagTables T;
    T.tab[0] = a_from_rows ? c->diagA_row : c->diagA_tile;
    T.rows[0] = a_from_rows ? (int)c->I : c->tilesA.n_tiles;
    T.tab[1] = c->diagB_tile, T.rows[1] = c->bp.diag_rows[1];
    T.tab[2] = c->diagC_tile, T.rows[2] = c->bp.diag_rows[2];
    for (int m = 0; m < 3; ++m) T.nreg[m] = c->regs[m].n;
    T.e1 = c->e1, T.I = (int)c->I, T.xsq = c->x_sq;
    return T;
}

int mcl_launch_diag_tables(mcl_context *c, const DiagTables &T, double *out, int include_replicated) {
    ProfScope prof_(c, MCL_PROF_DIAG);
    c->variant[MCL_PROF_DIAG] = "k_diag_final";
    // long tables (thousands of B tiles: config 4 / 5) are summed by 1024 threads per column: a quarter of the dependent loads
    const int nt = std::max(T.rows[0], std::max(T.rows[1], T.rows[2])) > 2048 ? 1024 : 256;
    hipLaunchKernelGGL(k_diag_final, dim3(3 * DIAG_COLS + 3), dim3(nt), 0, c->stream, T, include_replicated, out);
    MCL_CHECK_HIP(c, hipGetLastError());
    return 0;
}

static StopRuleDev rule_dev(const mcl_context *c, const mcl_stop_rule *rule, int it) {
    StopRuleDev R{};
    R.tol = rule->tol, R.abs_tol = rule->absolute_tol, R.feas_tol = rule->feasibility_tol;
    R.has_tol = rule->tol != 0.0, R.has_feas = rule->feasibility_tol != 0.0;  // Python truthiness of the keyword values
    R.loss_always = rule->evaluate_loss_always != 0, R.it = it;
    for (int m = 0; m < 3; ++m) {
        R.l2[m] = c->opt.l2_penalty[m];
        for (int k = 0; k < MCL_MAX_REGS; ++k) R.w[m][k] = rule->penalty_weight[m][k];
    }
    return R;
}

int mcl_launch_verdict(mcl_context *c, const double *vec, const mcl_stop_rule *rule, int it, double *verdict_row,
                       int *status_dev) {
    ProfScope prof_(c, MCL_PROF_DIAG);
    hipLaunchKernelGGL(k_verdict, dim3(1), dim3(64), 0, c->stream, vec, rule_dev(c, rule, it), c->regs[0].n, c->regs[1].n,
                       c->regs[2].n, c->gate, c->stop_state, verdict_row, status_dev);
    MCL_CHECK_HIP(c, hipGetLastError());
    return 0;
}

int mcl_launch_diag_verdict(mcl_context *c, double *out, const mcl_stop_rule *rule, int it, double *verdict_row,
                            int *status_dev) {
    const StopRuleDev R = rule_dev(c, rule, it);
    const DiagTables T = mcl_diag_tables(c, true);
    const int nt = std::max(T.rows[0], std::max(T.rows[1], T.rows[2])) > 2048 ? 1024 : 256;
    ProfScope prof_(c, MCL_PROF_DIAG);
    c->variant[MCL_PROF_DIAG] = "k_diag_verdict";
    hipLaunchKernelGGL(k_diag_verdict, dim3(3 * DIAG_COLS + 3), dim3(nt), 0, c->stream, T, out, R,
                       c->gate, c->stop_state, verdict_row, status_dev);
    MCL_CHECK_HIP(c, hipGetLastError());
    return 0;
}

int mcl_launch_diag_final(mcl_context *c, double *out, int include_replicated, bool a_from_rows) {
    return mcl_launch_diag_tables(c, mcl_diag_tables(c, a_from_rows), out, include_replicated);
}
