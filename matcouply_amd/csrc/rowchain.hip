// The chained B-mode row pass of a fused penalty stack with its loads SOFTWARE-PIPELINED: k_rows_chain_first / _mid / _last are
// the pipelined forms of k_rows_solve_stats / k_rows_finish_solve_stats / k_rows_finish_fused (rows.hip).
//
// The arithmetic of a pass - column scale, right-hand side, prox and dual of every penalty class, the Gram and column-square
// statistics, the diagnostics - is the shared code of rows_stack.h, the same functions the kernels of rows.hip call: there is
// one definition of every operation, its order and its rounding.  What this file adds is the pipeline around it.
//
// The un-pipelined pass reads the rows of a 16-row block (factor, right-hand side, the dual of every penalty, the auxiliary rows
// the column regressions wrote: 12 x 16 B per lane at rank 32 with three penalties), waits for them, runs the block's ~50
// matrix-core instructions and stores - one block after the other, two waves per SIMD: while a wave computes nothing of its own
// is in flight, and config 5's pass moved 19.3 GB in 4.68 ms (0.52 of the HBM peak, 4.1 TB/s) where a streaming read reaches
// 6.3.  Here the loads of block rb + 1 are issued BEFORE block rb is computed.  For the hardware's in-order return counter to
// let the block's wait cover exactly its own loads (s_waitcnt vmcnt(N) with N = everything younger), the number of memory
// operations between two waits has to be a compile-time constant:
//   * the composition of the stack (how many penalties, which of them PARAFAC2 / unimodality / L2 ball) is a TEMPLATE
//     argument - the stacks of the BASELINE configurations are instantiated, every other stack keeps the kernel of rows.hip;
//     the class of penalty k reaches the shared code as the constant sig_cls(SIG, k), where rows.hip passes class_of(kind);
//   * loads are unconditional at clamped addresses into a Blk and masked at use, stores are unconditional with the lanes outside
//     the matrix writing to a per-lane sink;
//   * a block is entered only from its predecessor (unrolled loop with an early exit).
// MCL_NO_ROW_PREFETCH=1 selects the un-pipelined kernels for A/B runs.  tests/test_gpu_rowchain.py holds every instantiation
// below to them bit for bit - with the arithmetic shared, that leg guards the loads, masks and sink stores of the pipeline - and
// to the oracle at the stack, rank and tile edges (partial blocks, slabs shorter than a block, padded column groups, shared sink
// slots), with the case table in tests/kernel_edge_cases.py.
#include "rows_stack.h"

namespace {

// SIG = n | cls_0 << 3 | cls_1 << 5 | cls_2 << 7 | cls_3 << 9
constexpr int sig_n(int sig) { return sig & 7; }
constexpr int sig_cls(int sig, int k) { return (sig >> (3 + 2 * k)) & 3; }
constexpr int sig_last(int sig, int cls) {
    int found = -1;
    for (int k = 0; k < sig_n(sig); ++k)
        if (sig_cls(sig, k) == cls) found = k;
    return found;
}
constexpr int make_sig(int n, int c0, int c1 = 0, int c2 = 0, int c3 = 0) { return n | c0 << 3 | c1 << 5 | c2 << 7 | c3 << 9; }

// The lane's part of the pipeline: the column of its 16-B access per column block, clamped into the matrix for the loads
// (r % 4 == 0, r >= 4), and its slot of the sink
#define CHAIN_LANE_COLUMNS()                                                                                  \
    int colc[NBR];                                                                                            \
    bool colok[NBR];                                                                                          \
    _Pragma("unroll") for (int h = 0; h < NBR; ++h) colok[h] = 16 * h + 4 * g < r, colc[h] = min(16 * h + 4 * g, r - 4); \
    float *sink = sink_base + (((tile & 63) * 64 + lane) << 2);                                               \
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f}

template <int NBR, bool R64, int SIG>
__global__ __launch_bounds__(256) void k_rows_chain_mid(ModeView mv, const float *__restrict__ rhs_src, const float *__restrict__ Arows,
                                                        const float *__restrict__ Linv, RegSet regs, int r,
                                                        const float *__restrict__ T, const double *__restrict__ colsq,
                                                        double *__restrict__ stat_gram, double *__restrict__ stat_colsq,
                                                        const double *__restrict__ Linv64, const double *__restrict__ T64,
                                                        float *__restrict__ sink_base) {
    typedef RowArith<R64> RA;
    constexpr int N = sig_n(SIG);
    constexpr int kpf2 = sig_last(SIG, CLS_PF2), kl2 = sig_last(SIG, CLS_L2);
    __shared__ double ytile[YGram<NBR, R64>::LDS_DOUBLES];
    ROW_TILE_PROLOGUE();
    const float rho = mv.rho[slab];
    typename RA::template Mat<NBR> L, Ts, D;
    load_slab_mat<R64>(L, Linv, Linv64, slab, r, lane);
    if constexpr (kpf2 >= 0) {
        load_slab_mat<R64>(Ts, T, T64, slab, r, lane);
        D.load(regs.aux2[kpf2], r, lane);
    }
    float av[NBR][4], l2s[NBR][4];
    a_col_scale(Arows, slab, r, g, av);
    l2_ball_scales(regs, kl2, colsq, mv.n_slabs, slab, r, g, l2s);
    YGram<NBR, R64> gram;
    gram.clear(row16, g);
    ColSq<NBR> csq;
    csq.clear();
    CHAIN_LANE_COLUMNS();

    struct Blk {
        f32x4 f[NBR], t[NBR], u[N > 0 ? N : 1][NBR], zu[N > 0 ? N : 1][NBR];
    };
    auto load_blk = [&](int rb, Blk &b) {
        const long j = row0 + min(16 * rb + row16, nrows - 1);
#pragma unroll
        for (int h = 0; h < NBR; ++h) {
            b.f[h] = *reinterpret_cast<const f32x4 *>(mv.F + j * r + colc[h]);
            b.t[h] = *reinterpret_cast<const f32x4 *>(rhs_src + j * r + colc[h]);
        }
#pragma unroll
        for (int k = 0; k < N; ++k)
#pragma unroll
            for (int h = 0; h < NBR; ++h) {
                b.u[k][h] = *reinterpret_cast<const f32x4 *>(regs.dual[k] + j * r + colc[h]);
                if (sig_cls(SIG, k) == CLS_UNI) b.zu[k][h] = *reinterpret_cast<const f32x4 *>(regs.aux[k] + j * r + colc[h]);
            }
    };

    Blk cur;
    load_blk(0, cur);
#pragma unroll
    for (int rb = 0; rb < 4; ++rb) {
        if (16 * rb >= nrows) break;  // (wave-uniform; a block is only entered from its predecessor)
        Blk nxt;
        load_blk((16 * (rb + 1) < nrows) ? rb + 1 : rb, nxt);  // the last block re-requests its own rows (cache hits): a fixed count
        __builtin_amdgcn_sched_barrier(0);
        const bool ok = 16 * rb + row16 < nrows;
        const long j = row0 + 16 * rb + (ok ? row16 : 0);
        f32x4 f[NBR], t[NBR], upf[NBR], ul2[NBR];  // new duals of the PARAFAC2 / L2-ball penalty (statistics below)
#pragma unroll
        for (int h = 0; h < NBR; ++h) {
            const bool m = ok && colok[h];
            f[h] = m ? cur.f[h] : zero;  // zeros for padding rows / columns, as row_ld4 returns them
            t[h] = m ? cur.t[h] : zero;
#pragma unroll
            for (int v = 0; v < 4; ++v) t[h][v] *= av[h][v];
        }
        // ---- iteration t: prox + dual of every penalty
#pragma unroll
        for (int k = 0; k < N; ++k) {
            f32x4 u[NBR], z[NBR], zg[NBR];
#pragma unroll
            for (int h = 0; h < NBR; ++h) u[h] = (ok && colok[h]) ? cur.u[k][h] : zero;
            const auto aux_rows = [&](int h) ROWS_INLINE { return (ok && colok[h]) ? cur.zu[k][h] : zero; };
            const auto l2_scale = [&](int h, int v) ROWS_INLINE { return l2s[h][v]; };
            stack_prox<RA, NBR>(sig_cls(SIG, k), regs, k, rho, Ts, D, f, u, aux_rows, l2_scale, z, zg);
            dual_step(f, zg, u);
            rhs_add(rho, zg, u, t);
#pragma unroll
            for (int h = 0; h < NBR; ++h) {
                float *dst = (ok && colok[h]) ? regs.dual[k] + j * r + 16 * h + 4 * g : sink;
                *reinterpret_cast<f32x4 *>(dst) = u[h];
                if (k == kpf2) upf[h] = u[h];
                if (k == kl2) ul2[h] = u[h];
            }
        }
        // ---- iteration t + 1: solve, store, statistics of the new rows
        f32x4 fn[NBR];
        L.apply(t, fn);
#pragma unroll
        for (int h = 0; h < NBR; ++h) {
            float *dst = (ok && colok[h]) ? mv.F + j * r + 16 * h + 4 * g : sink;
            *reinterpret_cast<f32x4 *>(dst) = fn[h];
        }
        if constexpr (kl2 >= 0) csq.add(fn, ul2, regs.nonneg[kl2], ok);
        if constexpr (kpf2 >= 0) gram.add(fn, upf, ok, ytile, row16, g);
        cur = nxt;
    }
    if constexpr (kpf2 >= 0) gram.store(stat_gram, tile, row16, g);
    if constexpr (kl2 >= 0) csq.reduce_store(stat_colsq, tile, kl2, r, row16, g);
}

// ---------------------------------------------------------------------------------------------------------
// The FIRST pass of the chain (pipelined k_rows_solve_stats): solve of inner iteration 0 from the aux / dual rows the phase
// starts with + the statistics of the new rows.  Same pipeline as above; every L2 ball of the stack has its column sums here.
// ---------------------------------------------------------------------------------------------------------
template <int NBR, bool R64, int SIG>
__global__ __launch_bounds__(256) void k_rows_chain_first(ModeView mv, const float *__restrict__ rhs_src, const float *__restrict__ Arows,
                                                          const float *__restrict__ Linv, RegSet regs, int r,
                                                          double *__restrict__ stat_gram, double *__restrict__ stat_colsq,
                                                          const double *__restrict__ Linv64, float *__restrict__ sink_base) {
    typedef RowArith<R64> RA;
    constexpr int N = sig_n(SIG);
    constexpr int kpf2 = sig_last(SIG, CLS_PF2);
    __shared__ double ytile[YGram<NBR, R64>::LDS_DOUBLES];
    ROW_TILE_PROLOGUE();
    const float rho = mv.rho[slab];
    typename RA::template Mat<NBR> L, D;
    load_slab_mat<R64>(L, Linv, Linv64, slab, r, lane);
    if constexpr (kpf2 >= 0) D.load(regs.aux2[kpf2], r, lane);
    float av[NBR][4];
    a_col_scale(Arows, slab, r, g, av);
    YGram<NBR, R64> gram;
    gram.clear(row16, g);
    ColSq<NBR> csq[N > 0 ? N : 1];
#pragma unroll
    for (int k = 0; k < N; ++k) csq[k].clear();
    CHAIN_LANE_COLUMNS();

    struct Blk {
        f32x4 t[NBR], z[N > 0 ? N : 1][NBR], u[N > 0 ? N : 1][NBR];
    };
    auto load_blk = [&](int rb, Blk &b) {
        const long j = row0 + min(16 * rb + row16, nrows - 1);
#pragma unroll
        for (int h = 0; h < NBR; ++h) b.t[h] = *reinterpret_cast<const f32x4 *>(rhs_src + j * r + colc[h]);
#pragma unroll
        for (int k = 0; k < N; ++k)
#pragma unroll
            for (int h = 0; h < NBR; ++h) {
                b.z[k][h] = *reinterpret_cast<const f32x4 *>(regs.aux[k] + j * r + colc[h]);
                b.u[k][h] = *reinterpret_cast<const f32x4 *>(regs.dual[k] + j * r + colc[h]);
            }
    };
    Blk cur;
    load_blk(0, cur);
#pragma unroll
    for (int rb = 0; rb < 4; ++rb) {
        if (16 * rb >= nrows) break;
        Blk nxt;
        load_blk((16 * (rb + 1) < nrows) ? rb + 1 : rb, nxt);
        __builtin_amdgcn_sched_barrier(0);
        const bool ok = 16 * rb + row16 < nrows;
        const long j = row0 + 16 * rb + (ok ? row16 : 0);
        f32x4 t[NBR], f[NBR], ukeep[N > 0 ? N : 1][NBR];
#pragma unroll
        for (int h = 0; h < NBR; ++h) {
            t[h] = (ok && colok[h]) ? cur.t[h] : zero;
#pragma unroll
            for (int v = 0; v < 4; ++v) t[h][v] *= av[h][v];
        }
#pragma unroll
        for (int k = 0; k < N; ++k) {
            f32x4 z[NBR];
#pragma unroll
            for (int h = 0; h < NBR; ++h) z[h] = (ok && colok[h]) ? cur.z[k][h] : zero;
            if (k == kpf2) times_delta(D, z);
#pragma unroll
            for (int h = 0; h < NBR; ++h) ukeep[k][h] = (ok && colok[h]) ? cur.u[k][h] : zero;
            rhs_add(rho, z, ukeep[k], t);
        }
        L.apply(t, f);
#pragma unroll
        for (int h = 0; h < NBR; ++h) {
            float *dst = (ok && colok[h]) ? mv.F + j * r + 16 * h + 4 * g : sink;
            *reinterpret_cast<f32x4 *>(dst) = f[h];
        }
#pragma unroll
        for (int k = 0; k < N; ++k) {
            if (sig_cls(SIG, k) == CLS_L2) csq[k].add(f, ukeep[k], regs.nonneg[k], ok);
            else if (k == kpf2) gram.add(f, ukeep[k], ok, ytile, row16, g);
        }
        cur = nxt;
    }
    if constexpr (kpf2 >= 0) gram.store(stat_gram, tile, row16, g);
#pragma unroll
    for (int k = 0; k < N; ++k)
        if (sig_cls(SIG, k) == CLS_L2) csq[k].reduce_store(stat_colsq, tile, k, r, row16, g);
}

// ---------------------------------------------------------------------------------------------------------
// The LAST pass of the chain (pipelined k_rows_finish_fused): prox + dual of the last inner iteration, the auxiliary rows
// written out, the mode's per-tile diagnostics.
// ---------------------------------------------------------------------------------------------------------
template <int NBR, bool R64, int SIG>
__global__ __launch_bounds__(256) void k_rows_chain_last(ModeView mv, RegSet regs, int r, const float *__restrict__ T,
                                                         const double *__restrict__ colsq, double *__restrict__ diag_tile,
                                                         int want_diag, const double *__restrict__ T64, float *__restrict__ sink_base) {
    typedef RowArith<R64> RA;
    constexpr int N = sig_n(SIG);
    constexpr int kpf2 = sig_last(SIG, CLS_PF2);
    ROW_TILE_PROLOGUE();
    TileDiag diag;
    diag.clear();
    const float rho = mv.rho[slab];
    typename RA::template Mat<NBR> Ts, D;
    if constexpr (kpf2 >= 0) {
        load_slab_mat<R64>(Ts, T, T64, slab, r, lane);
        D.load(regs.aux2[kpf2], r, lane);
    }
    float l2s[N > 0 ? N : 1][NBR][4];
#pragma unroll
    for (int k = 0; k < N; ++k) l2_ball_scales(regs, sig_cls(SIG, k) == CLS_L2 ? k : -1, colsq, mv.n_slabs, slab, r, g, l2s[k]);
    CHAIN_LANE_COLUMNS();

    struct Blk {
        f32x4 f[NBR], u[N > 0 ? N : 1][NBR], zu[N > 0 ? N : 1][NBR];
    };
    auto load_blk = [&](int rb, Blk &b) {
        const long j = row0 + min(16 * rb + row16, nrows - 1);
#pragma unroll
        for (int h = 0; h < NBR; ++h) b.f[h] = *reinterpret_cast<const f32x4 *>(mv.F + j * r + colc[h]);
#pragma unroll
        for (int k = 0; k < N; ++k)
#pragma unroll
            for (int h = 0; h < NBR; ++h) {
                b.u[k][h] = *reinterpret_cast<const f32x4 *>(regs.dual[k] + j * r + colc[h]);
                if (sig_cls(SIG, k) == CLS_UNI) b.zu[k][h] = *reinterpret_cast<const f32x4 *>(regs.aux[k] + j * r + colc[h]);
            }
    };
    Blk cur;
    load_blk(0, cur);
#pragma unroll
    for (int rb = 0; rb < 4; ++rb) {
        if (16 * rb >= nrows) break;
        Blk nxt;
        load_blk((16 * (rb + 1) < nrows) ? rb + 1 : rb, nxt);
        __builtin_amdgcn_sched_barrier(0);
        const bool ok = 16 * rb + row16 < nrows;
        const long j = row0 + 16 * rb + (ok ? row16 : 0);
        f32x4 f[NBR];
#pragma unroll
        for (int h = 0; h < NBR; ++h) f[h] = (ok && colok[h]) ? cur.f[h] : zero;
        if (want_diag) diag.add_f(f);
#pragma unroll
        for (int k = 0; k < N; ++k) {
            f32x4 u[NBR], z[NBR], zg[NBR];
#pragma unroll
            for (int h = 0; h < NBR; ++h) u[h] = (ok && colok[h]) ? cur.u[k][h] : zero;
            const auto aux_rows = [&](int h) ROWS_INLINE { return (ok && colok[h]) ? cur.zu[k][h] : zero; };
            const auto l2_scale = [&](int h, int v) ROWS_INLINE { return l2s[k][h][v]; };
            stack_prox<RA, NBR>(sig_cls(SIG, k), regs, k, rho, Ts, D, f, u, aux_rows, l2_scale, z, zg);
            dual_step(f, zg, u);
#pragma unroll
            for (int h = 0; h < NBR; ++h) {
                const bool m = ok && colok[h];
                if (sig_cls(SIG, k) != CLS_UNI) *reinterpret_cast<f32x4 *>(m ? regs.aux[k] + j * r + 16 * h + 4 * g : sink) = z[h];
                *reinterpret_cast<f32x4 *>(m ? regs.dual[k] + j * r + 16 * h + 4 * g : sink) = u[h];
            }
            if (want_diag) diag.add_gap(k, zg, f, ok, r, g);
        }
        cur = nxt;
    }
    if (want_diag) diag.store(diag_tile, tile, lane);
}

}  // namespace

// 0 when the stack / shape of mode 1 is not covered by the software-pipelined kernels, else the signature of its stack
static int chain_signature(const mcl_context *c, bool vec) {
    if (!vec || c->sw.no_row_prefetch || c->row_sink == nullptr || c->r < 4 || c->NB > 2) return 0;
    const RegSet &rs = c->regs[1];
    if (rs.n < 1 || rs.n > 3) return 0;
    int sig = rs.n;
    for (int k = 0; k < rs.n; ++k) {
        if (rs.kind[k] == MCL_PEN_EXTERNAL || rs.kind[k] == MCL_PEN_TV || rs.kind[k] == MCL_PEN_GL2 || rs.kind[k] == MCL_PEN_SIMPLEX) return 0;
        sig |= class_of(rs.kind[k]) << (3 + 2 * k);
    }
    // BASELINE config 4: PARAFAC2 + L2 ball; config 5: PARAFAC2 + unimodality + L2 ball; config 1 / the README's model family:
    // PARAFAC2 + a row-separable kind
    if (sig == make_sig(2, CLS_PF2, CLS_L2) || sig == make_sig(3, CLS_PF2, CLS_UNI, CLS_L2) || sig == make_sig(2, CLS_PF2, CLS_ROWSEP)) return sig;
    return 0;
}

#define MCL_RC_DISPATCH(LAUNCH)                                             \
    do {                                                                    \
        if (sig == make_sig(2, CLS_PF2, CLS_L2)) {                          \
            if (rows64) LAUNCH(1, true, make_sig(2, CLS_PF2, CLS_L2));      \
            else if (c->NB == 1) LAUNCH(1, false, make_sig(2, CLS_PF2, CLS_L2)); \
            else LAUNCH(2, false, make_sig(2, CLS_PF2, CLS_L2));            \
        } else if (sig == make_sig(3, CLS_PF2, CLS_UNI, CLS_L2)) {          \
            if (rows64) LAUNCH(1, true, make_sig(3, CLS_PF2, CLS_UNI, CLS_L2)); \
            else if (c->NB == 1) LAUNCH(1, false, make_sig(3, CLS_PF2, CLS_UNI, CLS_L2)); \
            else LAUNCH(2, false, make_sig(3, CLS_PF2, CLS_UNI, CLS_L2));   \
        } else {                                                            \
            if (rows64) LAUNCH(1, true, make_sig(2, CLS_PF2, CLS_ROWSEP));  \
            else if (c->NB == 1) LAUNCH(1, false, make_sig(2, CLS_PF2, CLS_ROWSEP)); \
            else LAUNCH(2, false, make_sig(2, CLS_PF2, CLS_ROWSEP));        \
        }                                                                   \
    } while (0)

// The software-pipelined forms of the three kernels of the chained B row pass.  Each returns 1 when it has launched, 0 when the
// stack / shape is not covered (the caller launches the kernel of rows.hip).
int mcl_try_rows_chain_mid(mcl_context *c, const ModeView &mv, const float *rhs, bool vec, bool rows64) {
    const int sig = chain_signature(c, vec);
    if (!sig) return 0;
    const RegSet &rs = c->regs[1];
    const dim3 grid((unsigned)((mv.n_tiles + 3) / 4)), block(256);
#define MCL_RC_MID(NBR_, R64_, SIG_)                                                                                      \
    hipLaunchKernelGGL((k_rows_chain_mid<NBR_, R64_, SIG_>), grid, block, 0, c->stream, mv, rhs, (const float *)c->A,      \
                       (const float *)c->LinvB, rs, c->r, (const float *)c->pf2_T, (const double *)c->colsq, c->stat_gram, \
                       c->stat_colsq, (const double *)c->LinvB64, (const double *)c->pf2_T64, c->row_sink)
    MCL_RC_DISPATCH(MCL_RC_MID);
#undef MCL_RC_MID
    return 1;
}

int mcl_try_rows_chain_first(mcl_context *c, const ModeView &mv, const float *rhs, bool vec, bool rows64) {
    const int sig = chain_signature(c, vec);
    if (!sig) return 0;
    const RegSet &rs = c->regs[1];
    const dim3 grid((unsigned)((mv.n_tiles + 3) / 4)), block(256);
#define MCL_RC_FIRST(NBR_, R64_, SIG_)                                                                                    \
    hipLaunchKernelGGL((k_rows_chain_first<NBR_, R64_, SIG_>), grid, block, 0, c->stream, mv, rhs, (const float *)c->A,    \
                       (const float *)c->LinvB, rs, c->r, c->stat_gram, c->stat_colsq, (const double *)c->LinvB64, c->row_sink)
    MCL_RC_DISPATCH(MCL_RC_FIRST);
#undef MCL_RC_FIRST
    return 1;
}

int mcl_try_rows_chain_last(mcl_context *c, const ModeView &mv, bool vec, bool rows64, double *diag, int want_diag) {
    const int sig = chain_signature(c, vec);
    if (!sig) return 0;
    const RegSet &rs = c->regs[1];
    const dim3 grid((unsigned)((mv.n_tiles + 3) / 4)), block(256);
#define MCL_RC_LAST(NBR_, R64_, SIG_)                                                                                     \
    hipLaunchKernelGGL((k_rows_chain_last<NBR_, R64_, SIG_>), grid, block, 0, c->stream, mv, rs, c->r, (const float *)c->pf2_T, \
                       (const double *)c->colsq, diag, want_diag, (const double *)(rows64 ? c->pf2_T64 : nullptr), c->row_sink)
    MCL_RC_DISPATCH(MCL_RC_LAST);
#undef MCL_RC_LAST
    return 1;
}
