// Register Gauss-Jordan inverse of the SPD r x r systems of the three ADMM phases (fp64, gfx950), in its two layouts, and
// the lane helpers it and its callers (admm.hip, afinish.h) share beyond those of rows_mfma.h.
#pragma once
#include <type_traits>
#include <utility>

#include "rows_mfma.h"

static __device__ __forceinline__ float readlane_f32(float v, int lane) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}

static __device__ __forceinline__ double bperm_f64(int src_lane, double v) {
    const int lo = __builtin_amdgcn_ds_bpermute(src_lane << 2, __double2loint(v));
    const int hi = __builtin_amdgcn_ds_bpermute(src_lane << 2, __double2hiint(v));
    return __hiloint2double(hi, lo);
}

static __device__ __forceinline__ float bperm_f32(int src_lane, float v) {
    return __int_as_float(__builtin_amdgcn_ds_bpermute(src_lane << 2, __float_as_int(v)));
}

template <class F, int... Ps>
static __device__ __forceinline__ void static_for_seq(F &&f, std::integer_sequence<int, Ps...>) {
    (f(std::integral_constant<int, Ps>{}), ...);
}

// 1 / x by v_rcp_f64 + two Newton steps (full double precision for the positive pivots of an SPD system; the IEEE
// division sequence is a third of an elimination step's latency)
static __device__ __forceinline__ double rcp_newton2(double x) {
    double y = __builtin_amdgcn_rcp(x);
    y = fma(fma(-x, y, 1.0), y, y);
    y = fma(fma(-x, y, 1.0), y, y);
    return y;
}

// The feasibility penalty of a system from its trace: rho = 1/2 tr * scale (decomposition.py:243-249), rounded to the fp32
// the reference keeps it in.
static __device__ __forceinline__ float rho_of_trace(double tr, float scale) { return (float)(0.5 * tr * scale); }

// Gauss-Jordan inverse of an SPD r x r matrix held ONE COLUMN PER LANE in registers (fp64): lane c (< r) owns
// col[i] = M[i][c]; lanes >= r and rows >= r hold identity padding.  Pivot column entries are fetched with
// v_readlane (compile-time lane index), so there is no LDS traffic and no barrier.  SPD => no pivoting.
// Replaces the reference's SVD-based solve `(v (U/s)) Uh` (decomposition.py:172,194) - identical for SPD systems.
template <int RP>
static __device__ __forceinline__ void gj_inverse_reg(double (&col)[RP], int r, int lane) {
#pragma unroll
    for (int p = 0; p < RP; ++p) {
        if (p < r) {
            double cp[RP];
#pragma unroll
            for (int i = 0; i < RP; ++i) cp[i] = readlane_f64_u(col[i], p);  // M[i][p]
            const double piv = rcp_newton2(cp[p]);
            const double myp = (lane == p) ? piv : col[p] * piv;  // scaled pivot-row entry of this column
#pragma unroll
            for (int i = 0; i < RP; ++i) {
                if (i != p) col[i] = (lane == p) ? -cp[i] * piv : col[i] - cp[i] * myp;
            }
            col[p] = myp;
        }
    }
}

// The same Gauss-Jordan with the ROWS of every column split over G = 64 / RP lane groups (RP = 16: 4 groups x 4 rows),
// so that all 64 lanes work instead of RP: lane l = g * RP + c holds col[j] = M[g * RL + j][c], j < RL = RP / G.
// Per pivot p the step needs M[i][p] for the lane's own rows (from lane g * RP + p: ds_bpermute, no LDS memory), the
// pivot-row entry M[p][c] (from lane pg * RP + c) and the pivot itself (v_readlane, uniform): 2 (RL + 1) permutes and
// RL updates instead of 2 RP readlanes and RP updates - about 4x shorter for RP = 16.
template <int RP>
struct GJRows {
    static constexpr int G = (64 / RP < RP) ? 64 / RP : RP;  // lane groups
    static constexpr int RL = RP / G;                        // rows per lane
    static constexpr int LANES = RP * G;
};

template <int RP>
static __device__ __forceinline__ void gj_inverse_rows(double (&col)[GJRows<RP>::RL], int r, int lane) {
    constexpr int RL = GJRows<RP>::RL;
    const int c = lane % RP, g = lane / RP;
    if constexpr (RP == 16) {
        // a lane group is exactly one DPP row of 16 lanes: M[i][p] of the lane's own rows is lane p of its row, which
        // row_newbcast delivers as an operand modifier of a v_mov (a few cycles) - the ds_bpermute round trips through the
        // LDS crossbar (8 of the 10 per pivot) were on the dependent chain of every elimination step
        static_for_seq(
            [&](auto P) {
                constexpr int p = decltype(P)::value;
                if (p < r) {  // wave-uniform
                    constexpr int pg = p / RL, pj = p % RL;
                    const double pivot = readlane_f64_u(col[pj], pg * RP + p);
                    double cp[RL];
#pragma unroll
                    for (int j = 0; j < RL; ++j) cp[j] = dpp_mov_f64<0x150 + p>(col[j]);  // M[g RL + j][p]
                    const double prow = bperm_f64(pg * RP + c, col[pj]);                  // M[p][c]
                    const double piv = rcp_newton2(pivot);
                    const double myp = (c == p) ? piv : prow * piv;
                    // column p itself becomes -M[i][p] piv = fma(-M[i][p], piv, 0): one select on the addend instead of
                    // two products and a select on the result (the elimination is bound by instruction issue)
#pragma unroll
                    for (int j = 0; j < RL; ++j) {
                        const double upd = fma(-cp[j], myp, (c == p) ? 0.0 : col[j]);
                        col[j] = (j == pj && g == pg) ? myp : upd;
                    }
                }
            },
            std::make_integer_sequence<int, 16>{});
        return;
    }
#pragma unroll
    for (int p = 0; p < RP; ++p) {
        if (p < r) {  // wave-uniform
            const int pg = p / RL, pj = p % RL;
            const double pivot = readlane_f64_u(col[pj], pg * RP + p);
            double cp[RL];
#pragma unroll
            for (int j = 0; j < RL; ++j) cp[j] = bperm_f64(g * RP + p, col[j]);  // M[g RL + j][p]
            const double prow = bperm_f64(pg * RP + c, col[pj]);                  // M[p][c]
            const double piv = rcp_newton2(pivot);
            const double myp = (c == p) ? piv : prow * piv;
#pragma unroll
            for (int j = 0; j < RL; ++j) {
                const bool is_p = (g == pg) && (j == pj);
                const double upd = (c == p) ? -cp[j] * piv : col[j] - cp[j] * myp;
                col[j] = is_p ? myp : upd;
            }
        }
    }
}
