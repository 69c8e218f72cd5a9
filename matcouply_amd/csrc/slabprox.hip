// The proxes of the rarer penalties that couple the rows of a slab, one kernel per step of the un-fused inner loop:
//   L2Ball                penalties.py:920-925    column norms over the rows of one slab
//   TotalVariation        penalties.py:750-841    per-column taut string (+ soft threshold)
//   GeneralizedL2Penalty  penalties.py:595-747    U (S + rho/2 I)^-1 U^T (rho/2) Y per slab
//   UnitSimplex           penalties.py:928-980    per-column projection onto the simplex
// The dispatcher of rows.hip (mcl_launch_generic_prox_local) calls one launcher per kind; wide.hip launches the GeneralizedL2
// and simplex kernels a second time on its fp64 state.
#include "rows_launch.h"

// ---------------------------------------------------------------------------------------------------------
// L2 ball: column sums of squares per slab (fp64), then scale + dual
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_slab_colsq(const int *__restrict__ ext, const float *__restrict__ F,
                                                    const float *__restrict__ U, int nonneg, int r, int RP,
                                                    double *__restrict__ colsq) {
    __shared__ double sm[256];
    const int slab = blockIdx.x;
    const int s = ext[slab], e = ext[slab + 1];
    const int col = threadIdx.x % RP, rl = threadIdx.x / RP, nrl = 256 / RP;
    double acc = 0.0;
    if (col < r) {
        for (long j = (long)s + rl; j < e; j += nrl) {
            float y = F[j * r + col] + U[j * r + col];
            if (nonneg) y = fmaxf(y, 0.f);
            acc += (double)y * (double)y;
        }
    }
    sm[threadIdx.x] = acc;
    __syncthreads();
    if ((int)threadIdx.x < RP && col < r) {
        double t = 0.0;
        for (int q = 0; q < nrl; ++q) t += sm[q * RP + col];
        colsq[(long)slab * r + col] = t;
    }
}

template <int NBR, bool VEC>
__global__ __launch_bounds__(256) void k_rows_l2ball(ModeView mv, RegSet regs, int k, int r,
                                                     const double *__restrict__ colsq) {
    ROW_TILE_PROLOGUE();
    const float bound = regs.p0[k];
    float scale[NBR][4];
#pragma unroll
    for (int h = 0; h < NBR; ++h)
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const int col = 16 * h + 4 * g + v;
            const float nrm = (col < r) ? (float)sqrt(colsq[(long)slab * r + col]) : 1.f;
            scale[h][v] = bound / fmaxf(nrm, bound);
        }
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
                float y = f[v] + u[v];
                if (regs.nonneg[k]) y = fmaxf(y, 0.f);
                z[v] = y * scale[h][v];
                u[v] = f[v] - (z[v] - u[v]);
            }
            row_st4<VEC>(regs.aux[k], j, col, ok, r, z);
            row_st4<VEC>(regs.dual[k], j, col, ok, r, u);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------
// Total variation (penalties.py:750-841): per column of a slab, aux = argmin 1/2 ||y - (F + U)||^2 + lam sum |y_n - y_{n-1}|
// with lam = 2 alpha / rho, then the L1 soft threshold with l1 / rho.  The reference calls condat_tv (GPL); this is
// L. Condat's direct algorithm (IEEE SPL 20(11), 2013) restated from the paper: one pass with occasional restarts at
// the last position where a bound was active; fp64 like the unimodal regression (its decisions are discontinuous).
// One lane per (slab, column): the r lanes of a slab read / write consecutive addresses.
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_slab_tv(const int *__restrict__ ext, int n_slabs, const float *__restrict__ F,
                                                const float *__restrict__ rho_arr, RegSet regs, int kreg, int r) {
    MCL_GATE(regs.gate);
    const long t = (long)blockIdx.x * 64 + threadIdx.x;
    if (t >= (long)n_slabs * r) return;
    const int slab = (int)(t / r), col = (int)(t - (long)slab * r);
    const long s = ext[slab];
    const int n = ext[slab + 1] - ext[slab];
    if (n <= 0) return;
    const float *U = regs.dual[kreg];
    float *Z = regs.aux[kreg];
    const double rho = (double)rho_arr[slab];
    const double lam = 2.0 * (double)regs.p0[kreg] / rho;
    const float l1 = (float)((double)regs.p1[kreg] / rho);
    auto in = [&](int k) -> double { return (double)(F[(s + k) * r + col] + U[(s + k) * r + col]); };
    auto emit = [&](int a, int b, double v) {  // y[a..b] = v, then soft threshold
        float z = (float)v;
        if (l1 > 0.f) z = copysignf(fmaxf(fabsf(z) - l1, 0.f), z);
        for (int k = a; k <= b; ++k) Z[(s + k) * r + col] = z;
    };
    int k = 0, k0 = 0, km = 0, kp = 0;
    double x0 = in(0);
    double vmin = x0 - lam, vmax = x0 + lam, umin = lam, umax = -lam;
    for (;;) {
        if (k == n - 1) {
            if (umin < 0.0) {
                emit(k0, km, vmin);
                k0 = km + 1;
                k = km = k0;
                vmin = in(k);
                umin = lam;
                umax = vmin + lam - vmax;
            } else if (umax > 0.0) {
                emit(k0, kp, vmax);
                k0 = kp + 1;
                k = kp = k0;
                vmax = in(k);
                umax = -lam;
                umin = vmax - lam - vmin;
            } else {
                vmin += umin / (double)(k - k0 + 1);
                emit(k0, k, vmin);
                return;
            }
        } else {
            const double xn = in(k + 1);
            umin += xn - vmin;
            umax += xn - vmax;
            if (umin < -lam) {
                emit(k0, km, vmin);
                k0 = km + 1;
                k = km = kp = k0;
                vmin = in(k);
                vmax = vmin + 2.0 * lam;
                umin = lam, umax = -lam;
            } else if (umax > lam) {
                emit(k0, kp, vmax);
                k0 = kp + 1;
                k = km = kp = k0;
                vmax = in(k);
                vmin = vmax - 2.0 * lam;
                umin = lam, umax = -lam;
            } else {
                ++k;
                if (umin >= lam) {
                    km = k;
                    vmin += (umin - lam) / (double)(km - k0 + 1);
                    umin = lam;
                }
                if (umax <= -lam) {
                    kp = k;
                    vmax += (umax + lam) / (double)(kp - k0 + 1);
                    umax = -lam;
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------
// GeneralizedL2Penalty (penalties.py:595-747): prox(Y) = U (S + rho/2 I)^-1 U^T (rho/2) Y with M = U S U^T, per slab.
// Two passes of ONE routine  out[a][c] = sum_b Mat[b][a] In[b][c]  (Mat = U for the projection onto the eigenvectors, Mat = U^T
// for the way back: both walk Mat along its rows, coalesced), fp64 accumulation in the order of b.  Workgroup = 64 values of
// `a` x 4 column phases; the rows of In are staged through LDS 16 at a time.  T: fp64 scratch [rows, r].
// TIN = float (the caller's buffers) or double (the fp64 state of wide.hip).
// ---------------------------------------------------------------------------------------------------------
template <typename TIN, bool BACK>
__global__ __launch_bounds__(256) void k_gl2_pass(const int *__restrict__ ext, const double *__restrict__ Mat,
                                                  const double *__restrict__ eig, int n, int r, const float *__restrict__ rho_arr,
                                                  const TIN *__restrict__ F, const TIN *__restrict__ D, double *__restrict__ T,
                                                  float *__restrict__ Z32, float *__restrict__ D32, double *__restrict__ Z64,
                                                  double *__restrict__ D64, const int *__restrict__ gate) {
    // !BACK: T[e][c] = (rho / 2) sum_j U[j][e] (F + D)[j][c]        (D = nullptr: F alone, unscaled - the penalty value)
    //  BACK: Z[j][c] = sum_e U^T[e][j] T[e][c] / (s_e + rho / 2), then the dual step D = F - (Z - D)
    MCL_GATE(gate);
    __shared__ double ins[16][64];
    // (the slab index is folded into blockIdx.x: gridDim.y stops at 65535, a GeneralizedL2 penalty on the B_i may see more matrices)
    const int tps = (n + 63) >> 6;
    const int slab = (int)(blockIdx.x / (unsigned)tps);
    const long s0 = ext[slab];
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int a = (int)(blockIdx.x - (unsigned)slab * (unsigned)tps) * 64 + tx;
    const double half_rho = 0.5 * (double)rho_arr[slab];
    double acc[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[q] = 0.0;
    for (int b0 = 0; b0 < n; b0 += 16) {
        const int nb = min(16, n - b0);
        __syncthreads();
        for (int e = threadIdx.x; e < nb * r; e += 256) {
            const int bb = e / r, c = e - bb * r;
            const long idx = (s0 + b0 + bb) * r + c;
            double v;
            if (BACK) v = T[idx] / (eig[b0 + bb] + half_rho);
            else v = (double)F[idx] + (D != nullptr ? (double)D[idx] : 0.0);
            ins[bb][c] = v;
        }
        __syncthreads();
        if (a < n)
            for (int bb = 0; bb < nb; ++bb) {
                const double m = Mat[(long)(b0 + bb) * n + a];
#pragma unroll
                for (int q = 0; q < 16; ++q)
                    if (ty + 4 * q < r) acc[q] = fma(m, ins[bb][ty + 4 * q], acc[q]);
            }
    }
    if (a >= n) return;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const int c = ty + 4 * q;
        if (c >= r) continue;
        const long idx = (s0 + a) * r + c;
        if (!BACK) {
            T[idx] = (D != nullptr ? half_rho : 1.0) * acc[q];
        } else {
            const double z = acc[q], f = (double)F[idx], u = (double)D[idx];
            const double un = f - (z - u);
            Z32[idx] = (float)z, D32[idx] = (float)un;
            if (Z64 != nullptr) Z64[idx] = z, D64[idx] = un;
        }
    }
}

// sum over all rows e of every slab of s_e sum_c T[e][c]^2 (T = U^T F): trace(F^T M F), one workgroup, fixed order
__global__ __launch_bounds__(256) void k_gl2_value(const double *__restrict__ T, const double *__restrict__ eig, long rows, int n,
                                                   int r, double *__restrict__ out) {
    __shared__ double sm[256];
    double acc = 0.0;
    for (long e = threadIdx.x; e < rows; e += 256) {
        double s = 0.0;
        for (int c = 0; c < r; ++c) s = fma(T[e * r + c], T[e * r + c], s);
        acc = fma(eig[e % n], s, acc);
    }
    sm[threadIdx.x] = acc;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sm[threadIdx.x] += sm[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = sm[0];
}

// ---------------------------------------------------------------------------------------------------------
// UnitSimplex (penalties.py:928-980): per column of a slab the multiplier mu of sum_j max(y_j - mu, 0) = 1 (the reference:
// scipy's bisection on the same bracket), aux = max(y - mu, 0).  One wave per (slab, column): 60 bisection steps narrow the
// bracket to the linear piece of the root, where mu = (sum of the active entries - 1) / their number exactly.
// ---------------------------------------------------------------------------------------------------------
template <typename TIN>
__global__ __launch_bounds__(256) void k_slab_simplex(const int *__restrict__ ext, int n_slabs, int r, const TIN *__restrict__ F,
                                                      const TIN *__restrict__ D, float *__restrict__ Z32, double *__restrict__ Z64,
                                                      const int *__restrict__ gate) {
    MCL_GATE(gate);
    const int lane = threadIdx.x & 63;
    const long w = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= (long)n_slabs * r) return;
    const int slab = (int)(w / r), col = (int)(w - (long)slab * r);
    const long s0 = ext[slab];
    const int n = ext[slab + 1] - ext[slab];
    if (n <= 0) return;
    auto y_at = [&](int j) { return (double)F[(s0 + j) * r + col] + (double)D[(s0 + j) * r + col]; };
    double mn = 1e300, mx = -1e300;
    for (int j = lane; j < n; j += 64) {
        const double y = y_at(j);
        mn = fmin(mn, y), mx = fmax(mx, y);
    }
    for (int o = 32; o > 0; o >>= 1) mn = fmin(mn, __shfl_xor(mn, o)), mx = fmax(mx, __shfl_xor(mx, o));
    double lo = mn - 1.0 - 1e-5, hi = mx + 1e-5;  // f(lo) > 0 > f(hi) = -1 (the reference's bracket, penalties.py:950-960)
    lo = fmin(0.9 * lo, 1.1 * lo), hi = fmax(0.9 * hi, 1.1 * hi);
    for (int it = 0; it < 60; ++it) {
        const double mid = 0.5 * (lo + hi);
        double s = 0.0;
        for (int j = lane; j < n; j += 64) s += fmax(y_at(j) - mid, 0.0);
        s = wave_sum_d(s) - 1.0;
        if (s > 0.0) lo = mid;
        else hi = mid;
    }
    // on [lo, hi] the active set is constant (unless a breakpoint sits within 2^-60 of the root): the root of the linear piece
    double sa = 0.0, cnt = 0.0;
    for (int j = lane; j < n; j += 64) {
        const double y = y_at(j);
        if (y > hi) sa += y, cnt += 1.0;
    }
    sa = wave_sum_d(sa), cnt = wave_sum_d(cnt);
    double mu = 0.5 * (lo + hi);
    if (cnt > 0.0) {
        const double m2 = (sa - 1.0) / cnt;
        if (m2 >= lo && m2 <= hi) mu = m2;
    }
    for (int j = lane; j < n; j += 64) {
        const double z = fmax(y_at(j) - mu, 0.0);
        Z32[(s0 + j) * r + col] = (float)z;
        if (Z64 != nullptr) Z64[(s0 + j) * r + col] = z;
    }
}

// =========================================================================================================
// host launchers
// =========================================================================================================
void mcl_launch_prox_l2ball(mcl_context *c, const ModeView &mv, const RegSet &rs, int k, bool vec, ProxForm form) {
    if (form.stack_fused) {  // statistics only; slot k of the colsq table
        if (form.stats_in_solve) return;  // already produced by k_rows_solve_stats + k_stats_reduce
        hipLaunchKernelGGL(k_slab_colsq, dim3((unsigned)mv.n_slabs), dim3(256), 0, c->stream, mv.ext, mv.F,
                           rs.dual[k], rs.nonneg[k], c->r, c->RP, c->colsq + (long)k * mv.n_slabs * c->r);
        return;
    }
    hipLaunchKernelGGL(k_slab_colsq, dim3((unsigned)mv.n_slabs), dim3(256), 0, c->stream, mv.ext, mv.F,
                       rs.dual[k], rs.nonneg[k], c->r, c->RP, c->colsq);
    dim3 grid((unsigned)((mv.n_tiles + 3) / 4)), block(256);
    DISPATCH_ROWS(c, vec, k_rows_l2ball, grid, block, mv, rs, k, c->r, (const double *)c->colsq);
}

void mcl_launch_prox_tv(mcl_context *c, const ModeView &mv, const RegSet &rs, int k) {
    const long nthreads = (long)mv.n_slabs * c->r;
    hipLaunchKernelGGL(k_slab_tv, dim3((unsigned)((nthreads + 63) / 64)), dim3(64), 0, c->stream, mv.ext, mv.n_slabs,
                       (const float *)mv.F, mv.rho, rs, k, c->r);
}

// The two passes of the GeneralizedL2 prox on the caller's fp32 buffers (TIN = float; Z64 = D64 = nullptr) or on the fp64 state
// of wide.hip, which also receives the results
template <typename TIN>
static void gl2_prox(mcl_context *c, const ModeView &mv, const RegSet &rs, int k, const TIN *F, const TIN *D, double *Z64, double *D64) {
    const int n = rs.mat_rows[k];
    const double *U = rs.mat[k], *eig = U + (long)n * n, *UT = eig + n;
    const dim3 g((unsigned)((n + 63) / 64) * (unsigned)mv.n_slabs);
    hipLaunchKernelGGL((k_gl2_pass<TIN, false>), g, dim3(256), 0, c->stream, mv.ext, U, eig, n, c->r, mv.rho, F, D, c->gl2_T,
                       (float *)nullptr, (float *)nullptr, (double *)nullptr, (double *)nullptr, mv.gate);
    hipLaunchKernelGGL((k_gl2_pass<TIN, true>), g, dim3(256), 0, c->stream, mv.ext, UT, eig, n, c->r, mv.rho, F, D, c->gl2_T,
                       rs.aux[k], rs.dual[k], Z64, D64, mv.gate);
}

void mcl_launch_prox_gl2(mcl_context *c, const ModeView &mv, const RegSet &rs, int k) {
    gl2_prox<float>(c, mv, rs, k, mv.F, rs.dual[k], nullptr, nullptr);
}

int mcl_launch_gl2_wide(mcl_context *c, int mode, int k, const double *F64, double *Z64, double *D64) {
    gl2_prox<double>(c, view_of(c, mode), c->regs[mode], k, F64, D64, Z64, D64);
    MCL_CHECK_HIP(c, hipGetLastError());
    return 0;
}

// trace(F^T M F) summed over the matrices of the mode (penalties.py:737-745) -> out[0]
int mcl_launch_gl2_value(mcl_context *c, int mode, int k, double *out) {
    ModeView mv = view_of(c, mode);
    const RegSet &rs = c->regs[mode];
    const int n = rs.mat_rows[k];
    const double *U = rs.mat[k], *eig = U + (long)n * n;
    const long rows = (long)n * mv.n_slabs;
    ProfScope prof(c, MCL_PROF_DIAG);
    if (rows == 0) {
        MCL_CHECK_HIP(c, hipMemsetAsync(out, 0, sizeof(double), c->stream));
        return 0;
    }
    hipLaunchKernelGGL((k_gl2_pass<float, false>), dim3((unsigned)((n + 63) / 64) * (unsigned)mv.n_slabs), dim3(256), 0, c->stream, mv.ext,
                       U, eig, n, c->r, mv.rho, (const float *)mv.F, (const float *)nullptr, c->gl2_T, (float *)nullptr, (float *)nullptr,
                       (double *)nullptr, (double *)nullptr, (const int *)nullptr);
    hipLaunchKernelGGL(k_gl2_value, dim3(1), dim3(256), 0, c->stream, (const double *)c->gl2_T, eig, rows, n, c->r, out);
    MCL_CHECK_HIP(c, hipGetLastError());
    return 0;
}

// the simplex projection of F + D: the caller's fp32 buffers (Z64 = nullptr), or the fp64 state of wide.hip
template <typename TIN>
static void simplex_prox(mcl_context *c, const ModeView &mv, const RegSet &rs, int k, const TIN *F, const TIN *D, double *Z64) {
    const long nw = (long)mv.n_slabs * c->r;
    hipLaunchKernelGGL((k_slab_simplex<TIN>), dim3((unsigned)((nw + 3) / 4)), dim3(256), 0, c->stream, mv.ext, mv.n_slabs, c->r, F, D,
                       rs.aux[k], Z64, mv.gate);
}

void mcl_launch_prox_simplex(mcl_context *c, const ModeView &mv, const RegSet &rs, int k) {
    simplex_prox<float>(c, mv, rs, k, mv.F, rs.dual[k], nullptr);
}

int mcl_launch_simplex_wide(mcl_context *c, int mode, int k, const double *F64, const double *D64, double *Z64) {
    simplex_prox<double>(c, view_of(c, mode), c->regs[mode], k, F64, D64, Z64);
    MCL_CHECK_HIP(c, hipGetLastError());
    return 0;
}
