// parafac2_project (projection.py): fit new matrices to a fixed PARAFAC2 model (Delta [r, r], C [K, r]).
// For every new matrix X [J, K], J >= r: minimise |X - P Delta diag(a) C^T|_F^2 over a and P with P^T P = I by alternation.
// With W = X C, G = W^T W, H = C^T C, nx = |X|^2, iteration t = 1, 2, ...:
//   Q = Delta (a a^T o G) Delta^T, symmetrised; Q^-1/2 by cyclic Jacobi on the eigenvalues lam > 0, lam > 1e-12 lam_max
//   T = diag(a) Delta^T Q^-1/2 (P = W T), PtP = T^T G T, S = (Delta^T PtP Delta) o H, d = diag(Delta^T T^T G)
//   a <- S^-1 d (spd_inverse_lds), e2_t = max(0, (nx - 2 a^T d + a^T S a) / nx)
//   stop after t when e2_t < absolute_tol, or t >= 2 and |e2_{t-1} - e2_t| <= tol e2_{t-1}, or t = n_iter_max
// Launches: k_proj_setup (one workgroup: the fragments of C, H), k_proj_norm (nx per matrix), k_proj_xc (W = X C on the fp32
// MFMA, xc_segment of cp_passes.h), k_proj_iterate (one workgroup per matrix: G - for a matrix of few rows from W formed again in
// fp64 - and the whole iteration in LDS, fp64),
// k_proj_out (P = W T and B = P Delta as fp32 rows).  Every sum has a fixed order that depends on the matrix's own shape only
// and no float atomics are used: a matrix's result does not depend on the other matrices of the call, two runs are bitwise equal.
#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "cp_passes.h"

namespace {

static ErrorSlot g_project_error{"mcl_pf2_project: "};
constexpr int PJ_MAX_RANK = 32;

// ---- set-up (one workgroup): Cfrag (zeroed by the caller) from C, H = C^T C -----------------------------------------------------
__global__ __launch_bounds__(256) void k_proj_setup(const double *__restrict__ C64, int K, int r, int NB, float *__restrict__ Cfrag,
                                                    double *__restrict__ H) {
    const int tid = threadIdx.x;
    for (long e = tid; e < (long)K * r; e += 256) {
        const int k = (int)(e / r), s = (int)(e - (long)k * r);
        Cfrag[cfrag_index(k, s, NB)] = (float)C64[e];
    }
    for (int e = tid; e < r * r; e += 256) {
        const int a = e / r, c = e - a * r;
        double s = 0.0;
        for (int k = 0; k < K; ++k) s = fma(C64[(long)k * r + a], C64[(long)k * r + c], s);
        H[e] = s;
    }
}

// ---- |X_i|^2: threads strided over the matrix's elements, then a fixed tree (the order of parafac2als.hip's k_pf2als_norm) ------
template <class XL>
__global__ __launch_bounds__(256) void k_proj_norm(const typename XL::T *__restrict__ X, const int *__restrict__ ext, int K,
                                                   double *__restrict__ stats) {
    __shared__ double red[256];
    const int i = blockIdx.x, tid = threadIdx.x;
    const long b = (long)ext[i] * K, n = (long)(ext[i + 1] - ext[i]) * K;
    double s = 0.0;
    for (long e = tid; e < n; e += 256) {
        const double x = (double)XL::ld1(X + b + e);
        s = fma(x, x, s);
    }
    red[tid] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) red[tid] += red[tid + o];
        __syncthreads();
    }
    if (tid == 0) stats[2 * i + 1] = red[0];
}

// ---- pass 1: W = X C, one wave per segment (xc_segment, cp_passes.h); the epilogue stores the rows of W -------------------------
template <class XL, int NB, bool VEC>
__global__ __launch_bounds__(256) void k_proj_xc(const typename XL::T *__restrict__ X, const int4 *__restrict__ segs, int nseg, int K, int r,
                                                 const float *__restrict__ Cfrag, float *__restrict__ W) {
    __shared__ f32x4 tiles[4][16 * 16];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, seg = blockIdx.x * 4 + w;
    if (seg >= nseg) return;  // whole waves; no barrier below
    const int4 sg = segs[seg];
    const int row0 = sg.y, n = sg.z;
    const int row16 = lane & 15, g = lane >> 4;
    f32x4 acc[4][NB];
    xc_segment<XL, NB, VEC>(X, sg, K, Cfrag, tiles[w], acc);
#pragma unroll
    for (int rb = 0; rb < 4; ++rb) {
        const int loc = 16 * rb + row16;
        if (loc >= n) continue;
#pragma unroll
        for (int hp = 0; hp < NB; ++hp)
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int q = 16 * hp + 4 * g + v;
                if (q < r) W[(long)(row0 + loc) * r + q] = acc[rb][hp][v];
            }
    }
}

// ---- the iteration: one workgroup per matrix ----------------------------------------------------------------------------------------
// Dynamic LDS (pj_lds_bytes): seven r x r fp64 matrices (G, Delta, H, T and the work matrices M1, M2, M3), the vectors a, d, Sa
// and the Jacobi scratch cs, then the stage of 64 rows of W (fp32, row stride r + 1; 32 rows of fp64 for a matrix of few rows).  At rank 32 that is 7 * 8 KB + 1 KB + 8.25 KB
// = 65.3 KB, above the 64 KB a kernel gets without asking: the launcher raises the limit of the RMAX = 32 instantiation.
// Every thread leaves the loop in the same iteration: thread 0 writes the verdict to LDS and all read it behind a barrier.
static inline size_t pj_lds_bytes(int r) {
    return sizeof(double) * (size_t)(7 * r * r + 3 * r + (r + 2) + 4) + sizeof(float) * (size_t)(64 * (r + 1));
}

template <class XL, int RMAX>
__global__ __launch_bounds__(256) void k_proj_iterate(const typename XL::T *__restrict__ X, const double *__restrict__ C64, int K,
                                                      const float *__restrict__ W, const int *__restrict__ ext, int r,
                                                      const double *__restrict__ Delta, const double *__restrict__ Hm,
                                                      const double *__restrict__ a_init, int n_iter_max, double tol, double absolute_tol,
                                                      double *__restrict__ A, double *__restrict__ Tout, double *__restrict__ stats,
                                                      int *__restrict__ n_iter, double *__restrict__ errors) {
    constexpr int NE = (RMAX * RMAX + 255) / 256;
    extern __shared__ double pj_sm[];
    const int i = blockIdx.x, tid = threadIdx.x, rr = r * r, ws = r + 1;
    double *G = pj_sm, *Dl = G + rr, *Hc = Dl + rr, *T = Hc + rr, *M1 = T + rr, *M2 = M1 + rr, *M3 = M2 + rr;
    double *a = M3 + rr, *d = a + r, *Sa = d + r, *cs = Sa + r, *sc = cs + (r + 2);  // sc: {e2, stop}
    float *Ws = reinterpret_cast<float *>(sc + 4);
    const int s0 = ext[i], n = ext[i + 1] - s0;
    for (int e = tid; e < rr; e += 256) Dl[e] = Delta[e], Hc[e] = Hm[e];
    if (tid < r) a[tid] = a_init[(long)i * r + tid];
    // G = W^T W: the rows in ascending order, 64 at a time from the fp32 W of pass 1 - or, for a matrix of few rows, 32 at a time
    // from W formed here in fp64 (the stage holds 32 rows of doubles in the same bytes).  An entry of the fp32 W is a chain of K
    // fp32 roundings, off by about 3e-8 sqrt(K) relative; G averages that over the J r entries of W, so e2 moves by about
    // 6e-8 sqrt(K / (J r)).  Three times that stays below a third of 1e-7 from J r = 4 K on; below, the J r K products cost less
    // than 4 K^2 FMAs and are done in fp64.  The choice depends on the matrix's own shape only.
    const bool few = (long)n * r < 4L * K;
    double *Wd = reinterpret_cast<double *>(Ws);
    const int rows = few ? 32 : 64;
    double acc[NE];
#pragma unroll
    for (int u = 0; u < NE; ++u) acc[u] = 0.0;
    for (int j0 = 0; j0 < n; j0 += rows) {
        const int cnt = min(rows, n - j0);
        __syncthreads();
        for (int e = tid; e < cnt * r; e += 256) {
            const int jj = e / r, q = e - jj * r;
            if (few) {
                const typename XL::T *x = X + (long)(s0 + j0 + jj) * K;
                double s = 0.0;
                for (int k = 0; k < K; ++k) s = fma((double)XL::ld1(x + k), C64[(long)k * r + q], s);
                Wd[jj * ws + q] = s;
            } else {
                Ws[jj * ws + q] = W[(long)(s0 + j0 + jj) * r + q];
            }
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < NE; ++u) {
            const int e = tid + 256 * u;
            if (e >= rr) continue;
            const int p = e / r, q = e - p * r;
            double s = acc[u];
            if (few)
                for (int jj = 0; jj < cnt; ++jj) s = fma(Wd[jj * ws + p], Wd[jj * ws + q], s);
            else
                for (int jj = 0; jj < cnt; ++jj) s = fma((double)Ws[jj * ws + p], (double)Ws[jj * ws + q], s);
            acc[u] = s;
        }
    }
#pragma unroll
    for (int u = 0; u < NE; ++u)
        if (tid + 256 * u < rr) G[tid + 256 * u] = acc[u];
    const double nx = stats[2 * i + 1];
    double prev = 0.0;
    int t = 0;
    __syncthreads();
    for (;;) {
        ++t;
        // M1[p][y] = sum_q a_p a_q G[p][q] Delta[y][q]
        for (int e = tid; e < rr; e += 256) {
            const int p = e / r, y = e - p * r;
            double s = 0.0;
            for (int q = 0; q < r; ++q) s = fma(a[p] * a[q] * G[p * r + q], Dl[y * r + q], s);
            M1[e] = s;
        }
        __syncthreads();
        // Q = Delta M1 (M2), symmetrised (M3)
        for (int e = tid; e < rr; e += 256) {
            const int x = e / r, y = e - x * r;
            double s = 0.0;
            for (int p = 0; p < r; ++p) s = fma(Dl[x * r + p], M1[p * r + y], s);
            M2[e] = s;
        }
        __syncthreads();
        for (int e = tid; e < rr; e += 256) {
            const int x = e / r, y = e - x * r;
            M3[e] = 0.5 * (M2[x * r + y] + M2[y * r + x]);
        }
        __syncthreads();
        jacobi_lds(M3, M2, cs, r);  // eigenvalues on the diagonal of M3, eigenvectors in the columns of M2
        double lmax = 0.0;
        for (int k = 0; k < r; ++k) lmax = fmax(lmax, M3[k * r + k]);
        // M1 = Q^-1/2 on the kept eigenvalues
        for (int e = tid; e < rr; e += 256) {
            const int x = e / r, y = e - x * r;
            double s = 0.0;
            for (int k = 0; k < r; ++k) {
                const double l = M3[k * r + k];
                if (l > 0.0 && l > 1e-12 * lmax) s += M2[x * r + k] * M2[y * r + k] / sqrt(l);
            }
            M1[e] = s;
        }
        __syncthreads();
        // T[p][q] = a_p sum_x Delta[x][p] M1[x][q]
        for (int e = tid; e < rr; e += 256) {
            const int p = e / r, q = e - p * r;
            double s = 0.0;
            for (int x = 0; x < r; ++x) s = fma(Dl[x * r + p], M1[x * r + q], s);
            T[e] = a[p] * s;
        }
        __syncthreads();
        // M3 = G T
        for (int e = tid; e < rr; e += 256) {
            const int p = e / r, q = e - p * r;
            double s = 0.0;
            for (int u = 0; u < r; ++u) s = fma(G[p * r + u], T[u * r + q], s);
            M3[e] = s;
        }
        __syncthreads();
        // PtP = T^T M3 (M1); d[s] = sum_x Delta[x][s] (T^T G)[x][s], (T^T G)[x][s] = M3[s][x] (G is symmetric bit for bit)
        for (int e = tid; e < rr; e += 256) {
            const int x = e / r, y = e - x * r;
            double s = 0.0;
            for (int p = 0; p < r; ++p) s = fma(T[p * r + x], M3[p * r + y], s);
            M1[e] = s;
        }
        if (tid < r) {
            double s = 0.0;
            for (int x = 0; x < r; ++x) s = fma(Dl[x * r + tid], M3[tid * r + x], s);
            d[tid] = s;
        }
        __syncthreads();
        // M2 = PtP Delta
        for (int e = tid; e < rr; e += 256) {
            const int p = e / r, s = e - p * r;
            double v = 0.0;
            for (int u = 0; u < r; ++u) v = fma(M1[p * r + u], Dl[u * r + s], v);
            M2[e] = v;
        }
        __syncthreads();
        // S = (Delta^T M2) o H, kept in M1; its inverse in M3
        for (int e = tid; e < rr; e += 256) {
            const int x = e / r, s = e - x * r;
            double v = 0.0;
            for (int p = 0; p < r; ++p) v = fma(Dl[p * r + x], M2[p * r + s], v);
            M1[e] = M3[e] = v * Hc[e];
        }
        __syncthreads();
        spd_inverse_lds<256>(M3, M2, cs, r, [&](int e) { return M1[e]; });
        if (tid < r) {
            double s = 0.0;
            for (int p = 0; p < r; ++p) s = fma(M3[tid * r + p], d[p], s);
            a[tid] = s;
        }
        __syncthreads();
        if (tid < r) {
            double s = 0.0;
            for (int p = 0; p < r; ++p) s = fma(M1[tid * r + p], a[p], s);
            Sa[tid] = s;
        }
        __syncthreads();
        if (tid == 0) {
            double ad = 0.0, asa = 0.0;
            for (int p = 0; p < r; ++p) ad = fma(a[p], d[p], ad), asa = fma(a[p], Sa[p], asa);
            const double e2 = nx > 0.0 ? fmax(0.0, nx - 2.0 * ad + asa) / nx : 0.0;
            if (errors) errors[(long)i * n_iter_max + (t - 1)] = e2;
            sc[0] = e2;
            sc[1] = (e2 < absolute_tol || (t >= 2 && fabs(prev - e2) <= tol * prev) || t >= n_iter_max) ? 1.0 : 0.0;
        }
        __syncthreads();
        prev = sc[0];
        if (sc[1] != 0.0) break;  // uniform: every thread reads the same word behind the barrier
    }
    // (no thread writes sc, a, T or Dl below)
    if (tid < r) A[(long)i * r + tid] = a[tid];
    if (tid == 0) stats[2 * i] = prev * nx, n_iter[i] = t;
    if (errors)
        for (int e = t + tid; e < n_iter_max; e += 256) errors[(long)i * n_iter_max + e] = __builtin_nan("");
    // T and T Delta for the rows of P and B
    for (int e = tid; e < rr; e += 256) {
        const int p = e / r, s = e - p * r;
        double v = 0.0;
        for (int q = 0; q < r; ++q) v = fma(T[p * r + q], Dl[q * r + s], v);
        Tout[(long)i * 2 * rr + e] = T[e];
        Tout[(long)i * 2 * rr + rr + e] = v;
    }
}

// ---- outputs: P = W T and B = W (T Delta) as fp32 rows -----------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_proj_out(const float *__restrict__ W, const double *__restrict__ Tm, const int *__restrict__ ext, int I,
                                                  long N, int r, float *__restrict__ P, float *__restrict__ B) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= N * r) return;
    const int row = (int)(e / r), q = (int)(e - (long)row * r);
    const double *T = Tm + (long)slab_of_row(ext, I, row) * 2 * r * r, *TD = T + r * r;
    double sp = 0.0, sb = 0.0;
    for (int p = 0; p < r; ++p) {
        const double w = (double)W[(long)row * r + p];
        sp = fma(w, T[p * r + q], sp);
        sb = fma(w, TD[p * r + q], sb);
    }
    P[e] = (float)sp;
    B[e] = (float)sb;
}

struct PjPlan {
    int64_t N, total;
    int nseg, NB, KH;
    int4 *segs;
    int *ext;
    float *Cfrag, *W;
    double *H, *Delta, *T;
};

// workspace NULL: the parts are null and `total` is the size (mcl_pf2_project_workspace_bytes)
PjPlan pj_plan(void *workspace, const int64_t *row_ptr, int64_t I, int64_t K, int rank) {
    PjPlan p{};
    p.N = row_ptr[I];
    const int64_t nseg = seg_count(row_ptr, I), r = rank;
    p.nseg = (int)nseg;
    p.NB = rank <= 16 ? 1 : 2;
    p.KH = 4 * (int)((K + 63) / 64);
    WsCursor ws(workspace);
    p.segs = ws.take<int4>(std::max<int64_t>(nseg, 1) * 16);
    p.ext = ws.take<int>((I + 1) * 4);
    p.Cfrag = ws.take<float>((int64_t)p.KH * p.NB * 64 * 4 * 4);
    p.H = ws.take<double>(r * r * 8);
    p.Delta = ws.take<double>(r * r * 8);
    p.W = ws.take<float>(p.N * r * 4);
    p.T = ws.take<double>(I * 2 * r * r * 8);
    p.total = ws.off;
    return p;
}

std::string pj_check_shape(const int64_t *row_ptr, int64_t I, int64_t K, int32_t rank) {
    if (!row_ptr || I < 1 || K < 1) return "need row_ptr, I >= 1, K >= 1";
    if (rank < 1 || rank > PJ_MAX_RANK) return "rank " + std::to_string(rank) + " is outside 1 ... 32";
    if (row_ptr[0] != 0) return "row_ptr[0] must be 0";
    for (int64_t i = 0; i < I; ++i)
        if (row_ptr[i + 1] - row_ptr[i] < rank) return "every matrix needs at least rank rows (matrix " + std::to_string(i) + ")";
    if (rank > K) return "rank " + std::to_string(rank) + " exceeds K = " + std::to_string(K) + ": W = X C has rank K and no orthonormal P exists";
    if (row_ptr[I] >= (int64_t(1) << 31) / PJ_MAX_RANK) return "more than 2^26 packed rows are not supported";
    if (K >= (int64_t(1) << 31) / PJ_MAX_RANK) return "K of 2^26 or more is not supported";
    return "";
}

template <class XL, int RMAX>
int pj_run(const typename XL::T *X, int32_t x_type, const int64_t *row_ptr, int64_t I, int64_t K, int32_t rank, const double *Delta,
           const double *C, const double *a_init, int32_t n_iter_max, double tol, double absolute_tol, double *A, float *B, float *P,
           double *stats, int32_t *n_iter, double *errors, const PjPlan &p, hipStream_t s) {
    constexpr int NB = RMAX / 16;
    ErrorSlot &fail = g_project_error;
    const int r = rank;

    // the model and the start are read back and checked before anything is launched
    std::vector<double> h((size_t)(r * r + K * r + I * r));
    CP_HIP(hipMemcpyAsync(h.data(), Delta, sizeof(double) * r * r, hipMemcpyDeviceToHost, s));
    CP_HIP(hipMemcpyAsync(h.data() + r * r, C, sizeof(double) * K * r, hipMemcpyDeviceToHost, s));
    CP_HIP(hipMemcpyAsync(h.data() + r * r + K * r, a_init, sizeof(double) * I * r, hipMemcpyDeviceToHost, s));
    CP_HIP(hipStreamSynchronize(s));
    for (size_t e = 0; e < h.size(); ++e)
        if (!std::isfinite(h[e]))
            return fail(std::string(e < (size_t)(r * r) ? "Delta" : e < (size_t)(r * r + K * r) ? "C" : "a_init") + " holds a non-finite entry");
    const size_t lds = pj_lds_bytes(r);
    CP_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(k_proj_iterate<XL, RMAX>), hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)pj_lds_bytes(RMAX)));

    const SegTables tb = seg_tables(row_ptr, I);
    CP_HIP(upload_tables(tb, p.segs, nullptr, p.ext, s));
    CP_HIP(hipMemsetAsync(p.Cfrag, 0, (size_t)p.KH * p.NB * 64 * 4 * 4, s));
    CP_HIP(hipMemcpyAsync(p.Delta, Delta, sizeof(double) * r * r, hipMemcpyDeviceToDevice, s));
    CP_HIP(hipStreamSynchronize(s));  // (the tables are locals)

    hipLaunchKernelGGL(k_proj_setup, dim3(1), dim3(256), 0, s, C, (int)K, r, NB, p.Cfrag, p.H);
    hipLaunchKernelGGL(k_proj_norm<XL>, dim3((unsigned)I), dim3(256), 0, s, X, (const int *)p.ext, (int)K, stats);
    vec_dispatch(K % 4 == 0 && mcl_x_vec_aligned(X, x_type), [&](auto vec) {
        hipLaunchKernelGGL((k_proj_xc<XL, NB, decltype(vec)::value>), dim3((unsigned)((p.nseg + 3) / 4)), dim3(256), 0, s, X, (const int4 *)p.segs,
                           p.nseg, (int)K, r, (const float *)p.Cfrag, p.W);
    });
    hipLaunchKernelGGL((k_proj_iterate<XL, RMAX>), dim3((unsigned)I), dim3(256), lds, s, X, C, (int)K, (const float *)p.W, (const int *)p.ext, r,
                       (const double *)p.Delta, (const double *)p.H, a_init, (int)n_iter_max, tol, absolute_tol, A, p.T, stats, n_iter, errors);
    hipLaunchKernelGGL(k_proj_out, dim3((unsigned)((p.N * r + 255) / 256)), dim3(256), 0, s, (const float *)p.W, (const double *)p.T,
                       (const int *)p.ext, (int)I, (long)p.N, r, P, B);
    CP_HIP(hipGetLastError());
    return 0;
}

}  // namespace

extern "C" {

const char *mcl_pf2_project_last_error(void) { return g_project_error.c_str(); }

int64_t mcl_pf2_project_workspace_bytes(const int64_t *row_ptr, int64_t I, int64_t K, int32_t rank) {
    if (!pj_check_shape(row_ptr, I, K, rank).empty()) return -1;
    return pj_plan(nullptr, row_ptr, I, K, rank).total;
}

int mcl_pf2_project_typed(const void *X, int32_t x_type, const int64_t *row_ptr, int64_t I, int64_t K, int32_t rank, const double *Delta,
                          const double *C, const double *a_init, int32_t n_iter_max, double tol, double absolute_tol, double *A, float *B,
                          float *P, double *stats, int32_t *n_iter, double *errors, void *workspace, int64_t workspace_bytes,
                          void *hip_stream) {
    ErrorSlot &fail = g_project_error;
    const std::string bad = pj_check_shape(row_ptr, I, K, rank);
    if (!bad.empty()) return fail(bad);
    if (!X || !Delta || !C || !a_init || !A || !B || !P || !stats || !n_iter || !workspace) return fail("NULL argument");
    if (!x_type_error(x_type).empty()) return fail(x_type_error(x_type));
    if (n_iter_max < 1 || !(tol >= 0.0) || !(absolute_tol >= 0.0)) return fail("need n_iter_max >= 1, tol >= 0 and absolute_tol >= 0");
    const PjPlan p = pj_plan(workspace, row_ptr, I, K, rank);
    if (workspace_refused(fail, workspace, workspace_bytes, p.total, "mcl_pf2_project_workspace_bytes")) return 1;
    hipStream_t s = reinterpret_cast<hipStream_t>(hip_stream);
    return mcl_x_dispatch(x_type, [&](auto xl) {
        using XL = decltype(xl);
        return rank_bucket(rank, [&](auto rmax) {
            return pj_run<XL, decltype(rmax)::value>(static_cast<const typename XL::T *>(X), x_type, row_ptr, I, K, rank, Delta, C, a_init,
                                                     n_iter_max, tol, absolute_tol, A, B, P, stats, n_iter, errors, p, s);
        });
    });
}

}  // extern "C"
