// multistart_evaluation (matcouply_amd/evaluation.py): fit, per-matrix SSE and core consistency of many
// fitted models of one data set, from one read of X per model.
//
// A model is [A; B; C] row-major, (I + N + K) x r fp64, the layout of mcl_fms_scores (similarity.hip).  Two entries:
//   mcl_eval_tables_typed   S_i = B_i^T X_i C and B_i^T B_i (r x r), sse_i = |X_i - B_i diag(a_i) C^T|^2 per model and matrix,
//                           norm_i = |X_i|^2 per matrix:
//     k_eval_prep    per model: the fp32 fragments of C for the two products of the table pass;
//     k_eval_tables  one wave per (model, segment of <= CP_SEG rows of one matrix): the staged 16 x 64 tile of X (the global ->
//                    LDS -> fragment path of xc_segment, cp_passes.h) is multiplied with C on the fp32 MFMA, and the model tile
//                    (B_i o a_i) C^T of the same 16 x 64 entries is formed on it too (reduction over r only), in the fragment
//                    layout of the X tile, so the residual x - m is taken entry by entry and squared and summed in fp64; the
//                    segment's X C goes through LDS to the fp64 MFMA for B_seg^T (X C)_seg and B_seg^T B_seg;
//     k_eval_reduce  per (model, matrix): the segments' partials summed in ascending order.
//   mcl_eval_core           k_eval_core, one workgroup per model, fp64: (C^T C)^+, (A^T A)^+, per matrix W_i = (B_i^T B_i)^+ S_i
//                           (C^T C)^+, the core G[p][q][s] = sum_i (A^+)[p][i] W_i[q][s] summed over i in ascending order, and the
//                           two consistency values.  ^+ is spd_inverse_lds of cp_passes.h.
// No atomics, every sum in an order that depends on the shape only: a model's tables and core are bitwise independent of the
// other models of the call, and two runs are bitwise equal.  The SSE is summed from the residual itself, never from
// |X|^2 - 2 <X, M> + |M|^2 (SURVEY.md finding 6: that form loses the residual to cancellation in fp32).
#include <cmath>
#include <string>
#include <vector>

#include "cp_passes.h"

namespace {

static ErrorSlot g_eval_error;
constexpr int EV_MAX_RANK = 32;
typedef double ev_f64x4 __attribute__((ext_vector_type(4)));

// ---- the fragments of C of one model -------------------------------------------------------------------------------------------
// Cfrag: cfrag_index of cp_passes.h (the A operand of X C).  Cmod[(16-row block kb16 of C) * RMAX / 4 + t][lane] =
// C[16 kb16 + (lane & 15)][4 t + (lane >> 4)]: the A operand of the model tile.  Rows past K and columns past r are zeros.
template <int NB>
__global__ __launch_bounds__(256) void k_eval_prep(const double *__restrict__ models, long len, long c_off, int K, int r, int KC,
                                                   float *__restrict__ Cfrag, float *__restrict__ Cmod) {
    constexpr int NT4 = 4 * NB;
    const long per = (long)KC * 64 * 16 * NB;
    const long f = (long)blockIdx.x * 256 + threadIdx.x;
    if (f >= per) return;
    const double *C = models + (long)blockIdx.y * len + c_off;
    {
        const int kq = (int)(f & 3), lane = (int)((f >> 2) & 63);
        const long rest = f >> 8;
        const int hp = (int)(rest % NB), kb16 = (int)(rest / NB);
        const int k = 16 * kb16 + 4 * (lane >> 4) + kq, s = 16 * hp + (lane & 15);
        Cfrag[(long)blockIdx.y * per + f] = (k < K && s < r) ? (float)C[(long)k * r + s] : 0.f;
    }
    {
        const int lane = (int)(f & 63);
        const long rest = f >> 6;
        const int t = (int)(rest % NT4), kb16 = (int)(rest / NT4);
        const int k = 16 * kb16 + (lane & 15), p = 4 * t + (lane >> 4);
        Cmod[(long)blockIdx.y * per + f] = (k < K && p < r) ? (float)C[(long)k * r + p] : 0.f;
    }
}

// ---- the table pass ----------------------------------------------------------------------------------------------------------------
// Workgroup = four waves = four consecutive segments of one model.  Per 64-column chunk H and 16-row block rb, lane
// (row16 = l & 15, g = l >> 4) holds x[h][v] = X[16 rb + row16][64 H + 16 h + 4 g + v] (rows clamped into the segment, columns past
// K zero) and:
//   X C         acc[rb][hp] += MFMA(A = Cfrag, B = x), lane l, reg v = XC[16 rb + row16][16 hp + 4 g + v]  (xc_segment's loop);
//   model tile  m[h] = sum_t MFMA(A = Cmod[h][t]: C[64 H + 16 h + i][4 t + g], B = ba[rb][t]: (B o a)[16 rb + row16][4 t + g]):
//               D[i = 4 g + v][j = row16] = M[16 rb + row16][64 H + 16 h + 4 g + v], the entry x[h][v] holds.
// part (per model and segment): S [r r], B^T B [r r], sum (x - m)^2, sum x^2.
template <class XL, int NB, bool VEC>
__global__ __launch_bounds__(256) void k_eval_tables(const typename XL::T *__restrict__ X, const int4 *__restrict__ segs, int nseg, int nwg,
                                                     int K, int r, int I, const double *__restrict__ models, long len,
                                                     const float *__restrict__ Cfrag, const float *__restrict__ Cmod, long cper,
                                                     double *__restrict__ part) {
    constexpr int RMAX = 16 * NB, NT4 = 4 * NB;
    __shared__ f32x4 tiles[4][16 * 16];
    __shared__ float xcs[4][64 * RMAX];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int model = blockIdx.x / nwg, seg = (blockIdx.x - model * nwg) * 4 + w;
    if (seg >= nseg) return;  // whole waves; no workgroup barrier below
    const int4 sg = segs[seg];
    const int row0 = sg.y, n = sg.z;
    const int row16 = lane & 15, g = lane >> 4, rr_ = lane >> 4, cc = lane & 15;
    const double *Am = models + (long)model * len + (long)sg.x * r;
    const double *Bm = models + (long)model * len + (long)I * r;
    Cfrag += (long)model * cper, Cmod += (long)model * cper;
    f32x4 *T = tiles[w];

    float ba[4][NT4];
#pragma unroll
    for (int rb = 0; rb < 4; ++rb)
#pragma unroll
        for (int t = 0; t < NT4; ++t) {
            const int p = 4 * t + g;
            ba[rb][t] = p < r ? (float)(Bm[(long)(row0 + min(16 * rb + row16, n - 1)) * r + p] * Am[p]) : 0.f;
        }
    f32x4 acc[4][NB];
#pragma unroll
    for (int rb = 0; rb < 4; ++rb)
#pragma unroll
        for (int hp = 0; hp < NB; ++hp) acc[rb][hp] = f32x4{0.f, 0.f, 0.f, 0.f};
    double sse = 0.0, sxx = 0.0;
    const int KC = (K + 63) >> 6;
    f32x4 xn[4];
    auto load = [&](int H, int rb) {
        const int col = 64 * H + 4 * cc;
#pragma unroll
        for (int t = 0; t < 4; ++t)
            xn[t] = x_ld4<XL, VEC>(X + (long)(row0 + min(16 * rb + 4 * t + rr_, n - 1)) * K + col, col, K);
    };
    load(0, 0);
    for (int H = 0; H < KC; ++H) {
        f32x4 cf[4][NB];
        float cm[4][NT4];
#pragma unroll
        for (int h = 0; h < 4; ++h) {
#pragma unroll
            for (int hp = 0; hp < NB; ++hp)
                cf[h][hp] = *reinterpret_cast<const f32x4 *>(Cfrag + (((long)(4 * H + h) * NB + hp) * 64 + lane) * 4);
#pragma unroll
            for (int t = 0; t < NT4; ++t) cm[h][t] = Cmod[((long)(4 * H + h) * NT4 + t) * 64 + lane];
        }
#pragma unroll
        for (int rb = 0; rb < 4; ++rb) {
#pragma unroll
            for (int t = 0; t < 4; ++t) T[(4 * t + rr_) * 16 + (cc ^ (4 * t + rr_))] = xn[t];
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
            const bool live = 16 * rb + row16 < n;
#pragma unroll
            for (int h = 0; h < 4; ++h) {
                f32x4 m = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int t = 0; t < NT4; ++t) m = MFMA16(cm[h][t], ba[rb][t], m);
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    const double xv = live ? (double)x[h][v] : 0.0, d = live ? (double)(x[h][v] - m[v]) : 0.0;
                    sxx = fma(xv, xv, sxx);
                    sse = fma(d, d, sse);
                }
            }
        }
    }
    // X C of the segment to LDS, row-major [64][RMAX] (LDS operations of one wave complete in order: no barrier)
    float *xc = xcs[w];
#pragma unroll
    for (int rb = 0; rb < 4; ++rb)
#pragma unroll
        for (int hp = 0; hp < NB; ++hp) *reinterpret_cast<f32x4 *>(xc + (16 * rb + row16) * RMAX + 16 * hp + 4 * g) = acc[rb][hp];
    double *out = part + ((long)model * nseg + seg) * (2 * r * r + 2);
    // fp64 MFMA, reduction over the rows four at a time: A[i = c][k = g] = B[4 s + g][16 pb + c], B[k = g][j = c] = XC / B of column
    // 16 qb + c; D lane l, reg v = [16 pb + g + 4 v][16 qb + c].  Rows past n are zeros in A.
    const int groups = (n + 3) >> 2;
#pragma unroll
    for (int pb = 0; pb < NB; ++pb)
#pragma unroll
        for (int qb = 0; qb < NB; ++qb) {
            ev_f64x4 sacc = {0.0, 0.0, 0.0, 0.0}, bacc = {0.0, 0.0, 0.0, 0.0};
            for (int s = 0; s < groups; ++s) {
                const int row = 4 * s + g;
                const bool ok = row < n;
                const double *Brow = Bm + (long)(row0 + min(row, n - 1)) * r;
                const double bp = (ok && 16 * pb + cc < r) ? Brow[16 * pb + cc] : 0.0;
                const double bq = (ok && 16 * qb + cc < r) ? Brow[16 * qb + cc] : 0.0;
                const double xq = (double)xc[row * RMAX + 16 * qb + cc];
                sacc = __builtin_amdgcn_mfma_f64_16x16x4f64(bp, xq, sacc, 0, 0, 0);
                bacc = __builtin_amdgcn_mfma_f64_16x16x4f64(bp, bq, bacc, 0, 0, 0);
            }
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int p = 16 * pb + g + 4 * v, q = 16 * qb + cc;
                if (p < r && q < r) out[p * r + q] = sacc[v], out[r * r + p * r + q] = bacc[v];
            }
        }
    sse = wave_sum(sse), sxx = wave_sum(sxx);
    if (lane == 0) out[2 * r * r] = sse, out[2 * r * r + 1] = sxx;
}

// per (matrix, model): the partials of its segments, summed in ascending order
__global__ __launch_bounds__(256) void k_eval_reduce(const double *__restrict__ part, const int *__restrict__ slab_seg, int nseg, int I, int r,
                                                     double *__restrict__ S, double *__restrict__ BtB, double *__restrict__ sse,
                                                     double *__restrict__ norm) {
    const int i = blockIdx.x, model = blockIdx.y, rr = r * r, E = 2 * rr + 2;
    const int s0 = slab_seg[i], s1 = slab_seg[i + 1];
    for (int e = threadIdx.x; e < E; e += 256) {
        double t = 0.0;
        for (int s = s0; s < s1; ++s) t += part[((long)model * nseg + s) * E + e];
        const long mi = (long)model * I + i;
        if (e < rr) S[mi * rr + e] = t;
        else if (e < 2 * rr) BtB[mi * rr + e - rr] = t;
        else if (e == 2 * rr) sse[mi] = t;
        else if (model == 0) norm[i] = t;  // (the same bits in every model's pass)
    }
}

// ---- the core pass -------------------------------------------------------------------------------------------------------------------
// One workgroup of RMAX^2 threads per model.  Thread tid < r r holds the entries G[p][q][s], q r + s = tid, of every p.
template <int RMAX>
__global__ __launch_bounds__(RMAX * RMAX) void k_eval_core(const double *__restrict__ models, long len, int I, long N, int K, int r,
                                                    const double *__restrict__ S, const double *__restrict__ BtB, double *__restrict__ core,
                                                    double *__restrict__ cc, double *__restrict__ ccn) {
    constexpr int RR = RMAX * RMAX, NT = RR;
    __shared__ double Ci[RR], Ai[RR], Gi[RR], Wj[RR], T1[RR], Wi[RR], cs[RMAX + 2], ap[RMAX], red[NT];
    const int tid = threadIdx.x, rr = r * r, rrr = rr * r;
    const long model = blockIdx.x;
    const double *A = models + model * len, *C = A + ((long)I + N) * r;
    auto gram = [&](const double *F, int rows, int e) {
        const int a = e / r, c = e - a * r;
        double s = 0.0;
        for (int k = 0; k < rows; ++k) s = fma(F[(long)k * r + a], F[(long)k * r + c], s);
        return s;
    };
    for (int e = tid; e < rr; e += NT) Ci[e] = gram(C, K, e), Ai[e] = gram(A, I, e);
    __syncthreads();
    spd_inverse_lds<NT>(Ci, Wj, cs, r, [&](int e) { return gram(C, K, e); });
    __syncthreads();  // (its verdict flag is shared by the calls)
    spd_inverse_lds<NT>(Ai, Wj, cs, r, [&](int e) { return gram(A, I, e); });
    double acc[RMAX];
#pragma unroll
    for (int p = 0; p < RMAX; ++p) acc[p] = 0.0;
    for (int i = 0; i < I; ++i) {
        const double *Si = S + (model * I + i) * rr, *Bi = BtB + (model * I + i) * rr;
        __syncthreads();
        for (int e = tid; e < rr; e += NT) Gi[e] = Bi[e];
        __syncthreads();
        spd_inverse_lds<NT>(Gi, Wj, cs, r, [&](int e) { return Bi[e]; });
        for (int e = tid; e < rr; e += NT) {  // T1 = (B_i^T B_i)^+ S_i
            const int a = e / r, c = e - a * r;
            double s = 0.0;
            for (int k = 0; k < r; ++k) s = fma(Gi[a * r + k], Si[k * r + c], s);
            T1[e] = s;
        }
        if (tid < r) {  // column i of A^+ = (A^T A)^+ A^T
            double s = 0.0;
            for (int k = 0; k < r; ++k) s = fma(Ai[tid * r + k], A[(long)i * r + k], s);
            ap[tid] = s;
        }
        __syncthreads();
        for (int e = tid; e < rr; e += NT) {  // W_i = T1 (C^T C)^+
            const int a = e / r, c = e - a * r;
            double s = 0.0;
            for (int k = 0; k < r; ++k) s = fma(T1[a * r + k], Ci[k * r + c], s);
            Wi[e] = s;
        }
        __syncthreads();
        if (tid < rr) {
            const double w = Wi[tid];
#pragma unroll
            for (int p = 0; p < RMAX; ++p)
                if (p < r) acc[p] = fma(ap[p], w, acc[p]);
        }
    }
    // sum (G - T)^2 and sum G^2: a thread's entries in ascending order, then a tree over the threads
    double dev = 0.0, sq = 0.0;
    if (tid < rr) {
        const int q = tid / r, s = tid - q * r;
#pragma unroll
        for (int p = 0; p < RMAX; ++p)
            if (p < r) {
                core[model * rrr + (long)p * rr + tid] = acc[p];
                const double d = acc[p] - ((p == q && q == s) ? 1.0 : 0.0);
                dev = fma(d, d, dev);
                sq = fma(acc[p], acc[p], sq);
            }
    }
    double tot[2];
    for (int h = 0; h < 2; ++h) {
        __syncthreads();
        red[tid] = h ? sq : dev;
        __syncthreads();
        for (int o = NT / 2; o > 0; o >>= 1) {
            if (tid < o) red[tid] += red[tid + o];
            __syncthreads();
        }
        tot[h] = red[0];
    }
    if (tid == 0) {
        cc[model] = 100.0 * (1.0 - tot[0] / r);
        ccn[model] = 100.0 * (1.0 - tot[0] / tot[1]);
    }
}

// ---- host side -------------------------------------------------------------------------------------------------------------------------
struct EvPlan {
    int nseg, nwg, KC, NB;
    int64_t cper;  // floats of one model's Cfrag (and of its Cmod)
    int4 *segs;
    int *slab_seg;
    float *Cfrag, *Cmod;
    double *part;
    int64_t total;
};

// ws NULL: the parts are null and `total` is the size (mcl_eval_workspace_bytes)
EvPlan ev_plan(void *ws, const int64_t *row_ptr, int64_t I, int64_t K, int rank, int64_t n_models) {
    EvPlan p{};
    p.nseg = (int)seg_count(row_ptr, I);
    p.nwg = (p.nseg + 3) / 4;
    p.KC = (int)((K + 63) / 64);
    p.NB = rank <= 16 ? 1 : 2;
    p.cper = (int64_t)p.KC * 64 * 16 * p.NB;
    WsCursor c(ws);
    p.segs = c.take<int4>((int64_t)p.nseg * 16);
    p.slab_seg = c.take<int>((I + 1) * 4);
    p.Cfrag = c.take<float>(n_models * p.cper * 4);
    p.Cmod = c.take<float>(n_models * p.cper * 4);
    p.part = c.take<double>(n_models * p.nseg * (2 * (int64_t)rank * rank + 2) * 8);
    p.total = c.off;
    return p;
}

std::string ev_check_shape(int64_t I, int64_t K, int32_t rank, int64_t n_models) {
    if (rank < 1 || rank > EV_MAX_RANK) return "rank " + std::to_string(rank) + " is outside 1 ... " + std::to_string(EV_MAX_RANK);
    if (n_models < 1 || n_models >= 65536) return "n_models " + std::to_string(n_models) + " is outside 1 ... 65535";
    if (I < 1 || K < 1) return "need I >= 1 and K >= 1";
    if (I >= 65536) return "more than 65535 matrices are not supported";
    if (K >= (int64_t(1) << 31) / 64) return "K >= 2^25 is not supported";
    return "";
}

std::string ev_check(const int64_t *row_ptr, int64_t I, int64_t K, int32_t rank, int64_t n_models) {
    const std::string bad = ev_check_shape(I, K, rank, n_models);
    if (!bad.empty()) return bad;
    if (!row_ptr) return "row_ptr is NULL";
    if (row_ptr[0] != 0) return "row_ptr[0] must be 0";
    for (int64_t i = 0; i < I; ++i)
        if (row_ptr[i + 1] <= row_ptr[i]) return "row_ptr must increase: matrix " + std::to_string(i) + " has no rows";
    if (row_ptr[I] >= (int64_t(1) << 31) / EV_MAX_RANK) return "more than 2^26 packed rows are not supported";
    if ((seg_count(row_ptr, I) + 3) / 4 * n_models >= (int64_t(1) << 31)) return "too many (model, segment) pairs for one launch";
    return "";
}

// "" when every entry of the n doubles at the device pointer is finite, else the message; read back in pieces, nothing is launched
std::string ev_models_finite(const double *models, int64_t n_models, int64_t len, hipStream_t s) {
    constexpr int64_t PIECE = int64_t(1) << 22;
    const int64_t n = n_models * len;
    std::vector<double> h((size_t)std::min(n, PIECE));
    for (int64_t b = 0; b < n; b += PIECE) {
        const int64_t cnt = std::min(PIECE, n - b);
        if (hipMemcpyAsync(h.data(), models + b, (size_t)cnt * 8, hipMemcpyDeviceToHost, s) != hipSuccess ||
            hipStreamSynchronize(s) != hipSuccess)
            return "reading the models back failed";
        for (int64_t e = 0; e < cnt; ++e)
            if (!std::isfinite(h[(size_t)e])) return "model " + std::to_string((b + e) / len) + " holds a non-finite entry";
    }
    return "";
}

template <class XL, int NB>
int ev_tables(const typename XL::T *X, int32_t x_type, const int64_t *row_ptr, int64_t I, int64_t K, int32_t rank, const double *models,
              int64_t n_models, double *S, double *BtB, double *sse, double *norm, const EvPlan &p, hipStream_t s) {
    ErrorSlot &fail = g_eval_error;
    const SegTables h = seg_tables(row_ptr, I);
    CP_HIP(upload_tables(h, p.segs, p.slab_seg, nullptr, s));
    CP_HIP(hipStreamSynchronize(s));  // (the tables are locals)
    const int64_t N = row_ptr[I];
    const long len = (long)(I + N + K) * rank;
    hipLaunchKernelGGL(k_eval_prep<NB>, dim3((unsigned)((p.cper + 255) / 256), (unsigned)n_models), dim3(256), 0, s, models, len,
                       (long)(I + N) * rank, (int)K, (int)rank, p.KC, p.Cfrag, p.Cmod);
    vec_dispatch(K % 4 == 0 && mcl_x_vec_aligned(X, x_type), [&](auto vec) {
        hipLaunchKernelGGL((k_eval_tables<XL, NB, decltype(vec)::value>), dim3((unsigned)(p.nwg * n_models)), dim3(256), 0, s, X, (const int4 *)p.segs,
                           p.nseg, p.nwg, (int)K, (int)rank, (int)I, models, len, (const float *)p.Cfrag, (const float *)p.Cmod, (long)p.cper, p.part);
    });
    hipLaunchKernelGGL(k_eval_reduce, dim3((unsigned)I, (unsigned)n_models), dim3(256), 0, s, (const double *)p.part, (const int *)p.slab_seg, p.nseg,
                       (int)I, (int)rank, S, BtB, sse, norm);
    CP_HIP(hipGetLastError());
    return 0;
}

}  // namespace

extern "C" {

const char *mcl_eval_last_error(void) { return g_eval_error.c_str(); }

int64_t mcl_eval_workspace_bytes(const int64_t *row_ptr, int64_t I, int64_t K, int32_t rank, int64_t n_models) {
    if (!ev_check(row_ptr, I, K, rank, n_models).empty()) return -1;
    return ev_plan(nullptr, row_ptr, I, K, rank, n_models).total;
}

int mcl_eval_tables_typed(const void *X, int32_t x_type, const int64_t *row_ptr, int64_t I, int64_t K, int32_t rank, const double *models,
                          int64_t n_models, double *S, double *BtB, double *sse, double *norm, void *ws, int64_t ws_bytes, void *stream) {
    ErrorSlot &fail = g_eval_error.named("mcl_eval_tables_typed: ");
    const std::string bad = ev_check(row_ptr, I, K, rank, n_models);
    if (!bad.empty()) return fail(bad);
    if (!x_type_error(x_type).empty()) return fail(x_type_error(x_type));
    if (!X || !models || !S || !BtB || !sse || !norm || !ws) return fail("NULL argument");
    const EvPlan p = ev_plan(ws, row_ptr, I, K, rank, n_models);
    if (workspace_refused(fail, ws, ws_bytes, p.total, "mcl_eval_workspace_bytes")) return 1;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const std::string inf = ev_models_finite(models, n_models, (I + row_ptr[I] + K) * rank, s);
    if (!inf.empty()) return fail(inf);
    return mcl_x_dispatch(x_type, [&](auto xl) {
        using XL = decltype(xl);
        return rank_bucket(rank, [&](auto rmax) {
            return ev_tables<XL, decltype(rmax)::value / 16>(static_cast<const typename XL::T *>(X), x_type, row_ptr, I, K, rank, models, n_models,
                                                            S, BtB, sse, norm, p, s);
        });
    });
}

int mcl_eval_core(const double *models, int64_t n_models, int64_t I, int64_t N, int64_t K, int32_t rank, const double *S, const double *BtB,
                  double *core, double *cc, double *cc_normalised, void *stream) {
    ErrorSlot &fail = g_eval_error.named("mcl_eval_core: ");
    const std::string bad = ev_check_shape(I, K, rank, n_models);
    if (!bad.empty()) return fail(bad);
    if (N < I || N >= (int64_t(1) << 31) / EV_MAX_RANK) return fail("need I <= N < 2^26 packed rows");
    if (!models || !S || !BtB || !core || !cc || !cc_normalised) return fail("NULL argument");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const long len = (long)(I + N + K) * rank;
    const std::string inf = ev_models_finite(models, n_models, len, s);
    if (!inf.empty()) return fail(inf);
    rank_bucket(rank, [&](auto rmax) {
        constexpr int RMAX = decltype(rmax)::value;
        hipLaunchKernelGGL(k_eval_core<RMAX>, dim3((unsigned)n_models), dim3(RMAX * RMAX), 0, s, models, len, (int)I, (long)N, (int)K,
                           (int)rank, S, BtB, core, cc, cc_normalised);
        return 0;
    });
    CP_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
