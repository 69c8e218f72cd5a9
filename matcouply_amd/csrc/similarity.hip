// factor_match_score / multistart_similarity (matcouply_amd/similarity.py): the factor match score of many
// pairs of fitted models in one launch.
//
// A model is [A; B; C] row-major, (I + N + K) x r fp64, the layout of the first part of a multi-start state slice.  Two kernels:
//   k_fms_norms  one wave per model: the column sums of squares of every mode, 1 / norm (0 for a zero column) and
//                w = weights * prod_modes norm, into the workspace;
//   k_fms_pairs  one wave per pair: F_lo^T F_hi of every mode that is not skipped on the fp64 matrix core
//                (v_mfma_f64_16x16x4_f64: r padded to 16 with zero columns, four rows per instruction, the last group
//                zero-filled), scaled by the norms, multiplied over the modes and by the weight factor, |.|; the r x r matrix
//                goes to LDS and an exact assignment solver (shortest augmenting paths with potentials, the Hungarian method
//                in O(r^3)) runs on it in the same wave: columns on the lanes, minima by lane shuffles.
//
// Numerics: fp64 throughout.  No atomics; every sum runs in an order that depends only on the shape (I, N, K, r), so a pair's
// score and permutation are bitwise independent of which other pairs share the launch.  A pair (s, t) is always computed as
// (lo, hi) = (min, max): score(s, t) and score(t, s) are then the same bits, and the permutation of the swapped pair is the
// inverse one.  A zero column has 1 / norm = 0, hence congruence 0 with every column and never a NaN.
//
// Where r <= 8 a wave could hold two pairs in one 16-wide operand; it does not: a pair is 45 matrix instructions at the examples'
// size, and the all-pairs matrix of 1024 models is bound by the solver, not by them.
#include <cmath>
#include <string>

#include "entry_host.h"
#include "mcl_internal.h"

namespace {

static ErrorSlot g_fms_error{"mcl_fms_scores: "};
constexpr int FMS_MAX_RANK = 16;
constexpr int FMS_WS_DOUBLES = 64;  // per model: inv_norm[3][16], w[16]
constexpr int FMS_WAVES = 4;        // pairs per workgroup
typedef double fms_f64x4 __attribute__((ext_vector_type(4)));

struct FmsArgs {
    const double *models;
    const double *weights;
    double *ws;
    double *score;  // in: the pair (two int32) in the bytes of every entry; out: the score
    int32_t *perm;
    int64_t n_models, n_pairs;
    int64_t rows[3];  // I, N, K
    int r, flags, skip_mode;
};

__global__ __launch_bounds__(64 * FMS_WAVES) void k_fms_norms(FmsArgs a) {
    const int lane = threadIdx.x & 63, q = lane >> 4, c = lane & 15;
    const int64_t model = (int64_t)blockIdx.x * FMS_WAVES + (threadIdx.x >> 6);
    if (model >= a.n_models) return;
    const int r = a.r;
    const int64_t len = (a.rows[0] + a.rows[1] + a.rows[2]) * r;
    const double *F = a.models + model * len;
    double *out = a.ws + model * FMS_WS_DOUBLES;
    double prod = 1.0;
    for (int m = 0; m < 3; ++m) {
        // lane (q, c) sums the rows q, q + 4, ... of column c; the four partial sums are then added as (0 + 1) + (2 + 3)
        double ss = 0.0;
        if (c < r)
            for (int64_t row = q; row < a.rows[m]; row += 4) {
                const double x = F[row * r + c];
                ss = fma(x, x, ss);
            }
        ss += __shfl_xor(ss, 16);
        ss += __shfl_xor(ss, 32);
        const double norm = sqrt(ss);
        if (q == 0) out[16 * m + c] = norm > 0.0 ? 1.0 / norm : 0.0;
        prod *= norm;
        F += a.rows[m] * r;
    }
    if (q == 0) out[48 + c] = c < r ? (a.weights ? a.weights[model * r + c] : 1.0) * prod : 0.0;
}

// lexicographic minimum of (value, index) over the 16 lanes of a quarter wave (all four quarters hold the same data)
static __device__ __forceinline__ void fms_argmin16(double &val, int &idx) {
#pragma unroll
    for (int d = 1; d < 16; d <<= 1) {
        const double ov = __shfl_xor(val, d);
        const int oi = __shfl_xor(idx, d);
        if (ov < val || (ov == val && oi < idx)) val = ov, idx = oi;
    }
}

__global__ __launch_bounds__(64 * FMS_WAVES) void k_fms_pairs(FmsArgs a) {
    __shared__ double Ms[FMS_WAVES][16 * 16];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, q = lane >> 4, c = lane & 15;
    const int r = a.r;
    const int64_t pair = (int64_t)blockIdx.x * FMS_WAVES + wave;
    const bool live = pair < a.n_pairs;
    int s = 0, t = 0;
    if (live) {
        const int2 st = reinterpret_cast<const int2 *>(a.score)[pair];
        s = st.x, t = st.y;
    }
    const bool swapped = s > t;
    const int64_t lo = swapped ? t : s, hi = swapped ? s : t;
    const int64_t len = (a.rows[0] + a.rows[1] + a.rows[2]) * r;
    const double *Fl = a.models + lo * len, *Fh = a.models + hi * len;
    const double *wl = a.ws + lo * FMS_WS_DOUBLES, *wh = a.ws + hi * FMS_WS_DOUBLES;

    // M[p][col] for p = q + 4 v (D layout of the f64 MFMA: col = lane & 15, row = (lane >> 4) + 4 reg)
    double val[4] = {1.0, 1.0, 1.0, 1.0};
    for (int m = 0; m < 3; ++m) {
        const int64_t R = a.rows[m];
        if (m != a.skip_mode) {
            fms_f64x4 acc = {0.0, 0.0, 0.0, 0.0};
            for (int64_t row0 = 0; row0 < R; row0 += 4) {
                const int64_t row = row0 + q;
                const bool in = row < R && c < r;  // the last partial group and the padding columns are zeros, not reads
                const double x = in ? Fl[row * r + c] : 0.0;
                const double y = in ? Fh[row * r + c] : 0.0;
                acc = __builtin_amdgcn_mfma_f64_16x16x4f64(x, y, acc, 0, 0, 0);
            }
            const double ih = wh[16 * m + c];
#pragma unroll
            for (int v = 0; v < 4; ++v) val[v] *= acc[v] * (wl[16 * m + q + 4 * v] * ih);
        }
        Fl += R * r, Fh += R * r;
    }
    const double w2 = wh[48 + c];
#pragma unroll
    for (int v = 0; v < 4; ++v) {
        double x = val[v];
        if (a.flags & 1) {
            const double w1 = wl[48 + q + 4 * v];
            x *= (w1 == 0.0 && w2 == 0.0) ? 1.0 : 1.0 - fabs(w1 - w2) / fmax(w1, w2);
        }
        if (a.flags & 2) x = fabs(x);
        Ms[wave][16 * (q + 4 * v) + c] = x;
    }
    __syncthreads();  // the only barrier: every wave reaches it, the solver below reads its own wave's matrix only
    if (!live) return;
    const double *M = Ms[wave];

    // Assignment that maximises sum_p M[p][perm[p]]: shortest augmenting paths on the cost -M with the potentials u (rows) and
    // v (columns).  Lane c is column c and, for u and `row_seen`, row c.  Every loop is bounded by r, so a matrix with a NaN (a
    // non-finite input the caller did not refuse) ends with a wrong answer, not with a hang.
    const double INF = __builtin_huge_val();
    double u = 0.0, vc = 0.0;
    int pcol = -1;  // the row matched to column c
    int way = -1;
    for (int i = 0; i < r; ++i) {
        double minv = INF;
        bool used = false, row_seen = false;
        int j0 = -1, i0 = i;  // column -1: the virtual column that holds the new row i
        for (int it = 0; it <= r; ++it) {
            if (c == j0) used = true;
            if (c == i0) row_seen = true;
            const double ui0 = __shfl(u, i0);
            const bool open = !used && c < r;
            if (open) {
                const double cur = -M[16 * i0 + c] - ui0 - vc;
                if (cur < minv) minv = cur, way = j0;
            }
            double delta = open ? minv : INF;
            int j1 = c;
            fms_argmin16(delta, j1);
            if (row_seen) u += delta;
            if (used) vc -= delta;
            else minv -= delta;
            j0 = j1;
            i0 = __shfl(pcol, j0);
            if (i0 < 0) break;
        }
        for (int it = 0; it <= r && j0 >= 0; ++it) {  // flip the path back to the virtual column
            const int j1 = __shfl(way, j0);
            const int row = j1 >= 0 ? __shfl(pcol, j1) : i;
            if (c == j0) pcol = row;
            j0 = j1;
        }
    }
    // the column of row c, then the mean of the r chosen entries
    int rcol = 0;
    for (int cc = 0; cc < r; ++cc)
        if (__shfl(pcol, cc) == c) rcol = cc;
    const double mine = c < r ? M[16 * c + rcol] : 0.0;
    // summed from the largest entry down, not in row order: the transposed problem (the two models in the other order, in
    // another call) chooses the same entries and so gives the same bits
    int pos = 0;
    for (int j = 0; j < r; ++j) {
        const double other = __shfl(mine, j);
        pos += other > mine || (other == mine && j < c);
    }
    int src = 0;
    for (int j = 0; j < r; ++j)
        if (__shfl(pos, j) == c) src = j;
    const double sorted = __shfl(mine, src);
    double sum = 0.0;
    for (int p = 0; p < r; ++p) sum += __shfl(sorted, p);
    if (lane == 0) a.score[pair] = sum / r;
    if (a.perm && lane < r) a.perm[pair * r + lane] = swapped ? pcol : rcol;
}

std::string fms_check(int64_t n_models, int32_t rank) {
    if (rank < 1 || rank > FMS_MAX_RANK) return "rank " + std::to_string(rank) + " is outside 1 ... " + std::to_string(FMS_MAX_RANK);
    if (n_models < 1 || n_models >= (int64_t(1) << 31)) return "n_models " + std::to_string(n_models) + " is outside 1 ... 2^31 - 1";
    return "";
}

}  // namespace

extern "C" {

const char *mcl_fms_last_error(void) { return g_fms_error.c_str(); }

int64_t mcl_fms_workspace_bytes(int64_t n_models, int32_t rank) {
    if (!fms_check(n_models, rank).empty()) return -1;
    return n_models * FMS_WS_DOUBLES * 8;
}

int mcl_fms_scores(const double *models, int64_t n_models, int64_t I, int64_t N, int64_t K, int32_t rank, const double *weights,
                   const int32_t *pairs, int64_t n_pairs, int32_t flags, int32_t skip_mode, double *score, int32_t *perm,
                   void *workspace, void *hip_stream) {
    ErrorSlot &fail = g_fms_error;
    const std::string bad = fms_check(n_models, rank);
    if (!bad.empty()) return fail(bad);
    if (I < 1 || N < 1 || K < 1) return fail("need I >= 1, N >= 1 and K >= 1");
    if ((I + N + K) >= (int64_t(1) << 31) / rank) return fail("a model of (I + N + K) * rank >= 2^31 elements");
    if (n_pairs < 0 || n_pairs >= (int64_t(1) << 31) * FMS_WAVES) return fail("n_pairs " + std::to_string(n_pairs) + " is out of range");
    if (flags & ~3) return fail("flags may hold bit 0 (consider_weights) and bit 1 (absolute_value) only");
    if (skip_mode < -1 || skip_mode > 2) return fail("skip_mode must be -1 (none), 0, 1 or 2");
    if (!models || !workspace || (n_pairs > 0 && (!pairs || !score))) return fail("NULL argument");
    if (workspace_refused(fail, workspace, 0, 0, nullptr)) return 1;  // (no size argument: mcl_fms_workspace_bytes(n_models, rank))
    for (int64_t i = 0; i < 2 * n_pairs; ++i)
        if (pairs[i] < 0 || pairs[i] >= n_models)
            return fail("pair " + std::to_string(i / 2) + " names model " + std::to_string(pairs[i]) + " of " + std::to_string(n_models));
    if (n_pairs == 0) return 0;
    hipStream_t s = reinterpret_cast<hipStream_t>(hip_stream);
    // a pair is two int32, a score one double: the pairs travel in the score buffer, and a wave reads its pair before it writes
    // its score
    if (hipMemcpyAsync(score, pairs, n_pairs * 8, hipMemcpyHostToDevice, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
        return fail("upload of the pairs failed");
    FmsArgs a{};
    a.models = models, a.weights = weights, a.ws = static_cast<double *>(workspace), a.score = score, a.perm = perm;
    a.n_models = n_models, a.n_pairs = n_pairs;
    a.rows[0] = I, a.rows[1] = N, a.rows[2] = K;
    a.r = rank, a.flags = flags, a.skip_mode = skip_mode;
    hipLaunchKernelGGL(k_fms_norms, dim3((unsigned)((n_models + FMS_WAVES - 1) / FMS_WAVES)), dim3(64 * FMS_WAVES), 0, s, a);
    hipLaunchKernelGGL(k_fms_pairs, dim3((unsigned)((n_pairs + FMS_WAVES - 1) / FMS_WAVES)), dim3(64 * FMS_WAVES), 0, s, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(std::string("launch failed: ") + hipGetErrorString(e));
    return 0;
}

}  // extern "C"
