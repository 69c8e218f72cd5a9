// The host plumbing of the stand-alone entry points - the families that take X, row_ptr, a caller-provided workspace and a stream
// (svdinit, alsinit, parafac2als, multistart, pf2als_multistart, similarity, evaluate, projection .hip): the error slot behind a
// family's *_last_error, the shape checks of packed matrices, the workspace carver that sizes and binds a plan with one piece of
// code, the refusal of a workspace, the segment tables and their upload, the [row_ptr | row -> slab | scratch] layout of the
// one-workgroup-per-start files, and the rank-bucket / VEC dispatch.  Host code only: nothing here is __global__ or __device__.
// A new stand-alone entry point starts from these pieces.
#pragma once
#include <algorithm>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "mcl_internal.h"

// ---- errors ---------------------------------------------------------------------------------------------------------------------
// What a family's mcl_*_last_error returns.  fail(msg) stores prefix + msg and returns 1; as_is(msg) stores a message that names
// its source itself (a HIP call, another family's entry).  `ErrorSlot &fail = slot;` gives CP_HIP the `fail` it calls.
struct ErrorSlot {
    std::string prefix, text;
    int fail(const std::string &msg) { return as_is(prefix + msg); }
    int as_is(const std::string &msg) {
        text = msg;
        return 1;
    }
    int operator()(const std::string &msg) { return fail(msg); }
    ErrorSlot &named(const char *entry) {  // the slot under the prefix of one of the family's entries
        prefix = entry;
        return *this;
    }
    const char *c_str() const { return text.c_str(); }
};

// returns fail(message) from the enclosing function (a `fail` in scope) when a HIP call does not succeed
#define CP_HIP(expr)                                                                    \
    do {                                                                                \
        const hipError_t e_ = (expr);                                                   \
        if (e_ != hipSuccess) return fail(std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

// "" for a known element type of X, else the message the entry points report after their own name
static inline std::string x_type_error(int32_t x_type) {
    if (x_type == MCL_X_F32 || x_type == MCL_X_BF16 || x_type == MCL_X_F16) return "";
    return "unknown x_type " + std::to_string(x_type) + " (MCL_X_F32 = 0, MCL_X_BF16 = 1, MCL_X_F16 = 2)";
}

// ---- the shape of packed matrices: "" or the message ------------------------------------------------------------------------------
static inline std::string packed_args_error(const int64_t *row_ptr, int64_t I, int64_t K, int32_t rank, int max_rank) {
    if (!row_ptr || I < 1 || K < 1) return "need row_ptr, I >= 1, K >= 1";
    if (rank < 1 || rank > max_rank) return "need 1 <= rank <= " + std::to_string(max_rank);
    return "";
}
// ... of matrices that each hold `rank` rows or more (an orthonormal P_i exists), fewer than 2^log2_rows packed rows in all
static inline std::string packed_rows_error(const int64_t *row_ptr, int64_t I, int64_t K, int32_t rank, int log2_rows) {
    if (row_ptr[0] != 0) return "row_ptr[0] must be 0";
    for (int64_t i = 0; i < I; ++i)
        if (row_ptr[i + 1] - row_ptr[i] < rank) return "every matrix needs at least rank rows";
    if (rank > K) return "rank exceeds K";
    if (row_ptr[I] >= int64_t(1) << log2_rows) return "more than 2^" + std::to_string(log2_rows) + " packed rows are not supported";
    return "";
}

// ---- the workspace ----------------------------------------------------------------------------------------------------------------
// The parts of a workspace in order: every part starts on a 256-byte boundary and has at least one byte.  A family's plan is
// filled by ONE function that takes its parts from a cursor: without a base the parts are null and `off` ends as the size
// (*_workspace_bytes), with the caller's workspace they are the pointers of the run.
struct WsCursor {
    char *base;
    int64_t off = 0;
    explicit WsCursor(void *workspace = nullptr) : base(static_cast<char *>(workspace)) {}
    template <class T>
    T *at() const {
        return base ? reinterpret_cast<T *>(base + off) : nullptr;
    }
    template <class T>
    T *take(int64_t bytes) {
        T *p = at<T>();
        off = (off + std::max<int64_t>(bytes, 1) + 255) & ~int64_t(255);
        return p;
    }
};

// true, after fail(the message), when the caller's workspace does not serve a plan of `need` bytes (sizer: the function that
// returns `need`; NULL for an entry without a size argument, which checks the alignment alone)
template <class Fail>
static inline bool workspace_refused(Fail &&fail, const void *workspace, int64_t bytes, int64_t need, const char *sizer) {
    if (sizer && bytes < need) return fail(std::string("workspace too small (") + sizer + ")") != 0;
    if (reinterpret_cast<uintptr_t>(workspace) & 255) return fail("workspace must be 256-byte aligned") != 0;
    return false;
}

// ---- the tables the X passes walk ---------------------------------------------------------------------------------------------------
constexpr int CP_SEG = 64;  // rows of one slab per segment (one wave of pass 1)

// segs = {slab, first packed row, rows, first row in slab} per segment of <= CP_SEG rows, the segments of slab i =
// [slab_seg[i], slab_seg[i + 1]), ext = row_ptr as int
struct SegTables {
    std::vector<int4> segs;
    std::vector<int> slab_seg, ext;
};
static inline SegTables seg_tables(const int64_t *row_ptr, int64_t I) {
    SegTables t;
    t.slab_seg.assign(1, 0);
    t.ext.resize((size_t)I + 1);
    for (int64_t i = 0; i < I; ++i) {
        const int J = (int)(row_ptr[i + 1] - row_ptr[i]);
        for (int j0 = 0; j0 < J; j0 += CP_SEG) t.segs.push_back(int4{(int)i, (int)row_ptr[i] + j0, std::min(CP_SEG, J - j0), j0});
        t.slab_seg.push_back((int)t.segs.size());
    }
    for (int64_t i = 0; i <= I; ++i) t.ext[(size_t)i] = (int)row_ptr[i];
    return t;
}
static inline int64_t seg_count(const int64_t *row_ptr, int64_t I) {
    int64_t nseg = 0;
    for (int64_t i = 0; i < I; ++i) nseg += (row_ptr[i + 1] - row_ptr[i] + CP_SEG - 1) / CP_SEG;
    return nseg;
}

// Host tables into their places in the workspace: the copies are enqueued, in the order segs, slab_seg, ext (a null place:
// the family has no such part), and NOT waited for.  The sources are the caller's locals: it enqueues what else the call
// uploads and then synchronises the stream once.
template <class T>
static inline hipError_t upload(T *dst, const std::vector<T> &src, hipStream_t s) {
    return hipMemcpyAsync(dst, src.data(), sizeof(T) * src.size(), hipMemcpyHostToDevice, s);
}
static inline hipError_t upload_tables(const SegTables &t, int4 *segs, int *slab_seg, int *ext, hipStream_t s) {
    hipError_t e = hipSuccess;
    if (segs) e = upload(segs, t.segs, s);
    if (slab_seg && e == hipSuccess) e = upload(slab_seg, t.slab_seg, s);
    if (ext && e == hipSuccess) e = upload(ext, t.ext, s);
    return e;
}

// ---- one workgroup per start: [row_ptr | row -> slab | scratch x n_starts] ---------------------------------------------------------
struct StartsPlan {
    int64_t N, total;
    int64_t *row_ptr;
    int32_t *slab_of_row;
    double *scratch;  // scratch_len doubles per start
};
static inline StartsPlan starts_plan(void *workspace, const int64_t *row_ptr, int64_t I, int64_t scratch_len, int32_t n_starts) {
    StartsPlan p{};
    WsCursor ws(workspace);
    p.N = row_ptr[I];
    p.row_ptr = ws.take<int64_t>((I + 1) * 8);
    p.slab_of_row = p.N ? ws.take<int32_t>(p.N * 4) : ws.at<int32_t>();  // (no rows: no bytes)
    p.scratch = ws.take<double>(scratch_len * 8 * int64_t(n_starts));
    p.total = ws.off;
    return p;
}
// row_ptr and the row -> slab map, built in the caller's `slab`, enqueued like upload_tables
static inline hipError_t upload_starts(const StartsPlan &p, const int64_t *row_ptr, int64_t I, std::vector<int32_t> &slab, hipStream_t s) {
    slab.resize((size_t)p.N);
    for (int64_t i = 0; i < I; ++i)
        for (int64_t j = row_ptr[i]; j < row_ptr[i + 1]; ++j) slab[(size_t)j] = (int32_t)i;
    const hipError_t e = hipMemcpyAsync(p.row_ptr, row_ptr, (I + 1) * 8, hipMemcpyHostToDevice, s);
    return e != hipSuccess || !p.N ? e : upload(p.slab_of_row, slab, s);
}

// ---- which instantiation serves a call ----------------------------------------------------------------------------------------------
// f(std::integral_constant<int, RMAX>): RMAX = 16 for rank <= 16, else 32
template <class F>
static inline auto rank_bucket(int rank, F &&f) {
    return rank <= 16 ? f(std::integral_constant<int, 16>{}) : f(std::integral_constant<int, 32>{});
}
// f(std::integral_constant<int, R>) for R = rank, 1 <= rank <= RANKS; no call for another rank.  (From RANKS down: the
// compiler emits what f instantiates in the reverse of this order, so the kernels of a file come out by ascending rank.)
template <int RANKS, class F, int... D>
static inline void rank_exact(int rank, F &&f, std::integer_sequence<int, D...>) {
    ((rank == RANKS - D ? (void)f(std::integral_constant<int, RANKS - D>{}) : (void)0), ...);
}
template <int RANKS, class F>
static inline void rank_exact(int rank, F &&f) {
    rank_exact<RANKS>(rank, f, std::make_integer_sequence<int, RANKS>{});
}
// f(std::bool_constant<VEC>): VEC when K % 4 == 0 and X is aligned for its element type's four-element loads
template <class F>
static inline auto vec_dispatch(bool vec, F &&f) {
    return vec ? f(std::true_type{}) : f(std::false_type{});
}
