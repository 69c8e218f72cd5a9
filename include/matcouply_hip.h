/*
 * matcouply_hip.h - C ABI of the MI355X-native AO-ADMM engine (libmatcouply_hip.so).
 *
 * The reference (MarieRoald/matcouply) is pure Python and has no FFI: its "operator interface" for the
 * hot path is the set of Python functions in src/matcouply/decomposition.py.  Each entry point below
 * replaces one of them; the Python front end `matcouply_amd` (and any other host)
 * binds these symbols with ctypes.  Plain pointers and sizes only - no torch/NumPy types cross the ABI.
 *
 * Conventions
 *   - every function returns 0 on success, non-zero on error; mcl_last_error() gives the message;
 *   - the caller owns EVERY buffer (data, factors, aux/dual variables, workspace); the library never
 *     allocates device memory and never synchronises the stream, except where stated;
 *   - all device work is enqueued on the HIP stream given to mcl_create();
 *   - one context per (device, stream); a context is not thread-safe;
 *   - all matrices are row-major fp32; the I coupled matrices X_i (J_i x K) and every B-mode variable are
 *     PACKED along rows: X[sum J_i, K], B[sum J_i, r], slab i = rows row_ptr[i] .. row_ptr[i+1].
 */
#ifndef MATCOUPLY_HIP_H
#define MATCOUPLY_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mcl_context mcl_context;

/* ABI version = what mcl_version() of a matching library returns.  History: 100 first release (fp32 [G | R]);
 * 200 mcl_c_normal_equations returns fp64 (the buffer a multi-GPU host all-reduces changed its element size);
 * 300 mcl_run and the stop-rule structs, the communication-buffer and event entry points;
 * 400 this header: named indices (enum mcl_buffer_id, enum mcl_profile_slot, MCL_VARIANT_EXACT_MODE - the exact-mode query
 *     moved from index 4 to 100), twelve profile slots, mcl_profile_launches, a failed state after mcl_run's watchdog,
 *     mcl_options.inner_tol / exact_products, native GeneralizedL2 / UnitSimplex kinds (mcl_penalty_desc grew two fields),
 *     mcl_penalty_value, mcl_svd_init;
 * 410 mcl_condition_probe, mcl_condition_monitor, mcl_read_bandwidth (nothing else changed).
 *     410 also gained, purely additively, mcl_set_problem_typed and mcl_svd_init_typed (16-bit X, enum mcl_x_type):
 *     the version stays 410; a host detects the capability by the presence of the symbols.
 * A host MUST compare mcl_version() with the MCL_ABI_VERSION it was built against before any other call. */
#define MCL_ABI_VERSION 410

#define MCL_MAX_REGS 4   /* penalties per mode */
#define MCL_MAX_RANK 64

/* Proximal operators with a native kernel (reference: src/matcouply/penalties.py). */
enum mcl_penalty_kind {
    MCL_PEN_NN = 1,       /* NonNegativity   penalties.py:488-508  */
    MCL_PEN_BOX = 2,      /* Box             penalties.py:511-542  */
    MCL_PEN_L1 = 3,       /* L1Penalty       penalties.py:545-592  */
    MCL_PEN_L2BALL = 4,   /* L2Ball          penalties.py:844-925  */
    MCL_PEN_UNIMODAL = 5, /* Unimodality     penalties.py:983-1015 */
    MCL_PEN_PARAFAC2 = 6, /* Parafac2        penalties.py:1018-1324 (mode 1 only) */
    MCL_PEN_EXTERNAL = 7, /* user prox evaluated by the host between mcl_*_solve and mcl_*_dual */
    MCL_PEN_TV = 8,       /* TotalVariationPenalty  penalties.py:750-841: p0 = TV strength, p1 = L1 strength; the prox
                             (condat_tv.tv_denoise_matrix in the reference) is L. Condat's direct 1-D TV algorithm */
    MCL_PEN_GL2 = 9,      /* GeneralizedL2Penalty   penalties.py:595-747: x^T M x per column, M = U diag(s) U^T given through
                             `matrix` (eigenvectors, then eigenvalues); every matrix of the mode has matrix_rows rows */
    MCL_PEN_SIMPLEX = 10  /* UnitSimplex            penalties.py:928-980: columns non-negative and summing to one */
};

typedef struct {
    int32_t kind;           /* enum mcl_penalty_kind */
    int32_t non_negativity; /* L1 / L2Ball / Unimodality: also clip at 0 */
    double p0;              /* Box: min_val; L1: reg_strength; L2Ball: norm_bound */
    double p1;              /* Box: max_val */
    float *aux;             /* [rows, r] auxiliary variable; PARAFAC2: packed orthogonal bases P_i */
    float *dual;            /* [rows, r] scaled dual variable */
    float *aux2;            /* PARAFAC2: coordinate matrix Delta [r, r]; otherwise NULL */
    const double *matrix;   /* GeneralizedL2: device fp64 [n * n + n]: U (row-major, columns = eigenvectors of M), then the n
                               eigenvalues s (M = U diag(s) U^T, penalties.py:720); otherwise NULL */
    int64_t matrix_rows;    /* GeneralizedL2: n = rows of every factor matrix of the mode */
} mcl_penalty_desc;

typedef struct {
    double feasibility_penalty_scale; /* decomposition.py:678 */
    double l2_penalty[3];             /* per mode; None -> 0 (decomposition.py:876-877) */
    double inner_tol;                 /* decomposition.py:90-117: > 0 ends the inner ADMM loop of a phase early - after an inner
                                         iteration with ||x - x_old|| <= inner_tol ||x|| and every feasibility gap of the mode
                                         below inner_tol.  Evaluated ON THE DEVICE (a flag the remaining inner launches test);
                                         the phases then take one launch per step instead of their fused kernels.  0: not set */
    int32_t inner_n_iter_max;         /* decomposition.py:689 */
    int32_t constant_A;               /* constant_feasibility_penalty for mode 0 (decomposition.py:937-939) */
    int32_t constant_B;               /* ... for mode 1 (decomposition.py:940-942) */
    int32_t exact_products;           /* 0: the library decides by THIS context's size (exact-products mode up to 2^20 elements
                                         of X); 1 / 2: force the mode on / off - a host that shards one problem over several
                                         contexts decides by the size of the WHOLE problem, so that every rank (and every
                                         rank layout) computes with the same arithmetic.  Looked at by mcl_set_workspace. */
} mcl_options;

/* Layout of the fp64 vector written by mcl_diagnostics(). */
#define MCL_DIAG_NORM_SQ 0     /* [3] ||A||^2, ||B||^2, ||C||^2 */
#define MCL_DIAG_INNER 3       /* <X, M>  = sum_i rhs_i . a_i            (decomposition.py:448) */
#define MCL_DIAG_MODEL_SQ 4    /* ||M||^2 = sum_i a_i^T Q_i a_i          (decomposition.py:449) */
#define MCL_DIAG_X_SQ 5        /* ||X||^2 of this context's slabs        (decomposition.py:906) */
#define MCL_DIAG_REG 8         /* + (mode*MCL_MAX_REGS + k)*2 : {||aux - factor||^2, sum |factor|} */
#define MCL_DIAG_LEN (8 + 3 * MCL_MAX_REGS * 2)

/* ---- life cycle ------------------------------------------------------------------------------------ */
int mcl_create(mcl_context **out, int device, void *hip_stream);
void mcl_destroy(mcl_context *ctx);
const char *mcl_last_error(const mcl_context *ctx); /* ctx may be NULL: last mcl_create() failure */
int mcl_version(void);

/* ---- problem definition (replaces the `matrices`, `rank` arguments of cmf_aoadmm, decomposition.py:662) */
/* X: device [row_ptr[I], K]; row_ptr: HOST int64[I+1], non-decreasing, row_ptr[0] = 0. */
int mcl_set_problem(mcl_context *ctx, const float *X, const int64_t *row_ptr, int64_t I, int64_t K, int32_t rank);
/* Element type of X.  A 16-bit X stays 16-bit in device memory; every kernel converts its elements exactly to fp32 on
 * load, so a run on 16-bit X gives bit for bit the results of the fp32 run on the upcast matrix. */
enum mcl_x_type { MCL_X_F32 = 0, MCL_X_BF16 = 1, MCL_X_F16 = 2 };
/* mcl_set_problem for X of element type x_type (mcl_x_type).  A 16-bit X must be 8-byte aligned (fp32: no requirement;
 * the vectorised kernels take it when it is 16-byte aligned); the kernels pick the same variants as for fp32 X of the same
 * shape.  mcl_set_problem(..) is mcl_set_problem_typed(.., MCL_X_F32, ..). */
int mcl_set_problem_typed(mcl_context *ctx, const void *X, int32_t x_type, const int64_t *row_ptr, int64_t I, int64_t K, int32_t rank);
int mcl_set_options(mcl_context *ctx, const mcl_options *opt);
/* Factors of the CMF (decomposition.py:133,235,307): A [I, r], B packed [sum J_i, r], C [K, r]; updated in place. */
int mcl_set_factors(mcl_context *ctx, float *A, float *B, float *C);
/* Penalty list of one mode, in the order of decomposition.py:571-612; descs are copied. */
int mcl_set_penalties(mcl_context *ctx, int32_t mode, int32_t n, const mcl_penalty_desc *descs);
/* Scratch memory: call after the four setters above; bytes needed for the current problem. */
int64_t mcl_workspace_bytes(mcl_context *ctx);
int mcl_set_workspace(mcl_context *ctx, void *workspace, int64_t bytes);

/* ---- phase calls: one per reference function -------------------------------------------------------- */
/* admm_update_B (decomposition.py:222-292) */
int mcl_update_B(mcl_context *ctx);
/* admm_update_C (decomposition.py:295-344), split at the cross-slab reduction so that a multi-GPU host can
 * all-reduce the normal equations:  local -> [all-reduce over ranks of mcl_c_normal_equations()] -> finish. */
int mcl_update_C_local(mcl_context *ctx);
double *mcl_c_normal_equations(mcl_context *ctx, int64_t *count); /* device [G (r x r) | R (K x r)], fp64 */
int mcl_update_C_finish(mcl_context *ctx);
/* admm_update_A (decomposition.py:120-219); also leaves (rhses, cross_products) for the fast error formula. */
int mcl_update_A(mcl_context *ctx);
/* compute_feasibility_gaps + _cmf_reconstruction_error + penalty sums (decomposition.py:351-452, 916-921):
 * writes MCL_DIAG_LEN fp64 partial sums of THIS context's slabs to device memory `out`.
 * include_replicated = 0 leaves the C-mode entries (identical on every rank) at zero so that a SUM all-reduce
 * over ranks is exact.  If no A-phase by-products are current, they are recomputed with a pass over X
 * (decomposition.py:430-444). */
int mcl_diagnostics(mcl_context *ctx, double *out, int32_t include_replicated);
/* mcl_diagnostics whose table reduction MAY be issued later: when the next calls on this context are mcl_update_B and
 * mcl_update_C_local on the one-pass path, it rides on a spare workgroup of the C-phase reduction kernel instead of a launch
 * of its own (the per-iteration pattern B -> C_local -> [all-reduce] -> C_finish -> A -> diagnostics of a fixed-count loop).
 * `out` is written at the latest when ANY other entry point of the context, or mcl_flush_diagnostics(), has been called;
 * the factors / tables it reports are those at the time of THIS call.  Same values as mcl_diagnostics up to the association
 * of the fp64 sums. */
int mcl_diagnostics_deferred(mcl_context *ctx, double *out, int32_t include_replicated);
int mcl_flush_diagnostics(mcl_context *ctx);
/* Value of penalty k of `mode` on the current factor, for the kinds whose value is not a column of the diagnostics vector:
 * GeneralizedL2 - sum over the mode's matrices of trace(F^T M F) (penalties.py:737-745).  One fp64 to device memory `out`. */
int mcl_penalty_value(mcl_context *ctx, int32_t mode, int32_t k, double *out);
/* Condition estimates of the r x r normal equations the PENALTY-FREE modes among `mode_mask` (bit m = mode m) would solve from
 * the CURRENT factors - the systems the reference solves with an fp64 SVD (decomposition.py:155-172 mode 0, :240-256 mode 1,
 * :312-321 mode 2; l2_penalty included): out[m] = ||M||_F ||M^-1||_F (between cond_2 and r cond_2; modes 0 / 1: the largest
 * over the matrices; 1e300: singular), 0 for a mode that has penalties or is not in the mask.  Computed from the factors alone
 * (fp64 Gram matrices of the B_i, no pass over X), three fp64 to DEVICE memory `out`, enqueued like everything else.  The
 * fp32 kernels leave 1e-8 .. 4e-7 relative in what such a solve sees and the solve multiplies it by this number: a host that
 * wants the reference's results on an ill-conditioned penalty-free mode switches to mcl_options.exact_products = 1 when the
 * estimate is large (matcouply_amd does so between 2^20 and 2^24 elements of X above 1e3, and warns beyond). */
int mcl_condition_probe(mcl_context *ctx, int32_t mode_mask, double *out);
/* The same estimate taken WHERE IT MATTERS: the phases are Gauss-Seidel - the A-phase of an iteration solves systems built
 * from the B_i and C of the same iteration - so the numbers that count are those at the start of each phase.  While a monitor is
 * installed (out != NULL: device fp64[4], zeroed by the caller), every phase of a penalty-free mode in `mode_mask` (mcl_update_B,
 * mcl_update_C_local, mcl_update_A / mcl_A_begin) first launches the probe for ITS system and keeps the running maximum in
 * out[mode]; out[3] collects the worst conditioning of the PARAFAC2 polar factors (~ ||sigma|| / sigma_min of Y_i Delta^T,
 * penalties.py:1233-1235; 1e8 for a matrix the Newton-Schulz route had to hand on) of every inner iteration, for ranks <= 32;
 * out = NULL removes it.  Two small launches per monitored phase: meant for a short trial (matcouply_amd runs two
 * iterations under the monitor, restores the initial state and then chooses the arithmetic) and for an occasional check. */
int mcl_condition_monitor(mcl_context *ctx, double *out, int32_t mode_mask);
/* n outer iterations B -> C -> A on ONE device (decomposition.py:945-988); if diag_ring != NULL,
 * MCL_DIAG_LEN doubles are appended per iteration (device memory, n * MCL_DIAG_LEN doubles). */
int mcl_iterate(mcl_context *ctx, int32_t n_iter, int32_t update_A, int32_t update_B, int32_t update_C,
                double *diag_ring);

/* The outer loop WITH its stopping rule on one device (decomposition.py:945-1053): the reduction of the diagnostics and
 * the stopping test (feasibility gaps :996, relative / absolute loss criterion :1037-1053, quirks Q8-Q10 of SURVEY.md
 * Appendix C kept) run in a kernel at the end of every iteration; the host enqueues up to max_run_ahead iterations
 * ahead of the verdicts it has seen and never waits for one.  Every kernel that writes a factor or an ADMM variable tests
 * the device-side stop flag first, so when the call returns the factors and ADMM variables are EXACTLY those of the
 * stopping iteration, however far the host had run ahead.
 *   rule          Python truthiness is kept: a tolerance of 0 means "not set" (None / 0 / False of the reference);
 *   diag_ring     device fp64 [n_iter_max, MCL_DIAG_LEN]: row `it` = the mcl_diagnostics vector after iteration `it`;
 *   verdict_ring  device fp64 [n_iter_max, 4]: {relative reconstruction error, regularised loss, worst feasibility gap,
 *                 flags: bit 0 feasible, bit 1 error / loss evaluated (Q10), bits 2.. stop code}; rows beyond the stopping
 *                 iteration are not written;
 *   status        int32[4] in PINNED host memory (hipHostMalloc / a registered buffer): written by the device.
 * Unlike every other entry point this one synchronises the stream before it returns (it reports the verdict).
 * Watchdog: a device that reports no verdict for MCL_RUN_WATCHDOG_S seconds (default 120) ends the call with an error and
 * WITHOUT that synchronisation (a wedged stream would block it forever).  The context is then FAILED: every later entry
 * point but mcl_last_error / mcl_destroy returns an error, and the caller must keep the workspace, both rings and `status`
 * allocated until it has synchronised or reset the device itself (kernels that refer to them may still be enqueued). */
typedef struct {
    double tol;                 /* relative loss criterion, decomposition.py:1039; 0 = not set */
    double absolute_tol;        /* decomposition.py:1040; only looked at when tol is set (Q8); tests the newest loss (Q9) */
    double feasibility_tol;     /* decomposition.py:996; 0 = not set: the feasibility criterion then never holds */
    double initial_loss;        /* losses[0]: regularised loss of the initial state (decomposition.py:916-921) */
    double penalty_weight[3][MCL_MAX_REGS]; /* loss += weight * sum |factor|: reg_strength of an L1Penalty, else 0 */
    int32_t evaluate_loss_always; /* return_errors of the reference: the loss is evaluated on infeasible iterates too (Q10) */
    int32_t max_run_ahead;      /* iterations the host may enqueue beyond the newest verdict it has seen; <= 0: 8 */
} mcl_stop_rule;
#define MCL_STOP_RELATIVE 1     /* "FEASIBILITY GAP CRITERION AND RELATIVE LOSS CRITERION SATISFIED" */
#define MCL_STOP_ABSOLUTE 2     /* "FEASIBILITY GAP CRITERION AND ABSOLUTE LOSS CRITERION SATISFIED" */
typedef struct {
    volatile int32_t stopped;         /* 1 once a criterion has fired */
    volatile int32_t stop_iteration;  /* 0-based outer iteration it fired on (n_iter of the reference = this + 1) */
    volatile int32_t code;            /* MCL_STOP_RELATIVE / MCL_STOP_ABSOLUTE */
    volatile int32_t progress;        /* iterations whose verdict has been evaluated so far */
} mcl_run_status;
int mcl_run(mcl_context *ctx, int32_t n_iter_max, int32_t update_A, int32_t update_B, int32_t update_C,
            const mcl_stop_rule *rule, double *diag_ring, double *verdict_ring, mcl_run_status *status);

/* The same rule for a host that drives the iterations itself - the sharded loop, whose diagnostics vector only exists after an
 * all-reduce over the ranks:  mcl_gate_begin -> per iteration { phase / step calls with their reductions, mcl_diagnostics(ctx,
 * vec, rank == 0) -> [SUM all-reduce of vec] -> mcl_verdict(ctx, vec, it, row) } -> (synchronise, read `status`) -> mcl_gate_end.
 * Between begin and end every state-writing kernel tests the stop flag, so iterations enqueued behind a hit do nothing
 * (their collectives still run: every rank must enqueue the SAME number of iterations before it looks at `status` - e.g.
 * fixed chunks with a synchronisation in between; the ranks reach identical verdicts because they evaluate identical bits).
 * mcl_gate_end(ctx, 1) after an early stop makes the context forget its cached by-products. */
int mcl_gate_begin(mcl_context *ctx, const mcl_stop_rule *rule, mcl_run_status *status);
int mcl_verdict(mcl_context *ctx, const double *diag_vec, int32_t iteration, double *verdict_row);
int mcl_gate_end(mcl_context *ctx, int32_t stopped_early);

/* ---- step calls (constant feasibility penalty / PARAFAC2 / EXTERNAL penalties on several devices) ---- */
/* B-phase prologue: CtC, rhs_i, rho_i; returns pointer to this rank's max rho (device fp32[1]) for a MAX all-reduce */
int mcl_B_begin(mcl_context *ctx);
float *mcl_B_rho_max(mcl_context *ctx);
int mcl_B_factor(mcl_context *ctx);          /* build and invert the r x r systems (decomposition.py:252-256) */
int mcl_B_solve(mcl_context *ctx);           /* one normal-equation solve (decomposition.py:266-273) */
int mcl_B_prox_local(mcl_context *ctx, int32_t k);  /* prox of penalty k; PARAFAC2: bases + local Delta sums */
float *mcl_B_prox_reduce_buffer(mcl_context *ctx, int32_t k, int64_t *count); /* PARAFAC2: [sum rho P^T Y | sum rho] */
int mcl_B_prox_finish(mcl_context *ctx, int32_t k); /* PARAFAC2: Delta; all: dual update (decomposition.py:282-285) */
/* Contract of one inner iteration: mcl_B_solve, then for EVERY penalty k in order: mcl_B_prox_local(k) [all-reduce of
 * mcl_B_prox_reduce_buffer(k) for PARAFAC2] mcl_B_prox_finish(k).  For stacks of row-separable kinds, L2 balls and
 * PARAFAC2 the library defers the aux / dual row updates of all penalties to ONE pass issued by the last
 * mcl_B_prox_finish of the round, so the rows are only final once the whole stack has been stepped. */
/* That pass is issued by the NEXT entry point: merged with the solve when it is mcl_B_solve (one row pass per inner
 * iteration), on its own otherwise.  mcl_B_end issues it explicitly - call it before reading B / aux / dual buffers
 * directly (not through the library) after the last inner iteration. */
int mcl_B_end(mcl_context *ctx);
int mcl_A_begin(mcl_context *ctx);           /* X C, rhs_i, Q_i, rho_i (decomposition.py:136-162) */
float *mcl_A_rho_max(mcl_context *ctx);
int mcl_A_finish(mcl_context *ctx);          /* systems, inner ADMM loop, by-products (decomposition.py:163-219) */
/* Host-evaluated (MCL_PEN_EXTERNAL) penalties on modes 0 / 2: the library does the linear algebra, the host the prox.
 *   mode 0:  mcl_A_begin -> [MAX all-reduce] -> mcl_A_factor -> { mcl_A_solve -> host prox/dual }* -> mcl_A_end
 *   mode 2:  mcl_update_C_local -> [all-reduce] -> mcl_C_begin -> { mcl_C_solve -> host prox/dual }* -> mcl_C_end
 *   mode 1:  mcl_B_begin -> mcl_B_factor -> { mcl_B_solve -> per penalty: native mcl_B_prox_* or host prox/dual }*
 * The aux buffer of an EXTERNAL penalty holds the auxiliary variable AS A MATRIX (aux_as_matrix of the reference). */
int mcl_A_factor(mcl_context *ctx);          /* Q_i, rho_i, L_i^-1 (decomposition.py:162-172) */
int mcl_A_solve(mcl_context *ctx);           /* one row solve for all rows (decomposition.py:184-195) */
int mcl_A_end(mcl_context *ctx);             /* by-products for the fast error formula (decomposition.py:219, 445-449) */
int mcl_C_begin(mcl_context *ctx);           /* rho, L^-1 from the reduced normal equations (decomposition.py:319-321) */
int mcl_C_solve(mcl_context *ctx);           /* decomposition.py:328-331 */
int mcl_C_end(mcl_context *ctx);             /* invalidates everything derived from C */

/* ---- ordering against other streams (a host that runs its collectives on a communication stream of its own) ------------ */
/* The library enqueues everything on the stream of mcl_create().  A host whose collective library wants its own stream
 * chains it with two events per collective:  mcl_update_C_local -> mcl_record_event(ctx, e1) -> [comm stream: wait e1,
 * all-reduce mcl_c_normal_equations() in place, record e2] -> mcl_wait_event(ctx, e2) -> mcl_update_C_finish.
 * (A host that can enqueue its collective on the engine's stream itself - RCCL takes any stream - needs neither: that
 * is what matcouply_amd/_rccl.py does, and it saves the ~8 us of the hand-over.)  `hip_event`: a hipEvent_t. */
int mcl_record_event(mcl_context *ctx, void *hip_event);
int mcl_wait_event(mcl_context *ctx, void *hip_event);

/* ---- the step after the solver: dense reconstruction (replaces cmf_to_matrices, coupled_matrices.py:365-497) ---------- */
/* M_i = (B_i diag(weights o a_i)) C^T for all matrices, packed along rows like X.  Stateless (no context): A [I, r],
 * B packed [N, r], C [K, r], weights [r] or NULL, slab_of_row int32 [N] (matrix index of every packed row), out [N, K] -
 * all device pointers; enqueued on hip_stream. */
int mcl_cmf_to_packed(const float *A, const float *B, const float *C, const float *weights, const int32_t *slab_of_row,
                      int64_t N, int64_t K, int32_t rank, float *out, void *hip_stream);

/* ---- before the solver: init="svd" / "threshold_svd" (decomposition.py:41-54) for data resident in HBM ---------------------- */
/* B_i = the leading `rank` left singular vectors of X_i (packed [N, rank]), C = the leading right singular vectors of the
 * stacked matrices [K, rank]; threshold != 0 clips negative entries (threshold_svd).  Stateless; X, B, C, workspace, info:
 * device pointers; row_ptr: HOST int64[I+1].  fp64 subspace iteration on the K x K Gram matrices (csrc/svdinit.hip).  The
 * entry of largest magnitude of every column of B_i and of C is positive: a singular vector's sign is the driver's choice,
 * so the vectors equal LAPACK's up to these signs.  info: int32[I+1] - iterations used per matrix (last: the stack), negative
 * when the Ritz values had not settled after 400.  Synchronises the stream once (the upload of row_ptr). */
int64_t mcl_svd_init_workspace_bytes(const int64_t *row_ptr, int64_t I, int64_t K, int32_t rank);
int mcl_svd_init(const float *X, const int64_t *row_ptr, int64_t I, int64_t K, int32_t rank, int32_t threshold, float *B, float *C,
                 void *workspace, int64_t workspace_bytes, int32_t *info, void *hip_stream);
/* mcl_svd_init for X of element type x_type (mcl_x_type); mcl_svd_init(..) is mcl_svd_init_typed(.., MCL_X_F32, ..) */
int mcl_svd_init_typed(const void *X, int32_t x_type, const int64_t *row_ptr, int64_t I, int64_t K, int32_t rank, int32_t threshold,
                       float *B, float *C, void *workspace, int64_t workspace_bytes, int32_t *info, void *hip_stream);
const char *mcl_svd_init_last_error(void);

/* ---- before the solver: init="parafac_als" / "cp_als", "parafac_hals" / "cp_hals" (decomposition.py:55-75) ------------------ */
/* CP-ALS (method MCL_ALS_CP) or CP-HALS (MCL_ALS_CP_HALS) on the zero-padded tensor [I, max J_i, K] for data resident in HBM.
 * Start: C = the C of mcl_svd_init, B = the leading eigenvectors of sum_i X~_i X~_i^T (entry of largest magnitude positive;
 * HALS: both clipped at 0), A = 1.  Sweeps over the modes A, B, C; stop after sweep t >= 1 when |e_{t-1} - e_t| < tol (tol = 0:
 * exactly n_iter_max sweeps).  Outputs A [I, rank], B packed [N, rank] (B_i = B[:J_i]), C [K, rank], errors fp64[n_iter_max]
 * (relative reconstruction error after every sweep; may be NULL), info int32[1] = sweeps used.  Stateless; X, A, B, C, errors,
 * info, workspace: device pointers; row_ptr: HOST int64[I+1].  Needs rank <= min(max J_i, K), K <= 2048, max J_i <= 2048,
 * rank <= 64.  Deterministic (fixed reduction orders).  Synchronises the stream at the start, once per sweep when tol > 0 and at
 * the end. */
enum mcl_als_method { MCL_ALS_CP = 0, MCL_ALS_CP_HALS = 1 };
int64_t mcl_als_init_workspace_bytes(const int64_t *row_ptr, int64_t I, int64_t K, int32_t rank);
int mcl_als_init_typed(const void *X, int32_t x_type, const int64_t *row_ptr, int64_t I, int64_t K, int32_t rank, int32_t method,
                       int32_t n_iter_max, double tol, float *A, float *B, float *C, double *errors, int32_t *info, void *workspace,
                       int64_t workspace_bytes, void *hip_stream);
const char *mcl_als_init_last_error(void);

/* ---- parafac2_als (decomposition.py, csrc/parafac2als.hip): unconstrained PARAFAC2-ALS for data resident in HBM ------------- */
/* Model X_i ~ P_i B diag(a_i) C^T, P_i^T P_i = I.  Start: A0 [I, rank], B0 [rank, rank], C0 [K, rank] (fp64, device), or all NULL:
 * A = 1, B = I, C = the C of mcl_svd_init (needs K <= 2048).  Per iteration: the projections from the polar factor of
 * X_i C diag(a_i) B^T, then n_iter_parafac CP sweeps (modes A, B, C) on the projected tensor; ALS normal equations, one HALS
 * column pass for the modes in nn_modes (bit 0: A, bit 2: C; mode B cannot be non-negative).  tol > 0: errors[t] = the relative
 * reconstruction error after iteration t; stop after t >= 1 when |e_{t-1}^2 - e_t^2| <= tol e_{t-1}^2 or e_t^2 < absolute_tol
 * (evaluated on the device; the host reads the verdict every 16 iterations).  Outputs A [I, rank], B [rank, rank], C [K, rank],
 * P packed [N, rank] (the projections), info int32[1] = iterations used.  Needs rank <= 32 and rank <= min(J_i, K).
 * Deterministic (fixed reduction orders).  row_ptr: HOST int64[I+1]; everything else: device pointers. */
int64_t mcl_parafac2_als_workspace_bytes(const int64_t *row_ptr, int64_t I, int64_t K, int32_t rank);
int mcl_parafac2_als_typed(const void *X, int32_t x_type, const int64_t *row_ptr, int64_t I, int64_t K, int32_t rank, const double *A0,
                           const double *B0, const double *C0, int32_t n_iter_max, int32_t n_iter_parafac, double tol,
                           double absolute_tol, int32_t nn_modes, float *A, float *B, float *C, float *P, double *errors,
                           int32_t *info, void *workspace, int64_t workspace_bytes, void *hip_stream);
const char *mcl_parafac2_als_last_error(void);

/* ---- many random starts of one problem at once (cmf_aoadmm_multistart, csrc/multistart.hip) ------------------------------- */
/* One workgroup per start runs the whole fit (phases B, C, A, diagnostics and the stopping rule of mcl_run) in fp64 with
 * workgroup barriers only; X is shared and read-only.  Stateless; X, state, diag, n_iter, stop, workspace: device pointers;
 * row_ptr: HOST int64[I+1].
 * state: fp64 [n_starts, state_len], in/out.  One start's slice: A [I, r], B packed [N, r], C [K, r], then for every mode
 * m = 0, 1, 2 and every penalty k of it: aux (rows of the mode x r; PARAFAC2: P packed [N, r] followed by Delta [r, r]) and
 * dual (rows x r).  state_len is the sum of these sizes (no padding).
 * diag: fp64 [n_starts, n_iter_max + 1, MCL_MS_DIAG]: row 0 the initial state, row t + 1 outer iteration t:
 * {rec_error, loss, flags (bit 0 feasible, bit 1 loss evaluated), regularisation, gap[m * MCL_MAX_REGS + k] ...}.
 * n_iter int32[n_starts]: outer iterations run; stop int32[n_starts]: 0 or the MCL_STOP_* code that ended the start.
 * Needs rank <= 16, penalties NN / Box / L1 / L2 ball on any mode (L2 ball on mode 0 with constant_A) and PARAFAC2 on mode 1
 * with every J_i >= rank.  Every reduction has a fixed order; a start's result does not depend on n_starts or its neighbours. */
#define MCL_MS_DIAG (4 + 3 * MCL_MAX_REGS)
typedef struct mcl_multistart_penalty {
    int32_t kind;           /* enum mcl_penalty_kind */
    int32_t non_negativity;
    double p0, p1;          /* Box: min, max; L1: reg_strength; L2 ball: norm_bound */
} mcl_multistart_penalty;
typedef struct mcl_multistart_options {
    int32_t n_regs[3];
    int32_t inner_n_iter_max;
    mcl_multistart_penalty regs[3][MCL_MAX_REGS];
    double l2_penalty[3];
    double feasibility_penalty_scale;
    double inner_tol;       /* <= 0: every inner iteration runs */
    double tol, absolute_tol, feasibility_tol;  /* 0 = not set */
    int32_t constant_A, constant_B;
    int32_t update_A, update_B, update_C;
    int32_t evaluate_loss_always;  /* return_errors: the loss of infeasible iterates is recorded too */
    int32_t n_iter_max;
    int32_t reserved;
} mcl_multistart_options;
int64_t mcl_multistart_workspace_bytes(const int64_t *row_ptr, int64_t I, int64_t K, int32_t rank, const mcl_multistart_options *opt,
                                       int32_t n_starts);
int mcl_multistart_run(const void *X, int32_t x_type, const int64_t *row_ptr, int64_t I, int64_t K, int32_t rank,
                       const mcl_multistart_options *opt, int32_t n_starts, double *state, double *diag, int32_t *n_iter, int32_t *stop,
                       void *workspace, int64_t workspace_bytes, void *hip_stream);
const char *mcl_multistart_last_error(void);
/* A grid of penalty strengths x random starts in the same launch (cmf_aoadmm_grid): options is a HOST array of n_jobs entries,
 * uploaded to the workspace; job s = workgroup s runs with options[s] on state slice s and writes diag slice s, n_iter[s] and
 * stop[s] as a start of mcl_multistart_run does.  All jobs share X, row_ptr, rank and ONE state layout: n_regs, the kind and
 * non_negativity of every penalty, constant_A/B and update_A/B/C must be equal in all jobs (else an error); p0 / p1,
 * l2_penalty, feasibility_penalty_scale, the tolerances, inner_n_iter_max, n_iter_max and evaluate_loss_always may differ.
 * diag: fp64 [n_jobs, max_s options[s].n_iter_max + 1, MCL_MS_DIAG]; job s fills its first options[s].n_iter_max + 1 rows.
 * A job's result does not depend on n_jobs, on its neighbours or on their options. */
int64_t mcl_multistart_grid_workspace_bytes(const int64_t *row_ptr, int64_t I, int64_t K, int32_t rank,
                                            const mcl_multistart_options *options, int32_t n_jobs);
int mcl_multistart_run_grid(const void *X, int32_t x_type, const int64_t *row_ptr, int64_t I, int64_t K, int32_t rank,
                            const mcl_multistart_options *options, int32_t n_jobs, double *state, double *diag, int32_t *n_iter,
                            int32_t *stop, void *workspace, int64_t workspace_bytes, void *hip_stream);
/* Weighted jobs in the same launch (cmf_aoadmm_resample: bootstrap, jackknife and K-fold over the matrices): job s minimises
 * 0.5 sum_i w_si |X_i - B_i D_i C^T|^2 / sum_i w_si |X_i|^2 + penalties + l2 terms, the AO-ADMM run of mcl_multistart_run with
 * every per-matrix Gram and right-hand side multiplied by w_si; rec_error is the weighted relative error.  slab_weights is a
 * HOST fp64 array [n_jobs, I], uploaded to the workspace: every weight finite and >= 0, a positive one in every job (else an
 * error, before any launch).  A matrix of weight 0 is not in the job: the caller zeroes its row of A, its B_i and its rows of
 * every aux and dual of modes 0 and 1 (its P_i for PARAFAC2) in the job's state slice; the kernel writes a zero inverse for its
 * systems, skips its prox and dual steps and its passes over X, and returns those rows as exact zeros.  Everything else is as
 * for mcl_multistart_run (one *opt for all jobs).  A job's result does not depend on n_jobs or on its neighbours' weights; with
 * every weight 1 the state, diag, n_iter and stop are bitwise those of mcl_multistart_run. */
int64_t mcl_multistart_weighted_workspace_bytes(const int64_t *row_ptr, int64_t I, int64_t K, int32_t rank,
                                                const mcl_multistart_options *opt, int32_t n_jobs);
int mcl_multistart_run_weighted(const void *X, int32_t x_type, const int64_t *row_ptr, int64_t I, int64_t K, int32_t rank,
                                const mcl_multistart_options *opt, int32_t n_jobs, const double *slab_weights, double *state,
                                double *diag, int32_t *n_iter, int32_t *stop, void *workspace, int64_t workspace_bytes,
                                void *hip_stream);
/* Jobs on data with missing entries in the same launch (cmf_aoadmm_missing: EM imputation, element-wise cross-validation).
 * observed: DEVICE uint8 [n_masks, N, K], 1 = observed; n_masks is 1 (one mask for all jobs) or n_jobs, job s reads mask
 * s % n_masks.  Every job keeps an fp64 copy X~ of X in the workspace: X at its observed entries; at the others its mask's row
 * of fill_values (DEVICE fp64 [n_masks, K], a constant per column) or, with fill_values NULL, the model B_i D_i C^T of its
 * start.  An outer iteration is the B, C and A phases of mcl_multistart_run on X~, then one pass with M = B_i D_i C^T that sums
 * (X - M)^2 over the observed entries and stores M into the others; rec_error = sqrt(that sum) / sqrt(sum of X^2 over the
 * observed entries), loss = 0.5 rec_error^2 + regularisation, gaps and the stopping rule as for mcl_multistart_run.  Row 0 of
 * diag is the same pass on the start (it stores M only with fill_values NULL).  The value of X at a missing entry is never
 * used: it may be NaN.  Errors, before any launch: what mcl_multistart_run refuses, n_masks not 1 or n_jobs, a NULL mask.
 * A job's result does not depend on n_jobs or on its neighbours. */
int64_t mcl_multistart_missing_workspace_bytes(const int64_t *row_ptr, int64_t I, int64_t K, int32_t rank,
                                               const mcl_multistart_options *opt, int32_t n_jobs);
int mcl_multistart_run_missing(const void *X, int32_t x_type, const int64_t *row_ptr, int64_t I, int64_t K, int32_t rank,
                               const mcl_multistart_options *opt, int32_t n_jobs, const uint8_t *observed, int32_t n_masks,
                               const double *fill_values, double *state, double *diag, int32_t *n_iter, int32_t *stop,
                               void *workspace, int64_t workspace_bytes, void *hip_stream);

/* ---- many random starts of parafac2_als at once (parafac2_als_multistart, csrc/pf2als_multistart.hip) ---------------------- */
/* One workgroup per start runs the whole unconstrained PARAFAC2-ALS fit of mcl_parafac2_als_typed (projections from the polar
 * factor of X_i C diag(a_i) B^T, n_iter_parafac CP sweeps per iteration, ALS or one HALS column pass for the modes in nn_modes:
 * bit 0 A, bit 2 C) in fp64 with workgroup barriers only; X is shared and read-only.  Stateless; X, factors, P, errors, n_iter,
 * workspace: device pointers; row_ptr: HOST int64[I+1].
 * factors: fp64 [n_starts, (I + rank + K) * rank], in/out: start s's A [I, rank], B [rank, rank], C [K, rank], row-major, no
 * padding.  P: fp64 [n_starts, N, rank], the projections packed like X (from the last iteration).  errors: fp64
 * [n_starts, n_iter_max] (may be NULL when tol = 0): tol > 0: errors[s][t] = the relative reconstruction error after iteration t,
 * and a start stops after t >= 1 when |e_{t-1}^2 - e_t^2| <= tol e_{t-1}^2 or e_t^2 < absolute_tol.  n_iter: int32[n_starts],
 * the iterations a start ran.  Needs 1 <= rank <= 16 and rank <= min(J_i, K).  Every reduction has a fixed order; a start's
 * result does not depend on n_starts or its neighbours. */
int64_t mcl_pf2als_multistart_workspace_bytes(const int64_t *row_ptr, int64_t I, int64_t K, int32_t rank, int32_t n_starts);
int mcl_pf2als_multistart_run(const void *X, int32_t x_type, const int64_t *row_ptr, int64_t I, int64_t K, int32_t rank, int32_t n_starts,
                              int32_t n_iter_max, int32_t n_iter_parafac, double tol, double absolute_tol, int32_t nn_modes,
                              double *factors, double *P, double *errors, int32_t *n_iter, void *workspace, int64_t workspace_bytes,
                              void *hip_stream);
/* The same fit of per-job scaled matrices (parafac2_als_resample: bootstrap, jackknife and K-fold over the matrices): job s =
 * workgroup s fits the matrices slab_scale[s][i] X_i, every element multiplied after its exact conversion to double, and no job
 * holds an X of its own.  slab_scale: DEVICE fp64 [n_starts, I], the square roots of the job's weights (finite, >= 0; NULL is an
 * error).  With w = slab_scale^2 the job minimises sum_i w_i |X_i - P_i B D_i C^T|^2 once row i of its A is divided by
 * slab_scale[s][i]; errors hold the weighted relative error.  A matrix of scale 0 whose start row of A is 0 keeps that row and
 * its P_i at exact zeros.  Everything else, the workspace included, is as for mcl_pf2als_multistart_run; with every scale 1 the
 * results are bitwise its results, and a job's result does not depend on its neighbours' scales. */
int mcl_pf2als_multistart_run_weighted(const void *X, int32_t x_type, const int64_t *row_ptr, int64_t I, int64_t K, int32_t rank,
                                       int32_t n_starts, const double *slab_scale, int32_t n_iter_max, int32_t n_iter_parafac, double tol,
                                       double absolute_tol, int32_t nn_modes, double *factors, double *P, double *errors, int32_t *n_iter,
                                       void *workspace, int64_t workspace_bytes, void *hip_stream);
const char *mcl_pf2als_multistart_last_error(void);

/* ---- factor match scores of many pairs of fitted models (multistart_similarity, csrc/similarity.hip) ---------------------- */
/* models: fp64 [n_models, (I + N + K) * rank], every model [A; B; C] row-major with B the stacked B_i (N = sum J_i): the layout
 * of the first (I + N + K) * rank doubles of a multi-start state slice.  weights: fp64 [n_models, rank] or NULL (ones).
 * pairs: HOST int32 [n_pairs, 2], checked against n_models before anything is launched; pair i = (s, t) compares model s with
 * model t.  flags: bit 0 consider_weights, bit 1 absolute_value; skip_mode: -1 (none), 0, 1 or 2.  score: fp64 [n_pairs];
 * perm: int32 [n_pairs, rank] or NULL: columns perm[i] of model t line it up with model s.  The definition of the score is in
 * DESIGN.md section 14; the assignment is the exact optimum.  models, weights, score, perm, workspace: device pointers;
 * workspace: mcl_fms_workspace_bytes(n_models, rank) bytes, 256-byte aligned (column norms and weights of every model).
 * Needs 1 <= rank <= 16 and finite models.  Stateless; work is enqueued on the stream (the pairs are uploaded first, into the
 * score buffer, and the stream is synchronised once for that).  No atomics and a fixed summation order: a pair's result does
 * not depend on the other pairs of the call, and score(s, t) = score(t, s) bit for bit. */
int64_t mcl_fms_workspace_bytes(int64_t n_models, int32_t rank);
int mcl_fms_scores(const double *models, int64_t n_models, int64_t I, int64_t N, int64_t K, int32_t rank, const double *weights,
                   const int32_t *pairs, int64_t n_pairs, int32_t flags, int32_t skip_mode, double *score, int32_t *perm,
                   void *workspace, void *hip_stream);
const char *mcl_fms_last_error(void);

/* ---- fit, per-matrix SSE and core consistency of many fitted models (multistart_evaluation, csrc/evaluate.hip) ------------ */
/* models: fp64 [n_models, (I + N + K) * rank], the layout of mcl_fms_scores (weights folded into A by the caller).  X: the packed
 * data [N, K] of element type x_type, row_ptr: HOST int64 [I + 1], strictly increasing from 0 (every matrix has a row).
 * mcl_eval_tables_typed reads X once per model and writes S [n_models, I, r, r] (S_i = B_i^T X_i C), BtB [n_models, I, r, r],
 * sse [n_models, I] (|X_i - B_i diag(a_i) C^T|_F^2, summed from the residual) and norm [I] (|X_i|_F^2).  mcl_eval_core takes
 * these tables and writes core [n_models, r, r, r] (G[p][q][s] = sum_i (A^+)[p][i] ((B_i^T B_i)^+ S_i (C^T C)^+)[q][s]), cc and
 * cc_normalised [n_models] (100 (1 - sum (G - T)^2 / r), resp. / sum G^2; T the superdiagonal of ones).  The definitions are in
 * DESIGN.md section 15.  X, models, the tables, the outputs and ws are device pointers; ws: mcl_eval_workspace_bytes bytes,
 * 256-byte aligned.  Needs 1 <= rank <= 32, 1 <= n_models <= 65535 and finite models: the models are read back and checked
 * before anything is launched (one synchronisation of the stream).  Stateless; the work is enqueued on the stream.  No atomics
 * and a fixed summation order: a model's results do not depend on the other models of the call, and two runs are bitwise equal.
 * mcl_eval_workspace_bytes returns -1 for arguments the entries refuse. */
int64_t mcl_eval_workspace_bytes(const int64_t *row_ptr, int64_t I, int64_t K, int32_t rank, int64_t n_models);
int mcl_eval_tables_typed(const void *X, int32_t x_type, const int64_t *row_ptr, int64_t I, int64_t K, int32_t rank,
                          const double *models, int64_t n_models, double *S, double *BtB, double *sse, double *norm, void *ws,
                          int64_t ws_bytes, void *stream);
int mcl_eval_core(const double *models, int64_t n_models, int64_t I, int64_t N, int64_t K, int32_t rank, const double *S,
                  const double *BtB, double *core, double *cc, double *cc_normalised, void *stream);
const char *mcl_eval_last_error(void);

/* ---- new matrices fitted to a fixed PARAFAC2 model (parafac2_project, csrc/projection.hip) --------------------------------- */
/* For every matrix X_i [J_i, K] of the packed data X [N, K] (element type x_type; row_ptr: HOST int64 [I + 1] from 0, every
 * J_i >= rank): minimise |X_i - P Delta diag(a) C^T|_F^2 over a [rank] and P [J_i, rank] with P^T P = I by alternation from
 * a_init[i]; the iteration and its stopping rule (per matrix: e2_t < absolute_tol, or t >= 2 and |e2_{t-1} - e2_t| <= tol e2_{t-1},
 * or t = n_iter_max) are in DESIGN.md section 16.  Delta [rank, rank], C [K, rank] and a_init [I, rank] are fp64 device arrays,
 * which the caller has rounded through fp32; they are read back and checked for non-finite entries before anything is launched
 * (one synchronisation of the stream).  Outputs (device): A fp64 [I, rank]; B fp32 [N, rank] (B_i = P_i Delta) and P fp32
 * [N, rank], packed like X; stats fp64 [I, 2] = {sse_i from the formula e2 |X_i|^2, |X_i|_F^2}; n_iter int32 [I]; errors fp64
 * [I, n_iter_max] or NULL: the e2 of every iteration of matrix i, NaN behind its stop.  workspace: device,
 * mcl_pf2_project_workspace_bytes bytes (-1 for shapes the entry refuses), 256-byte aligned.  Needs 1 <= rank <= 32 and rank <= K (W = X C has rank K at most: below, P would be a partial isometry).  Every bad
 * argument is refused with a message before any launch.  Stateless; the work is enqueued on the stream.  No atomics and a fixed
 * summation order that depends on a matrix's own shape only: a matrix's result does not depend on the other matrices of the call,
 * and two runs are bitwise equal. */
int64_t mcl_pf2_project_workspace_bytes(const int64_t *row_ptr, int64_t I, int64_t K, int32_t rank);
int mcl_pf2_project_typed(const void *X, int32_t x_type, const int64_t *row_ptr, int64_t I, int64_t K, int32_t rank, const double *Delta,
                          const double *C, const double *a_init, int32_t n_iter_max, double tol, double absolute_tol, double *A, float *B,
                          float *P, double *stats, int32_t *n_iter, double *errors, void *workspace, int64_t workspace_bytes,
                          void *hip_stream);
const char *mcl_pf2_project_last_error(void);

/* ---- introspection for tests / profiling ------------------------------------------------------------- */
/* device pointers to internal by-products / planner tables (the int32 tables: read the bits) */
enum mcl_buffer_id {
    MCL_BUF_RHSES = 0,          /* rhses [I, r] of the A-phase (decomposition.py:147-152) */
    MCL_BUF_CROSS_PRODUCTS = 1, /* cross_products [I, r, r] (decomposition.py:153-161) */
    MCL_BUF_XC = 2,             /* X C [sum J_i, r] */
    MCL_BUF_RHO_B = 3,          /* [I] */
    MCL_BUF_RHO_A = 4,          /* [I] */
    MCL_BUF_RHO_C = 5,          /* [1] */
    MCL_BUF_CTC = 6,            /* C^T C [r, r] */
    MCL_BUF_LINV_B = 7,         /* inverses of the B-phase systems [I, r, r] */
    MCL_BUF_PF2_STATUS = 8,     /* int32 [I]: which polar-factor kernel took the slab */
    MCL_BUF_PF2_ACC = 9,        /* fp64 bits */
    MCL_BUF_PF2_GRAM = 10,      /* fp64 bits [I, r, r] */
    MCL_BUF_SWEEP_CYCLES = 11,  /* int64 bits (MCL_SWEEP_DBG & 32) */
    MCL_BUF_SEG_ROW0 = 12,      /* int32: first row of every segment of the X passes */
    MCL_BUF_SEG_NROWS = 13,     /* int32: its length */
    MCL_BUF_WAVE_SEG_PTR = 14,  /* int32: first segment of every wave */
    MCL_BUF_BSEG_ROW0 = 15,     /* the same three tables for the bsegs of the one-pass sweep */
    MCL_BUF_BSEG_NROWS = 16,
    MCL_BUF_WAVE_BSEG_PTR = 17,
    MCL_BUF_NS_STAMPS = 18,     /* instrumented builds (-DMCL_NS_STAMPS) only */
    MCL_BUF_BSEG_PART = 19      /* int32 per bseg: bits 0-27 the partial image the sweep adds the bseg to */
};
float *mcl_internal_buffer(mcl_context *ctx, int32_t which /* enum mcl_buffer_id */, int64_t *count);
/* The hot launch sites of the library, for HIP-event timing (bench.py's roofline block) and for asking which kernel form a
 * problem gets.  A slot covers every launch of its role; roles that a configuration does not use stay empty. */
enum mcl_profile_slot {
    MCL_PROF_XC = 0,         /* X C pass (k_contract_xc_*) */
    MCL_PROF_XT = 1,         /* X^T (B o a) pass (k_contract_xt) */
    MCL_PROF_ROWS_FUSED = 2, /* fused inner ADMM loop of row-separable stacks (k_rows_fused) */
    MCL_PROF_SWEEP = 3,      /* one-pass sweep: X C -> B-phase -> X^T B in a single pass over X (k_sweep) */
    MCL_PROF_REDUCE = 4,     /* [G | R] from the partials (k_reduce_frag / k_reduce_partials / k_exact_gr) */
    MCL_PROF_C_FINISH = 5,   /* C-phase finish (k_C_finish_* / k_C_prepare + row kernels) */
    MCL_PROF_A_FINISH = 6,   /* A-phase finish (k_A_finish*; k_CA_finish when it also holds the C-phase finish) */
    MCL_PROF_ROWS_CHAIN = 7, /* one chained row pass of a generic B stack (k_rows_solve_stats / _finish_solve_stats / _finish_fused) */
    MCL_PROF_UNIMODAL = 8,   /* unimodal regressions (k_slab_unimodal_*) */
    MCL_PROF_PF2 = 9,        /* per-slab PARAFAC2 algebra of one inner iteration (polar factors + coordinate matrix) */
    MCL_PROF_DIAG = 10,      /* reduction of the diagnostics tables (k_diag_final / k_diag_verdict) */
    MCL_PROF_OTHER = 11,     /* every other launch of a phase (statistics reductions, system builds, ...) */
    MCL_PROF_SLOTS = 12
};
/* name of the kernel variant chosen for the current problem.  which = an mcl_profile_slot: the kernel last launched in that
 * role ("" when the problem has not used the role yet; MCL_PROF_SWEEP stays empty when the problem is not eligible for the
 * one-pass sweep); MCL_VARIANT_EXACT_MODE: non-empty when the problem runs in the exact-products mode (at most 2^20 elements
 * of X: every contraction as fp64 sums of exact products) */
#define MCL_VARIANT_EXACT_MODE 100
const char *mcl_kernel_variant(mcl_context *ctx, int32_t which);
/* HIP-event timing of the launch sites on the context's stream.
 * mcl_profile_enable(ctx, capacity): record up to `capacity` launches per slot (0 disables and frees);
 * mcl_profile_read(ctx, slot, &total_ms, &count): synchronises the recorded events of `slot`, returns their summed
 * duration and number, and resets the slot; mcl_profile_launches(ctx, slot): launches the slot has SEEN since
 * mcl_profile_enable / mcl_profile_set_stride (timed or not) - launches per step = this / steps. */
int mcl_profile_enable(mcl_context *ctx, int32_t capacity);
/* record only every `stride`-th launch of a slot (default 1): an event pair opens ~5 us dispatch gaps on either side of
 * the kernel, so a timed loop samples its launches instead of bracketing all of them */
int mcl_profile_set_stride(mcl_context *ctx, int32_t stride);
int mcl_profile_read(mcl_context *ctx, int32_t which /* enum mcl_profile_slot */, double *total_ms, int32_t *count);
int64_t mcl_profile_launches(mcl_context *ctx, int32_t which /* enum mcl_profile_slot */);
/* what an event pair adds to the launch it brackets (microseconds), calibrated by mcl_profile_enable on the context's stream:
 * a pair around one tiny operation minus that operation's marginal cost inside a pair around two of them - the part of every
 * timed launch that is the command processor's marker handling, not the kernel */
double mcl_profile_overhead_us(mcl_context *ctx);
/* The MCL_* environment switches (A/B experiments, debug paths; tools/README.md) are read once in mcl_create();
 * this re-reads them for an existing context (tests that compare kernel forms on one problem).
 * PRODUCTION NOTE: the parity statements of this library hold for a CLEAN environment - several
 * switches select other kernel forms or other summation orders (MCL_SEG_ROWS, MCL_XC_WAVES, MCL_NO_ROWS64, MCL_NO_SWEEP, ...)
 * and move results at the 1e-6 level.  mcl_active_switches() returns the space-separated names of the MCL_* switches the
 * context found in its environment ("" = clean); a host should refuse, or at least log, a non-empty answer
 * (matcouply_amd.cmf_aoadmm issues a RuntimeWarning).  A library built with -DMCL_NO_ENV_SWITCHES
 * (MCL_BUILD_DEFS=-DMCL_NO_ENV_SWITCHES python -c "import __graft_entry__ as g; g.build()") never consults the
 * environment: every switch keeps its default and mcl_active_switches() is always "". */
/* What the box's memory system delivers to a pure streaming READ of `bytes` of device memory at `buf` (>= 1 MiB; take more than
 * the 256 MB last-level cache for an HBM figure): the better of two access geometries, `repeats` timed launches each, GB/s to
 * HOST `gbps`.  Stateless measurement helper (bench.py: roofline.frac_achievable); `scratch`: one device float; synchronises. */
int mcl_read_bandwidth(const void *buf, int64_t bytes, int32_t repeats, float *scratch, void *hip_stream, double *gbps);
int mcl_reload_switches(mcl_context *ctx);
const char *mcl_active_switches(const mcl_context *ctx);

#ifdef __cplusplus
}
#endif
#endif /* MATCOUPLY_HIP_H */
