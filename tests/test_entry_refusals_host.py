"""CPU: every refusal of the stand-alone entry points (X, row_ptr, a caller-provided workspace and a stream) that comes before
the first HIP call, one table for the eight families: the complete message, the family's own *_last_error slot (the other
seven keep their text), the workspace sizes against the documented layouts, and what the sizers answer with -1.  The pointers
are fakes that no call dereferences; row_ptr, the options, the weights and the pairs are real host arrays."""
import ctypes
import functools

import numpy as np
import pytest

from matcouply_amd import _engine

FAKE = 256  # a non-null, aligned "device pointer": every call below is refused before it would be used
I, K, R = 3, 5, 3
ROWS = [0, 3, 70, 75]  # matrices of 3, 67 and 5 rows: four 64-row segments
N = ROWS[-1]
X_TYPE = " (MCL_X_F32 = 0, MCL_X_BF16 = 1, MCL_X_F16 = 2)"
SLOTS = ("mcl_svd_init_last_error", "mcl_als_init_last_error", "mcl_parafac2_als_last_error", "mcl_multistart_last_error",
         "mcl_pf2als_multistart_last_error", "mcl_fms_last_error", "mcl_eval_last_error", "mcl_pf2_project_last_error")
_keep = []  # the host arrays behind the pointers


def rp(rows):
    a = np.ascontiguousarray(rows, dtype=np.int64)
    _keep.append(a)
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))


@functools.lru_cache(maxsize=None)
def rp_steps(n, step):
    """row_ptr of n matrices of `step` rows each (built when its case runs)"""
    return rp(np.arange(n + 1, dtype=np.int64) * step)


GOOD = rp(ROWS)
al = lambda b: (b + 255) // 256 * 256
al1 = lambda b: al(max(b, 1))  # a part of at least one byte
al32 = lambda n: (n + 31) // 32 * 32


def seg_count(rows):
    return sum((b - a + 63) // 64 for a, b in zip(rows[:-1], rows[1:]))


# ---- the documented workspace layouts, every part rounded up to 256 bytes ------------------------------------------------------
def svd_bytes(rows, K, r):
    """ext, BS Gram matrices, the stack's, Q and Y [BS, K, m], theta [BS, m], U [rows of the largest batch, r]"""
    I = len(rows) - 1
    m, BS = min(K, r + 8), min(I, 256)
    batch_rows = max(rows[min(I, b + BS)] - rows[b] for b in range(0, I, BS))
    return (al((I + 1) * 4) + al(BS * K * K * 8) + al(K * K * 8) + 2 * al(BS * K * m * 8) + al(BS * m * 8) + al(max(batch_rows, 1) * r * 8))


def gram_vectors_bytes(n, r):
    m = min(n, r + 8)
    return 2 * al(n * m * 8) + al(m * 8)


def als_bytes(rows, K, r):
    I, N, Jm, nseg = len(rows) - 1, rows[-1], max(np.diff(rows)), seg_count(rows)
    nkb = (K + 63) // 64
    nchunk, ngrp = max(1, min(nseg, 1024 // nkb)), max(1, min(I, (262144 + Jm * r - 1) // max(Jm * r, 1)))
    NB = 1 if r <= 16 else 2 if r <= 32 else 4
    wgmax = max((I + 63) // 64, (Jm + 63) // 64, (K + 63) // 64)
    parts = [max(nseg, 1) * 16, (I + 1) * 4, (nchunk + 1) * 4, (I + 1) * 4, (ngrp + 1) * 4, I * r * 8, Jm * r * 8, K * r * 8,
             4 * nkb * NB * 64 * 16, N * r * 4, max(nseg, 1) * r * 8, ngrp * Jm * r * 8, Jm * r * 8, nchunk * K * r * 8, K * r * 8, I * r * 8,
             3 * wgmax * r * r * 8, (K + 63) // 64 * 8, 3 * r * r * 8, r * r * 8, 32, (I + 2) * 4]
    start_C = al(svd_bytes(rows, K, r)) + al(K * r * 4)  # mcl_svd_init's workspace + C0 (fp32)
    start_B = al(Jm * Jm * 8) + al(gram_vectors_bytes(Jm, r)) + al(Jm * r * 4)  # P [Jmax, Jmax], the subspace iteration's, B0
    return sum(al1(b) for b in parts) + max(start_C, start_B)


def pf2als_bytes(rows, K, r):
    I, N, nseg = len(rows) - 1, rows[-1], seg_count(rows)
    nkb, NB = (K + 63) // 64, 1 if r <= 16 else 2
    ngrp_ab, ngrp_mc = max(1, min(128, (I + 7) // 8)), max(1, min(I, max(1, 256 // nkb)))
    per = 256 // (16 * NB)
    wgC = (K + per - 1) // per
    parts = [max(nseg, 1) * 16, (I + 1) * 4, (I + 1) * 4, I * r * 8, r * r * 8, K * r * 8, 4 * nkb * NB * 64 * 16, N * r * 4, I * r * r * 8,
             I * r * r * 8, I * K * r * 8, ngrp_ab * 2 * r * r * 8, ngrp_mc * K * r * 8, wgC * r * r * 8, wgC * 8, ngrp_ab * 8, I * 8,
             3 * r * r * 8, r * r * 8, 32, 16, (I + 2) * 4]
    return sum(al1(b) for b in parts) + al(svd_bytes(rows, K, r)) + al(K * r * 4)


def multistart_bytes(rows, K, r, n_starts):
    """[row_ptr | row -> slab | scratch x n_starts]"""
    I, N = len(rows) - 1, rows[-1]
    scratch = 2 * al32(N * r) + al32(K * r) + 4 * al32(I * r * r) + 2 * al32(I) + 2 * al32(I * r) + al32(8 * r * r + 64)
    return al((I + 1) * 8) + al(N * 4) + al(scratch * 8 * n_starts)


def pf2als_multistart_bytes(rows, K, r, n_starts):
    I, N = len(rows) - 1, rows[-1]
    scratch = al32(N * r) + al32(I * r * K) + 3 * al32(I * r * r) + al32(I * r) + al32(K * r)
    return al((I + 1) * 8) + al(N * 4) + al(scratch * 8 * n_starts)


def eval_bytes(rows, K, r, n_models):
    I, nseg = len(rows) - 1, seg_count(rows)
    cper = (K + 63) // 64 * 64 * 16 * (1 if r <= 16 else 2)
    return al1(nseg * 16) + al1((I + 1) * 4) + 2 * al1(n_models * cper * 4) + al1(n_models * nseg * (2 * r * r + 2) * 8)


def project_bytes(rows, K, r):
    I, N, nseg = len(rows) - 1, rows[-1], seg_count(rows)
    return (al1(max(nseg, 1) * 16) + al1((I + 1) * 4) + al1(4 * ((K + 63) // 64) * (1 if r <= 16 else 2) * 64 * 16) + 2 * al1(r * r * 8)
            + al1(N * r * 4) + al1(I * 2 * r * r * 8))


# ---- the options of the multi-start entries -------------------------------------------------------------------------------------
def options(n=1, **fields):
    """n default options (no penalty, one iteration); fields: name = value, or regs = {(mode, k): kind}, n_regs = (a, b, c);
    a field given as {job: value} goes to that job only"""
    array = (_engine.MultistartOptions * n)()
    for j in range(n):
        o = array[j]
        o.n_iter_max, o.inner_n_iter_max, o.update_A, o.update_B, o.update_C = 1, 1, 1, 1, 1
        for name, value in fields.items():
            if name == "only":
                continue
            if fields.get("only", j) != j:
                continue
            if name == "n_regs":
                o.n_regs[0], o.n_regs[1], o.n_regs[2] = value
            elif name == "regs":
                for (m, k), kind in value.items():
                    o.regs[m][k].kind = kind
            else:
                setattr(o, name, value)
    _keep.append(array)
    return array


def weights(rows):
    a = np.ascontiguousarray(rows, dtype=np.float64)
    _keep.append(a)
    return ctypes.c_void_p(a.ctypes.data)  # (not the bare address: an int would go into the case's id, another in every process)


PEN = _engine
MS_OPTION_REFUSALS = [
    (dict(inner_n_iter_max=-1), "need inner_n_iter_max >= 0 and n_iter_max >= 0"),
    (dict(n_iter_max=-1), "need inner_n_iter_max >= 0 and n_iter_max >= 0"),
    (dict(n_regs=(5, 0, 0)), "at most MCL_MAX_REGS penalties per mode"),
    (dict(n_regs=(0, 0, -1)), "at most MCL_MAX_REGS penalties per mode"),
    (dict(n_regs=(1, 0, 0), regs={(0, 0): PEN.PEN_PARAFAC2}), "PARAFAC2 only on mode 1"),
    (dict(n_regs=(1, 0, 0), regs={(0, 0): PEN.PEN_L2BALL}), "an L2 ball on mode 0 needs constant_A"),
    (dict(n_regs=(0, 0, 1), regs={(2, 0): PEN.PEN_UNIMODAL}), "penalty kind 5 is not served (NN, Box, L1, L2 ball, PARAFAC2)"),
]
PF2_ON_B = dict(n_regs=(0, 1, 0), regs={(1, 0): PEN.PEN_PARAFAC2})

PACKED_HEAD = "need row_ptr, I >= 1, K >= 1"
ROWS_2_31 = "more than 2^31 packed rows are not supported"
ROWS_2_26 = "more than 2^26 packed rows are not supported"
NOT_DECREASING = "row_ptr must be non-decreasing"
FIRST_ZERO = "row_ptr[0] must be 0"
ALIGNED = "workspace must be 256-byte aligned"


def x_type(t):
    return f"unknown x_type {t}" + X_TYPE


class Entry:
    """one entry point: its name, its slot, the prefix of its messages, the arguments of a good call in order, its refusals as
    (changed arguments, message without the prefix) and the pointer arguments that may not be NULL"""

    def __init__(self, name, slot, prefix, good, refusals, not_null, null_message="NULL argument"):
        self.name, self.slot, self.prefix, self.good = name, slot, prefix, good
        self.refusals = list(refusals) + [({p: None}, null_message) for p in not_null]


def packed_tail(ws_bytes):
    return dict(ws=FAKE, ws_bytes=ws_bytes, stream=None)


def workspace_refusals(want, sizer):
    return [(dict(ws_bytes=want - 1), f"workspace too small ({sizer})"), (dict(ws=FAKE + 8), ALIGNED)]


# ---- mcl_svd_init* (the messages carry the entry's name themselves: the fp32 entry and the typed one share them) ----------------
SVD_WANT = svd_bytes(ROWS, K, R)
SVD_REFUSALS = [
    (dict(I=0), "need I >= 1, K >= 1, 1 <= rank <= 64"), (dict(K=0), "need I >= 1, K >= 1, 1 <= rank <= 64"),
    (dict(rank=0), "need I >= 1, K >= 1, 1 <= rank <= 64"), (dict(rank=65), "need I >= 1, K >= 1, 1 <= rank <= 64"),
    (dict(rank=6), "rank exceeds the number of columns"), (dict(rank=4), "a matrix has fewer rows than the rank"),
    (dict(rp=rp([0, 3, 70, 1 << 31])), ROWS_2_31)] + workspace_refusals(SVD_WANT, "mcl_svd_init_workspace_bytes")
SVD_GOOD = dict(X=FAKE, xt=0, rp=GOOD, I=I, K=K, rank=R, threshold=0, B=FAKE, C=FAKE, ws=FAKE, ws_bytes=SVD_WANT, info=FAKE, stream=None)
ENTRIES = [
    Entry("mcl_svd_init_typed", SLOTS[0], "mcl_svd_init: ", SVD_GOOD, SVD_REFUSALS, ("X", "rp", "B", "C", "ws", "info")),
    Entry("mcl_svd_init_typed", SLOTS[0], "mcl_svd_init_typed: ", SVD_GOOD, [(dict(xt=7), x_type(7)), (dict(xt=-1), x_type(-1))], ()),
    Entry("mcl_svd_init", SLOTS[0], "mcl_svd_init: ", {k: v for k, v in SVD_GOOD.items() if k != "xt"}, SVD_REFUSALS,
          ("X", "rp", "B", "C", "ws", "info")),
]

# ---- mcl_als_init_typed -------------------------------------------------------------------------------------------------------
ALS_WANT = als_bytes(ROWS, K, R)
ALS_SHAPE = [
    (dict(rp=None), PACKED_HEAD), (dict(I=0), PACKED_HEAD), (dict(K=0), PACKED_HEAD),
    (dict(rank=0), "need 1 <= rank <= 64"), (dict(rank=65), "need 1 <= rank <= 64"),
    (dict(rp=rp([1, 3, 70, 75])), FIRST_ZERO), (dict(rp=rp([0, 3, 2, 75])), NOT_DECREASING),
    (dict(K=2049), "K and the longest matrix must be at most 2048 (the start's Gram matrices)"),
    (dict(rp=rp([0, 3, 70, 3000])), "K and the longest matrix must be at most 2048 (the start's Gram matrices)"),
    (dict(rank=6), "rank exceeds min(longest matrix, K)"), (dict(rp=rp([0, 1, 2, 3]), rank=2), "rank exceeds min(longest matrix, K)"),
    (dict(rp=lambda: rp_steps(1 << 20, 2048), I=1 << 20), ROWS_2_31)]
ENTRIES.append(Entry(
    "mcl_als_init_typed", SLOTS[1], "mcl_als_init: ",
    dict(X=FAKE, xt=0, rp=GOOD, I=I, K=K, rank=R, method=0, n_iter_max=3, tol=1e-8, A=FAKE, B=FAKE, C=FAKE, errors=FAKE, info=FAKE,
         **packed_tail(ALS_WANT)),
    ALS_SHAPE + [(dict(xt=7), x_type(7)), (dict(method=2), "unknown method 2 (MCL_ALS_CP = 0, MCL_ALS_CP_HALS = 1)"),
                 (dict(n_iter_max=-1), "need n_iter_max >= 0 and tol >= 0"), (dict(tol=-1.0), "need n_iter_max >= 0 and tol >= 0"),
                 (dict(tol=float("nan")), "need n_iter_max >= 0 and tol >= 0")] + workspace_refusals(ALS_WANT, "mcl_als_init_workspace_bytes"),
    ("X", "A", "B", "C", "info", "ws")))

# ---- mcl_parafac2_als_typed ---------------------------------------------------------------------------------------------------
PA_WANT = pf2als_bytes(ROWS, K, R)
AT_LEAST_RANK, RANK_ABOVE_K = "every matrix needs at least rank rows", "rank exceeds K"
PA_SHAPE = [
    (dict(rp=None), PACKED_HEAD), (dict(I=0), PACKED_HEAD), (dict(K=0), PACKED_HEAD),
    (dict(rank=0), "need 1 <= rank <= 32"), (dict(rank=33), "need 1 <= rank <= 32"),
    (dict(rp=rp([1, 3, 70, 75])), FIRST_ZERO), (dict(rank=4), AT_LEAST_RANK), (dict(rp=rp([0, 3, 2, 75])), AT_LEAST_RANK),
    (dict(K=2), RANK_ABOVE_K), (dict(rp=rp([0, 3, 70, 1 << 26])), ROWS_2_26),
    (dict(rp=lambda: rp_steps(1 << 25, 1), I=1 << 25, rank=1), "more than 2^25 matrices are not supported")]
PA_OPTIONS = [(dict(nn_modes=2), "nn_modes may hold modes 0 and 2 only (bits 1 and 4)")] + [
    (change, "need n_iter_max >= 1, n_iter_parafac >= 1, tol >= 0 and absolute_tol >= 0")
    for change in (dict(n_iter_max=0), dict(n_iter_parafac=0), dict(tol=-1.0), dict(tol=float("nan")), dict(absolute_tol=-1.0))]
ENTRIES.append(Entry(
    "mcl_parafac2_als_typed", SLOTS[2], "mcl_parafac2_als: ",
    dict(X=FAKE, xt=0, rp=GOOD, I=I, K=K, rank=R, A0=None, B0=None, C0=None, n_iter_max=3, n_iter_parafac=1, tol=1e-8, absolute_tol=1e-13,
         nn_modes=0, A=FAKE, B=FAKE, C=FAKE, P=FAKE, errors=FAKE, info=FAKE, **packed_tail(PA_WANT)),
    PA_SHAPE + [(dict(A0=FAKE), "give all of A0, B0, C0 or none"), (dict(B0=FAKE, C0=FAKE), "give all of A0, B0, C0 or none"),
                (dict(K=2049), "the svd start needs K <= 2048"), (dict(xt=7), x_type(7))] + PA_OPTIONS
    + workspace_refusals(PA_WANT, "mcl_parafac2_als_workspace_bytes"),
    ("X", "A", "B", "C", "P", "errors", "info", "ws")))

# ---- mcl_multistart_run, _run_grid, _run_weighted -----------------------------------------------------------------------------
MS_HEAD = "need row_ptr, options, I >= 1, K >= 1"
MS_RANK = "need 1 <= rank <= 16"


def ms_shape(job=""):
    return [(dict(rp=None), job + MS_HEAD), (dict(I=0), job + MS_HEAD), (dict(K=0), job + MS_HEAD),
            (dict(rank=0), job + MS_RANK), (dict(rank=17), job + MS_RANK),
            (dict(rp=rp([1, 3, 70, 75])), job + FIRST_ZERO), (dict(rp=rp([0, 3, 2, 75])), job + NOT_DECREASING),
            (dict(rp=rp([0, 3, 70, 1 << 31])), job + ROWS_2_31)]


def ms_good(n, want, **extra):
    d = dict(X=FAKE, xt=0, rp=GOOD, I=I, K=K, rank=R, opt=options(n if "grid" in extra else 1), n=n)
    extra.pop("grid", None)
    d.update(extra)
    d.update(state=FAKE, diag=FAKE, n_iter=FAKE, stop=FAKE, **packed_tail(want))
    return d


MS_NOT_NULL = ("X", "state", "diag", "n_iter", "stop", "ws")
MS_WANT = multistart_bytes(ROWS, K, R, 2)
MS_GRID_WANT = MS_WANT + al(2 * _engine.MS_OPTIONS_BYTES)
MS_WEIGHTED_WANT = MS_WANT + al(2 * I * 8)
ENTRIES.append(Entry(
    "mcl_multistart_run", SLOTS[3], "mcl_multistart_run: ", ms_good(2, MS_WANT),
    ms_shape() + [(dict(opt=None), MS_HEAD), (dict(n=0), "need n_starts >= 1")]
    + [(dict(opt=options(1, **f)), m) for f, m in MS_OPTION_REFUSALS]
    + [(dict(opt=options(1, **PF2_ON_B), rank=4), "PARAFAC2 needs every J_i >= rank"), (dict(xt=7), x_type(7))]
    + workspace_refusals(MS_WANT, "mcl_multistart_workspace_bytes"), MS_NOT_NULL))
ENTRIES.append(Entry(
    "mcl_multistart_run_grid", SLOTS[3], "mcl_multistart_run_grid: ", ms_good(2, MS_GRID_WANT, grid=True),
    ms_shape("job 0: ") + [(dict(opt=None), "need options and n_jobs >= 1"), (dict(n=0), "need options and n_jobs >= 1")]
    + [(dict(opt=options(2, only=1, **f)), "job 1: " + m) for f, m in MS_OPTION_REFUSALS]
    + [(dict(opt=options(2, **PF2_ON_B), rank=4), "job 0: PARAFAC2 needs every J_i >= rank"), (dict(xt=7), x_type(7))]
    + [(dict(opt=options(2, only=1, **f)), "job 1 differs from job 0 in n_regs, a penalty's kind or non_negativity, constant_A/B or "
        "update_A/B/C: the jobs of a grid share one state layout")
       for f in (dict(constant_A=1), dict(update_C=0), dict(n_regs=(1, 0, 0), regs={(0, 0): PEN.PEN_NN}))]
    + workspace_refusals(MS_GRID_WANT, "mcl_multistart_grid_workspace_bytes"), MS_NOT_NULL))
ENTRIES.append(Entry(
    "mcl_multistart_run_weighted", SLOTS[3], "mcl_multistart_run_weighted: ", ms_good(2, MS_WEIGHTED_WANT, w=weights(np.ones((2, I)))),
    ms_shape() + [(dict(opt=None), MS_HEAD), (dict(n=0), "need n_starts >= 1")]
    + [(dict(opt=options(1, **f)), m) for f, m in MS_OPTION_REFUSALS]
    + [(dict(w=None), "NULL slab_weights"), (dict(w=weights([[1, 1, 1], [1, 1, -1]])), "slab_weights[1][2] is negative or not finite"),
       (dict(w=weights([[1, np.inf, 1], [1, 1, 1]])), "slab_weights[0][1] is negative or not finite"),
       (dict(w=weights([[1, 0, 1], [0, 0, 0]])), "job 1 has no positive weight"), (dict(xt=7), x_type(7))]
    + workspace_refusals(MS_WEIGHTED_WANT, "mcl_multistart_weighted_workspace_bytes"), MS_NOT_NULL))

# ---- mcl_pf2als_multistart_run, _run_weighted ---------------------------------------------------------------------------------
PM_WANT = pf2als_multistart_bytes(ROWS, K, R, 2)
PM_SHAPE = [
    (dict(rp=None), PACKED_HEAD), (dict(I=0), PACKED_HEAD), (dict(K=0), PACKED_HEAD), (dict(rank=0), MS_RANK), (dict(rank=17), MS_RANK),
    (dict(n=0), "need n_starts >= 1"), (dict(rp=rp([1, 3, 70, 75])), FIRST_ZERO), (dict(rank=4), AT_LEAST_RANK),
    (dict(rp=rp([0, 3, 2, 75])), AT_LEAST_RANK), (dict(K=2), RANK_ABOVE_K), (dict(rp=rp([0, 3, 70, 1 << 31])), ROWS_2_31)]
PM_REST = [(dict(xt=7), x_type(7))] + PA_OPTIONS + workspace_refusals(PM_WANT, "mcl_pf2als_multistart_workspace_bytes")
PM_NOT_NULL = ("X", "factors", "P", "errors", "n_iter", "ws")


def pm_good(**extra):
    return dict(X=FAKE, xt=0, rp=GOOD, I=I, K=K, rank=R, n=2, **extra, n_iter_max=3, n_iter_parafac=1, tol=1e-8, absolute_tol=1e-13,
                nn_modes=0, factors=FAKE, P=FAKE, errors=FAKE, n_iter=FAKE, **packed_tail(PM_WANT))


ENTRIES.append(Entry("mcl_pf2als_multistart_run", SLOTS[4], "mcl_pf2als_multistart_run: ", pm_good(), PM_SHAPE + PM_REST, PM_NOT_NULL))
ENTRIES.append(Entry(
    "mcl_pf2als_multistart_run_weighted", SLOTS[4], "mcl_pf2als_multistart_run_weighted: ", pm_good(scale=FAKE),
    PM_SHAPE + [(dict(scale=None), "slab_scale is NULL (a device array [n_starts, I] of the square roots of the weights)")] + PM_REST,
    PM_NOT_NULL))

# ---- mcl_fms_scores (no X, no row_ptr, a workspace without a size argument) ---------------------------------------------------
PAIRS = np.array([[0, 1], [2, 3]], dtype=np.int32)
pairs_of = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
BAD_PAIRS = np.array([[0, 1], [5, 3]], dtype=np.int32)
FMS_RANK = lambda r: f"rank {r} is outside 1 ... 16"
ENTRIES.append(Entry(
    "mcl_fms_scores", SLOTS[5], "mcl_fms_scores: ",
    dict(models=FAKE, n_models=4, I=I, N=N, K=K, rank=R, weights=None, pairs=pairs_of(PAIRS), n_pairs=2, flags=0, skip_mode=-1, score=FAKE,
         perm=None, ws=FAKE, stream=None),
    [(dict(rank=0), FMS_RANK(0)), (dict(rank=17), FMS_RANK(17)), (dict(n_models=0), "n_models 0 is outside 1 ... 2^31 - 1"),
     (dict(n_models=1 << 31), f"n_models {1 << 31} is outside 1 ... 2^31 - 1"),
     (dict(I=0), "need I >= 1, N >= 1 and K >= 1"), (dict(N=0), "need I >= 1, N >= 1 and K >= 1"), (dict(K=0), "need I >= 1, N >= 1 and K >= 1"),
     (dict(N=(1 << 31) // 3), "a model of (I + N + K) * rank >= 2^31 elements"), (dict(n_pairs=-1), "n_pairs -1 is out of range"),
     (dict(flags=4), "flags may hold bit 0 (consider_weights) and bit 1 (absolute_value) only"),
     (dict(skip_mode=3), "skip_mode must be -1 (none), 0, 1 or 2"), (dict(skip_mode=-2), "skip_mode must be -1 (none), 0, 1 or 2"),
     (dict(ws=FAKE + 8), ALIGNED), (dict(pairs=pairs_of(BAD_PAIRS)), "pair 1 names model 5 of 4")],
    ("models", "ws", "pairs", "score")))

# ---- mcl_eval_tables_typed, mcl_eval_core -------------------------------------------------------------------------------------
EV_WANT = eval_bytes(ROWS, K, R, 2)
EV_RANK = lambda r: f"rank {r} is outside 1 ... 32"
EV_SHAPE = [
    (dict(rank=0), EV_RANK(0)), (dict(rank=33), EV_RANK(33)), (dict(n_models=0), "n_models 0 is outside 1 ... 65535"),
    (dict(n_models=65536), "n_models 65536 is outside 1 ... 65535"), (dict(I=0), "need I >= 1 and K >= 1"), (dict(K=0), "need I >= 1 and K >= 1"),
    (dict(I=65536), "more than 65535 matrices are not supported"), (dict(K=1 << 25), "K >= 2^25 is not supported")]
ENTRIES.append(Entry(
    "mcl_eval_tables_typed", SLOTS[6], "mcl_eval_tables_typed: ",
    dict(X=FAKE, xt=0, rp=GOOD, I=I, K=K, rank=R, models=FAKE, n_models=2, S=FAKE, BtB=FAKE, sse=FAKE, norm=FAKE, **packed_tail(EV_WANT)),
    EV_SHAPE + [(dict(rp=None), "row_ptr is NULL"), (dict(rp=rp([1, 3, 70, 75])), FIRST_ZERO),
                (dict(rp=rp([0, 3, 3, 75])), "row_ptr must increase: matrix 1 has no rows"),
                (dict(rp=rp([0, 3, 2, 75])), "row_ptr must increase: matrix 1 has no rows"), (dict(rp=rp([0, 3, 70, 1 << 26])), ROWS_2_26),
                (dict(rp=rp([0, (1 << 26) - 1]), I=1, n_models=65535), "too many (model, segment) pairs for one launch"),
                (dict(xt=7), x_type(7))] + workspace_refusals(EV_WANT, "mcl_eval_workspace_bytes"),
    ("X", "models", "S", "BtB", "sse", "norm", "ws")))
ENTRIES.append(Entry(
    "mcl_eval_core", SLOTS[6], "mcl_eval_core: ",
    dict(models=FAKE, n_models=2, I=I, N=N, K=K, rank=R, S=FAKE, BtB=FAKE, core=FAKE, cc=FAKE, ccn=FAKE, stream=None),
    EV_SHAPE + [(dict(N=2), "need I <= N < 2^26 packed rows"), (dict(N=1 << 26), "need I <= N < 2^26 packed rows")],
    ("models", "S", "BtB", "core", "cc", "ccn")))

# ---- mcl_pf2_project_typed ----------------------------------------------------------------------------------------------------
PJ_WANT = project_bytes(ROWS, K, R)
ENTRIES.append(Entry(
    "mcl_pf2_project_typed", SLOTS[7], "mcl_pf2_project: ",
    dict(X=FAKE, xt=0, rp=GOOD, I=I, K=K, rank=R, Delta=FAKE, C=FAKE, a_init=FAKE, n_iter_max=10, tol=1e-8, absolute_tol=1e-13, A=FAKE, B=FAKE,
         P=FAKE, stats=FAKE, n_iter=FAKE, errors=None, **packed_tail(PJ_WANT)),
    [(dict(rp=None), PACKED_HEAD), (dict(I=0), PACKED_HEAD), (dict(K=0), PACKED_HEAD), (dict(rank=0), EV_RANK(0)), (dict(rank=33), EV_RANK(33)),
     (dict(rp=rp([1, 3, 70, 75])), FIRST_ZERO), (dict(rank=4), AT_LEAST_RANK + " (matrix 0)"),
     (dict(rp=rp([0, 3, 2, 75])), AT_LEAST_RANK + " (matrix 1)"),
     (dict(K=2), "rank 3 exceeds K = 2: W = X C has rank K and no orthonormal P exists"), (dict(rp=rp([0, 3, 70, 1 << 26])), ROWS_2_26),
     (dict(K=1 << 26), "K of 2^26 or more is not supported"), (dict(xt=7), x_type(7))]
    + [(change, "need n_iter_max >= 1, tol >= 0 and absolute_tol >= 0")
       for change in (dict(n_iter_max=0), dict(tol=-1.0), dict(tol=float("nan")), dict(absolute_tol=-1.0))]
    + workspace_refusals(PJ_WANT, "mcl_pf2_project_workspace_bytes"),
    ("X", "Delta", "C", "a_init", "A", "B", "P", "stats", "n_iter", "ws")))

CASES = [(e, change, message) for e in ENTRIES for change, message in e.refusals]


def _case_id(case):
    e, change, _ = case
    return e.name[4:] + "-" + ",".join(f"{k}={'...' if not isinstance(v, (int, float, type(None))) else v}" for k, v in change.items())


def _slots(lib):
    return {name: getattr(lib, name)() for name in SLOTS}


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_refusal_names_its_entry_in_its_own_slot(case):
    entry, change, message = case
    lib = _engine.load_library()
    args = {**entry.good, **{k: v() if callable(v) else v for k, v in change.items()}}
    before = _slots(lib)
    rc = getattr(lib, entry.name)(*args.values())
    after = _slots(lib)
    assert rc != 0
    assert after[entry.slot].decode() == entry.prefix + message
    assert {n: t for n, t in after.items() if n != entry.slot} == {n: t for n, t in before.items() if n != entry.slot}


def test_every_family_and_entry_is_in_the_table():
    assert {e.slot for e in ENTRIES} == set(SLOTS)
    assert {e.name for e in ENTRIES} == {
        "mcl_svd_init", "mcl_svd_init_typed", "mcl_als_init_typed", "mcl_parafac2_als_typed", "mcl_multistart_run", "mcl_multistart_run_grid",
        "mcl_multistart_run_weighted", "mcl_pf2als_multistart_run", "mcl_pf2als_multistart_run_weighted", "mcl_fms_scores",
        "mcl_eval_tables_typed", "mcl_eval_core", "mcl_pf2_project_typed"}


# ---- the sizers: the documented layout for a good call, -1 for what the run refuses by shape ----------------------------------
def _plain(name):
    return lambda rows, I_, K_, r: getattr(_engine.load_library(), name)(rows, I_, K_, r)


def _with_starts(name, n=2):
    return lambda rows, I_, K_, r: getattr(_engine.load_library(), name)(rows, I_, K_, r, n)


def _with_options(name, opt, n=2):
    return lambda rows, I_, K_, r: getattr(_engine.load_library(), name)(rows, I_, K_, r, opt, n)


# (the sizer, the bytes of the good call, the rank one above the family's limit)
SIZERS = {
    "mcl_svd_init_workspace_bytes": (_plain("mcl_svd_init_workspace_bytes"), SVD_WANT, None),  # (no upper limit: the run refuses)
    "mcl_als_init_workspace_bytes": (_plain("mcl_als_init_workspace_bytes"), ALS_WANT, 65),
    "mcl_parafac2_als_workspace_bytes": (_plain("mcl_parafac2_als_workspace_bytes"), PA_WANT, 33),
    "mcl_multistart_workspace_bytes": (_with_options("mcl_multistart_workspace_bytes", options(1)), MS_WANT, 17),
    "mcl_multistart_grid_workspace_bytes": (_with_options("mcl_multistart_grid_workspace_bytes", options(2)), MS_GRID_WANT, 17),
    "mcl_multistart_weighted_workspace_bytes": (_with_options("mcl_multistart_weighted_workspace_bytes", options(1)), MS_WEIGHTED_WANT, 17),
    "mcl_pf2als_multistart_workspace_bytes": (_with_starts("mcl_pf2als_multistart_workspace_bytes"), PM_WANT, 17),
    "mcl_eval_workspace_bytes": (_with_starts("mcl_eval_workspace_bytes"), EV_WANT, 33),
    "mcl_pf2_project_workspace_bytes": (_plain("mcl_pf2_project_workspace_bytes"), PJ_WANT, 33),
}


@pytest.mark.parametrize("name", sorted(SIZERS))
def test_sizer_gives_the_documented_layout_and_refuses_with_minus_one(name):
    size, want, above = SIZERS[name]
    assert size(GOOD, I, K, R) == want
    assert size(None, I, K, R) == -1 and size(GOOD, 0, K, R) == -1 and size(GOOD, I, 0, R) == -1 and size(GOOD, I, K, 0) == -1
    if above is not None:
        assert size(GOOD, I, K, above) == -1 and size(rp([0, 70, 140, 210]), I, 70, above) == -1  # (the rank alone: rows and K allow it)
    else:
        assert size(GOOD, I, K, 65) == svd_bytes(ROWS, K, 65)


def test_sizers_at_rank_17_where_the_family_allows_it():
    lib = _engine.load_library()
    assert lib.mcl_eval_workspace_bytes(GOOD, I, K, 17, 2) == eval_bytes(ROWS, K, 17, 2)  # (no rank <= K, no rows >= rank)
    assert lib.mcl_svd_init_workspace_bytes(GOOD, I, K, 17) == svd_bytes(ROWS, K, 17)
    tall = [0, 17, 84, 110]  # ... and on matrices and columns that allow it: 17 <= rows, K = 20
    assert lib.mcl_als_init_workspace_bytes(rp(tall), I, 20, 17) == als_bytes(tall, 20, 17)
    assert lib.mcl_parafac2_als_workspace_bytes(rp(tall), I, 20, 17) == pf2als_bytes(tall, 20, 17)
    assert lib.mcl_pf2_project_workspace_bytes(rp(tall), I, 20, 17) == project_bytes(tall, 20, 17)
    assert lib.mcl_eval_workspace_bytes(rp(tall), I, 20, 17, 2) == eval_bytes(tall, 20, 17, 2)
    for name in ("mcl_als_init_workspace_bytes", "mcl_parafac2_als_workspace_bytes", "mcl_pf2_project_workspace_bytes"):
        assert getattr(lib, name)(GOOD, I, K, 17) == -1  # rank > K, and fewer rows than the rank


def test_sizers_refuse_the_shapes_the_run_refuses():
    lib = _engine.load_library()
    short, first, back = rp([0, 2, 70, 75]), rp([1, 3, 70, 75]), rp([0, 3, 2, 75])
    for name in ("mcl_parafac2_als_workspace_bytes", "mcl_pf2_project_workspace_bytes"):
        assert [getattr(lib, name)(r_, I, K, R) for r_ in (short, first, back)] == [-1, -1, -1] and getattr(lib, name)(GOOD, I, 2, R) == -1
    assert [lib.mcl_pf2als_multistart_workspace_bytes(r_, I, K, R, 2) for r_ in (short, first, back)] == [-1, -1, -1]
    assert lib.mcl_pf2als_multistart_workspace_bytes(GOOD, I, 2, R, 2) == -1 and lib.mcl_pf2als_multistart_workspace_bytes(GOOD, I, K, R, 0) == -1
    assert lib.mcl_als_init_workspace_bytes(short, I, K, R) == als_bytes([0, 2, 70, 75], K, R)  # short matrices are allowed
    assert lib.mcl_als_init_workspace_bytes(first, I, K, R) == -1 and lib.mcl_als_init_workspace_bytes(back, I, K, R) == -1
    assert lib.mcl_als_init_workspace_bytes(GOOD, I, 2049, R) == -1 and lib.mcl_als_init_workspace_bytes(GOOD, I, K, 6) == -1
    assert lib.mcl_eval_workspace_bytes(rp([0, 3, 3, 75]), I, K, R, 2) == -1 and lib.mcl_eval_workspace_bytes(first, I, K, R, 2) == -1
    assert lib.mcl_eval_workspace_bytes(GOOD, I, K, R, 0) == -1 and lib.mcl_eval_workspace_bytes(GOOD, I, K, R, 65536) == -1
    one = options(1)
    for name in ("mcl_multistart_workspace_bytes", "mcl_multistart_weighted_workspace_bytes", "mcl_multistart_grid_workspace_bytes"):
        size = getattr(lib, name)
        assert size(first, I, K, R, one, 1) == -1 and size(back, I, K, R, one, 1) == -1 and size(GOOD, I, K, R, one, 0) == -1
        assert size(GOOD, I, K, R, None, 1) == -1 and size(GOOD, I, K, R, options(1, n_regs=(5, 0, 0)), 1) == -1
        assert size(short, I, K, R, one, 1) > 0 and size(short, I, K, R, options(1, **PF2_ON_B), 1) == -1
    assert lib.mcl_multistart_grid_workspace_bytes(GOOD, I, K, R, options(2, only=1, constant_A=1), 2) == -1
    assert lib.mcl_fms_workspace_bytes(4, R) == 4 * 64 * 8 and lib.mcl_fms_workspace_bytes(4, 16) == 4 * 64 * 8
    assert [lib.mcl_fms_workspace_bytes(4, 0), lib.mcl_fms_workspace_bytes(4, 17), lib.mcl_fms_workspace_bytes(0, R)] == [-1, -1, -1]
