"""`cmf_aoadmm` / `parafac2_aoadmm` on the MI355X engine.

Same signature, defaults, return types, error behaviour and stopping rules as
/root/reference/src/matcouply/decomposition.py (`cmf_aoadmm` :662-1100, `parafac2_aoadmm` :1103-1179,
`compute_feasibility_gaps` :351-417, `ADMMVars` :643-645, `DiagnosticMetrics` :648-659).  The host side only
parses arguments, draws the initial state with the reference's RNG order (:35-37, :904-905), keeps the loss /
stopping bookkeeping (:990-1053) and converts results; every per-mode ADMM update runs in the HIP library
(matcouply_amd/_engine.py -> libmatcouply_hip.so).  There is no CPU fallback.

Extensions (keyword-only, not in the reference): `group=` a torch.distributed process group - every rank passes
ITS OWN contiguous range of the I matrices; the replicated C-mode normal equations and the diagnostic sums are
all-reduced over the group (RCCL on MI355X, gloo in the CPU tests).
"""
from copy import copy
import inspect
import os
from types import SimpleNamespace
from typing import NamedTuple, Optional
import warnings

import numpy as np

from . import _engine, penalties
from ._utils import check_random_state, get_svd, is_iterable, is_tensor, is_torch, shape, to_numpy, torch
from .coupled_matrices import CoupledMatrixFactorization

__all__ = ["compute_feasibility_gaps", "ADMMVars", "DiagnosticMetrics", "cmf_aoadmm", "parafac2_aoadmm",
           "PackedMatrices", "partition_slabs", "parafac2_als", "parafac2_als_multistart",
           "cmf_aoadmm_grid", "parafac2_aoadmm_grid", "best_start"]

# TEST-ONLY seam.  The CPU test-suite (tests/oracle_engine.py) substitutes a checker engine here to exercise the host and
# multi-process logic without a GPU.  The substitution is honoured only under MATCOUPLY_AMD_TEST_ENGINE=1, which
# tests/conftest.py sets and the product never does: matcouply_amd has no CPU path of its own.
_ENGINE_FACTORY = None


# arithmetic="auto" (see cmf_aoadmm): problems of at most 2^20 elements always take the exact arithmetic (the library's own rule);
# up to _AUTO_EXACT_MAX_ELEMENTS a penalty-free mode whose normal equations have kappa = ||M||_F ||M^-1||_F above
# _AUTO_EXACT_KAPPA moves the run there; larger problems are only warned, above _AUTO_EXACT_WARN_KAPPA
_AUTO_EXACT_MAX_ELEMENTS = float(1 << 24)
_AUTO_EXACT_KAPPA = 1e3
_AUTO_EXACT_POLAR = 1e5  # ... or a PARAFAC2 polar factor (||sigma|| / sigma_min of Y_i Delta^T) above this
_AUTO_EXACT_WARN_KAPPA = 1e6
_AUTO_EXACT_PROBE_EVERY = 64
_AUTO_EXACT_TRIAL_ITERATIONS = 2


def _test_engine_factory():
    if _ENGINE_FACTORY is None:
        return None
    if os.environ.get("MATCOUPLY_AMD_TEST_ENGINE") != "1":
        raise RuntimeError("a substitute compute engine is installed outside the test-suite: matcouply_amd runs on the "
                           "HIP engine only (set MATCOUPLY_AMD_TEST_ENGINE=1 in a test harness to allow a checker)")
    return _ENGINE_FACTORY


def partition_slabs(n_rows, world_size, contiguous=True):
    """Split the I coupled matrices over `world_size` ranks so that every rank holds about the same number of ROWS
    (sum of J_i) - the per-rank work of every phase is proportional to its rows, not to its number of matrices.

    n_rows: J_i for every matrix (or anything with a `.shape[0]`).  Returns a list of `world_size` index arrays; rank k
    passes `[matrices[i] for i in parts[k]]` to `cmf_aoadmm(..., group=pg)` (the rows of A come back in that order).

    contiguous=True   consecutive ranges [lo_k, hi_k): the cut after slab i is placed where the prefix sum of rows is
                      closest to k / world_size of the total (keeps the matrices in order; imbalance <= max J_i / 2 rows);
    contiguous=False  longest-processing-time greedy (largest matrix first onto the least loaded rank; indices sorted
                      within a rank): within a fraction of a percent for ragged J_i such as BASELINE config 4.
    """
    J = np.asarray([getattr(m, "shape", (m,))[0] if not np.isscalar(m) else m for m in n_rows], dtype=np.int64)
    I, W = len(J), int(world_size)
    if W < 1:
        raise ValueError("world_size must be positive")
    if contiguous:
        prefix = np.concatenate([[0], np.cumsum(J)])
        total = prefix[-1]
        cuts = [0]
        for k in range(1, W):
            target = total * k / W
            i = int(np.searchsorted(prefix, target))
            if i > 0 and abs(prefix[i - 1] - target) <= abs(prefix[min(i, I)] - target):
                i -= 1
            cuts.append(min(max(i, cuts[-1]), I))
        cuts.append(I)
        return [np.arange(cuts[k], cuts[k + 1], dtype=np.int64) for k in range(W)]
    load = np.zeros(W, dtype=np.int64)
    parts = [[] for _ in range(W)]
    for i in np.argsort(-J, kind="stable"):
        k = int(np.argmin(load))
        parts[k].append(int(i))
        load[k] += J[i]
    return [np.array(sorted(p), dtype=np.int64) for p in parts]


class PackedMatrices:
    """The I coupled matrices already packed along rows in device memory: X [sum J_i, K] float32, bfloat16 or float16
    (contiguous torch CUDA tensor; a 16-bit X stays 16-bit, every kernel reads it as such) + row_ptr [I+1].  Behaves like the list of the I matrices (len / iteration / indexing give views),
    and lets callers that keep their data in HBM skip the host-side packing."""

    def __init__(self, X, row_ptr):
        self.X = X
        self.row_ptr = np.ascontiguousarray(row_ptr, dtype=np.int64)
        if self.row_ptr[0] != 0 or self.row_ptr[-1] != X.shape[0]:
            raise ValueError("row_ptr must start at 0 and end at X.shape[0]")

    def __len__(self):
        return len(self.row_ptr) - 1

    def __getitem__(self, i):
        return self.X[self.row_ptr[i]: self.row_ptr[i + 1]]

    def __iter__(self):
        for i in range(len(self)):
            yield self[i]


# ------------------------------------------------------------------------------------------------------------
# initialisation (decomposition.py:18-89)
# ------------------------------------------------------------------------------------------------------------
def _data_on_device(matrices):
    """the matrices already live in HBM: a PackedMatrices, or torch CUDA tensors"""
    if isinstance(matrices, PackedMatrices):
        return is_torch(matrices.X) and matrices.X.is_cuda
    try:
        return len(matrices) > 0 and all(is_torch(m) and m.is_cuda for m in matrices)
    except TypeError:
        return False


_DEVICE_SVD_MAX_K = 2048  # the device initialiser keeps K x K fp64 Gram matrices per matrix in flight (32 MB each at this K)


def _device_svd_applies(matrices, rank):
    """The device form of init="svd" serves the shapes its subspace iteration covers: rank > K, a matrix with fewer rows than
    components, or a K whose Gram matrices would not fit the initialiser's workspace take the host path, as the reference does
    (ADVICE r5).  (`svd=` only names the driver: every valid name is the same thin LAPACK SVD on the host, _utils.get_svd.)"""
    try:
        K = int(shape(matrices[0])[1])
        rows = [int(shape(m)[0]) for m in matrices] if not isinstance(matrices, PackedMatrices) else \
            [int(matrices.row_ptr[i + 1] - matrices.row_ptr[i]) for i in range(len(matrices))]
    except Exception:
        return False
    return rank <= K <= _DEVICE_SVD_MAX_K and min(rows) >= rank


# init= names of the CP initialisers (reference decomposition.py:64-73): the aliases name the same method
_CP_INITS = {"parafac_als": _engine.ALS_CP, "cp_als": _engine.ALS_CP, "parafac_hals": _engine.ALS_CP_HALS,
             "cp_hals": _engine.ALS_CP_HALS}


def _cp_init_options(matrices, rank, init, init_params):
    """(method, n_iter_max, tol) of a CP initialiser, or NotImplementedError for what the device form does not serve: init_params
    other than n_iter_max (default 50, as the reference sets it) and tol (TensorLy's defaults: 1e-8 for ALS, 1e-7 for HALS),
    and shapes where TensorLy would fill the start with random columns (rank > min(max J_i, K)) or whose Gram matrices exceed
    the start's bound (K or max J_i above _DEVICE_SVD_MAX_K, rank above 64)."""
    method = _CP_INITS[init]
    params = dict(init_params or {})
    n_iter_max = params.pop("n_iter_max", 50)
    tol = params.pop("tol", 1e-8 if method == _engine.ALS_CP else 1e-7)
    if params:
        raise NotImplementedError(
            f'init="{init}": init_params {sorted(params)} not supported (only "n_iter_max" and "tol"; TensorLy options such '
            "as normalize_factors, svd or linesearch are not served)")
    if int(n_iter_max) != n_iter_max or n_iter_max < 0:
        raise ValueError(f"init_params['n_iter_max'] must be a non-negative integer, not {n_iter_max!r}")
    tol = 0.0 if tol is None else float(tol)
    if not tol >= 0:
        raise ValueError(f"init_params['tol'] must be non-negative, not {tol!r}")
    K = int(shape(matrices[0])[1])
    rows = [int(shape(m)[0]) for m in matrices] if not isinstance(matrices, PackedMatrices) else \
        [int(matrices.row_ptr[i + 1] - matrices.row_ptr[i]) for i in range(len(matrices))]
    J_max = max(rows)
    if rank > min(J_max, K):
        raise NotImplementedError(
            f'init="{init}": rank {rank} exceeds min(max J_i, K) = {min(J_max, K)} (TensorLy would pad the start with random '
            "columns); pass an explicit (weights, (A, B_is, C)) tuple instead.")
    if K > _DEVICE_SVD_MAX_K or J_max > _DEVICE_SVD_MAX_K or rank > 64:
        raise NotImplementedError(
            f'init="{init}": the device start needs K <= {_DEVICE_SVD_MAX_K}, max J_i <= {_DEVICE_SVD_MAX_K} and rank <= 64 '
            f"(K = {K}, max J_i = {J_max}, rank = {rank})")
    return method, int(n_iter_max), tol


def initialize_cmf(matrices, rank, init, svd_fun, random_state=None, init_params=None):
    random_state = check_random_state(random_state)
    if isinstance(init, (tuple, list, CoupledMatrixFactorization)):
        weights, (A, B_is, C) = init
        if weights is not None:
            scaled_A = weights * A
            return CoupledMatrixFactorization((None, (scaled_A, B_is, C)))
        return CoupledMatrixFactorization(init)
    if init == "random":
        I = len(matrices)
        K = shape(matrices[0])[1]
        A = random_state.uniform(size=(I, rank))
        C = random_state.uniform(size=(K, rank))
        B_is = [random_state.uniform(size=(shape(matrix)[0], rank)) for matrix in matrices]
        return CoupledMatrixFactorization((None, [A, B_is, C]))
    if (init == "svd" or init == "threshold_svd") and _data_on_device(matrices) and _device_svd_applies(matrices, rank):
        # data resident in HBM: the singular vectors on the device, no copy of X to the host (mcl_svd_init: fp64 subspace
        # iteration on the Gram matrices).  The vectors are LAPACK's up to their SIGNS (largest-magnitude entry positive here):
        # B_i and C come from independent decompositions, so the reference's trajectory from this initialiser is reproduced
        # by the host path below only - which host-resident data keeps taking.
        X, row_ptr = _pack(matrices, _device())
        B, C, info = _engine.svd_init(X, row_ptr, rank, threshold=(init == "threshold_svd"))
        info_min = int(info.min().item())
        if info_min <= -1000:
            warnings.warn("svd initialisation on the device: a matrix has numerical rank below `rank` (its trailing singular "
                          "vectors are not determined by the data); taking the host (LAPACK) path, which completes the basis",
                          RuntimeWarning)
        else:
            if info_min < 0:
                    warnings.warn("svd initialisation on the device: the subspace iteration of some matrices had not settled after 400 "
                              "iterations (no gap behind the leading singular values); the vectors are approximate", RuntimeWarning)
            A = torch.ones((len(row_ptr) - 1, rank), dtype=torch.float32, device=X.device)
            B_is = [B[int(row_ptr[i]): int(row_ptr[i + 1])] for i in range(len(row_ptr) - 1)]
            return CoupledMatrixFactorization((None, [A, B_is, C]))
    if init == "svd" or init == "threshold_svd":
        # one-off set-up on the host (decomposition.py:42-53)
        if svd_fun is None:
            svd_fun = get_svd("truncated_svd")
        mats = [np.asarray(to_numpy(m.float() if is_torch(m) and m.dtype == torch.bfloat16 else m), dtype=np.float64)
                for m in matrices]  # (NumPy has no bfloat16: exact upcast first)
        A = np.ones((len(mats), rank))
        B_is = [svd_fun(m, n_eigenvecs=rank)[0] for m in mats]
        C = svd_fun(np.concatenate(mats, 0), n_eigenvecs=rank)[2].T
        if init == "threshold_svd":
            B_is = [np.clip(B_i, 0, float("inf")) for B_i in B_is]
            C = np.clip(C, 0, float("inf"))
        return CoupledMatrixFactorization((None, [A, B_is, np.ascontiguousarray(C)]))
    if init in _CP_INITS:
        # CP-ALS / CP-HALS on the zero-padded tensor (reference: TensorLy's parafac / non_negative_parafac_hals,
        # decomposition.py:64-73), on the device (mcl_als_init): every limit and option is checked before the device is touched
        method, n_iter_max, tol = _cp_init_options(matrices, rank, init, init_params)
        X, row_ptr = _pack(matrices, _device())
        A, B, C, _ = _engine.als_init(X, row_ptr, rank, method, n_iter_max, tol)
        out = _Out(matrices)
        return CoupledMatrixFactorization((None, [out(A), out.split(B, row_ptr), out(C)]))
    if init == "parafac2_als":
        raise NotImplementedError(
            f'init="{init}" delegates to TensorLy decompositions in the reference (decomposition.py:55-73) and is '
            "out of scope of this engine; pass an explicit (weights, (A, B_is, C)) tuple instead, e.g. "
            "CoupledMatrixFactorization.from_Parafac2Tensor(parafac2_als(matrices, rank)).")
    raise ValueError('Initialization method "{}" not recognized'.format(init))


def initialize_aux(matrices, rank, reg, random_state):
    A_aux_list = [A_reg.init_aux(matrices, rank, 0, random_state=random_state) for A_reg in reg[0]]
    B_aux_list = [B_reg.init_aux(matrices, rank, 1, random_state=random_state) for B_reg in reg[1]]
    C_aux_list = [C_reg.init_aux(matrices, rank, 2, random_state=random_state) for C_reg in reg[2]]
    return A_aux_list, B_aux_list, C_aux_list


def initialize_dual(matrices, rank, reg, random_state):
    A_dual_list = [A_reg.init_dual(matrices, rank, 0, random_state=random_state) for A_reg in reg[0]]
    B_dual_list = [B_reg.init_dual(matrices, rank, 1, random_state=random_state) for B_reg in reg[1]]
    C_dual_list = [C_reg.init_dual(matrices, rank, 2, random_state=random_state) for C_reg in reg[2]]
    return A_dual_list, B_dual_list, C_dual_list


# ------------------------------------------------------------------------------------------------------------
# public diagnostics helper (decomposition.py:347-417) on host/device arrays
# ------------------------------------------------------------------------------------------------------------
def _sq(x):
    return float((x.double() ** 2).sum()) if is_torch(x) else float(np.sum(np.asarray(x, dtype=np.float64) ** 2))


def _root_sum_squared_list(x_list):
    return np.sqrt(sum(_sq(x) for x in x_list))


def compute_feasibility_gaps(cmf, regs, A_aux_list, B_aux_list, C_aux_list):
    r"""Feasibility gaps ||aux - x|| / ||x|| per penalty and mode; the B-mode gap pools all B_i (:404-417)."""
    weights, (A, B_is, C) = cmf
    A_norm = np.sqrt(_sq(A))
    B_norm = _root_sum_squared_list(B_is)
    C_norm = np.sqrt(_sq(C))
    A_gaps = [np.sqrt(_sq(A_reg.subtract_from_aux(A_aux, A))) / A_norm for A_reg, A_aux in zip(regs[0], A_aux_list)]
    B_gaps = [_root_sum_squared_list(B_reg.subtract_from_auxes(B_is_aux, B_is)) / B_norm
              for B_reg, B_is_aux in zip(regs[1], B_aux_list)]
    C_gaps = [np.sqrt(_sq(C_reg.subtract_from_aux(C_aux, C))) / C_norm for C_reg, C_aux in zip(regs[2], C_aux_list)]
    return A_gaps, B_gaps, C_gaps


def _check_inner_convergence(factor_matrix, old_factor_matrix, cmf, reg_list, aux_list, mode, inner_tol):
    """Inner stopping rule on host objects (:92-116): relative change and every feasibility gap of the mode below
    `inner_tol`.  (Inside `cmf_aoadmm` the same test runs on device tensors between the step calls.)"""
    if not inner_tol or inner_tol < 0:
        return False
    if mode == 1:
        norm = _root_sum_squared_list(factor_matrix)
        change = _root_sum_squared_list([B_i - prev_B_i for B_i, prev_B_i in zip(factor_matrix, old_factor_matrix)])
    else:
        norm = np.sqrt(_sq(factor_matrix))
        change = np.sqrt(_sq(factor_matrix - old_factor_matrix))
    if change > inner_tol * norm:
        return False
    if len(reg_list) == 0:
        return True
    regs, auxes = [[], [], []], [[], [], []]
    regs[mode], auxes[mode] = reg_list, aux_list
    return max(compute_feasibility_gaps(cmf, regs, *auxes)[mode]) < inner_tol


def _cmf_reconstruction_error(matrices, cmf, norm_matrices=None, intermediate_A_calculations=None):
    """sqrt(max(0, ||X||^2 - 2 <X, M> + ||M||^2)) on host objects (:420-452); with the by-products of `admm_update_A`
    (`rhses`, `cross_products`) the two model terms need no pass over the matrices (:445-449).  fp64 accumulation.
    (Inside `cmf_aoadmm` the same quantity comes out of the A-phase kernels, `mcl_diagnostics`.)"""
    f64 = lambda x: to_numpy(x).astype(np.float64)
    norm_X_sq = sum(_sq(m) for m in matrices) if norm_matrices is None else float(norm_matrices) ** 2
    weights, (A, B_is, C) = cmf
    A = f64(A)
    if weights is not None:
        A = A * f64(weights)
    if intermediate_A_calculations is None:
        C64 = f64(C)
        CtC = C64.T @ C64
        inner_product = norm_cmf_sq = 0.0
        for i, B_i in enumerate(B_is):
            B_i = f64(B_i) * A[i]
            inner_product += float(np.sum((f64(matrices[i]) @ C64) * B_i))
            norm_cmf_sq += float(np.sum((B_i.T @ B_i) * CtC))
    else:
        A_rhses, cross_products = intermediate_A_calculations
        inner_product = sum(float(np.sum(f64(rhs_i) * a_i)) for rhs_i, a_i in zip(A_rhses, A))
        norm_cmf_sq = sum(float(a_i @ f64(cross_products[i]) @ a_i) for i, a_i in enumerate(A))
    return np.sqrt(max(0.0, norm_X_sq - 2 * inner_product + norm_cmf_sq))


def _compute_l2_penalty(cmf, l2_parameters):
    """sum over modes of l2_m / 2 ||factor_m||^2 (:617-627)"""
    weights, (A, B_is, C) = cmf
    l2reg = 0
    if l2_parameters[0]:
        l2reg += 0.5 * l2_parameters[0] * _sq(A)
    if l2_parameters[1]:
        l2reg += 0.5 * l2_parameters[1] * sum(_sq(B_i) for B_i in B_is)
    if l2_parameters[2]:
        l2reg += 0.5 * l2_parameters[2] * _sq(C)
    return l2reg


# ------------------------------------------------------------------------------------------------------------
# argument parsing (decomposition.py:455-614)
# ------------------------------------------------------------------------------------------------------------
def _listify(input_value, param_name):
    """One value per mode from a dict {mode: value}, a scalar (broadcast) or a length-3 iterable."""
    if hasattr(input_value, "get"):
        return [input_value.get(mode, None) for mode in range(3)]
    if not is_iterable(input_value):
        return [input_value, input_value, input_value]
    per_mode = list(input_value)
    if len(per_mode) != 3:
        raise ValueError(
            "All parameters must be a dictionary, non-iterable value or non-dictionary iterable of length 3."
            f" {param_name} is iterable of length {len(per_mode)}.")
    return per_mode


def _parse_all_penalties(non_negative, lower_bound, upper_bound, l2_norm_bound, unimodal, parafac2, l1_penalty,
                         tv_penalty, generalized_l2_penalty, svd, regs, dual_init, aux_init, verbose):
    if regs is None:
        regs = [[], [], []]
    elif is_iterable(regs):
        for modereg in regs:
            if not is_iterable(modereg):
                raise TypeError(
                    "regs should contain an iterable of iterables containting "
                    "matcouply.penalties.ADMMMPenalty instances at least one of the"
                    f"elements in regs were not iterable (regs={regs})")
            else:
                for reg in modereg:
                    if not isinstance(reg, penalties.ADMMPenalty):
                        raise TypeError(
                            "regs should contain an iterable of iterables containting "
                            "matcouply.penalties.ADMMMPenalty instances at least one of the"
                            f"elements in regs contained something other than an ADMMPenalty (regs={regs})")
    regs = [copy(reg_list) for reg_list in regs]  # avoid side effects on the input lists

    non_negative = _listify(non_negative, "non_negative")
    upper_bound = _listify(upper_bound, "upper_bound")
    lower_bound = _listify(lower_bound, "lower_bound")
    l2_norm_bound = _listify(l2_norm_bound, "l2_norm_bound")
    unimodal = _listify(unimodal, "unimodal")
    parafac2 = [False, True, False] if parafac2 else [False, False, False]
    l1_penalty = _listify(l1_penalty, "l1_penalty")
    generalized_l2_penalty = _listify(generalized_l2_penalty, "generalized_l2_penalty")
    tv_penalty = _listify(tv_penalty, "tv_penalty")

    for mode in range(3):
        parsed_regs = _parse_mode_penalties(
            non_negative=non_negative[mode], lower_bound=lower_bound[mode], upper_bound=upper_bound[mode],
            l2_norm_bound=l2_norm_bound[mode], unimodal=unimodal[mode], parafac2=parafac2[mode],
            l1_penalty=l1_penalty[mode], tv_penalty=tv_penalty[mode],
            generalized_l2_penalty=generalized_l2_penalty[mode], svd=svd, dual_init=dual_init, aux_init=aux_init)
        regs[mode] = parsed_regs + regs[mode]

    if verbose:
        print("All regularization penalties (including regs list):")
        for mode, reg in enumerate(regs):
            print(f"* Mode {mode}:")
            if len(reg) == 0:
                print("   - (no regularization added)")
            for single_reg in reg:
                print(f"   - {single_reg}")
    return regs


def _parse_mode_penalties(non_negative, lower_bound, upper_bound, l2_norm_bound, unimodal, parafac2, l1_penalty,
                          tv_penalty, generalized_l2_penalty, svd, dual_init, aux_init):
    """Keyword arguments of one mode -> its penalty list, in the reference's order Parafac2, Unimodality,
    GeneralizedL2, L2Ball, TV, L1, Box, NonNegativity (decomposition.py:571-612).  Table-driven: every row is
    (is the keyword set?, constructor, does the penalty absorb the non-negativity flag?); a plain NonNegativity is only
    appended when no earlier row absorbed the flag."""
    init = dict(aux_init=aux_init, dual_init=dual_init)
    l1 = l1_penalty or 0
    has_gl2 = generalized_l2_penalty is not None and generalized_l2_penalty is not False  # None, False or the norm matrix
    has_box = lower_bound is not None or upper_bound is not None

    def box():
        lo = -float("inf") if lower_bound is None else lower_bound
        return penalties.Box(max(lo, 0) if non_negative else lo, upper_bound, **init)

    rules = (
        (parafac2, lambda: penalties.Parafac2(svd=svd, **init), False),
        (unimodal, lambda: penalties.Unimodality(non_negativity=non_negative, **init), True),
        (has_gl2, lambda: penalties.GeneralizedL2Penalty(generalized_l2_penalty, svd=svd, **init), False),
        (l2_norm_bound, lambda: penalties.L2Ball(l2_norm_bound, non_negativity=non_negative, **init), True),
        (tv_penalty, lambda: penalties.TotalVariationPenalty(tv_penalty, l1_strength=l1, **init), False),
        # the L1 term rides inside the total-variation penalty when both are requested
        (l1 and not tv_penalty, lambda: penalties.L1Penalty(l1, non_negativity=non_negative, **init), True),
        (has_box, box, True),
    )
    regs, absorbed = [], False
    for requested, build, absorbs in rules:
        if requested:
            regs.append(build())
            absorbed = absorbed or absorbs
    if non_negative and not absorbed:
        regs.append(penalties.NonNegativity(**init))
    return regs


def _check_feasibility(feasibility_gaps, feasibility_tol):
    """True when every feasibility gap of every mode is below the tolerance (vacuously for no penalties)."""
    worst = max((gap for mode_gaps in feasibility_gaps for gap in mode_gaps), default=-float("inf"))
    return worst < feasibility_tol


class _StopRule:
    """The stopping test of the outer loop (decomposition.py:990-1053) as an object.  Quirks kept on purpose: the
    absolute criterion is only looked at when `tol` is set, and it tests the newest loss."""

    RELATIVE = "FEASIBILITY GAP CRITERION AND RELATIVE LOSS CRITERION SATISFIED"
    ABSOLUTE = "FEASIBILITY GAP CRITERION AND ABSOLUTE LOSS CRITERION SATISFIED"
    EXHAUSTED = "MAXIMUM NUMBER OF ITERATIONS REACHED"

    def __init__(self, tol, absolute_tol, feasibility_tol):
        self.tol, self.absolute_tol, self.feasibility_tol = tol, absolute_tol, feasibility_tol

    @property
    def active(self):
        return bool(self.tol or self.absolute_tol)

    def feasible(self, gaps):
        return self.feasibility_tol and _check_feasibility(gaps, self.feasibility_tol)

    @classmethod
    def message_of(cls, code):
        """the message of a stop code of the device rules (0: no criterion fired)"""
        if not code:
            return cls.EXHAUSTED
        return cls.RELATIVE if code == _engine.STOP_RELATIVE else cls.ABSOLUTE

    def verdict(self, feasible, losses):
        """message of the criterion that fires on the last two losses, or None"""
        if not self.tol:
            return None
        relative = abs(losses[-2] - losses[-1]) < (self.tol * losses[-2])
        absolute = losses[-1] < self.absolute_tol
        if feasible and relative:
            return self.RELATIVE
        if feasible and absolute:
            return self.ABSOLUTE
        return None


class _Progress:
    """Console output of the outer loop (`verbose`: 0 / None silent, n > 0 every n-th iteration, -1 final message only)."""

    def __init__(self, verbose):
        self.verbose = verbose

    def _due(self, it):
        return bool(self.verbose) and self.verbose > 0 and it % self.verbose == 0

    @staticmethod
    def _gaps(gaps):
        print("Feasibility gaps for A: {}".format(gaps[0]))
        print("Feasibility gaps for the Bi-matrices: {}".format(gaps[1]))
        print("Feasibility gaps for C: {}".format(gaps[2]))

    def initial(self, gaps):
        if self.verbose and self.verbose > 0:
            self._gaps(gaps)

    def iteration(self, it, rec_error=None, loss=None, variation=None, gaps=None):
        if not self._due(it):
            return
        if gaps is None:
            print("Coupled matrix factorization iteration={}".format(it))
            return
        shown = ("NOT COMPUTED",) * 3 if rec_error is None else (rec_error, loss, variation)
        print("Coupled matrix factorization iteration={}, ".format(it)
              + "reconstruction error={}, ".format(shown[0])
              + ("regularized loss={}, " if rec_error is None else "regularized loss={} ").format(shown[1])
              + "regularized loss variation={}.".format(shown[2]))
        self._gaps(gaps)

    def converged(self, it, message):
        if self.verbose:
            print("converged in {} iterations: {}".format(it, message))

    def exhausted(self):
        if self.verbose:
            print("REACHED MAXIMUM NUMBER OF ITERATIONS")


class ADMMVars(NamedTuple):
    auxes: tuple  #: Length three tuple containing a list of auxiliary factor matrices for each mode
    duals: tuple  #: Length three tuple containing a list of dual variables for each mode


class DiagnosticMetrics(NamedTuple):
    rec_errors: list  #: reconstruction errors, one per iteration plus the initial one
    feasibility_gaps: list  #: feasibility gaps, one per iteration plus the initial one
    regularized_loss: list  #: regularized loss, one per iteration plus the initial one
    satisfied_stopping_condition: Optional[bool]  #: None if no tolerance is set
    satisfied_feasibility_condition: Optional[bool]  #: None if no tolerance is set
    n_iter: int  #: Number of iterations ran
    message: str  #: Convergence message


# ------------------------------------------------------------------------------------------------------------
# parafac2_als: unconstrained PARAFAC2-ALS (TensorLy's parafac2) on the device
# ------------------------------------------------------------------------------------------------------------
# TensorLy keywords of parafac2 that are not served, with the value that is (their default)
_PF2ALS_TENSORLY_DEFAULTS = {"svd": "truncated_svd", "normalize_factors": False, "verbose": False, "linesearch": False}


def _parafac2_als_options(matrices, rank, init, nn_modes, n_iter_max, n_iter_parafac, kwargs):
    """the checked (I, K, rows, nn_modes) of a parafac2_als call; raises before the device is touched"""
    for key, value in kwargs.items():
        if key not in _PF2ALS_TENSORLY_DEFAULTS:
            raise TypeError(f"parafac2_als() got an unexpected keyword argument {key!r}")
        if value != _PF2ALS_TENSORLY_DEFAULTS[key]:
            raise NotImplementedError(f"parafac2_als: {key}={value!r} is not supported (only {key}="
                                      f"{_PF2ALS_TENSORLY_DEFAULTS[key]!r})")
    if not isinstance(init, str) or init not in ("random", "svd"):
        raise ValueError(f'parafac2_als: init must be "random" or "svd", not {init!r}')
    if nn_modes is None:
        modes = set()
    elif isinstance(nn_modes, str):
        if nn_modes != "all":
            raise ValueError(f'parafac2_als: nn_modes must be None, "all" or a collection of modes, not {nn_modes!r}')
        modes = {0, 1, 2}
    else:
        try:
            modes = set(nn_modes)
        except TypeError:
            raise ValueError(f"parafac2_als: nn_modes must be None, \"all\" or a collection of modes, not {nn_modes!r}") from None
        if not all(isinstance(m, (int, np.integer)) and not isinstance(m, bool) and 0 <= m <= 2 for m in modes):
            raise ValueError(f"parafac2_als: nn_modes may hold the modes 0, 1 and 2 only, not {sorted(modes, key=str)!r}")
    if 1 in modes:
        raise NotImplementedError("parafac2_als: non-negativity on mode 1 (B) cannot be met by PARAFAC2-ALS (TensorLy only warns "
                                  "and leaves it unconstrained); constrain the modes 0 and 2 only, or fit parafac2_aoadmm")
    for name, v in (("n_iter_max", n_iter_max), ("n_iter_parafac", n_iter_parafac)):
        if isinstance(v, bool) or int(v) != v or v < 1:
            raise ValueError(f"parafac2_als: {name} must be a positive integer, not {v!r}")
    K = int(shape(matrices[0])[1])
    rows = [int(shape(m)[0]) for m in matrices] if not isinstance(matrices, PackedMatrices) else \
        [int(matrices.row_ptr[i + 1] - matrices.row_ptr[i]) for i in range(len(matrices))]
    if rank > _engine.PF2ALS_MAX_RANK:
        raise NotImplementedError(f"parafac2_als: rank {rank} is above the served bound {_engine.PF2ALS_MAX_RANK}")
    if min(rows) < rank or K < rank:
        raise NotImplementedError(f"parafac2_als: every matrix needs J_i >= rank and K >= rank (min J_i = {min(rows)}, K = {K}, "
                                  f"rank = {rank})")
    if init == "svd" and K > _DEVICE_SVD_MAX_K:
        raise NotImplementedError(f'parafac2_als: init="svd" needs K <= {_DEVICE_SVD_MAX_K} (K = {K})')
    return len(rows), K, rows, sorted(modes)


def _pf2als_random_start(I, K, rank, random_state):
    """init="random" of parafac2_als: A [I, rank], B [rank, rank], C [K, rank] uniform from check_random_state(random_state), in
    that order"""
    rs = check_random_state(random_state)
    return rs.uniform(size=(I, rank)), rs.uniform(size=(rank, rank)), rs.uniform(size=(K, rank))


def parafac2_als(matrices, rank, n_iter_max=2000, init="random", tol=1e-8, absolute_tol=1e-13, nn_modes=None, n_iter_parafac=5,
                 random_state=None, return_errors=False, **kwargs):
    """Unconstrained PARAFAC2 fitted by alternating least squares (TensorLy's ``parafac2``), on the device.

    Model ``X_i ~ P_i B diag(a_i) C^T`` with orthonormal projections ``P_i``.  Every iteration forms the projections from the
    polar factor of ``X_i C diag(a_i) B^T``, projects the slabs and runs ``n_iter_parafac`` CP sweeps on the projected tensor
    (modes in ``nn_modes`` - 0 and/or 2 - take one non-negative HALS pass instead of the ALS normal equations).
    ``init="svd"``: A = 1, B = I, C = the right singular vectors of the stacked matrices; ``init="random"``: A, B, C drawn
    uniformly from ``check_random_state(random_state)`` in that order.  With a truthy ``tol`` the relative reconstruction error
    is tracked and the fit stops when ``|e_{t-1}^2 - e_t^2| <= tol e_{t-1}^2`` or ``e_t^2 < absolute_tol``.

    ``matrices``: as for :func:`cmf_aoadmm`.  Returns ``(weights, (A, B, C), projections)`` with ``weights`` None, B of shape
    rank x rank and ``projections[i]`` J_i x rank, in the input's array type; with ``return_errors=True`` also the list of
    errors.  Not served (``NotImplementedError``): nn_modes containing 1, rank above 32, J_i < rank or K < rank, and the
    TensorLy options ``svd``, ``normalize_factors``, ``linesearch`` and ``verbose`` other than their defaults.
    """
    rank = int(rank)
    I, K, rows, modes = _parafac2_als_options(matrices, rank, init, nn_modes, n_iter_max, n_iter_parafac, kwargs)
    start = _pf2als_random_start(I, K, rank, random_state) if init == "random" else None
    tol = float(tol) if tol else 0.0
    absolute_tol = float(absolute_tol) if absolute_tol else 0.0
    X, row_ptr = _pack(matrices, _device())
    A, B, C, P, errors = _engine.parafac2_als(X, row_ptr, rank, start, int(n_iter_max), int(n_iter_parafac), tol, absolute_tol, modes)
    out = _Out(matrices)
    result = (None, (out(A), out(B), out(C)), out.split(P, row_ptr))
    if return_errors:
        return result, [float(e) for e in errors.cpu().numpy()]
    return result


# ------------------------------------------------------------------------------------------------------------
# host <-> device plumbing
# ------------------------------------------------------------------------------------------------------------
def _device():
    if torch is None or not torch.cuda.is_available():
        raise _engine.EngineError(
            "no HIP device visible: matcouply_amd runs the AO-ADMM updates on an MI355X (gfx950); there is no CPU fallback")
    return torch.device("cuda", torch.cuda.current_device())


def _dtype():
    """float32 on the device; a substituted checker engine (tests) may ask for float64 state."""
    sub = _test_engine_factory()
    return getattr(sub, "dtype", torch.float32) if sub is not None else torch.float32


def _to_dev(x, device):
    if is_torch(x):
        return x.detach().to(device=device, dtype=_dtype()).contiguous().clone()
    return torch.as_tensor(np.ascontiguousarray(np.asarray(x)), device=device).to(_dtype()).contiguous()


def _x16_dtype(mats):
    """the torch dtype of a homogeneous list of 16-bit matrices (torch bfloat16 / float16 tensors, NumPy float16 arrays), else
    None: mixed lists and every other input are packed in float32"""
    def dt(m):
        if is_torch(m):
            return m.dtype if m.dtype in (torch.bfloat16, torch.float16) else None
        return torch.float16 if isinstance(m, np.ndarray) and m.dtype == np.float16 else None

    d = [dt(m) for m in mats]
    return d[0] if d and d[0] is not None and all(x == d[0] for x in d) else None


def _upcast_x16(matrices):
    """the matrices with 16-bit X upcast (exactly) to float32: for a substituted checker engine without `supports_x16`"""
    if isinstance(matrices, PackedMatrices):
        X = matrices.X
        return PackedMatrices(X.float(), matrices.row_ptr) if is_torch(X) and X.dtype in (torch.bfloat16, torch.float16) else matrices
    return [m.float() if is_torch(m) and m.dtype in (torch.bfloat16, torch.float16) else m for m in matrices]


def _pack(matrices, device):
    """-> (X [N, K] on device, row_ptr int64 [I+1]).  X is float32, or bfloat16 / float16 for a PackedMatrices of that dtype and
    for a homogeneous list of 16-bit matrices (_x16_dtype: packed at two bytes per element, no float32 copy)."""
    if isinstance(matrices, PackedMatrices):
        X = matrices.X
        if not (is_torch(X) and X.dtype in (torch.float32, torch.bfloat16, torch.float16)):
            raise TypeError("PackedMatrices.X must be a float32, bfloat16 or float16 torch tensor, not "
                            f"{getattr(X, 'dtype', type(X).__name__)}")
        if not (X.is_cuda and X.is_contiguous()):
            raise TypeError("PackedMatrices.X must be a contiguous CUDA tensor")
        return X, matrices.row_ptr
    mats = list(matrices)
    K = shape(mats[0])[1]
    for m in mats:
        if len(shape(m)) != 2 or shape(m)[1] != K:
            raise ValueError("All matrices must be second order tensors with the same number of columns")
    rows = [shape(m)[0] for m in mats]
    row_ptr = np.concatenate([[0], np.cumsum(rows)]).astype(np.int64)
    x16 = _x16_dtype(mats)
    if x16 is not None:  # one packed 16-bit copy on the device (CPU matrices are uploaded at two bytes per element)
        X = torch.empty((int(row_ptr[-1]), K), dtype=x16, device=device)
        for i, m in enumerate(mats):
            X[row_ptr[i]: row_ptr[i + 1]] = m.detach() if is_torch(m) else torch.from_numpy(np.ascontiguousarray(m))
        return X, row_ptr
    if all(is_torch(m) for m in mats):
        X = torch.cat([m.detach().to(device=device, dtype=torch.float32) for m in mats], 0).contiguous()
    else:
        host = np.empty((int(row_ptr[-1]), K), dtype=np.float32)
        for i, m in enumerate(mats):
            host[row_ptr[i]: row_ptr[i + 1]] = m.detach().cpu().numpy() if is_torch(m) else np.asarray(m)
        X = torch.from_numpy(host).to(device)
    return X, row_ptr


def _pack_rows(list_of_matrices, device):
    if len(list_of_matrices) == 0:
        return torch.zeros((0, 0), dtype=torch.float32, device=device)
    if all(is_torch(m) for m in list_of_matrices):
        return torch.cat([m.detach().to(device=device, dtype=_dtype()) for m in list_of_matrices], 0).contiguous()
    return _to_dev(np.concatenate([m.detach().cpu().numpy() if is_torch(m) else np.asarray(m)
                                   for m in list_of_matrices], 0), device)


class _Out:
    """Converts device results back to the array type / dtype / device of the caller's matrices."""

    def __init__(self, matrices):
        first = matrices.X if isinstance(matrices, PackedMatrices) else matrices[0]
        self.torch_out = is_torch(first)
        self.dtype = first.dtype
        self.device = first.device if self.torch_out else None

    def __call__(self, t):
        if self.torch_out:
            return t.detach().to(device=self.device, dtype=self.dtype).clone()
        return t.detach().cpu().numpy().astype(self.dtype if np.issubdtype(self.dtype, np.floating) else np.float64)

    def split(self, t, row_ptr):
        full = self(t)
        return [full[row_ptr[i]: row_ptr[i + 1]] for i in range(len(row_ptr) - 1)]


def _aux_to_device(aux, device):
    """Move an auxiliary variable in any parametrisation (array, list of arrays, tuple of those) to device tensors."""
    if isinstance(aux, tuple):
        return tuple(_aux_to_device(a, device) for a in aux)
    if isinstance(aux, list):
        return [_aux_to_device(a, device) for a in aux]
    return _to_dev(aux, device)


def _aux_out(aux, out):
    if isinstance(aux, tuple):
        return tuple(_aux_out(a, out) for a in aux)
    if isinstance(aux, list):
        return [_aux_out(a, out) for a in aux]
    return out(aux)


def _default_engine_factory(**kw):
    return _engine.HipEngine(**kw)


_DIRECT_COMMS = {}


def _direct_comm(group, device=None):
    """the cached direct RCCL communicator of a process group on `device` (None: use torch.distributed), see _rccl.py.
    The cache entry is tied to the RESOLVED group object (the default group changes identity when a host destroys and
    re-creates it), its world size, this rank and the device: an entry whose group is gone is dropped, not reused."""
    import torch.distributed as dist

    from . import _rccl

    resolved = group if group is not None else dist.group.WORLD
    try:
        if device is None or getattr(device, "index", None) is None:  # the caller's current device, as DirectComm resolves it
            device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else device
        key = (id(resolved), dist.get_world_size(group), dist.get_rank(group), str(device))
    except Exception:
        return None
    try:  # entries of process groups that have been destroyed since (their communicators are abandoned with them)
        alive = dist.distributed_c10d._world.pg_map
        for k in [k for k, (g, _) in _DIRECT_COMMS.items() if g not in alive]:
            del _DIRECT_COMMS[k]
    except Exception:
        pass
    if key not in _DIRECT_COMMS:
        _DIRECT_COMMS[key] = (resolved, _rccl.DirectComm.try_create(group, device))  # the group is kept alive with its communicator
    return _DIRECT_COMMS[key][1]


# ------------------------------------------------------------------------------------------------------------
# the solver in parts (collectives, penalties on the device, phases and diagnostics, arithmetic rule, outer loops) and whole
# ------------------------------------------------------------------------------------------------------------
class _Group:
    """The ranks of one run and their collectives.  `direct` is the cached RCCL communicator of the group (_direct_comm: the
    collectives go straight onto the engine's stream, no stream hand-over), set by the caller once the engine exists; None - any
    other backend (gloo in the CPU tests), or a failed self-test - takes torch.distributed's.  A run without `group=` is the
    same object with one rank, whose all_reduce returns at once."""

    def __init__(self, group=None):
        self.group, self.dist, self.direct, self.world, self.rank = group, None, None, 1, 0
        if group is not None:
            import torch.distributed as dist

            self.dist, self.world, self.rank = dist, dist.get_world_size(group), dist.get_rank(group)
        # the sharded code path (step calls with the reductions in between): taken with more than one rank - and, for
        # rehearsals of that path on a single-GPU box, with a one-rank group when MCL_FORCE_SHARDED_PATH=1
        self.sharded = self.world > 1 or (group is not None and os.environ.get("MCL_FORCE_SHARDED_PATH") == "1")
        self.counts = {}  # rows per rank of every gathered array, by name (exchanged at the first gather of that name)

    def all_reduce(self, t, op="sum"):
        if not self.sharded:
            return
        if (self.direct is not None and is_torch(t) and t.is_cuda and t.device == self.direct.device
                and t.dtype in (torch.float32, torch.float64) and t.is_contiguous()):
            self.direct.all_reduce(t, op)
        else:
            self.dist.all_reduce(t, op=(self.dist.ReduceOp.MAX if op == "max" else self.dist.ReduceOp.SUM), group=self.group)

    def gather_rows(self, t, key):
        """every rank's rows of `t` (a vector or a matrix), in rank order, as a list.  The shares are uneven: the counts are
        exchanged once per `key`, the rows padded to the largest share for the collective and trimmed after."""
        counts = self.counts.get(key)
        if counts is None:
            n_loc = torch.tensor([t.shape[0]], dtype=torch.int64, device=t.device)
            cnt = [torch.zeros_like(n_loc) for _ in range(self.world)]
            self.dist.all_gather(cnt, n_loc, group=self.group)
            counts = self.counts[key] = [int(c.item()) for c in cnt]
        padded = torch.zeros((max(counts),) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device)
        padded[: t.shape[0]] = t
        parts = [torch.empty_like(padded) for _ in range(self.world)]
        self.dist.all_gather(parts, padded, group=self.group)
        return [p[:c] for p, c in zip(parts, counts)]

    def own_rows(self, key):
        """(lo, hi): where this rank's rows lie among the gathered rows of `key`"""
        lo = sum(self.counts[key][:self.rank])
        return lo, lo + self.counts[key][self.rank]


def _native_penalties(regs, auxes, duals, matrices, device, host_only, has_group):
    """The penalties as the engine sees them: (native, ext_aux), native[mode][k] an _engine.NativeReg with the auxiliary and dual
    variable on the device.  Host-evaluated penalties (no native kernel; all of them with `host_only`; a generalised L2 norm
    matrix that does not fit the mode) are PEN_EXTERNAL: the Python object keeps the auxiliary variable in ITS parametrisation
    (on the device) in ext_aux[(mode, k)], the engine sees `aux_as_matrix` of it (reference penalties.py:311-343)."""
    native, ext_aux = [[], [], []], {}
    for mode in range(3):
        for k, (reg, aux, dual) in enumerate(zip(regs[mode], auxes[mode], duals[mode])):
            desc = None if host_only else penalties.native_descriptor_of(reg)
            gl2_matrix = None
            if desc is not None and desc[0] == _engine.PEN_GL2:
                # every matrix of the mode must have as many rows as the norm matrix (anything else fails in the reference's
                # product too: left to the penalty's own method); a sharded A holds only this rank's rows of the I x I problem
                gl2_matrix, n_gl2 = reg._native_matrix()
                rows_m = [shape(m_)[0] for m_ in matrices] if mode == 1 else [len(matrices) if mode == 0 else shape(matrices[0])[1]]
                if any(rw != n_gl2 for rw in rows_m) or (has_group and mode == 0):
                    desc = None
            dual_t = _pack_rows(dual, device) if mode == 1 else _to_dev(dual, device)
            if desc is None:
                obj = _aux_to_device(aux, device)
                mat = _pack_rows(reg.auxes_as_matrices(obj), device) if mode == 1 else _to_dev(reg.aux_as_matrix(obj), device)
                ext_aux[(mode, k)] = obj
                native[mode].append(_engine.NativeReg(_engine.PEN_EXTERNAL, mat, dual_t))
                continue
            kind, nonneg, p0, p1 = desc
            if kind == _engine.PEN_PARAFAC2:
                P_is, Delta = aux
                native[mode].append(_engine.NativeReg(kind, _pack_rows(P_is, device), dual_t, aux2=_to_dev(Delta, device)))
            else:
                aux_t = _pack_rows(aux, device) if mode == 1 else _to_dev(aux, device)
                extra = {}
                if kind == _engine.PEN_GL2:
                    extra = dict(matrix=torch.as_tensor(gl2_matrix, dtype=torch.float64, device=device).contiguous(), matrix_rows=n_gl2)
                native[mode].append(_engine.NativeReg(kind, aux_t, dual_t, non_negativity=nonneg, p0=p0, p1=p1, **extra))
    return native, ext_aux


def _diag_slot(mode, k):
    """where penalty k of a mode sits in the diagnostics vector: its squared feasibility gap there, its value in the next slot"""
    return _engine.DIAG_REG + (mode * _engine.MCL_MAX_REGS + k) * 2


def _local_on_A(nat, reg):
    """a penalty on mode 0 that acts on each row of A by itself: needs nothing from the other ranks"""
    return nat.kind in (_engine.PEN_NN, _engine.PEN_BOX, _engine.PEN_L1) or (
        nat.kind == _engine.PEN_EXTERNAL and isinstance(reg, penalties.RowVectorPenalty))


class _Run:
    """One fit on its engine: the B, C and A phase of an outer iteration - native calls where the engine serves the whole phase,
    stepped ones with the reductions and the host-evaluated proxes in between where it does not - and the diagnostics.
    `opt`: the scalar options of the cmf_aoadmm call."""

    def __init__(self, eng, regs, native, ext_aux, grp, row_ptr, device, opt):
        self.eng, self.regs, self.native, self.ext_aux, self.grp, self.device, self.opt = eng, regs, native, ext_aux, grp, device, opt
        self.updates = (opt.update_A, opt.update_B_is, opt.update_C)
        # inner_tol > 0 (early exit of the inner ADMM loops, decomposition.py:90-117) needs a convergence test after every
        # inner iteration.  Single-device runs: the ENGINE evaluates it (mcl_options.inner_tol: one launch per step, a device-side
        # flag the remaining inner launches test; native prox kernels stay native, no host synchronisation).  Sharded runs (the
        # norms must be all-reduced over the ranks) and the CPU checker keep the step path: native solves, every prox through
        # the penalty objects' own methods on device tensors, the test on the host
        self.check_inner = bool(opt.inner_tol) and opt.inner_tol > 0
        sharded = grp.sharded
        self.has_ext = [any(r.kind == _engine.PEN_EXTERNAL for r in native[m]) for m in range(3)]
        self.needs_B_steps = (sharded and (opt.constant_B or any(r.kind == _engine.PEN_PARAFAC2 for r in native[1]))) or self.has_ext[1]
        # mode 0 under sharding: the rows of A live on different ranks.  Row-separable penalties need nothing; an L2 ball
        # (the README case: l2_norm_bound on A with a constant feasibility penalty) needs the r column sums of squares of
        # A + U all-reduced in every inner iteration
        self.sharded_ball_A = sharded and any(r.kind == _engine.PEN_L2BALL for r in native[0])
        # ... any other matrix penalty (unimodality, total variation along the rows of A, a user's MatrixPenalty) is evaluated by
        # EVERY rank on the all-gathered matrix A + U (I x r floats: small) through the penalty's own prox, each rank keeping its
        # rows - the reference's arithmetic, replicated; row-separable kinds stay rank-local
        self.gathered_A = [sharded and nat.kind != _engine.PEN_L2BALL and not _local_on_A(nat, reg)
                           for nat, reg in zip(native[0], regs[0])]
        if (self.sharded_ball_A or any(self.gathered_A)) and not opt.constant_A:
            raise NotImplementedError("a matrix penalty on mode 0 needs constant_feasibility_penalty (as in the reference, "
                                      "which has no row update for it)")
        # the A phase in steps: a prox between the ranks or on the host; else its rho max alone is reduced, or nothing
        self.stepped_A = self.sharded_ball_A or any(self.gathered_A) or self.has_ext[0]
        self.needs_A_steps = sharded and opt.constant_A
        # host-evaluated penalties on mode 1 that act on ALL matrices at once (a user's MatricesPenalty) under group=: like PARAFAC2
        # they may couple the B_i of different ranks, so every rank evaluates the prox on the all-gathered matrices and keeps its own
        self.gathered_B = [sharded and nat.kind == _engine.PEN_EXTERNAL and not isinstance(reg, penalties.MatrixPenalty)
                           for reg, nat in zip(regs[1], native[1])]
        self.row_slices = [slice(int(row_ptr[i]), int(row_ptr[i + 1])) for i in range(len(row_ptr) - 1)]
        self.b_layout = None  # row counts of every rank's matrices, in rank order (gathered once)

    # ---- an outer iteration -------------------------------------------------------------------------------------------
    def iteration(self):
        if self.opt.update_B_is:
            self.update_B()
        if self.opt.update_C:
            self.update_C()
        if self.opt.update_A:
            self.update_A()

    def plain_iterations(self, n):
        if self.grp.sharded:  # n outer iterations without diagnostics, on whichever path this run takes
            for _ in range(n):
                self.iteration()
        else:
            self.eng.iterate(n, update_A=self.opt.update_A, update_B=self.opt.update_B_is, update_C=self.opt.update_C)

    def _inner_loop(self, mode, solve, proxes, before_test=None):
        """the inner ADMM loop of a stepped phase: solve, the prox of every penalty, the convergence test - at most
        inner_n_iter_max times, once without penalties"""
        n_it = self.opt.inner_n_iter_max if self.native[mode] else min(1, self.opt.inner_n_iter_max)
        for _ in range(n_it):
            F_old = getattr(self.eng, "ABC"[mode]).clone() if self.check_inner else None
            solve()
            proxes()
            if self.check_inner and before_test is not None:
                before_test()
            if self.inner_converged(mode, F_old):
                break

    def update_B(self):
        eng = self.eng
        if not self.needs_B_steps:
            eng.update_B()
            return
        eng.B_begin()
        if self.opt.constant_B:
            self.grp.all_reduce(eng.B_rho_max(), "max")
        eng.B_factor()
        self._inner_loop(1, eng.B_solve, self._proxes_B, before_test=eng.B_end)  # (the test reads B / aux on the host side)
        eng.B_end()

    def update_C(self):
        eng = self.eng
        self.grp.all_reduce(eng.update_C_local())
        if not self.has_ext[2]:
            eng.update_C_finish()
            return
        eng.C_begin()
        self._inner_loop(2, eng.C_solve, self._proxes_C)
        eng.C_end()

    def update_A(self):
        eng = self.eng
        if not (self.stepped_A or self.needs_A_steps):
            eng.update_A()
            return
        eng.A_begin()
        if self.opt.constant_A:
            self.grp.all_reduce(eng.A_rho_max(), "max")
        if not self.stepped_A:
            eng.A_finish()
            return
        eng.A_factor()
        rho_a = eng.rho(0).cpu().numpy()
        self._inner_loop(0, eng.A_solve, lambda: self._proxes_A(rho_a))
        eng.A_end()

    def inner_converged(self, mode, F_old):
        """decomposition.py:90-117 on device tensors: relative change and every feasibility gap of the mode below inner_tol"""
        if not self.check_inner:  # (host-driven modes - host-evaluated penalties - run the test here even when the engine has it too)
            return False
        # squared norms in fp64: [ |F|^2, |F - F_old|^2, |F - aux_k|^2 ... ].  With group= the rows of modes 0 and 1 live on
        # different ranks: the sums are all-reduced, so that every rank leaves the inner loop at the same iteration and the
        # test is the reference's (over ALL B_i); C is replicated and needs nothing
        F64 = getattr(self.eng, "ABC"[mode]).double()
        sq = torch.stack([(F64 ** 2).sum(), ((F64 - F_old.double()) ** 2).sum()]
                         + [((F64 - nat.aux.double()) ** 2).sum() for nat in self.native[mode]])
        if mode != 2:
            self.grp.all_reduce(sq)
        sq = sq.cpu().numpy()
        nrm = float(np.sqrt(sq[0]))
        if float(np.sqrt(sq[1])) > self.opt.inner_tol * nrm:
            return False
        if not self.native[mode]:
            return True
        return max(float(np.sqrt(v)) / nrm for v in sq[2:]) < self.opt.inner_tol

    def _proxes_B(self):
        eng = self.eng
        for k, nat in enumerate(self.native[1]):
            if nat.kind != _engine.PEN_EXTERNAL:
                eng.B_prox_local(k)
                if nat.kind == _engine.PEN_PARAFAC2:
                    self.grp.all_reduce(eng.B_prox_reduce_buffer(k))
                eng.B_prox_finish(k)
            elif self.gathered_B[k]:
                self.sharded_gathered_prox_B(k)
            else:  # a MatrixPenalty's prox acts on one matrix at a time: every rank evaluates it on its own matrices
                self.host_prox_B(k)

    def _proxes_C(self):
        rho_c = self.eng.rho(2).cpu().numpy()
        for k in range(len(self.native[2])):
            self.host_prox_matrix(2, k, self.eng.C, rho_c, True)

    def _proxes_A(self, rho_a):
        for k, nat in enumerate(self.native[0]):
            if self.sharded_ball_A and nat.kind == _engine.PEN_L2BALL:
                self.sharded_ball_prox_A(k)
            elif self.gathered_A[k]:
                self.sharded_gathered_prox_A(k, rho_a)
            else:
                self.host_prox_matrix(0, k, self.eng.A, rho_a, self.opt.constant_A)

    def host_prox_B(self, k):
        """user prox of penalty k on mode 1 (decomposition.py:276-285), evaluated on device tensors"""
        eng, reg, nat = self.eng, self.regs[1][k], self.native[1][k]
        rhos = [float(v) for v in eng.rho(1).cpu().numpy()]
        shifted = [eng.B[sl] + nat.dual[sl] for sl in self.row_slices]
        obj = reg.factor_matrices_update(shifted, rhos, self.ext_aux[(1, k)])
        self.ext_aux[(1, k)] = obj
        nat.aux.copy_(torch.cat([m.to(nat.aux.dtype) for m in reg.auxes_as_matrices(obj)], 0))
        nat.dual.copy_(eng.B - (nat.aux - nat.dual))

    def gather_matrices_B(self, t):
        """all ranks' matrices of a packed mode-1 array [rows of this rank, r], in rank order, as a list"""
        grp = self.grp
        if self.b_layout is None:
            mine = torch.tensor([sl.stop - sl.start for sl in self.row_slices], dtype=torch.int64, device=t.device)
            self.b_layout = [[int(v) for v in p.cpu().numpy()] for p in grp.gather_rows(mine, "B matrices")]
            grp.counts["B rows"] = [sum(js) for js in self.b_layout]
        out = []
        for p, js in zip(grp.gather_rows(t, "B rows"), self.b_layout):
            o = 0
            for j in js:
                out.append(p[o:o + j])
                o += j
        return out

    def sharded_gathered_prox_B(self, k):
        """a MatricesPenalty on the sharded B_i (decomposition.py:276-285): its prox on ALL matrices, this rank's kept"""
        eng, grp, row_slices = self.eng, self.grp, self.row_slices
        reg, nat = self.regs[1][k], self.native[1][k]
        obj = self.ext_aux[(1, k)]
        # the object the penalty keeps must be the list of matrices itself to be split over ranks by matrix
        if not (isinstance(obj, (list, tuple)) and len(obj) == len(row_slices)
                and all(is_torch(o) and tuple(o.shape) == (sl.stop - sl.start, nat.aux.shape[1]) for o, sl in zip(obj, row_slices))):
            raise NotImplementedError("a host-evaluated MatricesPenalty on mode 1 whose auxiliary variable is not the list of "
                                      "matrices itself is not supported with group=")
        shifted = self.gather_matrices_B(eng.B + nat.dual)
        auxes = self.gather_matrices_B(torch.cat([o.to(nat.aux.dtype) for o in obj], 0))
        # the feasibility penalties of all matrices (one per matrix, fp64), in the same order
        rho_parts = grp.gather_rows(eng.rho(1).to(device=nat.aux.device, dtype=torch.float64), "B matrices")
        rho_all = [float(v) for p in rho_parts for v in p.cpu().numpy()]
        full = reg.factor_matrices_update(shifted, rho_all, auxes)
        lo, hi = grp.own_rows("B matrices")
        own = [m.clone() for m in full[lo:hi]]
        self.ext_aux[(1, k)] = own
        nat.aux.copy_(torch.cat([m.to(nat.aux.dtype) for m in reg.auxes_as_matrices(own)], 0))
        nat.dual.copy_(eng.B - (nat.aux - nat.dual))

    def host_prox_matrix(self, mode, k, F, rho_rows, constant):
        """user prox of penalty k on mode 0 / 2 (decomposition.py:197-213 / 333-338)"""
        reg, nat = self.regs[mode][k], self.native[mode][k]
        shifted = F + nat.dual
        obj = self.ext_aux.get((mode, k))
        if obj is None:  # native kind evaluated through its host method inside a host-driven mode
            obj = nat.aux.clone()
        if constant:
            obj = reg.factor_matrix_update(shifted, float(rho_rows[0]), obj)
        else:
            obj = obj.clone() if is_torch(obj) else obj
            for i in range(F.shape[0]):
                obj[i] = reg.factor_matrix_row_update(shifted[i], float(rho_rows[i]), obj[i])
        if (mode, k) in self.ext_aux:
            self.ext_aux[(mode, k)] = obj
        nat.aux.copy_(reg.aux_as_matrix(obj).to(nat.aux.dtype))
        nat.dual.copy_(F - (nat.aux - nat.dual))

    def sharded_ball_prox_A(self, k):
        """L2-ball prox on the sharded A (penalties.py:920-925): column norms over ALL rows = all-reduced partial sums"""
        eng, nat = self.eng, self.native[0][k]
        y = eng.A + nat.dual
        if nat.non_negativity:
            y = torch.clamp(y, min=0)
        sq = (y.double() ** 2).sum(0)
        self.grp.all_reduce(sq)
        nrm = torch.sqrt(sq).to(y.dtype)
        bound = torch.as_tensor(nat.p0, dtype=y.dtype, device=y.device)
        z = y * (bound / torch.maximum(nrm, bound))
        nat.dual.copy_(eng.A - (z - nat.dual))
        nat.aux.copy_(z)

    def gather_rows_A(self, t):
        return torch.cat(self.grp.gather_rows(t, "A rows"), 0)  # all ranks' rows of a mode-0 matrix, in rank order

    def sharded_gathered_prox_A(self, k, rho_a):
        """matrix penalty on the sharded A (decomposition.py:203): the penalty's prox on the gathered A + U, own rows kept"""
        eng, reg, nat = self.eng, self.regs[0][k], self.native[0][k]
        obj = self.ext_aux.get((0, k))
        if obj is None:
            aux_rows = nat.aux  # native kind evaluated through its host method: its aux IS the matrix
        else:
            # host-evaluated penalty (a user's MatrixPenalty; any matrix penalty while inner_tol is set): the object it keeps
            # must be the matrix itself to be gathered by rows - another parametrisation cannot be split over ranks
            aux_rows = reg.aux_as_matrix(obj)
            if not (is_torch(obj) and is_torch(aux_rows) and tuple(obj.shape) == tuple(nat.aux.shape)
                    and tuple(aux_rows.shape) == tuple(nat.aux.shape)):
                raise NotImplementedError("a host-evaluated matrix penalty on mode 0 whose auxiliary variable is not the matrix "
                                          "itself (aux_as_matrix is not the identity) is not supported with group=")
        full = reg.factor_matrix_update(self.gather_rows_A(eng.A + nat.dual), float(rho_a[0]), self.gather_rows_A(aux_rows))
        lo, hi = self.grp.own_rows("A rows")
        z = reg.aux_as_matrix(full)[lo:hi].to(nat.aux.dtype)
        if obj is not None:
            self.ext_aux[(0, k)] = full[lo:hi].clone()  # this rank's rows of the object the penalty returned (what return_admm_vars hands out)
        nat.dual.copy_(eng.A - (z - nat.dual))
        nat.aux.copy_(z)

    # ---- diagnostics ----------------------------------------------------------------------------------------------------
    def l1_weights(self):
        """per mode and penalty, what multiplies sum |factor| in the loss: the table of the device stopping rules"""
        return [[(reg.reg_strength if isinstance(reg, penalties.L1Penalty) else 0.0) for reg in self.regs[m]] for m in range(3)]

    def read_diag(self, vec):
        """MCL_DIAG vector (already all-reduced) -> (rec_error, (A_gaps, B_gaps, C_gaps), reg_penalty + l2)"""
        eng, sharded, l2_penalty = self.eng, self.grp.sharded, self.opt.l2_penalty
        d = vec.detach().cpu().numpy() if is_torch(vec) else np.asarray(vec)
        xsq, inner, model = d[_engine.DIAG_X_SQ], d[_engine.DIAG_INNER], d[_engine.DIAG_MODEL_SQ]
        norm_matrices = np.sqrt(xsq)
        rec_error = np.sqrt(max(0.0, xsq - 2 * inner + model)) / norm_matrices
        gaps, reg_penalty = [], 0.0
        for mode in range(3):
            fnorm = np.sqrt(d[_engine.DIAG_NORM_SQ + mode])
            mode_gaps = []
            for k, reg in enumerate(self.regs[mode]):
                base, kind = _diag_slot(mode, k), self.native[mode][k].kind
                mode_gaps.append(np.sqrt(d[base]) / fnorm)
                if isinstance(reg, penalties.L1Penalty):
                    reg_penalty += reg.reg_strength * d[base + 1]
                elif sharded and mode == 1 and kind in (_engine.PEN_EXTERNAL, _engine.PEN_TV, _engine.PEN_GL2):
                    reg_penalty += d[base + 1]  # this rank's matrices only: summed over the ranks with the vector (diagnostics())
                elif kind == _engine.PEN_GL2:
                    reg_penalty += float(eng.penalty_value(mode, k))  # trace(F^T M F), evaluated by the engine
                elif kind in (_engine.PEN_EXTERNAL, _engine.PEN_TV) or (mode == 0 and sharded and self.gathered_A[k]):
                    # value computed on device tensors; a sharded A is gathered first (every rank adds the same, whole value)
                    factor = [eng.B[sl] for sl in self.row_slices] if mode == 1 else (
                        (self.gather_rows_A(eng.A) if sharded else eng.A) if mode == 0 else eng.C)
                    reg_penalty += float(reg.penalty(factor))
            gaps.append(mode_gaps)
            if l2_penalty[mode]:
                reg_penalty += 0.5 * l2_penalty[mode] * d[_engine.DIAG_NORM_SQ + mode]
        return rec_error, tuple(gaps), reg_penalty

    def read_diag_rows(self, rows):
        """read_diag for a whole ring of iterations at once (the same elementwise arithmetic in the same order, vectorised:
        the per-iteration Python of read_diag costs as much as 7 % of a config-3 iteration): (rec_errors, gaps per iteration,
        reg_penalties).  Only for stacks whose penalty values come out of the diagnostics vector (no host-evaluated value).
        (Kept beside read_diag, not under it: on a NaN sum `max(0.0, x)` there gives 0 where `np.maximum` here gives NaN.)"""
        l2_penalty = self.opt.l2_penalty
        d = np.asarray(rows, dtype=np.float64).reshape(-1, _engine.DIAG_LEN)
        xsq, inner, model = d[:, _engine.DIAG_X_SQ], d[:, _engine.DIAG_INNER], d[:, _engine.DIAG_MODEL_SQ]
        rec = np.sqrt(np.maximum(0.0, xsq - 2 * inner + model)) / np.sqrt(xsq)
        reg_pen = np.zeros(len(d))
        per_mode = []
        for mode in range(3):
            fnorm = np.sqrt(d[:, _engine.DIAG_NORM_SQ + mode])
            cols = []
            for k, reg in enumerate(self.regs[mode]):
                base = _diag_slot(mode, k)
                cols.append(np.sqrt(d[:, base]) / fnorm)
                if isinstance(reg, penalties.L1Penalty):
                    reg_pen = reg_pen + reg.reg_strength * d[:, base + 1]
                elif self.native[mode][k].kind in (_engine.PEN_EXTERNAL, _engine.PEN_TV, _engine.PEN_GL2):
                    raise AssertionError("read_diag_rows: host-evaluated penalty value")
            per_mode.append(np.stack(cols, axis=1) if cols else np.zeros((len(d), 0)))
            if l2_penalty[mode]:
                reg_pen = reg_pen + 0.5 * l2_penalty[mode] * d[:, _engine.DIAG_NORM_SQ + mode]
        gaps = [tuple(list(per_mode[m][i]) for m in range(3)) for i in range(len(d))]
        return rec, gaps, reg_pen

    def diagnostics(self):
        eng, grp = self.eng, self.grp
        vec = eng.diagnostics(include_replicated=(grp.rank == 0))
        if grp.sharded:
            # penalties on the B_i whose value is summed on the host (total variation, host-evaluated MatrixPenalty classes):
            # the value over THIS rank's matrices travels in the penalty-value slot of the vector and is summed over the
            # ranks with it
            for k, reg in enumerate(self.regs[1]):
                if isinstance(reg, penalties.L1Penalty):
                    continue  # read_diag takes reg_strength * sum|B| from the native slot, which is summed over the ranks already
                if self.native[1][k].kind == _engine.PEN_GL2:
                    vec[_diag_slot(1, k) + 1] = float(eng.penalty_value(1, k))
                elif self.gathered_B[k]:  # a value over ALL matrices (need not be a sum over them): counted once, by rank 0
                    value = float(reg.penalty(self.gather_matrices_B(eng.B)))
                    vec[_diag_slot(1, k) + 1] = value if grp.rank == 0 else 0.0
                elif self.native[1][k].kind in (_engine.PEN_EXTERNAL, _engine.PEN_TV):
                    vec[_diag_slot(1, k) + 1] = float(reg.penalty([eng.B[sl] for sl in self.row_slices]))
        grp.all_reduce(vec)
        return self.read_diag(vec)


class _ArithmeticRule:
    """arithmetic="auto" above the small-problem limit: decided by CONDITIONING, not by size alone.

    A mode without any penalty solves un-shifted normal equations (the reference: an fp64 SVD, decomposition.py:172, 252-256,
    319-321) and multiplies whatever the fp32 kernels left in its inputs (1e-8 .. 4e-7 relative) by the condition number of
    its system.  On large problems those roundings average out over 1e5 .. 1e7 rows (BASELINE config 4: C to 8e-8 at
    condition 600) and the exact arithmetic would cost passes over X; below _AUTO_EXACT_MAX_ELEMENTS elements neither
    holds.  The condition numbers that matter are those AT THE START OF EACH PHASE (Gauss-Seidel: the A-phase of an
    iteration solves systems built from the B_i and C of the same iteration - a random start has kappa ~30 where the first
    A-phase meets 3e4), so they are measured there: a TRIAL of _AUTO_EXACT_TRIAL_ITERATIONS iterations runs under the engine's
    condition monitor (mcl_condition_monitor: per phase of a penalty-free mode, kappa = ||M||_F ||M^-1||_F of its system, from
    the factors, no pass over X), the initial state is restored, and with a kappa above _AUTO_EXACT_KAPPA the run takes the
    exact arithmetic (fp64 sums of exact products, fp64 inner loops) from its first iteration - the result is that of one
    arithmetic from start to end.  Long runs look again every _AUTO_EXACT_PROBE_EVERY iterations (one monitored iteration) and
    switch forward.  Under `group=` the maxima are all-reduced (every rank switches, or none).  Larger problems keep the fast
    kernels; a badly conditioned one is told about `arithmetic="exact"`.

    `candidate`: the rule still has something to decide.  `with rule.watching(due):` runs its body under the monitor when the
    rule is a candidate and `due`, and decides on what the monitor saw."""

    def __init__(self, run, arithmetic, n_el_total, rank):
        self.run, self.n_el_total, self._mon = run, n_el_total, None
        native, opt = run.native, run.opt
        free_modes = [m for m in range(3) if run.updates[m] and len(run.regs[m]) == 0]
        all_native = not any(r.kind == _engine.PEN_EXTERNAL for m in range(3) for r in native[m])
        has_pf2 = opt.update_B_is and any(r_.kind == _engine.PEN_PARAFAC2 for r_ in native[1]) and rank <= 32
        self.candidate = (arithmetic == "auto" and (bool(free_modes) or (has_pf2 and n_el_total <= _AUTO_EXACT_MAX_ELEMENTS))
                          and n_el_total > float(1 << 20) and opt.n_iter_max > 0 and all_native
                          and hasattr(run.eng, "condition_monitor"))

    def trial(self, n):
        """n iterations under the monitor from the initial state, which is restored; then the decision"""
        eng = self.run.eng
        state = [eng.A, eng.B, eng.C] + [t for m in range(3) for r_ in self.run.native[m] for t in (r_.aux, r_.dual, r_.aux2)
                                         if t is not None]
        saved = [t.clone() for t in state]
        mon = eng.condition_monitor(True, *self.run.updates)
        try:
            self.run.plain_iterations(n)
        finally:
            eng.condition_monitor(False)
        self.run.grp.all_reduce(mon, "max")
        worst = self.kappa_of(mon)
        for t, t0 in zip(state, saved):
            t.copy_(t0)
        del saved
        eng.invalidate()  # the factors changed behind the engine's back
        self.decide(worst, stacklevel=5)

    def watching(self, due=True):
        self._due = self.candidate and due
        return self

    def __enter__(self):
        self._mon = self.run.eng.condition_monitor(True, *self.run.updates) if self._due else None

    def __exit__(self, exc_type, exc, tb):
        mon, self._mon = self._mon, None
        if mon is None:
            return
        self.run.eng.condition_monitor(False)
        if exc_type is None:
            self.run.grp.all_reduce(mon, "max")
            self.decide(self.kappa_of(mon), stacklevel=6)

    @staticmethod
    def kappa_of(mon):
        """monitor vector -> the number the rule looks at: the worst kappa of a penalty-free mode's system, or - on the same
        footing, _AUTO_EXACT_KAPPA / _AUTO_EXACT_POLAR apart - the worst conditioning of a PARAFAC2 polar factor (the Gram route of
        the fast kernels squares it: a factor of condition 1e5 sits at the edge of what fp32 statistics resolve)"""
        m = mon.cpu().numpy()
        return max(float(m[:3].max()), float(m[3]) * (_AUTO_EXACT_KAPPA / _AUTO_EXACT_POLAR))

    def decide(self, worst, stacklevel):
        """`stacklevel`: of the warning, counted from here to the caller of cmf_aoadmm's caller"""
        if self.n_el_total > _AUTO_EXACT_MAX_ELEMENTS:
            self.candidate = False  # (large problems are looked at once, for the warning only)
            if worst > _AUTO_EXACT_WARN_KAPPA:
                warnings.warn(
                    f"cmf_aoadmm: a mode without penalties has normal equations of condition ~{worst:.1e}; the fp32 kernels this "
                    f"problem size takes by default carry about 1e-8 x that in the factors. Pass arithmetic=\"exact\" for the "
                    "reference's fp64 solve (slower: fp64 passes over the matrices).", RuntimeWarning, stacklevel=stacklevel)
        elif worst > _AUTO_EXACT_KAPPA:
            self.run.eng.set_exact(True)
            self.candidate = False
            if self.run.opt.verbose:
                print(f"matcouply_amd: penalty-free mode with condition ~{worst:.1e}: the exact arithmetic from here on")


class _Record:
    """What the outer loop of one fit leaves behind: the diagnostics per iteration (the initial state first) and how it ended."""

    def __init__(self, initial):
        rec_error, gaps, reg_penalty = initial
        self.rec_errors, self.feasibility_gaps, self.losses = [rec_error], [gaps], [0.5 * rec_error ** 2 + reg_penalty]
        self.it = -1  # Needed if n_iter_max <= 0
        self.satisfied, self.message = False, _StopRule.EXHAUSTED
        self.feasible = None  # the feasibility verdict on the last iterate looked at
        self.final_gaps_known = False  # feasibility_gaps[-1] is of the state the fit returns

    def add_rows(self, rec, gaps, reg):
        """a ring of iterations as read_diag_rows reads it"""
        self.feasibility_gaps.extend(gaps)
        self.rec_errors.extend(rec)
        self.losses.extend(0.5 * rec ** 2 + reg)

    def add_verdicts(self, gaps, verdicts, feasibility_tol):
        """a chunk of a device stopping rule: its gaps and its verdict ring [rec_error, loss, worst gap, flags] per iteration"""
        self.feasibility_gaps.extend(gaps)
        if len(verdicts):
            flags = verdicts[:, 3].astype(np.int64)
            self.feasible = bool(flags[-1] & _engine.VERDICT_FEASIBLE) if feasibility_tol else feasibility_tol
            evaluated = (flags & _engine.VERDICT_LOSS_EVALUATED) != 0  # not on infeasible iterates unless errors are recorded (Q10)
            self.rec_errors.extend(verdicts[evaluated, 0].tolist())
            self.losses.extend(verdicts[evaluated, 1].tolist())

    def end_of_device_rule(self, done, code):
        self.it = done - 1
        if code:
            self.satisfied, self.message = True, _StopRule.message_of(code)
        self.final_gaps_known = True

    def metrics(self, rule_active):
        return DiagnosticMetrics(
            rec_errors=self.rec_errors, feasibility_gaps=self.feasibility_gaps, regularized_loss=self.losses,
            satisfied_stopping_condition=(self.satisfied if (self.satisfied or rule_active) else None),
            satisfied_feasibility_condition=self.feasible, message=self.message, n_iter=self.it + 1)


def _choose_loop(run):
    """the outer loop this fit takes"""
    eng, opt, sharded = run.eng, run.opt, run.grp.sharded
    tol, absolute_tol, verbose, n_iter_max, has_ext = opt.tol, opt.absolute_tol, opt.verbose, opt.n_iter_max, run.has_ext
    # penalty values that need a host call per iteration (the device-resident loops below do not apply)
    host_value = any(r.kind in (_engine.PEN_TV, _engine.PEN_EXTERNAL, _engine.PEN_GL2) for m in range(3) for r in run.native[m]) or any(run.gathered_A)
    fast_path = ((not (tol or absolute_tol)) and not sharded and not verbose and n_iter_max > 0 and not any(has_ext)
                 and not host_value)
    lazy_diag = (not (tol or absolute_tol)) and sharded and not verbose and n_iter_max > 0 and not host_value
    # stopping rule on the device (mcl_run): single device, every penalty native, silent.  (tol set with absolute_tol=None is
    # a TypeError in the reference's comparison - the host loop below raises it the same way.)
    device_stop = (bool(tol or absolute_tol) and not sharded and not verbose and n_iter_max > 0 and not any(has_ext)
                   and not host_value and not (tol and absolute_tol is None) and hasattr(eng, "run"))
    # ... and the same rule under sharding (mcl_gate_begin / mcl_verdict): the phases are stepped with their reductions, the
    # diagnostics vector is all-reduced and every rank evaluates the rule on the same bits.  Every rank must enqueue the same
    # number of iterations (their collectives pair up), so the loop runs in fixed chunks with one synchronisation each.
    sharded_stop = (bool(tol or absolute_tol) and sharded and not verbose and n_iter_max > 0 and not any(has_ext)
                    and not host_value and not run.sharded_ball_A and not (tol and absolute_tol is None)
                    and hasattr(eng, "gate_begin"))
    return (_loop_lazy_diag if lazy_diag else _loop_sharded_stop if sharded_stop else _loop_device_stop if device_stop
            else _loop_fast_path if fast_path else _loop_host)


def _loop_lazy_diag(run, rule, rec):
    """sharded, fixed iteration count: nothing depends on the diagnostics inside the loop, so their partial sums stay
    on the device and are all-reduced once for all iterations (one collective per iteration remains: [G | R])"""
    eng, grp, n_iter_max = run.eng, run.grp, run.opt.n_iter_max
    ring = torch.zeros((n_iter_max, _engine.DIAG_LEN), dtype=torch.float64, device=run.device) if run.opt.return_errors else None
    for it in range(n_iter_max):
        with rule.watching(it > 0 and it % _AUTO_EXACT_PROBE_EVERY == 0):
            run.iteration()
            if ring is not None:  # the table reduction rides on the next iteration's C-phase reduction kernel
                eng.diagnostics_deferred(include_replicated=(grp.rank == 0), out=ring[it])
    rec.it = n_iter_max - 1
    if ring is not None:
        eng.flush_diagnostics()
        grp.all_reduce(ring)
        rec.add_rows(*run.read_diag_rows(ring.cpu().numpy()))


def _loop_sharded_stop(run, rule, rec):
    """a stopping rule under sharding: evaluated on the device behind every iteration's all-reduced diagnostics (see _choose_loop)"""
    eng, grp, opt, device, n_iter_max = run.eng, run.grp, run.opt, run.device, run.opt.n_iter_max
    eng.gate_begin(opt.tol, opt.absolute_tol, opt.feasibility_tol, initial_loss=rec.losses[-1], penalty_weight=run.l1_weights(),
                   evaluate_loss_always=opt.return_errors)
    gate_closed = False
    try:
        chunk, done, code = 8, 0, 0
        ring = torch.zeros((n_iter_max if n_iter_max <= 4096 else 4096, _engine.DIAG_LEN), dtype=torch.float64, device=device)
        verdict = torch.zeros((ring.shape[0], 4), dtype=torch.float64, device=device)
        while done < n_iter_max and not code:
            n_now = min(chunk, n_iter_max - done)
            base = done % ring.shape[0]
            if base + n_now > ring.shape[0]:
                base = 0
            for j in range(n_now):
                run.iteration()
                eng.diagnostics(include_replicated=(grp.rank == 0), out=ring[base + j])
                grp.all_reduce(ring[base + j])
                eng.verdict(ring[base + j], done + j, verdict[base + j])
            if is_torch(ring) and ring.is_cuda:
                torch.cuda.synchronize(device)
            stopped, stop_it, code = eng.gate_status()
            n_ran = (stop_it - done + 1) if stopped else n_now
            ring_h, verdict_h = ring[base:base + n_ran].cpu().numpy(), verdict[base:base + n_ran].cpu().numpy()
            rec.add_verdicts(run.read_diag_rows(ring_h)[1], verdict_h, opt.feasibility_tol)
            done += n_ran
            if not stopped:
                code = 0
        eng.gate_end(bool(code))
        gate_closed = True
    finally:
        if not gate_closed:  # an exception inside the loop (a failed collective, a NotImplementedError of a step): never
            eng.gate_end(True)  # leave the context gated - its kernels would silently do nothing from then on
    rec.end_of_device_rule(done, code)


def _loop_device_stop(run, rule, rec):
    """a stopping rule is active (the DEFAULT call: tol=1e-8, absolute_tol=1e-10, feasibility_tol=1e-4): the rule is
    evaluated by a kernel at the end of every iteration (mcl_run), the host enqueues ahead of the verdicts and never
    blocks on one; state-writing kernels behind a stopping iteration see the device-side flag and do nothing, so
    the factors returned are exactly those of the stopping iteration.  Chunked so that the rings stay small."""
    opt, weights = run.opt, run.l1_weights()

    def run_chunk(n_now):
        n_ran, code, ring_h, verdict_h = run.eng.run(
            n_now, opt.tol, opt.absolute_tol, opt.feasibility_tol, initial_loss=rec.losses[-1], penalty_weight=weights,
            evaluate_loss_always=opt.return_errors, update_A=opt.update_A, update_B=opt.update_B_is, update_C=opt.update_C)
        rec.add_verdicts(run.read_diag_rows(ring_h)[1], verdict_h, opt.feasibility_tol)
        return n_ran, code

    done, code, chunk = 0, 0, 4096
    while done < opt.n_iter_max and not code:
        n_now = min(_AUTO_EXACT_PROBE_EVERY if rule.candidate else chunk, opt.n_iter_max - done)
        watched = rule.candidate and done > 0  # the first iteration of every further chunk runs under the condition monitor
        with rule.watching(watched):
            n_ran, code = run_chunk(1 if watched else n_now)
        done += n_ran
        if watched and not code and n_now > 1:
            n_ran, code = run_chunk(n_now - 1)
            done += n_ran
    rec.end_of_device_rule(done, code)


def _loop_fast_path(run, rule, rec):
    """fixed iteration count: the whole outer loop runs natively, diagnostics stay on the device until the end"""
    eng, opt = run.eng, run.opt
    n_iter_max, updates = opt.n_iter_max, dict(update_A=opt.update_A, update_B=opt.update_B_is, update_C=opt.update_C)
    ring = torch.zeros((n_iter_max, _engine.DIAG_LEN), dtype=torch.float64, device=run.device) if opt.return_errors else None
    done = 0
    while done < n_iter_max:  # (one call, unless the conditioning of a penalty-free mode is being watched)
        n_now = min(_AUTO_EXACT_PROBE_EVERY, n_iter_max - done) if rule.candidate else n_iter_max - done
        watched = rule.candidate and done > 0  # the first iteration of every further chunk runs under the monitor
        with rule.watching(watched):
            eng.iterate(1 if watched else n_now, **updates, diag_ring=(ring[done:] if ring is not None else None))
        if watched and n_now > 1:
            eng.iterate(n_now - 1, **updates, diag_ring=(ring[done + 1:] if ring is not None else None))
        done += n_now
    rec.it = n_iter_max - 1
    if ring is not None:
        rec.add_rows(*run.read_diag_rows(ring.cpu().numpy()))


def _loop_host(run, rule, rec):
    """the reference's loop (decomposition.py:990-1053): diagnostics, console output and the stopping rule on the host"""
    opt = run.opt
    progress, stop = _Progress(opt.verbose), _StopRule(opt.tol, opt.absolute_tol, opt.feasibility_tol)
    progress.initial(rec.feasibility_gaps[0])
    for it in range(opt.n_iter_max):
        rec.it = it
        with rule.watching(it > 0 and it % _AUTO_EXACT_PROBE_EVERY == 0):
            run.iteration()
        if not (stop.active or opt.return_errors):
            progress.iteration(it)
            continue
        rec_error, gaps, reg_pen = run.diagnostics()
        rec.feasibility_gaps.append(gaps)
        if stop.active:
            rec.feasible = stop.feasible(gaps)
            if not rec.feasible and not opt.return_errors:
                progress.iteration(it, gaps=gaps)  # the loss is not evaluated on infeasible iterates (Q10)
                continue
        rec.rec_errors.append(rec_error)
        losses = rec.losses
        losses.append(0.5 * rec_error ** 2 + reg_pen)
        progress.iteration(it, rec_error, losses[-1], abs(losses[-2] - losses[-1]) / losses[-2], gaps)
        fired = stop.verdict(rec.feasible, losses)
        if fired is not None:
            rec.satisfied, rec.message = True, fired
            progress.converged(it, fired)
            break
    else:
        progress.exhausted()


def _admm_vars_out(out, row_ptr, state):
    """ADMM variables in the caller's array type; state[mode]: (kind, aux, aux2, dual) per penalty, device tensors (a PEN_EXTERNAL's
    aux: the object its penalty keeps; aux2: the Delta of a PARAFAC2, else None)"""
    auxes, duals = [[], [], []], [[], [], []]
    for mode in range(3):
        for kind, aux, aux2, dual in state[mode]:
            if kind == _engine.PEN_EXTERNAL:
                auxes[mode].append(_aux_out(aux, out))
            elif kind == _engine.PEN_PARAFAC2:
                auxes[mode].append((out.split(aux, row_ptr), out(aux2)))
            else:
                auxes[mode].append(out.split(aux, row_ptr) if mode == 1 else out(aux))
            duals[mode].append(out.split(dual, row_ptr) if mode == 1 else out(dual))
    return ADMMVars(auxes=tuple(auxes), duals=tuple(duals))


def cmf_aoadmm(
    matrices,
    rank,
    init="random",
    n_iter_max=1000,
    l2_penalty=None,
    tv_penalty=None,
    l1_penalty=None,
    non_negative=None,
    unimodal=None,
    generalized_l2_penalty=None,
    l2_norm_bound=None,
    lower_bound=None,
    upper_bound=None,
    parafac2=None,
    regs=None,
    feasibility_penalty_scale=1,
    constant_feasibility_penalty=False,
    aux_init="random_uniform",
    dual_init="random_uniform",
    svd="truncated_svd",
    init_params=None,
    random_state=None,
    tol=1e-8,
    absolute_tol=1e-10,
    feasibility_tol=1e-4,
    inner_tol=None,
    inner_n_iter_max=5,
    update_A=True,
    update_B_is=True,
    update_C=True,
    return_admm_vars=False,
    return_errors=False,
    verbose=False,
    *,
    group=None,
    gather_A=False,
    arithmetic="auto",
    _byproducts=None,
):
    r"""Fit a regularized coupled matrix factorization model with AO-ADMM on an MI355X.

    Parameters, defaults, return values (``cmf`` or ``(cmf[, ADMMVars][, DiagnosticMetrics])``) and stopping rules are
    those of ``matcouply.decomposition.cmf_aoadmm`` (reference decomposition.py:662-1100): regularization parameters may
    be ``None``, a scalar (all modes), a length-3 list, or a ``{mode: value}`` dict; mode 0 is A, mode 1 the B_i, mode 2 C.

    ``matrices`` is a list of I arrays (NumPy or torch, J_i x K) or a :class:`PackedMatrices` already in HBM.  The
    arithmetic runs in fp32 on the device (rank x rank systems and all reductions in fp64); results are returned in the
    array type and dtype of the input.  ``init`` is ``"random"``, ``"svd"``, ``"threshold_svd"``, an explicit
    ``(weights, (A, B_is, C))`` tuple, or a CP start on the zero-padded tensor computed on the device: ``"parafac_als"`` /
    ``"cp_als"`` (CP-ALS) and ``"parafac_hals"`` / ``"cp_hals"`` (non-negative CP-HALS), deterministic (``random_state``
    draws nothing for them), with ``init_params`` keys ``n_iter_max`` (default 50) and ``tol`` (default 1e-8 / 1e-7; 0 runs
    every sweep).  Not supported (out of scope, raise ``NotImplementedError``): ``"parafac2_als"``, other ``init_params``
    keys, a CP start with rank above min(max J_i, K), K or max J_i above 2048, and CP starts under ``group=``.  ``inner_tol`` > 0
    is evaluated by the engine on the device (single-device runs; sharded runs: on a host-driven step path).  Penalties without
    a native kernel (user subclasses of ``matcouply_amd.penalties.ADMMPenalty``) are evaluated through their own Python methods
    on device tensors between the native solve and dual-update steps.

    Sharded runs (``group=``, keyword-only, not in the reference): every rank of the ``torch.distributed`` process group
    passes ITS matrices (see :func:`partition_slabs`) and gets back its rows of ``A``, its ``B_i`` and the replicated ``C``;
    ``arithmetic`` (keyword-only, not in the reference): ``"auto"`` - problems of at most 2^20 elements take every contraction
    as fp64 sums of exact products and their inner ADMM loops in fp64 (the reference's own regime: parity at the storage level
    of fp32), larger ones the fp32 matrix-core kernels; ``"exact"`` forces the former at any size (slower; for large problems
    with ill-conditioned penalty-free modes), ``"fast"`` the latter.
    ``gather_A=True`` all-gathers the rows of ``A`` once at the end (rank order, i.e. the original order for contiguous
    partitions): the factorization returned stays the rank's own, the whole ``A`` rides along as ``cmf.A_all`` with this
    rank's rows at ``cmf.rows_of_rank`` (the ADMM variables of mode 0 stay rank-local).  Per outer iteration
    the ranks exchange the fp64 normal equations ``[G | R]`` of the C-phase, the diagnostic sums while a stopping rule is
    active, one ``r*r + 1`` reduction per inner iteration with PARAFAC2 and a scalar MAX per phase with a constant
    feasibility penalty.  A ``TotalVariationPenalty`` on the ``B_i`` or on ``C`` works under ``group=`` (its value, summed on
    the host, travels with the diagnostic sums; the run then takes the host-driven loop), and so does a host-evaluated
    (user-defined / overridden) ``MatrixPenalty`` on the ``B_i`` - its prox acts on one matrix at a time.  NOT supported with
    ``group=`` (``NotImplementedError``): host-evaluated ``MatricesPenalty`` classes on mode 1 (they may couple matrices
    of different ranks).  Matrix penalties on mode 0 (L2 ball, unimodality, total variation along the rows of ``A``, a
    user's ``MatrixPenalty``) need ``constant_feasibility_penalty``, as in the reference; the L2 ball all-reduces its column
    norms, every other one is evaluated by each rank on the all-gathered ``A`` (I x rank floats).  None of these occurs in the
    BASELINE configurations.

    >>> import numpy as np, matcouply_amd
    >>> len(matcouply_amd.decomposition._listify({1: 0.5}, "l1_penalty"))
    3
    """
    # ---- arguments, and the start with the reference's draw order -------------------------------------------------------
    if arithmetic not in ("auto", "exact", "fast"):
        raise ValueError(f'arithmetic must be "auto", "exact" or "fast", not {arithmetic!r}')
    random_state = check_random_state(random_state)
    svd_fun = get_svd(svd)
    if group is not None and isinstance(init, str) and init in _CP_INITS:
        raise NotImplementedError(f'init="{init}" needs all matrices (its start is a decomposition of the whole padded '
                                  "tensor): not supported with group=; pass an explicit (weights, (A, B_is, C)) tuple instead.")
    kw = dict(init=init, init_params=init_params, non_negative=non_negative, lower_bound=lower_bound, upper_bound=upper_bound,
              l2_norm_bound=l2_norm_bound, unimodal=unimodal, parafac2=parafac2, l1_penalty=l1_penalty, tv_penalty=tv_penalty,
              generalized_l2_penalty=generalized_l2_penalty, svd=svd, regs=regs, dual_init=dual_init, aux_init=aux_init,
              update_A=update_A, update_B_is=update_B_is, update_C=update_C)
    cmf, regs, auxes, duals = _start_penalties(kw, matrices, rank, random_state, svd_fun=svd_fun, verbose=verbose)
    opt = SimpleNamespace(
        l2_penalty=[l2 if l2 is not None else 0 for l2 in _listify(l2_penalty, "l2_penalty")], inner_tol=inner_tol,
        inner_n_iter_max=inner_n_iter_max, update_A=update_A, update_B_is=update_B_is, update_C=update_C, n_iter_max=n_iter_max,
        tol=tol, absolute_tol=absolute_tol, feasibility_tol=feasibility_tol, return_errors=return_errors, verbose=verbose)
    opt.constant_A, opt.constant_B = _constant_flags(constant_feasibility_penalty)

    # ---- move everything to the device: the data, the factors, the penalties' variables -------------------------------------
    sub = _test_engine_factory()
    factory = sub or _default_engine_factory
    device = _device() if sub is None else getattr(sub, "device", torch.device("cpu"))
    # a checker engine without `supports_x16` is handed the exact float32 image of a 16-bit X
    X, row_ptr = _pack(matrices, device) if sub is None else sub.pack(
        matrices if getattr(sub, "supports_x16", False) else _upcast_x16(matrices))
    out = _Out(matrices)
    _, (A0, B0_is, C0) = cmf
    A, B, C = _to_dev(A0, device), _pack_rows(B0_is, device), _to_dev(C0, device)
    if B.shape != (X.shape[0], rank):
        raise ValueError("The B_i matrices of `init` do not match the shapes of `matrices`")
    check_inner = bool(inner_tol) and inner_tol > 0  # on a single device the engine's test, else every prox through the host
    device_inner = check_inner and sub is None and group is None
    native, ext_aux = _native_penalties(regs, auxes, duals, matrices, device, check_inner and not device_inner, group is not None)

    # ---- the engine and the run on it ------------------------------------------------------------------------------------
    grp = _Group(group)
    # the arithmetic of small problems (exact-products mode) is chosen by the size of the WHOLE problem:
    # every rank of a sharded run, and every rank layout of the same problem, then computes with the same kernels
    exact_products = {"auto": 0, "exact": 1, "fast": 2}[arithmetic]
    n_el_total = float(X.shape[0]) * float(X.shape[1])
    if grp.world > 1 and arithmetic == "auto":
        n_el = torch.tensor([n_el_total], dtype=torch.float64, device=X.device)
        grp.all_reduce(n_el)
        n_el_total = float(n_el.item())
        exact_products = 1 if n_el_total <= float(1 << 20) else 2
    eng = factory(X=X, row_ptr=row_ptr, rank=rank, A=A, B=B, C=C, regs=native, l2_penalty=opt.l2_penalty,
                  inner_n_iter_max=inner_n_iter_max, feasibility_penalty_scale=feasibility_penalty_scale,
                  constant_A=opt.constant_A, constant_B=opt.constant_B, exact_products=exact_products,
                  **(dict(inner_tol=inner_tol) if device_inner else {}))
    run = _Run(eng, regs, native, ext_aux, grp, row_ptr, device, opt)
    grp.direct = _direct_comm(group, X.device) if (grp.sharded and sub is None) else None

    # ---- the fit: arithmetic trial, initial diagnostics, one of the four loops, the final feasibility -----------------------
    rule = _ArithmeticRule(run, arithmetic, n_el_total, rank)
    if rule.candidate:
        rule.trial(min(_AUTO_EXACT_TRIAL_ITERATIONS, n_iter_max))
    rec = _Record(run.diagnostics())
    _choose_loop(run)(run, rule, rec)
    if feasibility_tol and return_errors and rec.final_gaps_known:
        # the reference re-evaluates the gaps of the final state here: the state the last verdict was taken on
        rec.feasible = _check_feasibility(rec.feasibility_gaps[-1], feasibility_tol)
    elif feasibility_tol and return_errors:
        _, final_gaps, _ = run.diagnostics()
        rec.feasible = _check_feasibility(final_gaps, feasibility_tol)
    elif not feasibility_tol:
        rec.feasible = None

    # ---- results back in the caller's array type ------------------------------------------------------------------
    cmf = CoupledMatrixFactorization((None, (out(eng.A), out.split(eng.B, row_ptr), out(eng.C))))
    if gather_A and group is not None:
        # the one all-gather of a sharded run, with a count exchange of its own.  The factorization returned
        # stays this rank's (its rows of A, its B_i); the whole A rides along as `cmf.A_all`, this rank's rows being
        # `cmf.A_all[cmf.rows_of_rank[0]:cmf.rows_of_rank[1]]`.
        cmf.A_all = out(torch.cat(grp.gather_rows(eng.A, "A at the end"), 0))
        cmf.rows_of_rank = grp.own_rows("A at the end")
    result = [cmf]
    if return_admm_vars:
        result.append(_admm_vars_out(out, row_ptr, [
            [(r.kind, ext_aux[(mode, k)] if r.kind == _engine.PEN_EXTERNAL else r.aux, r.aux2, r.dual)
             for k, r in enumerate(native[mode])] for mode in range(3)]))
    if return_errors:
        result.append(rec.metrics(rule_active=bool(tol or absolute_tol)))
    if _byproducts is not None and update_A:
        _byproducts["rhses"] = out(eng.rhses())
        _byproducts["cross_products"] = out(eng.cross_products())
    if hasattr(eng, "close"):
        eng.close()
    return result[0] if len(result) == 1 else tuple(result)


def _single_phase(mode, matrices, reg, cmf, aux_list, dual_list, l2_penalty, inner_n_iter_max, inner_tol,
                  feasibility_penalty_scale, constant_feasibility_penalty):
    """One call of one phase on the device, with the given ADMM variables as initial state."""
    if len(reg) != len(aux_list) or len(reg) != len(dual_list):
        raise ValueError("reg, aux and dual lists must have the same length")
    stack = []
    for r_k, aux, dual in zip(reg, aux_list, dual_list):
        r_c = copy(r_k)  # same penalty, initial state = the caller's variables
        r_c.aux_init, r_c.dual_init = aux, dual
        stack.append(r_c)
    weights, (A, B_is, C) = cmf
    regs = [[], [], []]
    regs[mode] = stack
    l2 = [0, 0, 0]
    l2[mode] = l2_penalty if l2_penalty else 0
    by = {}
    new_cmf, admm = cmf_aoadmm(
        matrices, A.shape[1], init=(None, (A, B_is, C)), regs=regs, l2_penalty=l2, n_iter_max=1, tol=None, absolute_tol=None,
        feasibility_tol=None, inner_tol=inner_tol, inner_n_iter_max=inner_n_iter_max,
        feasibility_penalty_scale=feasibility_penalty_scale,
        constant_feasibility_penalty=({0: "A", 1: "B"}.get(mode, False) if constant_feasibility_penalty else False),
        update_A=(mode == 0), update_B_is=(mode == 1), update_C=(mode == 2), return_admm_vars=True, _byproducts=by)
    out_cmf = (None, [new_cmf[1][0], new_cmf[1][1], new_cmf[1][2]])
    return out_cmf, list(admm.auxes[mode]), list(admm.duals[mode]), by


def admm_update_A(matrices, reg, cmf, A_aux_list, A_dual_list, l2_penalty, inner_n_iter_max, inner_tol,
                  feasibility_penalty_scale, constant_feasibility_penalty, svd_fun=None):
    """One A-phase (reference: decomposition.py:120-219, same positional arguments and return value
    ``(cmf, A_aux_list, A_dual_list, (rhses, cross_products))``) on the device.  `svd_fun` is accepted for compatibility:
    the r x r systems are symmetric positive definite and solved by Gauss-Jordan elimination in fp64 registers."""
    out_cmf, aux, dual, by = _single_phase(0, matrices, reg, cmf, A_aux_list, A_dual_list, l2_penalty, inner_n_iter_max,
                                           inner_tol, feasibility_penalty_scale, constant_feasibility_penalty)
    rhses, cross = by["rhses"], by["cross_products"]
    return out_cmf, aux, dual, ([rhses[i] for i in range(len(rhses))], [cross[i] for i in range(len(cross))])


def admm_update_B(matrices, reg, cmf, B_is_aux_list, B_is_dual_list, l2_penalty, inner_n_iter_max, inner_tol,
                  feasibility_penalty_scale, constant_feasibility_penalty, svd_fun=None):
    """One B-phase (reference: decomposition.py:222-292); returns ``(cmf, B_is_aux_list, B_is_dual_list)``."""
    out_cmf, aux, dual, _ = _single_phase(1, matrices, reg, cmf, B_is_aux_list, B_is_dual_list, l2_penalty,
                                          inner_n_iter_max, inner_tol, feasibility_penalty_scale,
                                          constant_feasibility_penalty)
    return out_cmf, aux, dual


def admm_update_C(matrices, reg, cmf, C_aux_list, C_dual_list, l2_penalty, inner_n_iter_max, inner_tol,
                  feasibility_penalty_scale, svd_fun=None):
    """One C-phase (reference: decomposition.py:295-344); returns ``(cmf, C_aux_list, C_dual_list)``."""
    out_cmf, aux, dual, _ = _single_phase(2, matrices, reg, cmf, C_aux_list, C_dual_list, l2_penalty, inner_n_iter_max,
                                          inner_tol, feasibility_penalty_scale, False)
    return out_cmf, aux, dual


def parafac2_aoadmm(
    matrices,
    rank,
    init="random",
    n_iter_max=1000,
    l2_penalty=0,
    tv_penalty=None,
    l1_penalty=None,
    non_negative=None,
    unimodal=None,
    generalized_l2_penalty=None,
    l2_norm_bound=None,
    lower_bound=None,
    upper_bound=None,
    regs=None,
    feasibility_penalty_scale=1,
    constant_feasibility_penalty=False,
    aux_init="random_uniform",
    dual_init="random_uniform",
    svd="truncated_svd",
    init_params=None,
    random_state=None,
    tol=1e-8,
    absolute_tol=1e-10,
    feasibility_tol=1e-4,
    inner_tol=None,
    inner_n_iter_max=5,
    update_A=True,
    update_B_is=True,
    update_C=True,
    return_errors=False,
    return_admm_vars=False,
    verbose=False,
    *,
    group=None,
    gather_A=False,
    arithmetic="auto",
):
    """Alias for cmf_aoadmm with the PARAFAC2 constraint on mode 1 (reference decomposition.py:1103-1179)."""
    return cmf_aoadmm(
        matrices=matrices, rank=rank, init=init, n_iter_max=n_iter_max, l2_penalty=l2_penalty, tv_penalty=tv_penalty,
        l1_penalty=l1_penalty, non_negative=non_negative, unimodal=unimodal,
        generalized_l2_penalty=generalized_l2_penalty, l2_norm_bound=l2_norm_bound, lower_bound=lower_bound,
        upper_bound=upper_bound, parafac2=True, regs=regs, feasibility_penalty_scale=feasibility_penalty_scale,
        constant_feasibility_penalty=constant_feasibility_penalty, aux_init=aux_init, dual_init=dual_init, svd=svd,
        init_params=init_params, random_state=random_state, tol=tol, absolute_tol=absolute_tol,
        feasibility_tol=feasibility_tol, inner_tol=inner_tol, inner_n_iter_max=inner_n_iter_max, update_A=update_A,
        update_B_is=update_B_is, update_C=update_C, return_errors=return_errors, return_admm_vars=return_admm_vars,
        verbose=verbose, group=group, gather_A=gather_A, arithmetic=arithmetic)


def _cmf_kwargs(kwargs, signature=None):
    """a cmf_aoadmm call's keyword arguments (`signature`: another fit's) as a complete dict of its parameters (TypeError for unknown ones)"""
    bound = (signature or inspect.signature(cmf_aoadmm)).bind(None, 1, **kwargs)
    bound.apply_defaults()
    kw = dict(bound.arguments)
    del kw["matrices"], kw["rank"]
    return kw


def _start_penalties(kw, matrices, rank, random_state, svd_fun=None, verbose=False):
    """The one draw of a start, for cmf_aoadmm and the fused kernels alike, in the reference's order: the factors, then - the
    penalty lists of modes that are not updated emptied first - the aux of modes 0, 1, 2, then the duals.  `kw`: cmf_aoadmm keywords."""
    cmf = initialize_cmf(matrices, rank, kw["init"], svd_fun=svd_fun, random_state=random_state, init_params=kw["init_params"])
    regs = _parse_all_penalties(
        non_negative=kw["non_negative"], lower_bound=kw["lower_bound"], upper_bound=kw["upper_bound"],
        l2_norm_bound=kw["l2_norm_bound"], unimodal=kw["unimodal"], parafac2=kw["parafac2"], l1_penalty=kw["l1_penalty"],
        tv_penalty=kw["tv_penalty"], generalized_l2_penalty=kw["generalized_l2_penalty"], svd=kw["svd"], regs=kw["regs"],
        dual_init=kw["dual_init"], aux_init=kw["aux_init"], verbose=verbose)
    for mode, on in enumerate((kw["update_A"], kw["update_B_is"], kw["update_C"])):
        if not on:
            regs[mode] = []
    auxes = initialize_aux(matrices, rank, regs, random_state=random_state)
    duals = initialize_dual(matrices, rank, regs, random_state=random_state)
    return cmf, regs, auxes, duals


def _constant_flags(constant_feasibility_penalty):
    c = constant_feasibility_penalty
    if isinstance(c, str) and c not in {"A", "B"}:
        raise ValueError(f"If `constant_feasibility_penalty` is a string, it must be 'A' or 'B', not {c}")
    return bool((c and not isinstance(c, str)) or c == "A"), bool((c and not isinstance(c, str)) or c == "B")


def __getattr__(name):  # the re-export: what moved to multistart.py (which imports this module) stays readable here
    from . import multistart
    if name.startswith("__") or name not in vars(multistart):
        raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
    return getattr(multistart, name)
