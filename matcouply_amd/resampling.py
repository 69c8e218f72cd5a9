"""Resample a PARAFAC2-ALS fit over its matrices, mode 0: bootstrap replicates, the jackknife and K folds.

Every such scheme is the same fit with a non-negative weight per matrix: minimise ``sum_i w_i ||X_i - P_i B diag(a_i) C^T||^2``.
That weighted fit is exactly the unweighted fit of the matrices ``sqrt(w_i) X_i`` with row i of A divided by ``sqrt(w_i)``
afterwards, so the jobs of one call share the one X on the device and differ by I scale factors each.

* :func:`resampling_weights` draws the weights of a scheme, one row per job;
* :func:`parafac2_als_resample` fits all jobs, in one launch of the fused kernel (csrc/pf2als_multistart.hip) where it serves
  the call;
* :func:`resample_summary` lines the replicates up with a reference model and returns mean, spread and quantiles per entry;
* :func:`resample_heldout_sse` projects every job's left-out matrices on the job's model (``parafac2_project``): the
  cross-validated error of a K-fold run.
"""
from collections import namedtuple
import warnings

import numpy as np

from . import _engine
from . import decomposition as dec
from ._utils import check_random_state, is_tensor, to_numpy

try:
    import torch
except ImportError:  # pragma: no cover
    torch = None

__all__ = ["resampling_weights", "parafac2_als_resample", "resample_summary", "resample_heldout_sse", "ResampleSummary",
           "FactorSummary", "HeldOut"]

FactorSummary = namedtuple("FactorSummary", ["mean", "std", "quantiles"])
ResampleSummary = namedtuple("ResampleSummary", ["A", "B", "C", "fms", "permutations"])
HeldOut = namedtuple("HeldOut", ["indices", "slab_sse", "slab_norm"])


def _positive_int(name, v):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1:
        raise ValueError(f"{name} must be a positive integer, not {v!r}")
    return int(v)


def resampling_weights(n_matrices, scheme, n=None, random_state=None):
    """The weights of a resampling scheme over ``n_matrices`` matrices: a float64 array [n_jobs, n_matrices], one row per job.

    * ``"bootstrap"``: ``n`` jobs; each draws ``n_matrices`` indices with replacement and counts them (rows sum to
      ``n_matrices``);
    * ``"jackknife"``: ``n_matrices`` jobs, job i leaves matrix i out (ones minus the identity); ``n`` must be None;
    * ``"kfold"``: ``n`` folds (2 <= n <= n_matrices) of a shuffled index; job f has weight 0 on fold f and 1 elsewhere.

    Draws come from ``check_random_state(random_state)``.  ``ValueError`` for an unknown scheme, a bad ``n`` and a scheme that
    would leave a job without any matrix (a row of zeros)."""
    I = _positive_int("n_matrices", n_matrices)
    if scheme == "jackknife":
        if n is not None:
            raise ValueError(f'scheme "jackknife" has one job per matrix: n must be None, not {n!r}')
        w = np.ones((I, I)) - np.eye(I)
    elif scheme == "bootstrap":
        n = _positive_int("n", n)
        rs = check_random_state(random_state)
        w = np.stack([np.bincount(rs.randint(0, I, size=I), minlength=I) for _ in range(n)]).astype(np.float64)
    elif scheme == "kfold":
        n = _positive_int("n", n)
        if n > I:
            raise ValueError(f"{n} folds of {I} matrices: a fold would be empty")
        rs = check_random_state(random_state)
        w = np.ones((n, I))
        for f, fold in enumerate(np.array_split(rs.permutation(I), n)):
            w[f, fold] = 0.0
    else:
        raise ValueError(f'scheme must be "bootstrap", "jackknife" or "kfold", not {scheme!r}')
    if not (w.sum(1) > 0).all():
        raise ValueError(f"scheme {scheme!r} over {I} matrices (n = {n}) leaves a job without any matrix")
    return w


def _check_weights(slab_weights, I):
    try:
        w = np.array(to_numpy(slab_weights) if is_tensor(slab_weights) else slab_weights, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("slab_weights must be a real array [n_jobs, n_matrices]") from None
    if w.ndim != 2 or w.shape[1] != I:
        raise ValueError(f"slab_weights must have shape [n_jobs, {I}] (one weight per matrix and job), not {list(w.shape)}")
    if not np.isfinite(w).all() or (w < 0).any():
        raise ValueError("slab_weights must be finite and >= 0")
    if not (w > 0).any(1).all():
        raise ValueError(f"job {int(np.argmin((w > 0).any(1)))} has no positive weight: it would fit no matrix")
    return w


def _model_factors(model):
    """(A, B, C) as float64 arrays of `model`: a triple (A, B, C), what parafac2_als returns, or that with its errors; None when
    `model` is none of these"""
    def triple(x):
        return isinstance(x, (tuple, list)) and len(x) == 3 and all(is_tensor(f) and len(f.shape) == 2 for f in x)

    if triple(model):
        weights, factors = None, model
    elif isinstance(model, (tuple, list)) and len(model) in (2, 3) and triple(model[1]) and (model[0] is None or is_tensor(model[0])):
        weights, factors = model[0], model[1]
    elif isinstance(model, tuple) and len(model) == 2 and isinstance(model[0], (tuple, list)) and len(model[0]) in (2, 3) \
            and triple(model[0][1]):
        weights, factors = model[0][0], model[0][1]
    else:
        return None
    A, B, C = (to_numpy(f).astype(np.float64) for f in factors)
    if weights is not None:
        A = A * to_numpy(weights).astype(np.float64)
    return A, B, C


def _job_starts(starts, n_jobs, I, K, rank):
    """the start (A0, B0, C0) of every job, in the weighted problem's own units"""
    model = _model_factors(starts)
    if model is not None:
        if [f.shape for f in model] != [(I, rank), (rank, rank), (K, rank)]:
            raise ValueError(f"the start model must hold A [{I}, {rank}], B [{rank}, {rank}] and C [{K}, {rank}], not "
                             f"{[list(f.shape) for f in model]}")
        if not all(np.isfinite(f).all() for f in model):
            raise ValueError("the start model holds a non-finite entry")
        return [model] * n_jobs
    try:
        states = list(starts)
    except TypeError:
        raise TypeError("starts is a list of one random state per job, or a fitted model: (A, B, C) or what parafac2_als "
                        "returns") from None
    if len(states) != n_jobs:
        raise ValueError(f"starts holds {len(states)} random states for {n_jobs} jobs (or pass a fitted model)")
    return [dec._pf2als_random_start(I, K, rank, rs) for rs in states]


def _tolerances(kw):
    return (float(kw["tol"]) if kw["tol"] else 0.0), (float(kw["absolute_tol"]) if kw["absolute_tol"] else 0.0)


def _fused(matrices, rank, weights, starts, modes, kw):
    device = dec._device()
    X, row_ptr = dec._pack(matrices, device)
    I, K = len(row_ptr) - 1, int(X.shape[1])
    scale = np.sqrt(weights)
    factors = torch.from_numpy(np.stack([np.concatenate([np.ravel(A0 * scale[j][:, None]), np.ravel(B0), np.ravel(C0)])
                                         for j, (A0, B0, C0) in enumerate(starts)])).to(device)
    slab_scale = torch.from_numpy(np.ascontiguousarray(scale)).to(device)
    tol, absolute_tol = _tolerances(kw)
    P, errors, n_iter = _engine.pf2als_multistart_run_weighted(X, row_ptr, rank, factors, slab_scale, int(kw["n_iter_max"]),
                                                               int(kw["n_iter_parafac"]), tol, absolute_tol, modes)
    errors, n_iter = errors.cpu().numpy(), n_iter.cpu().numpy()
    out = dec._Out(matrices)
    results = []
    for j in range(len(starts)):
        f = factors[j]
        A, B, C = f[: I * rank].view(I, rank), f[I * rank: (I + rank) * rank].view(rank, rank), f[(I + rank) * rank:].view(K, rank)
        s = slab_scale[j][:, None]
        A = torch.where(s > 0, A / torch.where(s > 0, s, torch.ones_like(s)), torch.zeros_like(A))
        result = (None, (out(A), out(B), out(C)), out.split(P[j], row_ptr))
        if kw["return_errors"]:
            result = (result, [float(e) for e in errors[j, : int(n_iter[j]) if tol > 0 else 0]])
        results.append(result)
    return results


def _sequential(matrices, rank, weights, starts, modes, kw):
    device = dec._device()
    X, row_ptr = dec._pack(matrices, device)
    I, N = len(row_ptr) - 1, int(row_ptr[-1])
    rows = np.diff(row_ptr)
    tol, absolute_tol = _tolerances(kw)
    out = dec._Out(matrices)
    results = []
    for w, (A0, B0, C0) in zip(weights, starts):
        keep = np.flatnonzero(w > 0)  # zero-weight matrices are dropped from the pack, not passed as zero matrices
        scale = np.sqrt(w[keep])
        row_idx = torch.from_numpy(np.concatenate([np.arange(row_ptr[i], row_ptr[i + 1]) for i in keep])).to(device)
        row_scale = torch.from_numpy(np.repeat(scale, rows[keep]).astype(np.float32)).to(device)
        Xj = (X.index_select(0, row_idx).float() * row_scale[:, None]).contiguous()
        rp = np.concatenate([[0], np.cumsum(rows[keep])]).astype(np.int64)
        A, B, C, P, errors = _engine.parafac2_als(Xj, rp, rank, (A0[keep] * scale[:, None], B0, C0), int(kw["n_iter_max"]),
                                                  int(kw["n_iter_parafac"]), tol, absolute_tol, modes)
        A_full = torch.zeros((I, rank), dtype=A.dtype, device=A.device)
        A_full[torch.from_numpy(keep).to(A.device)] = A / torch.from_numpy(scale).to(device=A.device, dtype=A.dtype)[:, None]
        P_full = torch.zeros((N, rank), dtype=P.dtype, device=P.device)
        P_full[row_idx.to(P.device)] = P
        result = (None, (out(A_full), out(B), out(C)), out.split(P_full, row_ptr))
        if kw["return_errors"]:
            result = (result, [float(e) for e in errors.cpu().numpy()])
        results.append(result)
    return results


def parafac2_als_resample(matrices, rank, slab_weights, *, starts, method="auto", **parafac2_als_kwargs):
    """Fit one PARAFAC2-ALS problem under several sets of non-negative weights on its matrices: element ``j`` of the list
    returned is the ``parafac2_als`` result tuple (with the errors when ``return_errors=True``) of the problem
    ``min sum_i slab_weights[j, i] ||X_i - P_i B diag(a_i) C^T||^2``; the errors are the weighted relative errors.  A bootstrap
    count k weighs like k copies of the matrix, weight 0 leaves it out: its row of A and its ``P_i`` come back as exact zeros.
    Rows for the usual schemes come from :func:`resampling_weights`.

    ``starts`` is a list of one random state per job - job ``j`` then draws its start as
    ``parafac2_als(random_state=starts[j])`` does - or a fitted model, ``(A, B, C)`` or what ``parafac2_als`` returns, from
    which every job starts: the usual bootstrap practice, which keeps the components in the model's order.  A start is in the
    weighted problem's own units.  ``parafac2_als_kwargs``: the other arguments of ``parafac2_als`` (``init`` and
    ``random_state`` are replaced by ``starts``).

    ``method="fused"`` fits all jobs in one launch, one workgroup per job on the one shared X (each job scales the elements it
    reads by ``sqrt(w_i)``); it serves rank <= 16 and X of at most ``_MULTISTART_MAX_ELEMENTS`` elements and raises
    ``NotImplementedError`` otherwise.  ``method="sequential"`` packs, per job, the positive-weight matrices scaled by
    ``sqrt(w_i)`` and fits them with the ``parafac2_als`` kernels (rank <= 32).  ``method="auto"`` follows
    ``parafac2_als_multistart``.  Weights that are not finite, negative or not [n_jobs, I], a job without a positive weight and
    ``parafac2_als``'s own refusals raise before the device is touched."""
    if method not in ("auto", "fused", "sequential"):
        raise ValueError(f'method must be "auto", "fused" or "sequential", not {method!r}')
    for key in ("random_state", "init"):
        if key in parafac2_als_kwargs:
            raise TypeError(f"parafac2_als_resample takes starts, not {key}")
    kw = dec._pf2als_kwargs(parafac2_als_kwargs)
    rank = int(rank)
    I, K, rows, modes = dec._parafac2_als_options(matrices, rank, "random", kw["nn_modes"], kw["n_iter_max"], kw["n_iter_parafac"],
                                                  kw["kwargs"])
    weights = _check_weights(slab_weights, I)
    job_starts = _job_starts(starts, len(weights), I, K, rank)
    if method != "sequential":
        reason = dec._pf2als_unfused_reason(rank, rows, K)
        if reason is None and method == "auto" and len(weights) < dec._PF2ALS_MS_AUTO_MIN_N \
                and sum(rows) * K * rank > dec._PF2ALS_MS_AUTO_ANY_WORK:
            reason = f"{len(weights)} jobs of {sum(rows) * K} elements at rank {rank} run faster one by one"
        if reason is None:
            return _fused(matrices, rank, weights, job_starts, modes, kw)
        if method == "fused":
            raise NotImplementedError(f"parafac2_als_resample(method=\"fused\"): {reason}")
    return _sequential(matrices, rank, weights, job_starts, modes, kw)


def _sign(x):
    return np.where(x < 0, -1.0, 1.0)


def _stats(stack, quantiles):
    """mean, standard deviation (n - 1) and quantiles over axis 0, skipping NaN entries (a replicate that did not hold the row)"""
    count = np.sum(~np.isnan(stack), 0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)  # a row that no replicate held is all NaN, and stays NaN
        mean = np.nanmean(stack, 0)
        std = np.where(count == 1, 0.0, np.nanstd(stack, 0, ddof=1))
        q = np.nanquantile(stack, quantiles, axis=0)
    return FactorSummary(mean, std, q)


def resample_summary(replicates, reference, slab_weights=None, quantiles=(0.025, 0.975)):
    """Line every replicate of :func:`parafac2_als_resample` up with ``reference`` and summarise the entries of the factors (host,
    NumPy float64).

    ``reference``: what ``parafac2_als`` returns, or ``(A, B, C)``.  Per replicate: the column permutation comes from
    ``multistart_similarity(replicates, reference=reference, return_permutations=True)`` (without the B mode when the reference
    has no projections); per component ``s_C = sign <c_r, c_ref_r>`` and ``s_A = sign <a_r, a_ref_r>`` over the replicate's
    positive-weight rows; column r of A, C and B is multiplied by ``s_A``, ``s_C`` and ``s_A s_C``, which leaves every ``X_i``
    model unchanged.

    Returns ``ResampleSummary(A, B, C, fms, permutations)``: A, B and C are ``FactorSummary(mean, std, quantiles)`` with
    ``quantiles`` of shape [len(quantiles), *factor.shape] and ``std`` the n - 1 standard deviation; for A the statistics of
    row i run over the replicates in which matrix i had positive weight (``slab_weights`` [n_jobs, I]; None: all), NaN for a
    row that never had; ``fms`` is every replicate's factor match score against the reference."""
    from .similarity import _model_of_result, multistart_similarity

    replicates = list(replicates)
    if not replicates:
        raise ValueError("resample_summary needs at least one replicate")
    ref = _model_factors(reference)
    if ref is None:
        raise TypeError("reference is (A, B, C) or what parafac2_als returns")
    A_ref, B_ref, C_ref = ref
    I, r = A_ref.shape
    models = [_model_of_result(rep) for rep in replicates]
    weights = np.ones((len(models), I)) if slab_weights is None else _check_weights(slab_weights, I)
    if len(weights) != len(models):
        raise ValueError(f"slab_weights has {len(weights)} rows for {len(models)} replicates")
    q = np.asarray(quantiles, dtype=np.float64).reshape(-1)
    if ((q < 0) | (q > 1)).any():
        raise ValueError("quantiles lie in [0, 1]")
    has_projections = not _is_triple(reference) and len(_model_of_result(reference)) == 3
    if has_projections:
        fms, perms = multistart_similarity(models, reference=_model_of_result(reference), return_permutations=True, method="host")
    else:
        fms, perms = multistart_similarity([(m[0], m[1]) for m in models], reference=(None, (A_ref, B_ref, C_ref)), skip_mode=1,
                                           return_permutations=True, method="host")
    As, Bs, Cs = [], [], []
    for model, w, perm in zip(models, weights, perms):
        A, B, C = (to_numpy(f).astype(np.float64)[:, perm] for f in model[1])
        if model[0] is not None:
            A = A * to_numpy(model[0]).astype(np.float64)[perm]
        held = w > 0
        s_C = _sign(np.sum(C * C_ref, 0))
        s_A = _sign(np.sum(A[held] * A_ref[held], 0))
        A = A * s_A
        A[~held] = np.nan
        As.append(A), Bs.append(B * (s_A * s_C)), Cs.append(C * s_C)
    return ResampleSummary(_stats(np.stack(As), q), _stats(np.stack(Bs), q), _stats(np.stack(Cs), q), np.asarray(fms), np.asarray(perms))


def _is_triple(x):
    return isinstance(x, (tuple, list)) and len(x) == 3 and all(is_tensor(f) for f in x)


def resample_heldout_sse(matrices, replicates, slab_weights, **parafac2_project_kwargs):
    """The error of every job's model on the matrices the job left out: per job ``j``, the matrices with
    ``slab_weights[j, i] == 0`` are passed through ``parafac2_project`` on the job's ``(B, C)``.  Returns a list of
    ``HeldOut(indices, slab_sse, slab_norm)``, the indices of the left-out matrices and the ``slab_sse`` / ``slab_norm`` of
    their projections; ``sum(slab_sse) / sum(slab_norm)`` over the jobs of a K-fold run is its cross-validated relative error.
    ``parafac2_project_kwargs`` (``method``, ``a_init``, ``n_iter_max``, ...) are passed through."""
    from .projection import parafac2_project
    from .similarity import _model_of_result

    if isinstance(matrices, dec.PackedMatrices):
        matrices = [matrices.X[matrices.row_ptr[i]: matrices.row_ptr[i + 1]] for i in range(len(matrices))]
    matrices = list(matrices)
    replicates = list(replicates)
    weights = _check_weights(slab_weights, len(matrices))
    if len(weights) != len(replicates):
        raise ValueError(f"slab_weights has {len(weights)} rows for {len(replicates)} replicates")
    out = []
    for rep, w in zip(replicates, weights):
        idx = np.flatnonzero(w == 0)
        if not len(idx):
            out.append(HeldOut(idx, np.empty(0), np.empty(0)))
            continue
        _, B, C = _model_of_result(rep)[1]
        proj = parafac2_project([matrices[i] for i in idx], (B, C), **parafac2_project_kwargs)
        out.append(HeldOut(idx, proj.slab_sse, proj.slab_norm))
    return out
