"""Resample a fit over its matrices, mode 0: bootstrap replicates, the jackknife and K folds - of PARAFAC2-ALS (DESIGN.md
section 17, below) and of the constrained AO-ADMM fits cmf_aoadmm / parafac2_aoadmm (section 18, the second half of the module).

Every such scheme is the same fit with a non-negative weight per matrix: minimise ``sum_i w_i ||X_i - P_i B diag(a_i) C^T||^2``.
That weighted fit is exactly the unweighted fit of the matrices ``sqrt(w_i) X_i`` with row i of A divided by ``sqrt(w_i)``
afterwards, so the jobs of one call share the one X on the device and differ by I scale factors each.

* :func:`resampling_weights` draws the weights of a scheme, one row per job;
* :func:`parafac2_als_resample` fits all jobs, in one launch of the fused kernel (csrc/pf2als_multistart.hip) where it serves
  the call;
* :func:`resample_summary` lines the replicates up with a reference model and returns mean, spread and quantiles per entry;
* :func:`resample_heldout_sse` projects every job's left-out matrices on the job's model (``parafac2_project``): the
  cross-validated error of a K-fold run.

The AO-ADMM fits carry penalties on A that are not scale-invariant (an L1 penalty, a norm ball), so the weights go into the
algorithm there: :func:`cmf_aoadmm_resample` / :func:`parafac2_aoadmm_resample` fit the loss of ``cmf_aoadmm`` with the data
term ``0.5 sum_i w_i ||X_i - B_i D_i C^T||^2 / sum_i w_i ||X_i||^2`` (csrc/multistart.hip, k_multistart_weighted),
:func:`cmf_resample_summary` summarises the replicates and :func:`parafac2_aoadmm_heldout_sse` scores the left-out matrices.
"""
from collections import namedtuple
import warnings

import numpy as np

from . import _engine, decomposition as dec, multistart as ms
from ._utils import check_random_state, is_tensor, to_numpy, torch

__all__ = ["resampling_weights", "parafac2_als_resample", "resample_summary", "resample_heldout_sse", "ResampleSummary",
           "FactorSummary", "HeldOut", "cmf_aoadmm_resample", "parafac2_aoadmm_resample", "cmf_resample_summary",
           "parafac2_aoadmm_heldout_sse", "CmfResampleSummary"]

FactorSummary = namedtuple("FactorSummary", ["mean", "std", "quantiles"])
ResampleSummary = namedtuple("ResampleSummary", ["A", "B", "C", "fms", "permutations"])
HeldOut = namedtuple("HeldOut", ["indices", "slab_sse", "slab_norm"])
CmfResampleSummary = namedtuple("CmfResampleSummary", ["A", "B_is", "C", "fms", "permutations"])


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


def _sequential(matrices, rank, weights, starts, modes, kw):
    device = dec._device()
    X, row_ptr = dec._pack(matrices, device)
    I, N = len(row_ptr) - 1, int(row_ptr[-1])
    rows = np.diff(row_ptr)
    tol, absolute_tol = ms._pf2als_tolerances(kw)
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
    ms._check_method(method)
    for key in ("random_state", "init"):
        if key in parafac2_als_kwargs:
            raise TypeError(f"parafac2_als_resample takes starts, not {key}")
    kw = ms._pf2als_kwargs(parafac2_als_kwargs)
    rank = int(rank)
    I, K, rows, modes = dec._parafac2_als_options(matrices, rank, "random", kw["nn_modes"], kw["n_iter_max"], kw["n_iter_parafac"],
                                                  kw["kwargs"])
    weights = _check_weights(slab_weights, I)
    job_starts = _job_starts(starts, len(weights), I, K, rank)
    if ms._pf2als_fused_serves("parafac2_als_resample", method, rank, rows, K, len(weights), "jobs"):
        return ms._pf2als_fused(matrices, rank, job_starts, modes, kw, scale=np.sqrt(weights))
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


# ------------------------------------------------------------------------------------------------------------
# the constrained AO-ADMM fits under weights on the matrices
# ------------------------------------------------------------------------------------------------------------
# parafac2_aoadmm_heldout_sse takes a result for a PARAFAC2 fit when every B_i^T B_i of its positive-weight matrices lies within
# this relative distance (Frobenius) of their mean: a fit that met feasibility_tol = 1e-4 is within ~2e-4, an unconstrained B_i
# is of order one away
_PARAFAC2_GRAM_TOL = 0.05


def _scaling_refusal(kw, regs):
    """why the fit of the matrices sqrt(w_i) X_i is not the weighted fit (a sentence), or None: the identity needs penalties on
    A that are positively homogeneous and no other term that sees the scale of a row of A"""
    from . import penalties

    if any(type(reg) is not penalties.NonNegativity for reg in regs[0]):
        return "a penalty on A other than NonNegativity is not invariant under the scaling of a row of A"
    l2 = dec._listify(kw["l2_penalty"], "l2_penalty")
    if l2[0]:
        return "l2_penalty on A is not invariant under the scaling of a row of A"
    if dec._constant_flags(kw["constant_feasibility_penalty"])[0] and regs[0]:
        return "a constant feasibility penalty on A takes its maximum over the scaled rows"
    return None


def _rows_back(x, keep, n, divide=None):
    """x [len(keep), r] as rows `keep` of an [n, r] array of zeros of its type, row k divided by divide[k]"""
    if torch is not None and torch.is_tensor(x):
        full = torch.zeros((n,) + tuple(x.shape[1:]), dtype=x.dtype, device=x.device)
        if divide is not None:
            x = (x.double() / torch.as_tensor(divide, device=x.device)[:, None]).to(x.dtype)
        full[torch.as_tensor(keep, device=x.device)] = x
        return full
    x = np.asarray(x)
    full = np.zeros((n,) + x.shape[1:], dtype=x.dtype)
    full[keep] = x if divide is None else (x / np.asarray(divide)[:, None]).astype(x.dtype)
    return full


def _list_back(xs, keep, rows):
    """the list xs of the kept matrices with zero matrices [rows[i], r] of its type in the places left out"""
    like, xs = xs[0], iter(xs)
    kept = set(int(i) for i in keep)
    zeros = (lambda n: like.new_zeros((n, like.shape[1]))) if torch is not None and torch.is_tensor(like) \
        else (lambda n: np.zeros((n, like.shape[1]), dtype=like.dtype))
    return [next(xs) if i in kept else zeros(rows[i]) for i in range(len(rows))]


def _sequential_job(matrices, rank, w, random_state, call_kwargs, kw, refusal):
    I = len(matrices)
    keep = np.flatnonzero(w > 0)
    scale = np.sqrt(w[keep])
    scaled = bool((scale != 1).any())
    if scaled and refusal is not None:
        raise NotImplementedError(f"cmf_aoadmm_resample(method=\"sequential\") with weights other than 0 and 1: {refusal}")
    rows = [int(dec.shape(matrices[i])[0]) for i in range(I)]
    mats = [matrices[i] if f == 1 else matrices[i] * float(f) for i, f in zip(keep, scale)]
    args = dict(call_kwargs)
    init = kw["init"]
    if not isinstance(init, str):
        weights, (A0, B0_is, C0) = init
        A0 = to_numpy(A0).astype(np.float64) if weights is None else to_numpy(A0).astype(np.float64) * to_numpy(weights)
        args["init"] = (None, (A0[keep] * scale[:, None], [B0_is[i] for i in keep], C0))
    result = dec.cmf_aoadmm(mats, rank, random_state=random_state, **args)
    parts = list(result) if isinstance(result, tuple) and not isinstance(result, dec.CoupledMatrixFactorization) else [result]
    _, (A, B_is, C) = parts[0]
    parts[0] = dec.CoupledMatrixFactorization((None, (_rows_back(A, keep, I, scale), _list_back(B_is, keep, rows), C)))
    for k, part in enumerate(parts):
        if isinstance(part, dec.ADMMVars):
            def mode0(x):
                return _rows_back(x, keep, I, scale)

            def mode1(x):
                return (_list_back(x[0], keep, rows), x[1]) if isinstance(x, tuple) else _list_back(x, keep, rows)

            parts[k] = dec.ADMMVars(*[([mode0(x) for x in v[0]], [mode1(x) for x in v[1]], list(v[2])) for v in part])
    return parts[0] if len(parts) == 1 else tuple(parts)


def cmf_aoadmm_resample(matrices, rank, slab_weights, random_states, *, method="auto", **cmf_aoadmm_kwargs):
    """Fit one ``cmf_aoadmm`` problem under several sets of non-negative weights on its matrices: element ``j`` of the list
    returned is what ``cmf_aoadmm`` returns for these keywords (``return_errors`` and ``return_admm_vars`` included) for the loss

        ``0.5 sum_i w_ji ||X_i - B_i D_i C^T||^2 / sum_i w_ji ||X_i||^2 + penalties + l2 terms``,

    ``w_j = slab_weights[j]``; ``rec_errors`` are the weighted relative errors.  The AO-ADMM run is ``cmf_aoadmm``'s with every
    per-matrix Gram and right-hand side multiplied by ``w_i``; the penalties are not touched, which is why an L1 penalty or a norm
    ball on A is served (fitting ``sqrt(w_i) X_i`` would change them).  A matrix of weight 0 is not in the job: its row of A, its
    ``B_i`` and its rows of every auxiliary and dual variable come back as exact zeros.  Rows for the usual schemes come from
    :func:`resampling_weights`.

    ``random_states``: one random state per job.  ``init`` is ``"random"`` - job ``j`` draws the start of
    ``cmf_aoadmm(random_state=random_states[j])`` for the full list of matrices, then the part of the zero-weight matrices is set
    to zero - or a fitted model ``(weights, (A, B_is, C))``, a ``CoupledMatrixFactorization`` or a result tuple that starts with
    one: every job then starts from the model's factors with auxiliary and dual variables drawn from its own state, the usual
    bootstrap practice (the jobs differ in their weights).

    ``method="fused"`` fits all jobs in one launch, one workgroup per job on the one shared X (k_multistart_weighted); it serves
    exactly what ``cmf_aoadmm_multistart(method="fused")`` serves and raises ``NotImplementedError`` with the reason otherwise,
    before the device is touched.  ``method="sequential"`` calls ``cmf_aoadmm`` per job on the job's positive-weight matrices
    scaled by ``sqrt(w_i)`` and divides row i of A back; that is the weighted fit only with no penalty on A or NonNegativity,
    ``l2_penalty[0] == 0`` and no constant feasibility penalty with a penalty on A (weights of 0 and 1 are always served: nothing
    is scaled) and raises ``NotImplementedError`` otherwise.  It solves the same problem from a start drawn for the shortened
    list, which is not the fused job's start: the two agree in what they converge to, not iterate by iterate.
    ``method="auto"`` follows the rule of ``cmf_aoadmm_multistart``.  Weights that are not finite, negative or not [n_jobs, I]
    and a job without a positive weight raise ``ValueError`` before the device is touched."""
    ms._check_method(method)
    ms._check_start_keywords("cmf_aoadmm_resample", cmf_aoadmm_kwargs, check_init=False)  # init: "random" or a model, below
    kwargs = dict(cmf_aoadmm_kwargs)
    init = kwargs.get("init", "random")
    if isinstance(init, str):
        if init != "random":
            raise ValueError(f'cmf_aoadmm_resample needs init="random" or a fitted model, not init={init!r}')
    else:
        if isinstance(init, tuple) and init and isinstance(init[0], dec.CoupledMatrixFactorization):
            init = init[0]  # a result tuple: (cmf, diagnostics) or (cmf, admm_vars, diagnostics)
        try:
            weights, (A0, B0_is, C0) = init
        except (TypeError, ValueError):
            raise TypeError("init is \"random\" or a fitted model: (weights, (A, B_is, C)), a CoupledMatrixFactorization or a "
                            "result that starts with one") from None
        kwargs["init"] = dec.CoupledMatrixFactorization((weights, (A0, list(B0_is), C0)))
    rank = int(rank)
    kw = dec._cmf_kwargs(kwargs)
    I = len(matrices)
    weights = _check_weights(slab_weights, I)
    random_states = list(random_states)
    if len(random_states) != len(weights):
        raise ValueError(f"random_states holds {len(random_states)} states for {len(weights)} jobs (one per row of slab_weights)")
    if ms._fused_serves("cmf_aoadmm_resample", method, lambda: ms._multistart_unfused_reason(matrices, rank, kw), len(weights),
                        lambda n: ms._few_aoadmm_jobs(matrices, n, "jobs")):
        run = lambda X, row_ptr, r, options, state: _engine.multistart_run_weighted(X, row_ptr, r, options[0], weights, state)
        return ms._multistart_fused(matrices, rank, random_states, [kw], run, zero_weights=weights)
    if isinstance(matrices, dec.PackedMatrices):
        matrices = [matrices[i] for i in range(I)]
    _, regs, _, _ = dec._start_penalties(kw, matrices, rank, np.random.RandomState(0))
    refusal = _scaling_refusal(kw, regs)
    return [_sequential_job(matrices, rank, w, rs, kwargs, kw, refusal) for w, rs in zip(weights, random_states)]


def parafac2_aoadmm_resample(matrices, rank, slab_weights, random_states, *, method="auto", **parafac2_aoadmm_kwargs):
    """:func:`cmf_aoadmm_resample` with the PARAFAC2 constraint on mode 1 (``parafac2_aoadmm``'s defaults)."""
    kwargs = ms._parafac2_keywords("parafac2_aoadmm_resample", parafac2_aoadmm_kwargs)
    return cmf_aoadmm_resample(matrices, rank, slab_weights, random_states, method=method, **kwargs)


def cmf_resample_summary(replicates, reference, slab_weights, quantiles=(0.025, 0.975)):
    """Line every replicate of :func:`cmf_aoadmm_resample` up with ``reference`` and summarise the entries of the factors (host,
    NumPy float64).

    ``reference``: a model ``(weights, (A, B_is, C))``, a ``CoupledMatrixFactorization`` or a result that starts with one.  Per
    replicate the column permutation comes from ``multistart_similarity(replicates, reference=reference,
    return_permutations=True)``; the signs per component follow :func:`resample_summary`: ``s_C = sign <c_r, c_ref_r>``,
    ``s_A = sign <a_r, a_ref_r>`` over the replicate's positive-weight rows, column r of A, C and every ``B_i`` multiplied by
    ``s_A``, ``s_C`` and ``s_A s_C``, which leaves every ``X_i`` model unchanged.

    Returns ``CmfResampleSummary(A, B_is, C, fms, permutations)``: A and C are ``FactorSummary(mean, std, quantiles)``, ``B_is``
    a list of one per matrix; ``std`` is the n - 1 standard deviation and ``quantiles`` has shape [len(quantiles),
    *factor.shape].  The statistics of row i of A and of ``B_i`` run over the replicates in which matrix i had positive weight
    (``slab_weights`` [n_jobs, I]), NaN where it never had; ``fms`` is every replicate's factor match score."""
    from .similarity import _model_of_result, multistart_similarity

    replicates = list(replicates)
    if not replicates:
        raise ValueError("cmf_resample_summary needs at least one replicate")
    ref = _model_of_result(reference)
    w_ref, (A_ref, B_ref, C_ref) = ref
    A_ref, C_ref = to_numpy(A_ref).astype(np.float64), to_numpy(C_ref).astype(np.float64)
    if w_ref is not None:
        A_ref = A_ref * to_numpy(w_ref).astype(np.float64)
    I = A_ref.shape[0]
    models = [_model_of_result(rep) for rep in replicates]
    weights = _check_weights(slab_weights, I)
    if len(weights) != len(models):
        raise ValueError(f"slab_weights has {len(weights)} rows for {len(models)} replicates")
    q = np.asarray(quantiles, dtype=np.float64).reshape(-1)
    if ((q < 0) | (q > 1)).any():
        raise ValueError("quantiles lie in [0, 1]")
    fms, perms = multistart_similarity(models, reference=ref, return_permutations=True, method="host")
    As, Bs, Cs = [], [[] for _ in range(I)], []
    for model, w, perm in zip(models, weights, perms):
        A, C = (to_numpy(f).astype(np.float64)[:, perm] for f in (model[1][0], model[1][2]))
        if model[0] is not None:
            A = A * to_numpy(model[0]).astype(np.float64)[perm]
        held = w > 0
        s_C = _sign(np.sum(C * C_ref, 0))
        s_A = _sign(np.sum(A[held] * A_ref[held], 0))
        A = A * s_A
        A[~held] = np.nan
        As.append(A), Cs.append(C * s_C)
        for i, B_i in enumerate(model[1][1]):
            B_i = to_numpy(B_i).astype(np.float64)[:, perm] * (s_A * s_C)
            Bs[i].append(B_i if held[i] else np.full_like(B_i, np.nan))
    return CmfResampleSummary(_stats(np.stack(As), q), [_stats(np.stack(b), q) for b in Bs], _stats(np.stack(Cs), q),
                              np.asarray(fms), np.asarray(perms))


def parafac2_aoadmm_heldout_sse(matrices, replicates, slab_weights, **parafac2_project_kwargs):
    """The error of every job's PARAFAC2 model on the matrices the job left out: per job ``j`` of
    :func:`parafac2_aoadmm_resample`, the matrices with ``slab_weights[j, i] == 0`` are passed through ``parafac2_project`` on the
    job's model restricted to its positive-weight matrices (the zero rows of A and the zero ``B_i`` would bias the mean Gram
    the projection takes its blueprint from).  Returns a list of ``HeldOut(indices, slab_sse, slab_norm)`` as
    :func:`resample_heldout_sse` does.  ``ValueError`` for a result that does not come from a PARAFAC2 fit: the ``B_i^T B_i`` of
    its positive-weight matrices are not one matrix (within ``_PARAFAC2_GRAM_TOL``)."""
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
    for j, (rep, w) in enumerate(zip(replicates, weights)):
        model_weights, (A, B_is, C) = _model_of_result(rep)
        if is_tensor(B_is):
            raise ValueError(f"replicate {j} does not come from parafac2_aoadmm_resample: its B is not a list of B_i")
        keep = np.flatnonzero(w > 0)
        grams = [(lambda b: b.T @ b)(to_numpy(B_is[i]).astype(np.float64)) for i in keep]
        mean = sum(grams) / len(grams)
        worst = max(np.linalg.norm(g - mean) for g in grams) / max(np.linalg.norm(mean), 1e-300)
        if not worst <= _PARAFAC2_GRAM_TOL:
            raise ValueError(f"replicate {j} does not come from a PARAFAC2 fit: the B_i^T B_i of its matrices differ from their "
                             f"mean by {worst:.3g} (relative), more than {_PARAFAC2_GRAM_TOL}")
        idx = np.flatnonzero(w == 0)
        if not len(idx):
            out.append(HeldOut(idx, np.empty(0), np.empty(0)))
            continue
        A = to_numpy(A).astype(np.float64)
        if model_weights is not None:
            A = A * to_numpy(model_weights).astype(np.float64)
        model = (None, (A[keep], [B_is[i] for i in keep], C))
        proj = parafac2_project([matrices[i] for i in idx], model, **parafac2_project_kwargs)
        out.append(HeldOut(idx, proj.slab_sse, proj.slab_norm))
    return out
