"""Fits on matrices with missing entries: expectation-maximisation imputation inside the fused
one-workgroup-per-job kernel (csrc/multistart.hip: k_multistart_missing), and what element-wise cross-validation needs around
it - masks that hold out folds of entries, the imputed matrices and the error on the held-out entries.

A job keeps a filled copy of the data: the observed entries, and at the missing ones first the fill, then after every outer
iteration the model ``B_i D_i C^T`` of that iteration.  Each outer iteration is ``cmf_aoadmm``'s on the filled copy; the
reconstruction error and the loss are taken over the observed entries alone."""
import numpy as np

from . import _engine, decomposition as dec, multistart as ms
from ._utils import check_random_state, is_torch, shape, to_numpy, torch

FILLS = ("column_mean", "zero", "model")


def _host64(m):
    """a matrix as a NumPy fp64 array (16-bit torch tensors upcast exactly first: NumPy has no bfloat16)"""
    if is_torch(m) and m.dtype in (torch.bfloat16, torch.float16):
        m = m.float()
    return np.asarray(to_numpy(m), dtype=np.float64)


def _matrix_list(matrices):
    return [matrices[i] for i in range(len(matrices))]


def _one_mask(mask, shapes, where):
    """a list of I boolean arrays shaped like the matrices -> one packed boolean array [N, K]"""
    if len(mask) != len(shapes):
        raise ValueError(f"{where} holds {len(mask)} arrays for {len(shapes)} matrices")
    out = []
    for i, (m, shp) in enumerate(zip(mask, shapes)):
        m = np.asarray(to_numpy(m))
        if m.shape != shp:
            raise ValueError(f"{where}[{i}] has shape {m.shape}, its matrix {shp}")
        out.append(m.astype(bool))
    return np.concatenate(out, 0)


def _is_array(x):
    return hasattr(x, "shape") and len(shape(x)) == 2


def observed_masks(matrices, observed, n_jobs=None):
    """The masks of a call as packed boolean arrays: (masks [n_masks, N, K], X [N, K] fp64 on the host, row_ptr).  ``observed``
    None: the entries that are not NaN, one mask; a list of I boolean arrays shaped like the matrices: one mask, shared by all
    jobs; a list of ``n_jobs`` such lists: one mask per job.  ``ValueError`` for a mask of the wrong shape, a mask under which a
    matrix has no observed entry, and a NaN at an observed entry."""
    mats = [_host64(m) for m in _matrix_list(matrices)]
    shapes = [m.shape for m in mats]
    row_ptr = np.concatenate([[0], np.cumsum([s[0] for s in shapes])]).astype(np.int64)
    X = np.concatenate(mats, 0)
    if observed is None:
        masks = ~np.isnan(X)[None]
    else:
        observed = list(observed)
        if len(observed) and all(_is_array(m) for m in observed):
            masks = _one_mask(observed, shapes, "observed")[None]
        else:
            if n_jobs is not None and len(observed) != n_jobs:
                raise ValueError(f"observed holds {len(observed)} masks for {n_jobs} jobs (one list of {len(shapes)} boolean "
                                 "arrays for all jobs, or one such list per job)")
            masks = np.stack([_one_mask(list(m), shapes, f"observed[{s}]") for s, m in enumerate(observed)])
    for s, mask in enumerate(masks):
        for i in range(len(shapes)):
            if row_ptr[i + 1] > row_ptr[i] and not mask[row_ptr[i]: row_ptr[i + 1]].any():
                raise ValueError(f"mask {s}: matrix {i} has no observed entry")
        if np.isnan(X[mask]).any():
            raise ValueError(f"mask {s}: NaN at an observed entry")
    return masks, X, row_ptr


def column_means(X, masks):
    """[n_masks, K] fp64: per mask the mean of the observed entries of every column over all matrices; 0 for a column without one"""
    Xz = np.where(masks, X[None], 0.0)
    count = masks.sum(axis=1)
    return np.where(count > 0, Xz.sum(axis=1) / np.maximum(count, 1), 0.0)


def cmf_aoadmm_missing(matrices, rank, observed, random_states, *, fill="column_mean", **cmf_aoadmm_kwargs):
    """Fit matrices with missing entries from several random starts, or under several masks, in one launch: element ``s`` of the
    list returned is what ``cmf_aoadmm(matrices, rank, random_state=random_states[s], **cmf_aoadmm_kwargs)`` returns (same tuple
    structure, array types and ``DiagnosticMetrics``) for the loss over the observed entries ``O``,

        ``0.5 sum_O (X - B_i D_i C^T)^2 / sum_O X^2 + penalties + l2 terms``,

    by expectation-maximisation: every outer iteration is ``cmf_aoadmm``'s on a filled copy of the data, and then the missing
    entries of the copy are set to the new model.  ``rec_errors`` and ``regularized_loss`` use the observed entries alone.

    ``observed``: ``None`` - the NaN entries are missing; a list of I boolean arrays shaped like the matrices (True = observed),
    shared by all jobs; or a list of ``len(random_states)`` such lists, one mask per job (:func:`entry_kfold`).  What the
    matrices hold at a missing entry is never used.  ``fill`` is where the missing entries start: ``"column_mean"`` (the mean of
    the job's observed entries of that column k over all matrices; 0 for a column without one), ``"zero"`` or ``"model"`` (the
    start's ``B_i D_i C^T``).

    The jobs run in the fused fp64 kernel of ``cmf_aoadmm_multistart(method="fused")``, one workgroup per job, and what that does
    not serve raises ``NotImplementedError`` with its sentence before the device is touched: there is no sequential method.
    Only ``init="random"``.  ``ValueError``, before the device is touched: a mask of the wrong shape, a job in which a matrix has
    no observed entry, a NaN at an observed entry.  16-bit matrices are read as stored; results come back in the input's dtype."""
    ms._check_start_keywords("cmf_aoadmm_missing", cmf_aoadmm_kwargs)
    if fill not in FILLS:
        raise ValueError(f"fill must be one of {FILLS}, not {fill!r}")
    random_states = list(random_states)
    rank = int(rank)
    kw = dec._cmf_kwargs(cmf_aoadmm_kwargs)
    reason = ms._multistart_unfused_reason(matrices, rank, kw)
    if reason is not None:
        raise NotImplementedError(f"cmf_aoadmm_missing: {reason}")
    masks, X, _ = observed_masks(matrices, observed, len(random_states))
    if not random_states:
        return []
    if fill == "column_mean":
        fill_values = column_means(X, masks)
    else:
        fill_values = np.zeros((len(masks), X.shape[1])) if fill == "zero" else None

    def run(X, row_ptr, rank, options, state):  # the masks and fills follow the state to the device
        observed, fills = (None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(state.device)
                           for a in (masks.astype(np.uint8), fill_values))
        return _engine.multistart_run_missing(X, row_ptr, rank, options[0], observed, fills, state)
    return ms._multistart_fused(matrices, rank, random_states, [kw], run)


def parafac2_aoadmm_missing(matrices, rank, observed, random_states, *, fill="column_mean", **parafac2_aoadmm_kwargs):
    """:func:`cmf_aoadmm_missing` with the PARAFAC2 constraint on mode 1 (``parafac2_aoadmm``'s defaults)."""
    kwargs = ms._parafac2_keywords("parafac2_aoadmm_missing", parafac2_aoadmm_kwargs)
    return cmf_aoadmm_missing(matrices, rank, observed, random_states, fill=fill, **kwargs)


def _model_of(result):
    """the (A, B_is, C) of a fitted model: a CoupledMatrixFactorization, (weights, (A, B_is, C)) or a result tuple led by one"""
    if isinstance(result, tuple) and result and isinstance(result[0], dec.CoupledMatrixFactorization):
        result = result[0]
    weights, (A, B_is, C) = result
    A = _host64(A)
    if weights is not None:
        A = A * _host64(weights)
    return A, [_host64(B) for B in B_is], _host64(C)


def _reconstruction(result):
    A, B_is, C = _model_of(result)
    return [(B * A[i]) @ C.T for i, B in enumerate(B_is)]


def impute(matrices, cmf, observed=None):
    """The matrices with their missing entries replaced by the model's ``B_i D_i C^T`` (computed in fp64 on the host), in the
    array type, dtype and device of the input.  ``observed``: None (NaN entries are missing) or one list of I boolean arrays."""
    masks, X, row_ptr = observed_masks(matrices, observed, None)
    if len(masks) != 1:
        raise ValueError("impute takes one mask: a list of I boolean arrays")
    out = []
    for i, (m, model) in enumerate(zip(_matrix_list(matrices), _reconstruction(cmf))):
        full = np.where(masks[0][row_ptr[i]: row_ptr[i + 1]], X[row_ptr[i]: row_ptr[i + 1]], model)
        if is_torch(m):
            out.append(torch.as_tensor(full).to(device=m.device, dtype=m.dtype))
        else:
            dtype = m.dtype if isinstance(m, np.ndarray) and np.issubdtype(m.dtype, np.floating) else np.float64
            out.append(full.astype(dtype))
    return out


def entry_kfold(matrices, n_folds, random_state=None, observed=None):
    """``n_folds`` per-job masks for element-wise cross-validation: a random partition of the observed entries into ``n_folds``
    folds of sizes that differ by at most one; mask ``f`` is the observed entries without fold ``f``.  Returned as the
    ``observed`` argument of :func:`cmf_aoadmm_missing`: a list of ``n_folds`` lists of I boolean arrays."""
    n_folds = int(n_folds)
    masks, _, row_ptr = observed_masks(matrices, observed, None)
    if len(masks) != 1:
        raise ValueError("entry_kfold takes one mask: a list of I boolean arrays")
    where = np.flatnonzero(masks[0].ravel())
    if not 2 <= n_folds <= len(where):
        raise ValueError(f"need 2 <= n_folds <= {len(where)} observed entries, not {n_folds}")
    fold = np.empty(len(where), dtype=np.int64)
    fold[check_random_state(random_state).permutation(len(where))] = np.arange(len(where)) % n_folds
    out = []
    for f in range(n_folds):
        mask = masks[0].copy()
        mask.ravel()[where[fold == f]] = False
        out.append([mask[row_ptr[i]: row_ptr[i + 1]] for i in range(len(row_ptr) - 1)])
    return out


def heldout_entry_sse(matrices, results, job_observed, observed=None):
    """Per job, the squared error of its model over the entries that are observed in the data (``observed``: None for not NaN, or
    one list of I boolean arrays) but were held out of the job (``job_observed``: the per-job masks the jobs were fitted under),
    and their number: (sse float64 [n_jobs], count int64 [n_jobs]).  ``sse.sum() / count.sum()`` over the jobs of an
    :func:`entry_kfold` run is the cross-validated mean squared error.  NumPy fp64 on the host."""
    data, X, _ = observed_masks(matrices, observed, None)
    if len(data) != 1:
        raise ValueError("heldout_entry_sse takes one data mask: a list of I boolean arrays")
    results = list(results)
    shapes = [tuple(shape(m)) for m in _matrix_list(matrices)]
    job_observed = list(job_observed)
    if len(job_observed) != len(results):
        raise ValueError(f"job_observed holds {len(job_observed)} masks for {len(results)} results")
    sse, count = np.zeros(len(results)), np.zeros(len(results), dtype=np.int64)
    for s, (res, mask) in enumerate(zip(results, job_observed)):
        held = data[0] & ~_one_mask(list(mask), shapes, f"job_observed[{s}]")
        model = np.concatenate(_reconstruction(res), 0)
        sse[s] = float(np.sum((X[held] - model[held]) ** 2))
        count[s] = int(held.sum())
    return sse, count
