"""Scores of fitted models against the data: fit, per-matrix SSE and core consistency.

A model is ``(weights, (A, B_is, C))`` of rank r; ``weights`` (``None`` = ones) are folded into A, as ``initialize_cmf`` does.
For the data matrices ``X_i`` (J_i x K):

* ``sse_i = ||X_i - B_i diag(a_i) C^T||_F^2``, ``norm_i = ||X_i||_F^2``, ``relative_sse = sum sse_i / sum norm_i``,
  ``fit = 1 - relative_sse``;
* ``S_i = B_i^T X_i C`` and ``W_i = (B_i^T B_i)^+ S_i (C^T C)^+``, which is ``B_i^+ X_i (C^+)^T`` for factors of full column rank;
* the least-squares core ``G[p, q, s] = sum_i (A^+)[p, i] W_i[q, s]``, ``A^+ = (A^T A)^+ A^T``;
* ``core_consistency = 100 (1 - sum (G - T)^2 / r)`` with T the superdiagonal tensor of ones; ``normalised=True`` divides by
  ``sum G^2`` instead of r.

For a PARAFAC2 model (``B_i = P_i Delta`` with orthonormal ``P_i``) this is the core consistency of the projected tensor, for
equal ``B_i`` the one of the CP model.  ``^+`` of a symmetric matrix keeps the eigenvalues above 1e-12 of the largest.

``method="host"`` is NumPy in float64.  ``method="device"`` reads X once per model in a HIP kernel (csrc/evaluate.hip) that forms
``S_i``, ``B_i^T B_i`` and the residual of the same tile, and a second kernel does the r x r and r x r x r algebra in float64.
"""
from collections import namedtuple

import numpy as np

from . import _engine
from ._utils import is_torch, to_numpy
from .coupled_matrices import CoupledMatrixFactorization
from .similarity import _Model, _device_present, _model_of_result, _pack

try:
    import torch
except ImportError:  # pragma: no cover
    torch = None

__all__ = ["core_consistency", "slabwise_sse", "relative_sse", "fit", "multistart_evaluation", "ModelEvaluation"]

ModelEvaluation = namedtuple("ModelEvaluation", ["fit", "relative_sse", "slab_sse", "core_consistency",
                                                 "core_consistency_normalised", "core"])

_EIG_CUT = 1e-12  # relative eigenvalue cut of the pseudo-inverse: the one of csrc/cp_passes.h


def _check_method(method):
    if method not in ("auto", "host", "device"):
        raise ValueError(f'method must be "auto", "host" or "device", not {method!r}')


def _b_rows(cmf):
    """the rows of every B_i of a model, or None where B is given stacked"""
    if isinstance(cmf, CoupledMatrixFactorization):
        B = cmf.factors[1]
    elif len(cmf) == 3:  # a PARAFAC2 tensor: B_i = P_i B
        B = cmf[2]
    else:
        B = cmf[1][1]
    if hasattr(B, "ndim") and B.ndim == 2:
        return None
    return [int(B_i.shape[0]) for B_i in B]


class _Data:
    """the data as the scores see it: its row_ptr and K, the matrices as they were given"""

    def __init__(self, matrices):
        from .decomposition import PackedMatrices

        self.matrices = matrices
        if isinstance(matrices, PackedMatrices):
            self.row_ptr = np.asarray(matrices.row_ptr, dtype=np.int64)
            self.K = int(matrices.X.shape[1])
            self.dtypes = {str(matrices.X.dtype).replace("torch.", "")}
        else:
            self.matrices = mats = list(matrices)
            if not mats:
                raise ValueError("the data holds no matrix")
            if any(m.ndim != 2 for m in mats) or any(int(m.shape[1]) != int(mats[0].shape[1]) for m in mats):
                raise ValueError("All matrices must be second order tensors with the same number of columns")
            self.row_ptr = np.concatenate([[0], np.cumsum([int(m.shape[0]) for m in mats])]).astype(np.int64)
            self.K = int(mats[0].shape[1])
            self.dtypes = {str(m.dtype).replace("torch.", "") for m in mats}
        self.rows = np.diff(self.row_ptr)
        self.I, self.N = len(self.rows), int(self.row_ptr[-1])
        self._host = None

    def host(self):
        """the matrices in float64 on the host"""
        if self._host is None:
            self._host = [(m.detach().to(torch.float64).cpu().numpy() if is_torch(m) else np.asarray(m, dtype=np.float64))
                          for m in self.matrices]
        return self._host


def _models_and_data(cmfs, matrices):
    """[_Model], _Data; ValueError where a model's shape is not the data's"""
    data = _Data(matrices)
    models = []
    for k, cmf in enumerate(cmfs):
        m = _Model(cmf)
        if m.rows != (data.I, data.N, data.K):
            raise ValueError(f"shape mismatch: model {k} has (I, sum J_i, K) = {m.rows}, the data {(data.I, data.N, data.K)}")
        rows = _b_rows(cmf)
        if rows is not None and rows != data.rows.tolist():
            raise ValueError(f"shape mismatch: the B_i of model {k} have {rows} rows, the matrices {data.rows.tolist()}")
        models.append(m)
    if not models:
        raise ValueError("no model to evaluate")
    return models, data


def _pinv_sym(G):
    lam, V = np.linalg.eigh(0.5 * (G + G.T))
    keep = lam > _EIG_CUT * max(lam.max(), 0.0)
    return (V[:, keep] / lam[keep]) @ V[:, keep].T


def _host_factors(model):
    A, B, C = (to_numpy(f).astype(np.float64) for f in model.factors)
    if model.weights is not None:
        A = A * to_numpy(model.weights).astype(np.float64)
    return A, B, C


def _host_tables(model, data):
    """(S [I, r, r], BtB [I, r, r], sse [I], norm [I]) of one model from the definitions"""
    A, B, C = _host_factors(model)
    r = model.rank
    S, BtB = np.empty((data.I, r, r)), np.empty((data.I, r, r))
    sse, norm = np.empty(data.I), np.empty(data.I)
    for i, X in enumerate(data.host()):
        B_i = B[data.row_ptr[i]: data.row_ptr[i + 1]]
        S[i] = B_i.T @ (X @ C)
        BtB[i] = B_i.T @ B_i
        sse[i] = np.sum((X - (B_i * A[i]) @ C.T) ** 2)
        norm[i] = np.sum(X ** 2)
    return S, BtB, sse, norm


def _host_core(model, S, BtB):
    """(core [r, r, r], core_consistency, core_consistency_normalised) from the tables (the Gram route)"""
    A, _, C = _host_factors(model)
    r = model.rank
    CtC_pinv = _pinv_sym(C.T @ C)
    A_pinv = _pinv_sym(A.T @ A) @ A.T
    W = np.stack([_pinv_sym(BtB[i]) @ S[i] @ CtC_pinv for i in range(len(S))])
    core = np.einsum("pi,iqs->pqs", A_pinv, W)
    T = np.zeros((r, r, r))
    T[np.arange(r), np.arange(r), np.arange(r)] = 1.0
    dev = np.sum((core - T) ** 2)
    return core, 100.0 * (1.0 - dev / r), 100.0 * (1.0 - dev / np.sum(core ** 2))


def _device_unserved_reason(models, data, core):
    """why the kernels cannot score these models on this data (a sentence), or None.  Looks at shapes, types and host data only:
    no device call."""
    first = models[0]
    r = first.rank
    if not 1 <= r <= _engine.EVAL_MAX_RANK:
        return f"rank {r} is outside 1 ... {_engine.EVAL_MAX_RANK}"
    if len(models) > _engine.EVAL_MAX_MODELS:
        return f"{len(models)} models in one call (at most {_engine.EVAL_MAX_MODELS})"
    bad = data.dtypes - {"float32", "float64", "bfloat16", "float16"}
    if bad:
        return f"the data holds {sorted(bad)[0]} matrices (float32, bfloat16 and float16 are read as they are, float64 is rounded to float32)"
    if data.rows.min() < 1:
        return "a matrix has no rows"
    if core and (data.rows.min() < r or data.K < r or data.I < r):
        return (f"the core on the device inverts B_i^T B_i, C^T C and A^T A, which are singular with fewer rows than components "
                f"(rank {r}, min J_i {int(data.rows.min())}, K {data.K}, I {data.I})")
    for k, m in enumerate(models):
        if m.rank != r:
            return f"model {k} has rank {m.rank}, model 0 rank {r}: one launch holds models of one shape"
        for t in m.tensors():
            name = str(t.dtype).replace("torch.", "")
            if name not in ("float64", "float32"):
                return f"model {k} holds {name} factors (float64 and float32 are widened exactly, nothing else)"
            if not is_torch(t) and not np.isfinite(t).all():
                return f"model {k} holds a non-finite entry"
    return None


def _device_evaluate(models, data, core):
    """the tables (and the cores) of all models from one call of each C entry, as NumPy arrays"""
    from .decomposition import _device, _pack as pack_data

    device = _device()
    packed, weights = _pack(models, device)
    I, N, K, r = data.I, data.N, data.K, models[0].rank
    if weights is not None:  # folded into A
        packed[:, :I * r] = (packed[:, :I * r].reshape(-1, I, r) * weights[:, None, :]).reshape(-1, I * r)
    if not bool(torch.isfinite(packed).all()):
        raise NotImplementedError("model evaluation on the device: a model holds a non-finite entry")
    X, row_ptr = pack_data(data.matrices, device)
    S, BtB, sse, norm = _engine.eval_tables(X, row_ptr, r, packed)
    out = [sse.cpu().numpy(), norm.cpu().numpy()]
    if core:
        out += [t.cpu().numpy() for t in _engine.eval_core(packed, I, N, K, r, S, BtB)]
    return out


def _evaluate(models, data, method, core):
    """(sse [n, I], norm [I], core [n, r, r, r], cc [n], ccn [n]); the last three None unless `core`.  All the validation of a
    call happens before any device call."""
    _check_method(method)
    if method != "host":
        reason = _device_unserved_reason(models, data, core)
        if reason is None and method == "auto" and not _device_present():
            reason = "no device is present"  # "auto" only: the host serves it
        if reason is None:
            out = _device_evaluate(models, data, core)
            return tuple(out) if core else (out[0], out[1], None, None, None)
        if method == "device":
            raise NotImplementedError(f'model evaluation with method="device": {reason}')
    n, r = len(models), models[0].rank
    sse = np.empty((n, data.I))
    cores, cc, ccn = (np.empty((n, r, r, r)), np.empty(n), np.empty(n)) if core else (None, None, None)
    norm = None
    for k, m in enumerate(models):
        if m.rank != r:
            raise ValueError(f"rank mismatch: model {k} has rank {m.rank}, model 0 rank {r}")
        S, BtB, sse[k], norm = _host_tables(m, data)
        if core:
            cores[k], cc[k], ccn[k] = _host_core(m, S, BtB)
    return sse, norm, cores, cc, ccn


def slabwise_sse(cmf, matrices, normalise=False, method="auto"):
    """The array ``[I]`` of ``||X_i - B_i diag(a_i) C^T||_F^2``; with ``normalise=True`` divided by its sum.  ``cmf`` is a
    ``CoupledMatrixFactorization`` or ``(weights, (A, B_is, C))``, ``matrices`` a list of NumPy arrays or torch tensors or a
    ``PackedMatrices`` (a bfloat16 / float16 one is read as it is).  ``ValueError`` where the model's shape is not the data's.
    ``method``: see :func:`multistart_evaluation`."""
    _check_method(method)
    models, data = _models_and_data([cmf], matrices)
    sse = _evaluate(models, data, method, False)[0][0]
    return sse / sse.sum() if normalise else sse


def relative_sse(cmf, matrices, method="auto"):
    """``sum_i sse_i / sum_i ||X_i||_F^2`` (see :func:`slabwise_sse`)"""
    _check_method(method)
    models, data = _models_and_data([cmf], matrices)
    sse, norm = _evaluate(models, data, method, False)[:2]
    return float(sse[0].sum() / norm.sum())


def fit(cmf, matrices, method="auto"):
    """``1 - relative_sse``"""
    return 1.0 - relative_sse(cmf, matrices, method=method)


def core_consistency(cmf, matrices, normalised=False, method="auto"):
    """The core consistency (CORCONDIA) of the model on the data, in percent: 100 for a model whose least-squares core is the
    superdiagonal of ones (the definition at the top of this module).  ``normalised=True`` divides the deviation by the squared
    norm of the core instead of the rank."""
    _check_method(method)
    models, data = _models_and_data([cmf], matrices)
    out = _evaluate(models, data, method, True)
    return float(out[4][0] if normalised else out[3][0])


def multistart_evaluation(matrices, results, method="auto"):
    """Fit, relative SSE, per-matrix SSE, core consistency (plain and normalised) and the least-squares core of every start of a
    multi-start fit.  ``results`` is what ``cmf_aoadmm_multistart``, ``parafac2_aoadmm_multistart``, ``parafac2_als_multistart``
    or one point of ``cmf_aoadmm_grid`` return: models, or tuples whose first element is the model.  Returns the named tuple
    ``ModelEvaluation(fit [n], relative_sse [n], slab_sse [n, I], core_consistency [n], core_consistency_normalised [n],
    core [n, r, r, r])`` of float64 arrays.

    ``method="host"`` is NumPy in float64 and serves every call.  ``method="device"`` scores all models in one call of each of
    two kernels entries; it serves rank 1 ... 32, models of one rank with finite float64 or float32 factors, float32 / bfloat16 /
    float16 data (float64 data is rounded to float32) and, because the core inverts the Gram matrices of the factors, J_i, K and
    I of at least the rank; otherwise it raises ``NotImplementedError`` with the reason, before the device is touched.
    ``method="auto"`` takes the device when it serves the call and one is present, else the host."""
    _check_method(method)
    results = list(results)
    if not results:
        raise ValueError("multistart_evaluation needs at least one result")
    models, data = _models_and_data([_model_of_result(result) for result in results], matrices)
    sse, norm, core, cc, ccn = _evaluate(models, data, method, True)
    rel = sse.sum(1) / norm.sum()
    return ModelEvaluation(1.0 - rel, rel, sse, cc, ccn, core)
