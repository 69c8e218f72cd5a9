"""Fit new matrices to a fixed PARAFAC2 model.

A fitted PARAFAC2 model describes every matrix as ``X_i ~ P_i Delta diag(a_i) C^T`` with orthonormal ``P_i``.  The model proper
is ``(Delta, C)``: Delta (r x r) and C (K x r) are shared by all matrices, ``a_i`` and ``P_i`` belong to matrix i.  For a new
matrix X (J x K, J >= r) :func:`parafac2_project` finds the ``a`` and the orthonormal ``P`` (J x r) that minimise
``||X - P Delta diag(a) C^T||_F^2``, by alternation from a start ``a^0``.  With ``W = X C``, ``G = W^T W``, ``H = C^T C`` and
``nx = ||X||_F^2``, iteration t = 1, 2, ...:

1. ``Q = Delta (a a^T o G) Delta^T``, symmetrised; ``Q^-1/2`` from its eigen-decomposition on the eigenvalues ``lam > 0`` and
   ``lam > 1e-12 lam_max``;
2. ``T = diag(a) Delta^T Q^-1/2`` and ``P = W T`` (the polar factor of ``X C diag(a) Delta^T``);
3. ``PtP = T^T G T`` (the identity unless eigenvalues were dropped);
4. ``S = (Delta^T PtP Delta) o H`` and ``d = diag(Delta^T T^T G)``;
5. ``a <- S^-1 d`` (the pseudo-inverse on the eigenvalues above 1e-12 of the largest when S is not positive definite);
6. ``e2_t = max(0, (nx - 2 a^T d + a^T S a) / nx)``, the relative squared residual of the new ``a`` with the ``P`` of step 2;

and the matrix stops after iteration t when ``e2_t < absolute_tol``, or t >= 2 and ``|e2_{t-1} - e2_t| <= tol e2_{t-1}``, or
``t = n_iter_max``: the rule of ``parafac2_als``, per matrix.  A converged ``parafac2_als`` fit is a fixed point of this map on
its own matrices.

Delta and C are taken in float32, as the engine holds its factors; the float32 value is the value used everywhere.
``method="host"`` is NumPy in float64.  ``method="device"`` forms W on the fp32 matrix core and runs the whole iteration of a
matrix inside one workgroup in float64 (csrc/projection.hip), thousands of matrices in one launch; for a matrix of few rows
(J r < 4 K), where nothing averages the float32 rounding of W out of ``e2``, that workgroup forms W again in float64.
"""
from collections import namedtuple

import numpy as np

from . import _engine
from ._utils import is_tensor, is_torch, to_numpy
from .coupled_matrices import CoupledMatrixFactorization
from .decomposition import _data_on_device
from .evaluation import _EIG_CUT, _Data, _check_method
from .similarity import _device_present

try:
    import torch
except ImportError:  # pragma: no cover
    torch = None

__all__ = ["parafac2_project", "Projection"]

Projection = namedtuple("Projection", ["cmf", "projections", "slab_sse", "slab_norm", "n_iter"])
ProjectionWithErrors = namedtuple("Projection", Projection._fields + ("errors",))

# method="auto" takes the host for fewer matrices than this when they are not on the device already.  From
# profiles/projection_rate.txt: the host loop costs 0.20 ms per matrix at 110 x 21, rank 2 and 0.30 ms at 64 x 64, rank 16; a
# device call from NumPy inputs costs 0.53 ms and 2.2 ms at 16 matrices (launches, the upload, the read-back of the model), so
# the two meet at about 3 and about 7 matrices; from 16 matrices on the device is 2 to 37 times faster
_AUTO_MIN_MATRICES = 8


def _f32(x):
    """float64 array holding the float32 values of x"""
    return np.ascontiguousarray(to_numpy(x).astype(np.float32).astype(np.float64))


def _upper_root(M, what):
    """the upper-triangular R with R^T R = M (float64 Cholesky); ValueError when M is not positive definite"""
    M = 0.5 * (M + M.T)
    try:
        if not np.isfinite(M).all():
            raise np.linalg.LinAlgError
        return np.linalg.cholesky(M).T
    except np.linalg.LinAlgError:
        raise ValueError(f"{what} is not positive definite: the model has no r x r blueprint Delta") from None


class _FixedModel:
    """(Delta [r, r], C [K, r], the default start [r] or None) of the three forms of `model`, float64 holding float32 values"""

    def __init__(self, model):
        weights = A = None
        if isinstance(model, CoupledMatrixFactorization):
            weights, (A, B, C) = model.weights, model.factors
        else:
            try:
                n = len(model)
                if n == 2 and is_tensor(model[0]) and is_tensor(model[1]):  # (blueprint, C)
                    B, C = model
                elif n in (2, 3) and len(model[1]) == 3:
                    weights, (A, B, C) = model[0], model[1]
                else:
                    raise TypeError
            except (TypeError, IndexError, KeyError):
                raise TypeError("model is what parafac2_als returns, a CoupledMatrixFactorization, (weights, (A, B_is, C)) or "
                                "(blueprint, C)") from None
        C = to_numpy(C).astype(np.float64)
        if C.ndim != 2:
            raise ValueError("shape mismatch: C of the model is not a matrix")
        r = int(C.shape[1])
        if is_tensor(B):
            B = to_numpy(B).astype(np.float64)
            if B.ndim != 2 or B.shape[1] != r or B.shape[0] < r:
                raise ValueError(f"shape mismatch: the blueprint of a rank-{r} model is [m, {r}] with m >= {r}, not {list(B.shape)}")
            if B.shape[0] == r:
                Delta = B
            elif A is not None:
                Delta = _upper_root(B.T @ B / max(len(to_numpy(A)), 1), "the mean of B_i^T B_i")  # the B_i stacked
            else:
                Delta = _upper_root(B.T @ B, "blueprint^T blueprint")
        else:
            B_is = [to_numpy(B_i).astype(np.float64) for B_i in B]
            if not B_is or any(B_i.ndim != 2 or B_i.shape[1] != r for B_i in B_is):
                raise ValueError(f"shape mismatch: every B_i of a rank-{r} model has {r} columns")
            Delta = _upper_root(sum(B_i.T @ B_i for B_i in B_is) / len(B_is), "the mean of B_i^T B_i")
        self.rank, self.K = r, int(C.shape[0])
        self.Delta, self.C = _f32(Delta), _f32(C)
        self.a0 = None
        if A is not None:
            A = to_numpy(A).astype(np.float64)
            if A.ndim != 2 or A.shape[1] != r:
                raise ValueError(f"shape mismatch: A of a rank-{r} model has {r} columns")
            if weights is not None:
                w = to_numpy(weights).astype(np.float64)
                if w.shape != (r,):
                    raise ValueError(f"shape mismatch: weights of shape {tuple(w.shape)} for a rank-{r} model")
                A = A * w
            self.a0 = A.mean(0)


def _start(a_init, model, I):
    """the start of every matrix [I, r], float64 holding float32 values"""
    r = model.rank
    if a_init is None:
        a0 = np.ones(r) if model.a0 is None else model.a0
    else:
        a0 = to_numpy(a_init).astype(np.float64)
        if a0.shape not in ((r,), (I, r)):
            raise ValueError(f"shape mismatch: a_init is [{r}] or [{I}, {r}], not {list(a0.shape)}")
    return _f32(np.broadcast_to(a0, (I, r)))


def _spd_inverse(S):
    """S^-1, or the pseudo-inverse on the eigenvalues above 1e-12 of the largest when S is not positive definite"""
    try:
        L = np.linalg.cholesky(S)
        Li = np.linalg.inv(L)
        return Li.T @ Li
    except np.linalg.LinAlgError:
        lam, V = np.linalg.eigh(0.5 * (S + S.T))
        keep = lam > _EIG_CUT * max(lam.max(), 0.0)
        return (V[:, keep] / lam[keep]) @ V[:, keep].T


def _host_matrix(X, Delta, C, a, n_iter_max, tol, absolute_tol, w_dtype=np.float64):
    """the iteration of the module docstring on one matrix in float64 (W rounded to `w_dtype` first: the device holds it in
    float32) -> (a, P, sse, nx, n_iter, [e2_1 ... e2_n_iter])"""
    W = (X @ C).astype(w_dtype).astype(np.float64)
    G, H, nx = W.T @ W, C.T @ C, float(np.sum(X ** 2))
    errors, prev = [], 0.0
    for t in range(1, n_iter_max + 1):
        Q = Delta @ (np.outer(a, a) * G) @ Delta.T
        lam, V = np.linalg.eigh(0.5 * (Q + Q.T))
        keep = (lam > 0.0) & (lam > _EIG_CUT * max(lam.max(), 0.0))
        T = a[:, None] * (Delta.T @ ((V[:, keep] / np.sqrt(lam[keep])) @ V[:, keep].T))
        GT = G @ T
        S = (Delta.T @ (T.T @ GT) @ Delta) * H
        d = np.sum(Delta * GT.T, 0)
        a = _spd_inverse(S) @ d
        e2 = max(0.0, nx - 2.0 * (a @ d) + a @ S @ a) / nx if nx > 0.0 else 0.0
        errors.append(e2)
        if e2 < absolute_tol or (t >= 2 and abs(prev - e2) <= tol * prev):
            break
        prev = e2
    return a, W @ T, errors[-1] * nx, nx, len(errors), errors


def _unserved_reason(model, data, start):
    """why the kernels cannot project these matrices (a sentence), or None.  Looks at shapes, types and host data only: no
    device call."""
    r = model.rank
    if not 1 <= r <= _engine.PROJECT_MAX_RANK:
        return f"rank {r} is outside 1 ... {_engine.PROJECT_MAX_RANK}"
    if int(data.rows.min()) < r:
        return f"a matrix has {int(data.rows.min())} rows, fewer than the rank {r}: it has no orthonormal P"
    if data.K < r:
        return (f"K = {data.K} is below the rank {r}: W = X C has rank K, the polar factor is a partial isometry, and the zero "
                "eigenvalues it rests on are not told from the float32 rounding of W with a safe margin")
    if data.N >= _engine.PROJECT_MAX_ROWS or data.K >= _engine.PROJECT_MAX_ROWS:
        return f"{data.N} packed rows or K = {data.K}: the kernels index with 32 bits (fewer than {_engine.PROJECT_MAX_ROWS} each)"
    bad = data.dtypes - {"float32", "float64", "bfloat16", "float16"}
    if bad:
        return f"the data holds {sorted(bad)[0]} matrices (float32, bfloat16 and float16 are read as they are, float64 is rounded to float32)"
    for name, t in (("Delta", model.Delta), ("C", model.C), ("a_init", start)):
        if not np.isfinite(t).all():
            return f"{name} holds a non-finite entry"
    return None


def _device_project(model, data, start, n_iter_max, tol, absolute_tol, return_errors):
    from .decomposition import _device, _pack as pack_data

    device = _device()
    X, row_ptr = pack_data(data.matrices, device)
    up = lambda t: torch.from_numpy(t).to(device)
    A, B, P, stats, n_iter, errors = _engine.pf2_project(X, row_ptr, model.rank, up(model.Delta), up(model.C), up(start), n_iter_max, tol,
                                                         absolute_tol, return_errors)
    stats = stats.cpu().numpy()
    return (A.cpu().numpy(), B.cpu().numpy(), P.cpu().numpy(), stats[:, 0].copy(), stats[:, 1].copy(), n_iter.cpu().numpy().astype(np.int64),
            errors.cpu().numpy() if return_errors else None)


def _host_project(model, data, start, n_iter_max, tol, absolute_tol, w_dtype=np.float64):
    I, r = data.I, model.rank
    A, B, P = np.empty((I, r)), np.empty((data.N, r)), np.empty((data.N, r))
    sse, nx, n_iter = np.empty(I), np.empty(I), np.empty(I, dtype=np.int64)
    errors = np.full((I, n_iter_max), np.nan)
    for i, X in enumerate(data.host()):
        if len(X) < r:
            raise ValueError(f"shape mismatch: matrix {i} has {len(X)} rows, fewer than the rank {r}: it has no orthonormal P")
        lo, hi = data.row_ptr[i], data.row_ptr[i + 1]
        A[i], P[lo:hi], sse[i], nx[i], n_iter[i], e = _host_matrix(X, model.Delta, model.C, start[i], n_iter_max, tol, absolute_tol, w_dtype)
        B[lo:hi] = P[lo:hi] @ model.Delta
        errors[i, :len(e)] = e
    return A, B, P, sse, nx, n_iter, errors


class _Like:
    """NumPy results in the array type, dtype and device of the caller's matrices (as decomposition._Out does for the fits)"""

    def __init__(self, matrices):
        from .decomposition import PackedMatrices

        first = matrices.X if isinstance(matrices, PackedMatrices) else matrices[0]
        self.torch_out, self.dtype = is_torch(first), first.dtype
        self.device = first.device if self.torch_out else None

    def __call__(self, t):
        if self.torch_out:
            return torch.from_numpy(np.ascontiguousarray(t)).to(device=self.device, dtype=self.dtype)
        return t.astype(self.dtype if np.issubdtype(self.dtype, np.floating) else np.float64)

    def split(self, t, row_ptr):
        full = self(t)
        return [full[row_ptr[i]: row_ptr[i + 1]] for i in range(len(row_ptr) - 1)]


def parafac2_project(matrices, model, *, a_init=None, n_iter_max=100, tol=1e-8, absolute_tol=1e-13, method="auto", return_errors=False):
    """The ``a`` and the orthonormal ``P`` that fit every new matrix best to a fixed PARAFAC2 model ``(Delta, C)``: the
    alternation of the module docstring, every matrix on its own and to its own stop.

    ``matrices``: a list of NumPy arrays or torch tensors (J_i x K, J_i >= rank) or a ``PackedMatrices``; float32, bfloat16 or
    float16 data is used as stored, float64 data is rounded to float32 by the device form.  ``model`` is one of

    * what ``parafac2_als`` returns, ``(weights, (A, B, C), projections)``: its rank x rank B is Delta;
    * a ``CoupledMatrixFactorization`` or ``(weights, (A, B_is, C))``, as ``parafac2_aoadmm`` returns: Delta is the upper-triangular
      R with ``R^T R = mean_i B_i^T B_i`` (``a`` and ``B_new`` do not depend on which square root is taken); ``ValueError`` when
      that mean is not positive definite;
    * a pair ``(blueprint, C)`` with ``blueprint`` [m, rank], m >= rank, reduced the same way when m > rank.

    ``a_init``: a vector [rank] for all matrices, an array [I_new, rank], or ``None``: the column means of the model's A with the
    weights folded in, ones when the model has no A.  The weights of a model are used for nothing else.

    Returns the named tuple ``Projection(cmf, projections, slab_sse, slab_norm, n_iter)``: ``cmf`` is
    ``CoupledMatrixFactorization((None, (A_new, B_is_new, C)))`` with ``B_is_new[i] = P_i Delta``, ``projections`` the ``P_i``,
    ``slab_sse[i] = e2 ||X_i||^2`` from the formula of step 6 (it carries the float32 rounding of W, about 1e-7 ||X_i||^2:
    :func:`~matcouply_amd.evaluation.slabwise_sse` of ``cmf`` gives the residual itself), ``slab_norm[i] = ||X_i||^2`` and
    ``n_iter`` the iterations every matrix took.  ``return_errors=True`` appends ``errors``: the ``e2`` sequences as a float64
    array [I_new, n_iter_max], NaN behind each matrix's stop.  Factors come in the array type and dtype of the matrices; the
    three score arrays are float64 (int64) NumPy arrays.

    ``method="host"`` is NumPy in float64 and serves every call; with ``K < rank`` the matrix ``W = X C`` has rank K only, the
    eigenvalue cut of step 1 drops ``rank - K`` directions, and the returned P is a partial isometry: ``P^T P`` is a projector of
    rank K, not the identity.  ``method="device"`` runs all matrices in one launch; it serves rank 1 ... 32, ``K >= rank``,
    matrices of at least rank rows, fewer than 2^26 packed rows and finite Delta, C and ``a_init``, and raises ``NotImplementedError`` with the
    reason otherwise, before the device is touched.  ``method="auto"`` takes the device when one is present and it serves the
    call, except for fewer than 8 matrices that are not on the device already (the host loop is then faster,
    ``profiles/projection_rate.txt``), else the host.  ``ValueError`` for shape mismatches, an unknown ``method``, ``n_iter_max < 1`` and negative
    tolerances."""
    _check_method(method)
    if isinstance(n_iter_max, bool) or not isinstance(n_iter_max, (int, np.integer)) or n_iter_max < 1:
        raise ValueError(f"n_iter_max must be a positive integer, not {n_iter_max!r}")
    tol = 0.0 if tol is None else float(tol)
    absolute_tol = 0.0 if absolute_tol is None else float(absolute_tol)
    if not tol >= 0.0 or not absolute_tol >= 0.0:
        raise ValueError(f"tol and absolute_tol must not be negative (tol {tol}, absolute_tol {absolute_tol})")
    fixed = _FixedModel(model)
    data = _Data(matrices)
    if data.K != fixed.K:
        raise ValueError(f"shape mismatch: the matrices have {data.K} columns, C of the model {fixed.K} rows")
    start = _start(a_init, fixed, data.I)
    out = None
    if method != "host":
        reason = _unserved_reason(fixed, data, start)
        if reason is None and method == "auto" and not (
                _device_present() and (data.I >= _AUTO_MIN_MATRICES or _data_on_device(data.matrices))):
            reason = f"no device is present, or fewer than {_AUTO_MIN_MATRICES} matrices on the host"  # "auto" only: the host serves it
        if reason is None:
            out = _device_project(fixed, data, start, int(n_iter_max), tol, absolute_tol, return_errors)
        elif method == "device":
            raise NotImplementedError(f'parafac2_project with method="device": {reason}')
    if out is None:
        out = _host_project(fixed, data, start, int(n_iter_max), tol, absolute_tol)
    A, B, P, sse, nx, n_iter, errors = out
    like = _Like(data.matrices)
    cmf = CoupledMatrixFactorization((None, (like(A), like.split(B, data.row_ptr), like(fixed.C))))
    result = (cmf, like.split(P, data.row_ptr), sse, nx, n_iter)
    return ProjectionWithErrors(*result, errors) if return_errors else Projection(*result)
