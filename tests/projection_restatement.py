"""float64 NumPy restatement of parafac2_project, written from the definition and independent of matcouply_amd/projection.py:
minimise ||X - P Delta diag(a) C^T||_F^2 over a and P with P^T P = I by alternation,

* P = U V^T of the thin SVD of X C diag(a) Delta^T (the orthogonal Procrustes solution; over the singular values above 1e-6 of
  the largest, which is all of them unless K < r: X C has rank K then, and P^T P is a projector of rank K),
* a from numpy.linalg.lstsq on the Khatri-Rao design vec(X) ~ (C (.) P Delta) a,
* e2 = ||X - P Delta diag(a) C^T||^2 / ||X||^2, the residual itself,

stopping after iteration t when e2_t < absolute_tol, or t >= 2 and |e2_{t-1} - e2_t| <= tol e2_{t-1}, or t = n_iter_max.
Nothing here forms W = X C, G = W^T W or the r x r systems of the package.  The file also holds the fixture generator of the
projection tests."""
import numpy as np


def project_one(X, Delta, C, a0, n_iter_max=100, tol=1e-8, absolute_tol=1e-13):
    """-> dict(a, P, B, sse, nx, n_iter, errors [n_iter], criteria [n_iter]: |e2_{t-1} - e2_t| / e2_{t-1}, NaN at t = 1)"""
    X, Delta, C = (np.asarray(M, dtype=np.float64) for M in (X, Delta, C))
    a = np.array(a0, dtype=np.float64)
    J, K = X.shape
    nx = float(np.sum(X ** 2))
    errors, criteria = [], []
    for t in range(1, n_iter_max + 1):
        U, sv, Vt = np.linalg.svd(X @ C @ np.diag(a) @ Delta.T, full_matrices=False)
        keep = sv > 1e-6 * sv[0]  # all of them unless K < r: X C has rank K then, and P is the partial isometry on that range
        P = U[:, keep] @ Vt[keep]
        B = P @ Delta
        design = np.stack([np.outer(B[:, s], C[:, s]).ravel() for s in range(len(a))], 1)  # [J K, r]
        a = np.linalg.lstsq(design, X.ravel(), rcond=None)[0]
        e2 = float(np.sum((X - (B * a) @ C.T) ** 2)) / nx
        criteria.append(abs(errors[-1] - e2) / errors[-1] if errors else np.nan)
        errors.append(e2)
        if e2 < absolute_tol or (t >= 2 and abs(errors[-2] - e2) <= tol * errors[-2]):
            break
    return dict(a=a, P=P, B=B, sse=errors[-1] * nx, nx=nx, n_iter=len(errors), errors=np.array(errors), criteria=np.array(criteria))


def project(Xs, Delta, C, a0, **options):
    """every matrix on its own; a0 is [r] or [I, r]"""
    a0 = np.broadcast_to(np.asarray(a0, dtype=np.float64), (len(Xs), np.shape(C)[1]))
    return [project_one(X, Delta, C, a0[i], **options) for i, X in enumerate(Xs)]


def _f32(M):
    return M.astype(np.float32).astype(np.float64)


def _factor(rng, rows, rank, kappa):
    """[rows, rank] with its min(rows, rank) non-zero singular values between 1 and kappa"""
    m = min(rows, rank)
    U = np.linalg.qr(rng.standard_normal((rows, m)))[0]
    V = np.linalg.qr(rng.standard_normal((rank, m)))[0]
    return (U * np.linspace(1.0, kappa, m)) @ V.T


def fixture(seed, rows, K, rank, noise=0.3, kappa=2.0):
    """A fixed model and new matrices that follow it: Delta [r, r] and C [K, r] with singular values in [1, kappa],
    X_i = P*_i Delta diag(a*_i) C^T with orthonormal P*_i and a*_i in [0.5, 1.5], plus Gaussian noise of relative Frobenius norm
    `noise` (0: none, the recovery fixtures).  Delta, C and every X_i hold float32 values (as float64 arrays).
    -> dict(Delta, C, Xs, a_true [I, r], P_true)"""
    rng = np.random.RandomState(seed)
    Delta, C = _f32(_factor(rng, rank, rank, kappa)), _f32(_factor(rng, K, rank, kappa))
    a_true = rng.uniform(0.5, 1.5, (len(rows), rank))
    Xs, Ps = [], []
    for i, J in enumerate(rows):
        P = np.linalg.qr(rng.standard_normal((J, rank)))[0]
        X = (P @ Delta * a_true[i]) @ C.T
        if noise:
            E = rng.standard_normal(X.shape)
            X = X + noise * np.linalg.norm(X) / np.linalg.norm(E) * E
        Xs.append(_f32(X))
        Ps.append(P)
    return dict(Delta=Delta, C=C, Xs=Xs, a_true=a_true, P_true=Ps)


# the shapes of the parity tests: per rank one call with J_i at the segment edges of CP_SEG = 64 and the square P, and the K that
# take the vector path (K % 4 == 0) and the tail path below and above one 64-column block.  Five of the 40 (rank, K) pairs have
# K < rank: (16, 9), (17, 9), (17, 16), (32, 9), (32, 16).  There a is still determined (S is positive definite), but W = X C has
# rank K, Q loses r - K eigenvalues and P is a partial isometry.  The host serves them (tested against this file), the device
# refuses them (tested too): in the fp32 W the lost eigenvalues are rounding noise of about 1e-13 lam_max, a factor of ten
# below the 1e-12 cut, and one that slipped through would be inverted.
RANKS = (1, 2, 3, 8, 9, 16, 17, 32)


def rows_of(rank):
    return [rank, rank + 1, 63, 64, 65, 130]


def columns_of(rank, device=False):
    """the K of a rank; device=True: those the device serves (K >= rank)"""
    return sorted({K for K in (max(rank, 3), 9, 16, 33, 68) if K >= rank or not device})


def parity_fixture(rank, K, noise=0.3):
    return fixture(1000 * rank + K, rows_of(rank), K, rank, noise=noise)


# the stopping tests: one call (rank 3, K = 9) whose matrices stop at different iterations from a = 1, for two tolerances.  The
# seeds were searched for: at every matrix's stop the criterion |e2_{t-1} - e2_t| / e2_{t-1} is below 0.9 tol, one iteration
# earlier above 1.1 tol (the tests assert it), so the float32 rounding of W cannot move a stop, and no
# matrix is so close to singular that the package's route over G = W^T W and this file's route over the SVD part by 1e-9.
STOP_ROWS = [3, 4, 20, 63, 64, 65, 130, 40]
STOP_SEEDS = {1e-4: 11, 1e-5: 6}


def stopping_fixture(tol):
    return fixture(STOP_SEEDS[tol], STOP_ROWS, 9, 3, noise=0.3, kappa=4.0)
