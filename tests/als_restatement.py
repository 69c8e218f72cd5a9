"""fp64 NumPy restatement of the CP initialisers init="parafac_als" / "parafac_hals" (matcouply_amd/csrc/alsinit.hip): CP-ALS and
CP-HALS on the zero-padded tensor with the deterministic start of the device form.  Used by tests/test_gpu_als_init.py."""
import numpy as np


def signed_columns(V):
    """every column multiplied by the sign of its entry of largest magnitude (the first one on ties)"""
    idx = np.argmax(np.abs(V), axis=0)
    s = np.sign(V[idx, np.arange(V.shape[1])])
    s[s == 0] = 1.0
    return V * s


def leading_eigenvectors(G, rank):
    w, V = np.linalg.eigh(G)
    return signed_columns(V[:, ::-1][:, :rank])


def padded_tensor(matrices):
    mats = [np.asarray(m, dtype=np.float64) for m in matrices]
    J = [m.shape[0] for m in mats]
    X = np.zeros((len(mats), max(J), mats[0].shape[1]))
    for i, m in enumerate(mats):
        X[i, : J[i]] = m
    return X, J


def als_step(M, G):
    """M G^-1; the pseudo-inverse (eigenvalues <= 1e-12 lam_max dropped) when G is not positive definite"""
    try:
        L = np.linalg.cholesky(G)
    except np.linalg.LinAlgError:
        w, V = np.linalg.eigh(G)
        keep = w > 1e-12 * w.max()
        return M @ ((V[:, keep] / w[keep]) @ V[:, keep].T)
    return np.linalg.solve(L.T, np.linalg.solve(L, M.T)).T


def hals_step(F, M, G):
    F = F.copy()
    for q in range(F.shape[1]):
        if G[q, q] == 0:
            continue
        F[:, q] = np.maximum(0.0, F[:, q] + (M[:, q] - F @ G[:, q]) / G[q, q])
    return F


def cp_start(matrices, rank, hals):
    X, J = padded_tensor(matrices)
    C = leading_eigenvectors(np.einsum("ijk,ijl->kl", X, X), rank)
    B = leading_eigenvectors(np.matmul(X, X.transpose(0, 2, 1)).sum(0), rank)
    if hals:
        B, C = np.maximum(B, 0.0), np.maximum(C, 0.0)
    return np.ones((len(J), rank)), B, C


def cp_init(matrices, rank, hals=False, n_iter_max=50, tol=None):
    """-> (A, [B[:J_i]], C, errors): the spec of mcl_als_init in fp64"""
    if tol is None:
        tol = 1e-7 if hals else 1e-8
    X, J = padded_tensor(matrices)
    A, B, C = cp_start(matrices, rank, hals)
    step = (lambda F, M, G: hals_step(F, M, G)) if hals else (lambda F, M, G: als_step(M, G))
    nx2 = float(np.sum(X * X))
    errors = []
    for t in range(n_iter_max):
        XC = X @ C
        A = step(A, np.einsum("ijr,jr->ir", XC, B), (B.T @ B) * (C.T @ C))
        B = step(B, np.einsum("ijr,ir->jr", XC, A), (A.T @ A) * (C.T @ C))
        MC = sum(X[i].T @ (B * A[i]) for i in range(len(J)))
        C = step(C, MC, (A.T @ A) * (B.T @ B))
        fit = np.sum((A.T @ A) * (B.T @ B) * (C.T @ C))
        errors.append(np.sqrt(max(0.0, nx2 - 2.0 * np.sum(MC * C) + fit)) / np.sqrt(nx2))
        if t >= 1 and abs(errors[-2] - errors[-1]) < tol:
            break
    return A, [B[:j] for j in J], C, np.array(errors)


def cp_problem(I, J_range, K, rank, seed, noise=0.01, J=None):
    """X_i = X~_i[:J_i] for a padded tensor X~ = CP(A, B, C) + `noise` relative Gaussian noise on the stored rows, rounded to float32.
    Component q has B[:, q] supported on the rows below L_q and a_i[q] = 0 for the slabs shorter than L_q, so the zero padding
    is part of the low-rank model; sparse non-negative factors with decaying weights: a clear gap behind the rank-th eigenvalue
    of both Gram matrices of the start and well-conditioned normal equations.  `J`: explicit row counts (J_range unused; a 0 is
    an empty matrix)."""
    rng = np.random.RandomState(seed)
    J = rng.randint(J_range[0], J_range[1] + 1, size=I) if J is None else np.asarray(J, dtype=np.int64)
    Js = np.sort(J[J > 0])  # (an empty matrix carries no component)
    L = Js[(np.arange(rank) * I) // (2 * rank)]  # every component is active on at least half of the slabs
    w = np.linspace(1.0, 0.5, rank)
    A = rng.uniform(0.5, 1.0, size=(I, rank)) * w * (J[:, None] >= L[None, :])
    B = rng.uniform(0.5, 1.0, size=(J.max(), rank)) * (rng.uniform(size=(J.max(), rank)) < 0.3)
    B *= np.arange(J.max())[:, None] < L[None, :]
    C = rng.uniform(0.5, 1.0, size=(K, rank)) * (rng.uniform(size=(K, rank)) < 0.3)
    mats = []
    for i in range(I):
        M = (B[: J[i]] * A[i]) @ C.T
        E = rng.standard_normal(M.shape)
        mats.append((M + noise * np.linalg.norm(M) / max(np.linalg.norm(E), 1e-300) * E).astype(np.float32))
    return mats
