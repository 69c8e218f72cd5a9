"""fp64 NumPy restatement of parafac2_als (matcouply_amd/csrc/parafac2als.hip): TensorLy's unconstrained PARAFAC2-ALS with the
projections from the Gram route, ALS / one HALS pass per mode of the inner CP sweeps and the error without a third read of X.
Used by tests/test_gpu_parafac2_als.py and tests/test_parafac2_als_host.py."""
import numpy as np

from tests.als_restatement import als_step, hals_step, leading_eigenvectors


def inv_sqrt(G):
    """G^-1/2 on the eigenvalues above 1e-12 lam_max"""
    w, V = np.linalg.eigh(G)
    keep = (w > 0) & (w > 1e-12 * w.max())
    return (V[:, keep] / np.sqrt(w[keep])) @ V[:, keep].T


def start(mats, rank, init, random_state=None):
    I, K = len(mats), mats[0].shape[1]
    if init == "svd":
        C = leading_eigenvectors(sum(m.T @ m for m in mats), rank)
        return np.ones((I, rank)), np.eye(rank), C
    rs = random_state if isinstance(random_state, np.random.RandomState) else np.random.RandomState(random_state)
    return rs.uniform(size=(I, rank)), rs.uniform(size=(rank, rank)), rs.uniform(size=(K, rank))


def parafac2_als(matrices, rank, n_iter_max=2000, init="random", tol=1e-8, absolute_tol=1e-13, nn_modes=None, n_iter_parafac=5,
                 random_state=None, factors=None):
    """-> (A, B, C, [P_i], errors (e_t, not squared), e2 (squared errors)): the spec of mcl_parafac2_als in fp64.  `factors`: an
    explicit start (A, B, C)."""
    mats = [np.asarray(m, dtype=np.float64) for m in matrices]
    nn = set(nn_modes or ())
    A, B, C = factors if factors is not None else start(mats, rank, init, random_state)
    A, B, C = (np.array(F, dtype=np.float64) for F in (A, B, C))

    def step(mode, F, M, G):
        return hals_step(F, M, G) if mode in nn else als_step(M, G)

    nx2 = sum(float(np.sum(m * m)) for m in mats)
    errors, e2s, P = [], [], None
    for t in range(n_iter_max):
        W = [m @ C for m in mats]
        WtW = [w.T @ w for w in W]
        T = []
        for i in range(len(mats)):
            D = np.diag(A[i])
            G = B @ D @ WtW[i] @ D @ B.T
            T.append(D @ B.T @ inv_sqrt(0.5 * (G + G.T)))
        P = [w @ Ti for w, Ti in zip(W, T)]
        Y = np.stack([Ti.T @ (w.T @ m) for Ti, w, m in zip(T, W, mats)])  # [I, r, K]
        PtP = [Ti.T @ g @ Ti for Ti, g in zip(T, WtW)]
        for _ in range(n_iter_parafac):
            V = np.einsum("iqk,ks->iqs", Y, C)
            A = step(0, A, np.einsum("qs,iqs->is", B, V), (B.T @ B) * (C.T @ C))
            B = step(1, B, np.einsum("iqs,is->qs", V, A), (A.T @ A) * (C.T @ C))
            MC = np.einsum("iqk,qs,is->ks", Y, B, A)
            C = step(2, C, MC, (A.T @ A) * (B.T @ B))
        if tol:
            cross = float(np.sum(MC * C))
            CtC = C.T @ C
            fit = sum(float(np.sum((np.diag(A[i]) @ B.T @ PtP[i] @ B @ np.diag(A[i])) * CtC)) for i in range(len(mats)))
            e2 = max(0.0, nx2 - 2.0 * cross + fit) / nx2
            e2s.append(e2)
            errors.append(np.sqrt(e2))
            if t >= 1 and (abs(e2s[-2] - e2) <= tol * e2s[-2] or e2 < absolute_tol):
                break
    return A, B, C, P, np.array(errors), np.array(e2s)


def parafac2_problem(I, J_range, K, rank, seed, noise=0.1, nonneg=False, J=None):
    """X_i = P_i B diag(a_i) C^T + `noise` relative Gaussian noise, rounded to float32; P_i random orthonormal, A, C positive (or
    sparse non-negative with nonneg), B well conditioned.  `J`: explicit row counts (J_range unused).  -> (mats, (A, B, C, [P_i]))"""
    rng = np.random.RandomState(seed)
    J = rng.randint(J_range[0], J_range[1] + 1, size=I) if J is None else np.asarray(J, dtype=np.int64)
    A = rng.uniform(0.5, 1.5, size=(I, rank))
    B = np.eye(rank) + 0.3 * rng.uniform(size=(rank, rank))
    C = rng.uniform(0.0, 1.0, size=(K, rank))
    if nonneg:
        C *= rng.uniform(size=(K, rank)) < 0.5
    Ps, mats = [], []
    for i in range(I):
        Pi = np.linalg.qr(rng.standard_normal((J[i], rank)))[0]
        M = Pi @ B @ np.diag(A[i]) @ C.T
        E = rng.standard_normal(M.shape)
        mats.append((M + noise * np.linalg.norm(M) / np.linalg.norm(E) * E).astype(np.float32))
        Ps.append(Pi)
    return mats, (A, B, C, Ps)


def congruence(F, G):
    """mean over the matched components of |cos| between the columns of F and G (greedy matching)"""
    Fn = F / np.linalg.norm(F, axis=0)
    Gn = G / np.linalg.norm(G, axis=0)
    S = np.abs(Fn.T @ Gn)
    return S


def factor_match(est, true):
    """minimum over the components of the product of the congruences of A, C and the stacked B_i = P_i B, under the best
    permutation found greedily on the product"""
    (A, B, C, P), (At, Bt, Ct, Pt) = est, true
    Bs = np.concatenate([p @ B for p in P])
    Bst = np.concatenate([p @ Bt for p in Pt])
    S = congruence(A, At) * congruence(C, Ct) * congruence(Bs, Bst)
    r = S.shape[0]
    used, score = set(), []
    for a in np.argsort(-S.max(axis=1)):
        b = max((j for j in range(r) if j not in used), key=lambda j: S[a, j])
        used.add(b)
        score.append(S[a, b])
    return min(score)
