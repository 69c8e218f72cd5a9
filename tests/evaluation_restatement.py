"""Dense float64 restatement of the model scores of matcouply_amd/evaluation.py, written with
``np.linalg.pinv`` on B_i, C and A themselves: the pinv route, where the package goes through the Gram matrices.  Also the
problems the tests of the scores share."""
import numpy as np

RAGGED = lambda rank: [1, rank, 15, 16, 17, 63, 64, 65, 129]  # the block and segment edges and a one-row matrix


def split(B, rows):
    ptr = np.concatenate([[0], np.cumsum(rows)])
    return [B[ptr[i]: ptr[i + 1]] for i in range(len(rows))]


def tables(A, B_is, C, Xs):
    """(S [I, r, r], BtB [I, r, r], sse [I], norm [I]): S_i = B_i^T X_i C, sse_i = ||X_i - B_i diag(a_i) C^T||^2"""
    S = np.stack([B_i.T @ X @ C for B_i, X in zip(B_is, Xs)])
    BtB = np.stack([B_i.T @ B_i for B_i in B_is])
    sse = np.array([np.sum((X - (B_i * A[i]) @ C.T) ** 2) for i, (B_i, X) in enumerate(zip(B_is, Xs))])
    norm = np.array([np.sum(X ** 2) for X in Xs])
    return S, BtB, sse, norm


def core(A, B_is, C, Xs):
    """G[p, q, s] = sum_i (A^+)[p, i] (B_i^+ X_i (C^+)^T)[q, s]"""
    Cp = np.linalg.pinv(C)
    W = np.stack([np.linalg.pinv(B_i) @ X @ Cp.T for B_i, X in zip(B_is, Xs)])
    return np.einsum("pi,iqs->pqs", np.linalg.pinv(A), W)


def core_of_tables(A, C, S, BtB):
    """the same core from given tables: W_i = (B_i^T B_i)^+ S_i (C^T C)^+"""
    CtCp = np.linalg.pinv(C.T @ C)
    W = np.stack([np.linalg.pinv(BtB[i]) @ S[i] @ CtCp for i in range(len(S))])
    return np.einsum("pi,iqs->pqs", np.linalg.pinv(A), W)


def superdiagonal(r):
    T = np.zeros((r, r, r))
    T[np.arange(r), np.arange(r), np.arange(r)] = 1.0
    return T


def consistency(G, normalised=False):
    r = len(G)
    dev = np.sum((G - superdiagonal(r)) ** 2)
    return 100.0 * (1.0 - dev / (np.sum(G ** 2) if normalised else r))


def evaluate(cmf, Xs):
    """dict of every score of the model (weights, (A, B_is, C)) on the matrices Xs"""
    weights, (A, B_is, C) = cmf
    A = np.asarray(A, dtype=np.float64) * (1.0 if weights is None else np.asarray(weights, dtype=np.float64))
    B_is = [np.asarray(B_i, dtype=np.float64) for B_i in B_is]
    C = np.asarray(C, dtype=np.float64)
    Xs = [np.asarray(X, dtype=np.float64) for X in Xs]
    S, BtB, sse, norm = tables(A, B_is, C, Xs)
    G = core(A, B_is, C, Xs)
    rel = sse.sum() / norm.sum()
    return dict(S=S, BtB=BtB, slab_sse=sse, norm=norm, relative_sse=rel, fit=1.0 - rel, core=G,
                core_consistency=consistency(G), core_consistency_normalised=consistency(G, True))


def conditioned(rng, rows, rank, kappa):
    """rows x rank, singular values from 1 to kappa: orthonormal columns times a diagonal, times a rotation"""
    Q = np.linalg.qr(rng.standard_normal((rows, rank)))[0]
    V = np.linalg.qr(rng.standard_normal((rank, rank)))[0]
    return (Q * np.linspace(1.0, kappa, rank)) @ V


def orthonormal_times_diagonal(rng, rows, rank, lo=1.0, hi=3.0):
    return np.linalg.qr(rng.standard_normal((rows, rank)))[0] * rng.uniform(lo, hi, rank)


def random_problem(rng, rows, K, rank, noise=0.1, kappa=None, weights=False):
    """(cmf, Xs): a model and its data plus `noise` (relative, per matrix).  kappa: the condition number of A, every B_i and C
    (needs rows, K and len(rows) >= rank), else standard normal factors"""
    I = len(rows)
    make = (lambda n: conditioned(rng, n, rank, kappa)) if kappa else (lambda n: rng.standard_normal((n, rank)))
    A, B_is, C = make(I), [make(J) for J in rows], make(K)
    w = rng.uniform(0.5, 2.0, rank) if weights else None
    Xs = []
    for i, B_i in enumerate(B_is):
        M = (B_i * A[i] * (1.0 if w is None else w)) @ C.T
        E = rng.standard_normal(M.shape)
        Xs.append(M + noise * np.linalg.norm(M) / np.linalg.norm(E) * E)
    return (w, (A, B_is, C)), Xs


def known_core_problem(rng, rank, kind, deviation):
    """(cmf, Xs, G0): factors of condition number <= 3 (orthonormal columns times a diagonal in [1, 3]) and data generated from the
    core G0 = T + E, ||E||^2 = deviation * rank: X_i = B_i (sum_p A[i, p] G0[p]) C^T.  The least-squares core is G0 and the core
    consistency 100 (1 - deviation).  kind "cp": equal B_i; "parafac2": B_i = P_i Delta with orthonormal P_i."""
    I, J, K = rank + 2, rank + 5, rank + 3
    A = orthonormal_times_diagonal(rng, I, rank)
    C = orthonormal_times_diagonal(rng, K, rank)
    if kind == "cp":
        B_is = [orthonormal_times_diagonal(rng, J, rank)] * I
    else:
        Delta = orthonormal_times_diagonal(rng, rank, rank)
        B_is = [np.linalg.qr(rng.standard_normal((J + i, rank)))[0] @ Delta for i in range(I)]
    for F in [A, C] + B_is:
        assert np.linalg.cond(F) <= 3.0 + 1e-9
    E = rng.standard_normal((rank, rank, rank))
    G0 = superdiagonal(rank) + E * np.sqrt(deviation * rank) / np.linalg.norm(E)
    Xs = [B_i @ np.einsum("p,pqs->qs", A[i], G0) @ C.T for i, B_i in enumerate(B_is)]
    return (None, (A, B_is, C)), Xs, G0
