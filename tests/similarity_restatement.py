"""The factor match score restated in NumPy and SciPy for the similarity tests (the definition of DESIGN.md section 14; never the
package's own method="host"), a brute force over all permutations for small ranks, the margin by which an optimum is isolated,
and the seeded models the host and GPU tests share."""
import itertools

import numpy as np
from scipy.optimize import linear_sum_assignment


def match_matrix(cmf1, cmf2, consider_weights=True, skip_mode=None, absolute_value=True):
    sides = []
    for weights, (A, B, C) in (cmf1, cmf2):
        B = B if isinstance(B, np.ndarray) else np.concatenate([np.asarray(B_i) for B_i in B])
        F = [np.asarray(f, dtype=np.float64) for f in (A, B, C)]
        norms = [np.sqrt((f * f).sum(0)) for f in F]
        w = (1.0 if weights is None else np.asarray(weights, dtype=np.float64)) * norms[0] * norms[1] * norms[2]
        sides.append(([f / np.where(n == 0, 1.0, n) for f, n in zip(F, norms)], w))
    (F1, w1), (F2, w2) = sides
    M = np.ones((len(w1), len(w2)))
    for mode in range(3):
        if mode != skip_mode:
            M *= F1[mode].T @ F2[mode]
    if consider_weights:
        for p, q in itertools.product(range(len(w1)), range(len(w2))):
            M[p, q] *= 1.0 if w1[p] == 0 and w2[q] == 0 else 1.0 - abs(w1[p] - w2[q]) / max(w1[p], w2[q])
    return np.abs(M) if absolute_value else M


def fms(cmf1, cmf2, **options):
    """(score, permutation, M) with the optimal assignment of SciPy"""
    M = match_matrix(cmf1, cmf2, **options)
    rows, cols = linear_sum_assignment(-M)
    return M[rows, cols].mean(), cols, M


def brute_force(M):
    """(best score, its permutation, margin of the mean to the second best assignment) over all r! permutations (r <= 5)"""
    r = len(M)
    scored = sorted(((M[np.arange(r), list(p)].mean(), p) for p in itertools.permutations(range(r))), reverse=True)
    return scored[0][0], np.array(scored[0][1]), scored[0][0] - scored[1][0] if r > 1 else np.inf


def margin(M):
    """the optimum's mean minus the mean of the best OTHER assignment, exactly: the second best assignment lacks at least one
    edge of the best, so it is the best of the r problems with one of those edges forbidden"""
    r = len(M)
    rows, cols = linear_sum_assignment(-M)
    best, second = M[rows, cols].sum(), -np.inf
    for p in range(r):
        if r == 1:
            break
        N = M.copy()
        N[p, cols[p]] = -1e9
        rr, cc = linear_sum_assignment(-N)
        second = max(second, N[rr, cc].sum())
    return (best - second) / r


def score_of(M, perm):
    return M[np.arange(len(M)), np.asarray(perm)].mean()


def random_model(rng, rows, rank, weights=False, J=None):
    """a model of Gaussian factors as (weights, (A, B_is, C)); N = rows[1] split into rows[0] matrices B_i as evenly as it goes"""
    I, N, K = rows
    cuts = np.linspace(0, N, I + 1).astype(int)
    B = rng.standard_normal((N, rank))
    return (rng.uniform(0.5, 2.0, rank) if weights else None,
            (rng.standard_normal((I, rank)), [B[cuts[i]: cuts[i + 1]] for i in range(I)], rng.standard_normal((K, rank))))


def planted_model(rng, cmf, noise=1e-3):
    """`cmf` with its columns permuted, the sign of some columns flipped in two modes at once (their product keeps its sign) and
    relative noise on every entry -> (model, the permutation p with model[:, k] ~ cmf[:, p[k]])"""
    weights, (A, B_is, C) = cmf
    rank = A.shape[1]
    p = rng.permutation(rank)
    sign = rng.choice([-1.0, 1.0], rank)
    jig = lambda F: F * (1.0 + noise * rng.standard_normal(F.shape))
    return (None if weights is None else weights[p], (jig(A[:, p]) * sign, [jig(B_i[:, p]) for B_i in B_is], jig(C[:, p]) * sign)), p


# the shapes of the parity tests: a mode shorter than one group of four rows, tails of 1, 2 and 3 rows, exact multiples
ROWS = [(1, 4, 2), (3, 7, 5), (10, 150, 20), (16, 64, 32)]
RANKS = [1, 3, 4, 5, 8, 9, 16]
OPTION_CASES = [(4, (3, 7, 5)), (9, (10, 150, 20))]  # (rank, rows) at which every option is tried


def parity_pair(rank, rows, seed=0):
    """the two models of a parity case: independent Gaussian models (the assignment is a real problem, not a planted one); at
    rank 16 model 2 is a planted permutation of model 1"""
    rng = np.random.RandomState(1000 * rank + 10 * ROWS.index(tuple(rows)) + seed)
    one = random_model(rng, rows, rank, weights=True)
    two = planted_model(rng, one)[0] if rank == 16 else random_model(rng, rows, rank, weights=True)
    return one, two
