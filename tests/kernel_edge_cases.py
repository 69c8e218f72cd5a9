"""Fixtures of the rank-bucket / load-path / boundary tests of the CP initialisers (csrc/alsinit.hip), parafac2_als
(csrc/parafac2als.hip) and the fused multi-start kernel (csrc/multistart.hip), and the fp64 checks that they are well posed.
Shared by the GPU tests (tests/test_gpu_als_init.py, tests/test_gpu_parafac2_als.py, tests/test_gpu_multistart.py) and their
CPU checks (tests/test_als_init_host.py, tests/test_parafac2_als_host.py, tests/test_multistart_host.py)."""
import numpy as np

from tests import als_restatement as R
from tests import parafac2_als_restatement as R2

NOISE = 0.2  # as in the GPU test files: e_t ~ 0.2

# ---- CP initialisers.  als_nb(rank): NB = 1 (rank <= 16), 2 (<= 32), 4 (<= 64) column blocks of 16 ------------------------------
ALS_CASES = {
    "r17": dict(I=24, J_range=(40, 120), K=80, rank=17, seed=0),  # NB = 2, last block partial
    "r32_rank_is_K": dict(I=24, J_range=(40, 120), K=32, rank=32, seed=5),  # NB = 2, full; rank == min(max J_i, K)
    "r33": dict(I=32, J_range=(64, 160), K=100, rank=33, seed=2),  # NB = 4, last block partial
    "r64": dict(I=40, J_range=(96, 200), K=128, rank=64, seed=4, noise=0.05),  # NB = 4, full
    "r16": dict(I=64, J_range=(64, 256), K=128, rank=16, seed=0),  # NB = 1 (the MID fixture of the GPU test file)
    # VEC = false: K % 4 != 0
    "k13": dict(I=10, J_range=(8, 40), K=13, rank=4, seed=4),
    "k130": dict(I=16, J_range=(40, 100), K=130, rank=20, seed=5),
    # ragged: one empty matrix, the ALS_SEG = 64 segment edges
    "ragged": dict(I=6, J=[64, 0, 65, 128, 129, 40], K=48, rank=6, seed=6),
}
ALS_START_CASES = ["r16", "r17", "r64"]  # n_iter_max = 0, one per NB bucket


def als_problem(name):
    p = dict(ALS_CASES[name])
    rank = p.pop("rank")
    I, J_range, K, seed = p.pop("I"), p.pop("J_range", None), p.pop("K"), p.pop("seed")
    p.setdefault("noise", NOISE)
    return R.cp_problem(I, J_range, K, rank, seed=seed, **p), rank


# ---- parafac2_als.  NB = 1 (RMAX = 16) for rank <= 16, NB = 2 (RMAX = 32) above ---------------------------------------------------
PF2_CASES = {
    "r17": dict(I=24, J_range=(32, 96), K=64, rank=17, seed=0),
    "r24": dict(I=24, J_range=(32, 96), K=64, rank=24, seed=1),
    "r32": dict(I=24, J_range=(32, 96), K=64, rank=32, seed=2),
    # VEC = false: K % 4 != 0
    "k37": dict(I=12, J_range=(16, 60), K=37, rank=8, seed=3),
    "k130": dict(I=12, J_range=(24, 80), K=130, rank=20, seed=4),
    # boundaries
    "j_is_rank": dict(I=8, J=[6, 20, 6, 33, 6, 12, 40, 6], K=24, rank=6, seed=5),
    "k_is_rank": dict(I=10, J_range=(20, 60), K=12, rank=12, seed=6),
    "seg_edges": dict(I=5, J=[64, 65, 128, 129, 63], K=40, rank=5, seed=7),
    "one_slab": dict(I=1, J=[90], K=30, rank=5, seed=8),
    "many_slabs": dict(I=1100, J_range=(4, 12), K=16, rank=4, seed=9),  # ngrp_ab = min(128, (I + 7) / 8) = 128
    "unaligned": dict(I=16, J_range=(30, 90), K=64, rank=20, seed=10),
}


def pf2_problem(name):
    p = dict(PF2_CASES[name])
    rank = p.pop("rank")
    I, J_range, K, seed = p.pop("I"), p.pop("J_range", None), p.pop("K"), p.pop("seed")
    return R2.parafac2_problem(I, J_range, K, rank, seed=seed, noise=NOISE, **p)[0], rank


# ---- fused multi-start: k_multistart<R, XL> for R = 1..16 ------------------------------------------------------------------------
MS_RANKS = list(range(1, 17))


def ms_problem(I, J_range, K, r, seed):
    """orc.synthetic_problem with ragged J_i drawn from J_range (a tuple) or given (a list) -> (mats (float64 views of the fp32
    data), X fp32, row_ptr)"""
    from oracle import aoadmm_oracle as orc

    rng = np.random.RandomState(seed)
    J = rng.randint(J_range[0], J_range[1] + 1, size=I) if not isinstance(J_range, list) else np.asarray(J_range)
    X, row_ptr = orc.synthetic_problem(I, J, K, r, seed=seed, dtype=np.float32)
    return [X[row_ptr[i]: row_ptr[i + 1]].astype(np.float64) for i in range(I)], X, row_ptr


MS_CASES = {
    # every rank: J_i >= 16 keeps PARAFAC2 served at rank 16
    **{f"r{r}": dict(I=6, J_range=(16, 24), K=20, r=r, seed=r) for r in MS_RANKS},
    "batches_r16": dict(I=40, J_range=(24, 32), K=20, r=16, seed=21),  # invert_systems: nb = 10 -> 4 batches
    "rows_reduce_r12": dict(I=8, J_range=(16, 30), K=24, r=12, seed=22),  # R * R = 144 > 128: one thread per entry
    "strides_r3": dict(I=300, J_range=(4, 9), K=10, r=3, seed=23),  # I > 256: the per-slab loops take a second stride
    "near_bound_r16": dict(I=64, J_range=(60, 68), K=60, r=16, seed=24),  # sum J_i * K close to 2^18
    "empty_r3": dict(I=6, J_range=[12, 0, 15, 9, 20, 11], K=10, r=3, seed=5),  # one empty matrix
}
# the stacks of tests/test_gpu_multistart.py.STACKS each case runs with there
MS_RUNS = {**{f"r{r}": ["parafac2_nn", "ridge_constant"] for r in MS_RANKS}, "batches_r16": ["parafac2_nn", "ridge_constant"],
           "rows_reduce_r12": ["nn_l1C"], "strides_r3": ["parafac2_nn", "box_l2ball"], "near_bound_r16": ["ridge_constant"],
           "empty_r3": ["ridge_constant", "box_l2ball"]}


# ---- well-posedness -------------------------------------------------------------------------------------------------------------
# A computed eigenvector v_k moves by about |dG| / min_j |lam_k - lam_j| under a perturbation dG of its Gram matrix.  Both sides
# form the Gram matrices in fp64 from the same fp32 data (|dG| ~ 1e-14 lam_1), and the device's subspace iteration stops when
# the Ritz values move by less than 1e-13 relative: the effective |dG| stays near 1e-12 lam_1.  A gap of GAP_MIN lam_1 between
# each of the leading rank + 1 eigenvalues and its neighbours therefore pins the start's vectors to 1e-6.  (The GPU tests of
# the start alone, test_gpu_als_init.py::test_start_alone, measure what this argument predicts.)
GAP_MIN = 1e-6
# the subspace iteration (rank + 8 vectors, at most 400 steps) converges at the rate (lam_{rank+9} / lam_rank)^2 per step: the
# rank-th eigenvalue must stand clear of the rest
TAIL_RATIO_MAX = 0.9
KAPPA_MAX = 1e6  # of the ALS normal equations (HALS divides by the diagonal G_qq only)


def gram_gaps(G, rank):
    """(min over k <= rank of the gap of lam_k to its neighbours among lam_1..lam_{rank+1}, / lam_1;  lam_{rank+9} / lam_rank)"""
    w = np.linalg.eigvalsh(G)[::-1]
    lead = w[: rank + 1]
    gaps = np.abs(np.diff(lead)) / w[0]
    tail = w[rank + 8] / w[rank - 1] if len(w) > rank + 8 else 0.0
    return float(gaps.min()) if len(gaps) else 1.0, float(tail)


def als_start_grams(mats):
    X, _ = R.padded_tensor(mats)
    return np.einsum("ijk,ijl->kl", X, X), np.matmul(X, X.transpose(0, 2, 1)).sum(0)


class StepRecorder:
    """wraps als_step / hals_step of a restatement module: the condition numbers of every normal-equation matrix G and whether
    the Cholesky factorisation of G (als_step's path) succeeded"""

    def __init__(self, monkeypatch, *modules):
        self.kappa, self.cholesky_failed = [], 0
        orig_als, orig_hals = R.als_step, R.hals_step

        def als(M, G):
            self._note(G)
            try:
                np.linalg.cholesky(G)
            except np.linalg.LinAlgError:
                self.cholesky_failed += 1
            return orig_als(M, G)

        def hals(F, M, G):
            self._note(G)
            return orig_hals(F, M, G)

        for m in modules:
            monkeypatch.setattr(m, "als_step", als)
            monkeypatch.setattr(m, "hals_step", hals)

    def _note(self, G):
        self.kappa.append(float(np.linalg.cond(G)))
