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


# ---- the software-pipelined chained B row pass (csrc/rowchain.hip) ------------------------------------------------------------
# k_rows_chain_{first,mid,last}<NBR, R64, SIG>: SIG = make_sig(n, class of each penalty) for the three stacks the parser builds in
# this order - 10 = PARAFAC2 + a row-separable kind, 106 = PARAFAC2 + L2 ball, 459 = PARAFAC2 + unimodality + L2 ball; (1, true)
# for rank 4..16 (fp64 row algebra, R64), (2, false) for rank 20..32 and (1, false) for rank <= 16 with MCL_NO_ROWS64=1.  Mode 1
# runs on 64-row tiles inside one slab (four to a workgroup), each a chain of up to four 16-row blocks.  Modes 0 and 2 carry NN
# and a small ridge, so that the X passes of the trajectory legs stay far from the 1e-5 bar.
PF2 = {"kind": "parafac2"}
_NN = {"kind": "nn"}
_L2 = {"kind": "l2ball", "norm_bound": 1.0}
_L2NN = {"kind": "l2ball", "norm_bound": 1.0, "non_negativity": True}
_UNI = {"kind": "unimodal"}
_UNINN = {"kind": "unimodal", "non_negativity": True}
ROWCHAIN_RIDGE = 1e-2
ROWCHAIN_CASES = {
    # R64 (rank <= 16).  Slabs shorter than one block; last tiles of 1, 15, 16, 17, 63 and 64 rows; 10 tiles (% 4 = 2)
    "pf2_l2_r4": dict(J=[4, 15, 16, 17, 64, 65, 129, 63, 128], K=48, rank=4, B=[PF2, _L2], inner=5, seed=0),
    "pf2_l1_r4": dict(J=[4, 9, 16, 65, 80], K=32, rank=4, B=[PF2, {"kind": "l1", "reg_strength": 0.05}], inner=2, seed=1),
    "pf2_uni_l2_r8": dict(J=[8, 15, 33, 64, 65, 200, 129], K=64, rank=8, B=[PF2, _UNINN, _L2], inner=2, seed=2),
    # more than 64 tiles: waves 64 apart share their sink slots
    "pf2_l2_many_r8": dict(J=("randint", 300, 8, 41), K=32, rank=8, B=[PF2, _L2], inner=5, seed=3),
    # a box that excludes 0: the padding rows of a partial block are not 0 after the prox (prox(0) = 0.05), so the row masks of
    # the statistics and of the stores matter
    "pf2_box_r12": dict(J=[12, 79, 80, 63, 128, 17], K=64, rank=12, B=[PF2, {"kind": "box", "min_val": 0.05, "max_val": 0.6}],
                        inner=2, seed=4),
    "pf2_uni_l2_r12": dict(J=[12, 40, 81, 127, 64], K=48, rank=12, B=[PF2, _UNI, _L2NN], inner=5, seed=5),
    # a slab of 18 tiles (more than 16): 23 tiles (% 4 = 3)
    "pf2_l2_r16": dict(J=[16, 31, 127, 1100, 48], K=96, rank=16, B=[PF2, _L2NN], inner=5, seed=6),
    "pf2_nn_r16": dict(J=[16, 100, 65, 200], K=64, rank=16, B=[PF2, _NN], inner=1, seed=7),
    # NB = 2 (rank 20..32), J_i >= 3 r; rank 20 and 28 leave the second column block partial (three or one of its four groups
    # on the sink)
    "pf2_l2_r20": dict(J=[60, 64, 65, 100, 129, 250], K=96, rank=20, B=[PF2, _L2], inner=1, seed=8),
    "pf2_nn_r24": dict(J=[72, 80, 150, 200], K=96, rank=24, B=[PF2, _NN], inner=5, seed=9, constant_B=True, l2B=0.05),
    "pf2_l1nn_r28": dict(J=[84, 127, 200, 145], K=96, rank=28, B=[PF2, {"kind": "l1", "reg_strength": 0.05, "non_negativity": True}],
                         inner=2, seed=10),
    "pf2_uni_l2_r20": dict(J=[60, 64, 129, 193], K=80, rank=20, B=[PF2, _UNINN, _L2NN], inner=5, seed=11),
    # 28 tiles (% 4 = 0), a slab of 18 tiles
    "pf2_uni_l2_r32": dict(J=[96, 130, 300, 1100], K=128, rank=32, B=[PF2, _UNI, _L2NN], inner=2, seed=12),
    "pf2_l2_r32": dict(J=[96, 191, 257], K=96, rank=32, B=[PF2, _L2NN], inner=5, seed=13),
}
# the fp32 NB = 1 forms <1, false, SIG>: rank <= 16 with MCL_NO_ROWS64=1 (one case per signature)
ROWCHAIN_NB1_CASES = ["pf2_l2_r16", "pf2_uni_l2_r8", "pf2_box_r12"]
# first + last in every inner iteration (MCL_NO_PASS_CHAIN=1): one case per signature x bucket, inner_n_iter_max >= 3
ROWCHAIN_NO_PASS_CHAIN_CASES = {"pf2_l2_r4": 5, "pf2_l2_r20": 3, "pf2_uni_l2_r12": 5, "pf2_uni_l2_r32": 3, "pf2_box_r12": 4,
                                "pf2_nn_r24": 5}
# two full outer iterations through the public call against the oracle (every signature x bucket)
ROWCHAIN_TRAJECTORY_CASES = ["pf2_l2_r4", "pf2_l2_r20", "pf2_uni_l2_r8", "pf2_uni_l2_r32", "pf2_box_r12", "pf2_l1nn_r28"]
# stacks and shapes the chain does not serve: the kernels of generic.hip (or checked_inner_loop) must take them
ROWCHAIN_OTHER_CASES = {
    "r6_not_multiple_of_4": dict(J=[18, 40, 65, 100], K=48, rank=6, B=[PF2, _L2], inner=3, seed=20),
    "pf2_l2_r36_nb4": dict(J=[108, 150, 200], K=96, rank=36, B=[PF2, _L2], inner=3, seed=21),
    "pf2_nn_l2_three_members": dict(J=[16, 40, 65, 129], K=48, rank=8, B=[PF2, _NN, _L2], inner=3, seed=22),
    "pf2_two_l2_balls": dict(J=[16, 40, 65, 129], K=48, rank=8, B=[PF2, _L2, {"kind": "l2ball", "norm_bound": 2.0}], inner=3,
                             seed=23),
    "uni_l2_without_pf2": dict(J=[16, 40, 65, 129], K=48, rank=8, B=[_UNINN, _L2], inner=3, seed=24),
    "pf2_l2_inner_tol": dict(J=[16, 40, 65, 129], K=48, rank=8, B=[PF2, _L2], inner=3, seed=25, inner_tol=1e-12),
}


def rowchain_case(name):
    return ROWCHAIN_CASES[name] if name in ROWCHAIN_CASES else ROWCHAIN_OTHER_CASES[name]


def rowchain_J(case):
    J = case["J"]
    if isinstance(J, tuple):  # ("randint", I, lo, hi)
        _, I, lo, hi = J
        return np.random.RandomState(case["seed"]).randint(lo, hi, size=I).astype(np.int64)
    return np.asarray(J, dtype=np.int64)


def rowchain_state(name):
    """orc.OracleState of a case (X rounded to fp32, as the engine stores it): uniform factors, aux and duals, P_i = eye"""
    from oracle import aoadmm_oracle as orc

    c = rowchain_case(name)
    J, r = rowchain_J(c), c["rank"]
    X, row_ptr = orc.synthetic_problem(len(J), J, c["K"], r, seed=c["seed"], dtype=np.float64)
    X = X.astype(np.float32).astype(np.float64)
    regs = [[_NN], [dict(d) for d in c["B"]], [_NN]]
    st = orc.random_state_for(X, row_ptr, r, regs, seed=c["seed"] + 100, l2=(ROWCHAIN_RIDGE, c.get("l2B", 0.0), ROWCHAIN_RIDGE),
                              inner_n_iter_max=c["inner"], constant_B=c.get("constant_B", False))
    if c.get("inner_tol"):
        st.inner_tol = c["inner_tol"]
    return st
