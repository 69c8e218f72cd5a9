"""Fixtures of the rank-bucket / load-path / boundary tests of the CP initialisers (csrc/alsinit.hip), parafac2_als
(csrc/parafac2als.hip) and the fused multi-start kernel (csrc/multistart.hip), and the fp64 checks that they are well posed.
Shared by the GPU tests (tests/test_gpu_als_init.py, tests/test_gpu_parafac2_als.py, tests/test_gpu_multistart.py) and their
CPU checks (tests/test_als_init_host.py, tests/test_parafac2_als_host.py, tests/test_multistart_host.py)."""
import functools
import zlib

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
# stacks and shapes the chain does not serve: the kernels of rows.hip (or checked_inner_loop) must take them
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


# ---- the two passes over X: X C and [G | R] (csrc/contract.hip, csrc/xclds.hip; tests/test_gpu_contract.py) -----------------------
# A case: J (rows per slab), K, rank, env (the MCL_* switches it sets), unaligned (X starts one element past a 16-byte boundary:
# VEC = 1 although K % 4 = 0; fp32 only - a 16-bit X must be 8-byte aligned), A: the penalties of mode 0 - "nn" ([nn]: the fused
# reductions in fp32 chains, GRAM = 1), "ridge" ([] with a ridge: fp64, GRAM = 2) or "both" (two runs), nt (a second run with
# MCL_X_NT_MB=1: the non-temporal forms; needs N K 4 > 1 MiB), f32_only (the depth-8 LDS ring has no 16-bit twin), legB (the
# real-valued leg runs it), twins (switch overlays whose results must equal the case's own bit for bit on the real-valued data;
# None removes a switch).  Small problems get one 16-row block per wave from the planner; MCL_XC_WAVES=n (W below) makes waves of
# many blocks, segments of up to 256 rows and waves of several segments.
_JP8 = [0, 1, 15, 16, 17, 255, 256, 257]      # every slab length next to a block / segment edge; 817 rows, 54 blocks
_JR7 = [300, 64, 41, 257, 0, 130, 400]        # 1192 rows: K >= 256 is more than 1 MiB
_JW = [600, 40]                               # one slab spread over several waves
_JBIG = [2100, 1500, 700, 130]                # 4430 rows: more than 1 MiB from K = 60 on
_J1 = [1100]                                  # a single slab
CONTRACT_RIDGE = 0.5


def _cc(J, K, rank, A="nn", W=0, unaligned=False, nt=False, legB=False, f32_only=False, twins=(), **env):
    e = {k: str(v) for k, v in env.items()}
    if W:
        e["MCL_XC_WAVES"] = str(W)
    e.setdefault("MCL_EXACT", "0")  # the size-independent kernels, however small the case (tests/conftest.py: fast_kernels)
    return dict(J=list(J), K=K, rank=rank, A=A, env=e, unaligned=unaligned, nt=nt, legB=legB, f32_only=f32_only, twins=list(twins))


_NT = {"MCL_X_NT_MB": "1"}
CONTRACT_CASES = {
    # k_contract_xc<NB, VEC, KCT>: K that is no multiple of 256, an unaligned X, or MCL_XC_NOROW
    "xc_nb1_kct2_k100": _cc(_JP8, 100, 1, W=3),
    "xc_nb1_kct2_k90": _cc(_JP8, 90, 3, A="ridge"),
    "xc_nb1_kct2_k33": _cc(_JP8, 33, 3),
    "xc_nb1_kct2_k128_unaligned": _cc(_JR7, 128, 5, W=5, unaligned=True),
    "xc_nb1_kct4_k200": _cc(_JR7, 200, 12, A="ridge", W=2),
    "xc_nb1_kct4_k250": _cc(_JP8, 250, 16),
    "xc_nb1_kct4_k256_unaligned": _cc(_JP8, 256, 16, unaligned=True),
    "xc_nb1_kct4_k256_norow": _cc(_JP8, 256, 5, W=3, MCL_XC_NOROW=1),
    "xc_nb1_kct0_k300": _cc(_JP8, 300, 16, W=3, legB=True),  # 5 chunks padded to 8; two slices of k_contract_xt, the second short
    "xc_nb1_kct0_k301": _cc(_JR7, 301, 5),
    "xc_nb1_kct0_k512_unaligned": _cc(_JP8, 512, 12, unaligned=True),
    "xc_nb2_kct2_k100": _cc(_JP8, 100, 17, W=3, legB=True),
    "xc_nb2_kct2_k66": _cc(_JR7, 66, 20),
    "xc_nb2_kct2_k62": _cc(_JP8, 62, 17),
    "xc_nb2_kct2_k64_unaligned": _cc(_JP8, 64, 32, unaligned=True),
    "xc_nb2_kct0_k200": _cc(_JP8, 200, 32, A="ridge"),
    "xc_nb2_kct0_k130": _cc(_JP8, 130, 20, W=6),
    "xc_nb2_kct0_k256_unaligned": _cc(_JR7, 256, 17, unaligned=True),
    "xc_nb4_k100": _cc(_JP8, 100, 33, W=3, legB=True),
    "xc_nb4_k70": _cc(_JR7, 70, 40, A="ridge"),
    "xc_nb4_k128_unaligned": _cc(_JP8, 128, 64, unaligned=True),
    # a sweep-eligible shape whose fragment image of C is longer when the sweep is planned (4 chunks against 2)
    "xc_sweep_k128_r20": _cc([300, 257, 130], 128, 20, W=2, legB=True, twins=[{"MCL_NO_SWEEP": "1"}]),
    "xc_nosweep_k128_r20": _cc([300, 257, 130], 128, 20, W=2, MCL_NO_SWEEP=1),
    # k_contract_xt at K <= 128 (KB = 1, 2 and NB = 2 at KB = 1), default planner: 279 waves, 70 row ranges (XCD-padded to 72)
    "xt_kb1_nb1_k60": _cc(_JBIG, 60, 5, nt=True),
    "xt_kb1_nb1_k60_depth2": _cc(_JBIG, 60, 5, nt=True, MCL_XT_DEPTH=2),
    "xt_kb2_nb1_k100": _cc(_JBIG, 100, 12, nt=True, legB=True, twins=[{"MCL_XT_DEPTH": "2"}]),
    "xt_kb2_nb1_k100_depth2": _cc(_JBIG, 100, 12, nt=True, MCL_XT_DEPTH=2),
    "xt_kb1_nb2_k64": _cc(_JBIG, 64, 20, nt=True, W=9),
    "xt_kb1_nb2_k64_depth2": _cc(_JBIG, 64, 20, nt=True, MCL_XT_DEPTH=2),
    "xt_kb4_nb1_k300_depth2": _cc(_JR7, 300, 16, nt=True, W=5, MCL_XT_DEPTH=2),
    # k_contract_xc_256<GRAM> (K = 256, rank <= 16) and its one-slot twin k_contract_xc_row<1, true, GRAM>.  Their sums run in
    # different orders BY DESIGN (eight fp32 chains added as a tree in fp64 against four added pairwise in fp32): no bitwise pair
    "xc256_r16": _cc(_JR7, 256, 16, A="both", W=5, nt=True, legB=True),
    "xc256_r1_default_waves": _cc(_JP8, 256, 1),
    "xc256_single_slab": _cc(_J1, 256, 16, W=7),
    "xcrow_creg_r12": _cc(_JR7, 256, 12, A="both", W=3, nt=True, legB=True, MCL_XC_DEPTH1=1),
    # k_contract_xc_row<NB, false, GRAM>
    "xcrow_nb2_k256": _cc(_JR7, 256, 17, A="both", W=4, nt=True),
    "xcrow_nb4_k256": _cc(_JR7, 256, 40, A="both", W=6, nt=True),
    "xcrow_nb1_k768": _cc(_JP8, 768, 5, A="both", W=3, nt=True, legB=True),
    "xcrow_nb1_k768_seg32": _cc(_JP8, 768, 12, W=3, MCL_SEG_ROWS=32),
    "xcrow_nb2_k768": _cc(_JP8, 768, 20, A="both", W=2, nt=True, legB=True, MCL_XT_DEPTH=2),
    "xcrow_nb4_k768": _cc(_JP8, 768, 48, A="both", W=1, nt=True),
    "xcrow_nb2_k1536": _cc(_JW, 1536, 32, A="both", W=4, nt=True),
    "xcrow_nb4_k512": _cc(_JP8, 512, 64, A="both", W=3, nt=True, legB=True, MCL_XT_DEPTH=2),
    "xcrow_nb1_k1024_no_lds": _cc(_JP8, 1024, 16, A="both", W=3, nt=True, MCL_NO_XC_LDS=1),
    # k_contract_xc_lds<NB, GRAM, XNT, DEPTH>: 1 .. 4 rounds of the depth-4 ring; depth 8 where K % 1024 = 0, else back to 4
    "xclds_nb1_k512": _cc(_JP8, 512, 16, A="both", W=3, nt=True, legB=True, twins=[{"MCL_XC_LDS_DEPTH": "8"}]),
    "xclds_nb1_k512_depth8_falls_back": _cc(_JP8, 512, 16, W=3, MCL_XC_LDS_DEPTH=8),
    "xclds_nb1_k1024": _cc(_JP8, 1024, 12, A="both", W=3, nt=True, legB=True, twins=[{"MCL_XC_LDS_DEPTH": "8"}]),
    "xclds_nb1_k1024_depth8": _cc(_JP8, 1024, 12, A="both", W=3, nt=True, f32_only=True, MCL_XC_LDS_DEPTH=8),
    "xclds_nb1_k1536": _cc(_JW, 1536, 3, A="both", W=4, nt=True),
    "xclds_nb1_k1536_depth8_falls_back": _cc(_JW, 1536, 3, W=4, MCL_XC_LDS_DEPTH=8),
    "xclds_nb1_k2048": _cc(_JW, 2048, 16, A="both", W=2, nt=True),
    "xclds_nb1_k2048_depth8": _cc(_JW, 2048, 16, A="both", W=2, nt=True, f32_only=True, MCL_XC_LDS_DEPTH=8),
    "xclds_nb2_k512": _cc(_JP8, 512, 20, A="both", W=5, nt=True),
    "xclds_nb2_k1024": _cc(_JP8, 1024, 32, A="both", W=3, nt=True, legB=True, twins=[{"MCL_XC_LDS_DEPTH": "8"}]),
    "xclds_nb2_k1024_depth8": _cc(_JP8, 1024, 32, A="both", W=3, nt=True, f32_only=True, MCL_XC_LDS_DEPTH=8),
    # the exact-products forms (MCL_EXACT=1): 1, 2, 8 and 9 chunks of 256 rows; N % 256 = 255, 1, 0, 1; K % 16 != 0
    "exact_nb1_n255": _cc([100, 0, 155], 40, 5, legB=True, MCL_EXACT=1),
    "exact_nb2_n257": _cc([256, 1], 24, 20, A="ridge", legB=True, MCL_EXACT=1),
    "exact_nb4_n2048": _cc([1000, 1048], 20, 40, legB=True, MCL_EXACT=1),
    "exact_nb1_n2049": _cc([1024, 1000, 25], 33, 16, A="ridge", MCL_EXACT=1),
}

# Built instantiations no dispatch can choose (kept: profiles/kernel_resources.json pins the kernel list).  Patterns over the names
# tools/kernel_resources.py prints, `_h<TYPE, ` twins included; tests/test_contract_cases.py proves none is ever predicted.
CONTRACT_UNREACHABLE = {
    r"k_contract_xc(_h)?<(\w+, )?2, [14], 4>": "mcl_xc_chunks: at NB = 2 only two chunks of C fragments fit the registers (KCT = 2 or 0)",
    r"k_contract_xc(_h)?<(\w+, )?4, [14], [24]>": "mcl_xc_chunks: at NB = 4 not even two chunks fit (KCT = 0 always)",
    r"k_contract_xt(_h)?<(\w+, )?[124], [124], 1, 2, [012], true>": "launch_xt: the non-temporal load is the vector load (VEC = 4 only)",
    r"k_contract_xt(_h)?<(\w+, )?1, 4, 1, 2, 2, true>": "launch_xt: the G-only launch (MODE = 2) does not read X",
}


def contract_runs():
    """[(run name, case name, switches, 'nn' | 'ridge')]: every case, with A = both and nt expanded"""
    out = []
    for n, c in CONTRACT_CASES.items():
        for a in (("nn", "ridge") if c["A"] == "both" else (c["A"],)):
            for nt in ((False, True) if c["nt"] else (False,)):
                out.append((n + ("/" + a if c["A"] == "both" else "") + ("/nt" if nt else ""), n, {**c["env"], **(_NT if nt else {})}, a))
    return out


def contract_x_types(case):
    return ("f32",) if case["unaligned"] or case["f32_only"] else ("f32", "bf16", "f16")


def contract_int_ranges(case):
    """(xm, cm, bm, am): integer magnitudes of X, C, B, A - as large as keeps every sum of absolute products of the case below 2^24
    by its worst case (and |x| <= 256: exact in bf16).  The conditions themselves are asserted on the data, not on this rule."""
    J, K = case["J"], case["K"]
    N, Jm = sum(J), max(J)
    m, cap = [1, 1, 1, 1], [256, 16, 16, 4]

    def ok(xm, cm, bm, am):
        return max(K * xm * cm, N * xm * bm * am, N * (bm * am) ** 2, Jm * bm * K * xm * cm, Jm * bm * bm * K * cm * cm) < 2 ** 24

    grown = True
    while grown:
        grown = False
        for k in range(4):
            t = list(m)
            t[k] *= 2
            if t[k] <= cap[k] and ok(*t):
                m, grown = t, True
    return tuple(m)


@functools.lru_cache(maxsize=None)
def contract_data(name, kind):
    """X [N, K], A [I, r], B [N, r], C [K, r] as float64 arrays of fp32-representable values, and row_ptr.  kind 'int': small random
    integers (contract_int_ranges); 'real': normal X and B, uniform A in [0.5, 1.5) and C in [-1, 1), rounded to fp32"""
    c = CONTRACT_CASES[name]
    J, K, r = c["J"], c["K"], c["rank"]
    N, I = sum(J), len(J)
    rng = np.random.RandomState(zlib.crc32(name.encode()) % (2 ** 31))
    if kind == "int":
        xm, cm, bm, am = contract_int_ranges(c)
        f = lambda m, *s: rng.randint(-m, m + 1, size=s).astype(np.float64)
        X, C, B, A = f(xm, N, K), f(cm, K, r), f(bm, N, r), f(am, I, r)
    else:
        f32 = lambda a: a.astype(np.float32).astype(np.float64)
        X, C, B, A = f32(rng.standard_normal((N, K))), f32(rng.uniform(-1, 1, (K, r))), f32(rng.standard_normal((N, r))), f32(rng.uniform(0.5, 1.5, (I, r)))
    return dict(X=X, A=A, B=B, C=C, row_ptr=np.concatenate([[0], np.cumsum(J)]).astype(np.int64))


@functools.lru_cache(maxsize=None)
def contract_reference(name, kind):
    """fp64 NumPy reference of every by-product (exact on the integer data: every value is an integer far below 2^53), and the
    sums of absolute products the bounds of both legs are stated in (suffix _abs)"""
    d = contract_data(name, kind)
    X, A, B, C, rp = d["X"], d["A"], d["B"], d["C"], d["row_ptr"]
    I, r = A.shape
    slab = np.repeat(np.arange(I), np.diff(rp))
    Ba = B * A[slab]
    out = dict(XC=X @ C, XC_abs=np.abs(X) @ np.abs(C), G=Ba.T @ Ba, G_abs=np.abs(Ba).T @ np.abs(Ba), R=X.T @ Ba, R_abs=np.abs(X).T @ np.abs(Ba))
    seg = lambda M: np.stack([M[rp[i]:rp[i + 1]].sum(axis=0) for i in range(I)]) if I else np.zeros((0,) + M.shape[1:])
    out["rhs"], out["rhs_abs"] = seg(B * out["XC"]), seg(np.abs(B) * out["XC_abs"])
    CtC, CtC_abs = C.T @ C, np.abs(C).T @ np.abs(C)
    out["Q"] = seg(B[:, :, None] * B[:, None, :]) * CtC
    out["Q_abs"] = seg(np.abs(B)[:, :, None] * np.abs(B)[:, None, :]) * CtC_abs
    return out
