"""GPU: cmf_aoadmm_resample / parafac2_aoadmm_resample with the fused kernel k_multistart_weighted (csrc/multistart.hip,
DESIGN.md section 18) against the fp64 NumPy restatement of the weighted AO-ADMM run (tests/weighted_aoadmm_restatement.py),
from each job's exact start: parity per job, every rank, the kernel's edges, exact zeros for zero-weight matrices, the unweighted
kernel's bits with all weights 1, bitwise independence of the batch, 16-bit X, the default stopping rule, resources and rate."""
import os
import sys
import time

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from matcouply_amd import decomposition as dec  # noqa: E402
from matcouply_amd import resampling as rs  # noqa: E402
from oracle import aoadmm_oracle as orc  # noqa: E402
from tests import kernel_edge_cases as E  # noqa: E402
from tests import weighted_aoadmm_restatement as W  # noqa: E402

pytestmark = pytest.mark.gpu

# the bars of tests/test_gpu_multistart.py::test_oracle_parity_per_start: the added arithmetic is one multiply
BAR = 1e-5

STACKS = {
    "nn_l1C": dict(non_negative={0: True, 1: True}, l1_penalty={2: 0.05}),
    "box_l2ball": dict(lower_bound={1: -0.5}, upper_bound={1: 2.0}, l2_norm_bound={0: 3.0, 2: 2.0},
                       constant_feasibility_penalty=True),
    "parafac2_nn": dict(parafac2=True, non_negative=True),
    "ridge_constant": dict(l2_penalty=[0.1, 0.2, 0.05], non_negative={2: True}, constant_feasibility_penalty=True),
    "l1_on_A": dict(l1_penalty={0: 0.05}, non_negative={1: True}),
    "box_B_positive_lower": dict(lower_bound={1: 0.1}, upper_bound={1: 2.0}, non_negative={0: True}),
}
# weights from {0, 0.5, 1, 2, 3}, a zero first and a zero last, one row per job
PARITY_WEIGHTS = np.array([[0, 1, 2, 0.5, 3, 1], [1, 0.5, 0, 3, 2, 0], [0, 2, 1, 1, 0.5, 0], [3, 0, 0.5, 2, 1, 1]], dtype=np.float64)
# start seeds per job: kept only where a one-ulp move of the start changes the restatement's own result by less than a fifth of
# the bar (checked on the CPU; the replaced seeds are listed in DESIGN.md section 18)
# and, under PARAFAC2, where every polar factor the restatement takes has a condition number kappa of at most POLAR_COND_MAX: the
# kernel takes the polar factor of M through the Gram matrix M^T M (gram_inv_sqrt), whose condition is
# kappa^2, so its polar factor carries a relative error of about kappa^2 2^-53 where the SVD of the restatement carries kappa 2^-53.
# The same fifth of the bar, kappa^2 2^-53 <= BAR / 5, gives kappa <= 1.3e5 (from kappa = 3.2e6 on, the kernel drops directions)
POLAR_COND_MAX = (BAR / 5 * 2.0 ** 53) ** 0.5
PARITY_SEEDS = {stack: [0, 1, 2, 3] for stack in STACKS}
RANK_SEEDS = {(rank, stack): [0, 1] for rank in E.MS_RANKS for stack in ("parafac2_nn", "ridge_constant")}
RANK_SEEDS[(16, "parafac2_nn")] = [4, 0]  # job 0: polar factors of condition 3.5e7, 2.7e5, 5.6e5, 3.5e5 from seeds 0 to 3


def _ragged(seed=0, I=6, K=9, r=3):
    rng = np.random.RandomState(seed)
    J = rng.randint(5, 12, size=I)
    X, row_ptr = orc.synthetic_problem(I, J, K, r, seed=seed, dtype=np.float32)
    return [X[row_ptr[i]: row_ptr[i + 1]].astype(np.float64) for i in range(I)], X, row_ptr


def _one_zero(I, n_jobs):
    """weights from {0.5, 1, 2, 3} with one zero per job, at another place in every job"""
    w = np.resize(np.array([2, 0.5, 1, 3, 1, 2, 0.5]), (n_jobs, I)).astype(np.float64)
    for j in range(n_jobs):
        w[j, (2 * j + 1) % I] = 0.0
    return w


def _zero_rows_are_zero(result, w):
    cmf, admm = result[0], result[1]
    _, (A, B_is, C) = cmf
    for i in np.flatnonzero(np.asarray(w) == 0):
        assert not np.asarray(A)[i].any() and not np.asarray(B_is[i]).any(), i
        for aux in admm.auxes[0] + admm.duals[0]:
            assert not np.asarray(aux)[i].any()
        for aux in admm.auxes[1] + admm.duals[1]:
            assert not np.asarray((aux[0] if isinstance(aux, tuple) else aux)[i]).any()


def _parity(mats, X, row_ptr, rank, kw, weights, seeds, n_iter=20, gap_bar=BAR):
    kw = dict(kw, n_iter_max=n_iter, tol=None)
    got = rs.cmf_aoadmm_resample(mats, rank, weights, seeds, method="fused", return_errors=True, return_admm_vars=True, **kw)
    assert len(got) == len(weights)
    for j, (w, seed) in enumerate(zip(weights, seeds)):
        cmf, admm, diag = got[j]
        st = W.weighted_state(mats, X, row_ptr, rank, seed, kw, w)
        orc.POLAR_COND["max"] = 1.0
        res = orc.run(st, n_iter, tol=None, absolute_tol=None)
        assert orc.POLAR_COND["max"] <= POLAR_COND_MAX, (j, seed, "the fixture is ill-posed", orc.POLAR_COND["max"])
        errs, gap, worst = W.compare(cmf, diag, st, res)
        print(f"job {j} seed {seed}: factors / errors {max(errs):.3g}, gaps {gap:.3g}")
        assert diag.n_iter == n_iter
        _zero_rows_are_zero(got[j], w)
        assert max(errs) < BAR, (j, seed, errs)
        bar = BAR
        if gap_bar != BAR and worst is not None and worst[2] < 1e-3:  # the wider bar only where the oracle's gap is below the floor
            bar = gap_bar
        assert gap < bar, (j, seed, gap, "mode, device gap, restatement gap:", worst)


@pytest.mark.parametrize("stack", sorted(STACKS))
def test_parity_against_the_restatement_per_job(stack):
    mats, X, row_ptr = _ragged()
    _parity(mats, X, row_ptr, 3, STACKS[stack], PARITY_WEIGHTS, PARITY_SEEDS[stack])


@pytest.mark.parametrize("stack", ["parafac2_nn", "ridge_constant"])
@pytest.mark.parametrize("rank", E.MS_RANKS)
def test_parity_every_rank(rank, stack):
    # k_multistart_weighted<R, float> for every R.  PARAFAC2 at rank 16: section 11's precedent of 6e-5 for a gap the oracle
    # has below the comparison's 1e-3 floor (the factors' relative difference enters such a gap as an absolute error)
    c = E.MS_CASES[f"r{rank}"]
    mats, X, row_ptr = E.ms_problem(c["I"], c["J_range"], c["K"], c["r"], c["seed"])
    _parity(mats, X, row_ptr, rank, STACKS[stack], _one_zero(c["I"], 2), RANK_SEEDS[(rank, stack)],
            gap_bar=6e-5 if rank == 16 and stack == "parafac2_nn" else BAR)


EDGES = {
    # the inverse batch nb = min(256, 40960 / (16 R^2)) at I = nb + 1, a zero weight in the second batch
    "batch_rank16": dict(I=11, J=[16] * 11, K=12, r=16, seed=31, stack="ridge_constant", zero=[10], seeds=[0, 1]),
    "batch_rank2": dict(I=257, J=[2] * 257, K=3, r=2, seed=32, stack="ridge_constant", zero=[256, 3], seeds=[0, 1]),
    # N and I K below 256 (one stride of every loop, idle threads)
    "below_a_block": dict(I=4, J=[5, 7, 6, 9], K=7, r=3, seed=33, stack="nn_l1C", zero=[2], seeds=[0, 1]),
    # J_i = rank under PARAFAC2
    "J_equals_rank": dict(I=5, J=[4, 4, 6, 4, 5], K=8, r=4, seed=34, stack="parafac2_nn", zero=[1], seeds=[0, 2]),  # job 1, seed 1: condition 6.6e5
    # one matrix with weight 3, and a job with one positive weight
    "one_matrix": dict(I=1, J=[9], K=8, r=2, seed=35, stack="nn_l1C", weights=[[3.0], [3.0]], seeds=[0, 1]),
    "one_positive_weight": dict(I=5, J=[6, 8, 5, 9, 7], K=8, r=3, seed=36, stack="parafac2_nn",
                                weights=[[0, 0, 2.0, 0, 0], [0.5, 0, 0, 0, 0]], seeds=[0, 1]),
}


def edge_problem(name):
    c = EDGES[name]
    mats, X, row_ptr = E.ms_problem(c["I"], list(c["J"]), c["K"], c["r"], c["seed"])
    if "weights" in c:
        w = np.array(c["weights"], dtype=np.float64)
    else:
        w = np.resize(np.array([1, 2, 0.5, 3.0]), (2, c["I"]))
        w[0, c["zero"]] = 0.0
        w[1, c["zero"][:1]] = 0.0
    return mats, X, row_ptr, c["r"], STACKS[c["stack"]], w, c["seeds"]


@pytest.mark.parametrize("name", sorted(EDGES))
def test_parity_at_the_edges(name):
    _parity(*edge_problem(name))


def _bits(res):
    cmf, admm, diag = res
    _, (A, B_is, C) = cmf
    flat = lambda mode: [x for a in mode for x in (a if isinstance(a, tuple) else [a]) for x in (x if isinstance(x, list) else [x])]
    arrays = [A, *B_is, C] + [x for mode in admm.auxes for x in flat(mode)] + [x for mode in admm.duals for x in flat(mode)]
    return [np.asarray(a).tobytes() for a in arrays] + [np.array(diag.regularized_loss).tobytes(), np.array(diag.rec_errors).tobytes(),
                                                        repr(diag.feasibility_gaps), diag.n_iter, diag.message]


@pytest.mark.parametrize("stack", ["parafac2_nn", "box_l2ball"])
def test_all_weights_one_is_the_unweighted_kernel_bit_for_bit(stack):
    mats, _, _ = _ragged(seed=2)
    kw = dict(STACKS[stack], n_iter_max=300, return_errors=True, return_admm_vars=True)
    plain = dec.cmf_aoadmm_multistart(mats, 3, range(8), method="fused", **kw)
    ones = rs.cmf_aoadmm_resample(mats, 3, np.ones((8, len(mats))), range(8), method="fused", **kw)
    assert all(_bits(a) == _bits(b) for a, b in zip(plain, ones))


def test_rank16_all_weights_one_is_the_unweighted_kernel_bit_for_bit():
    c = E.MS_CASES["r16"]
    mats, _, _ = E.ms_problem(c["I"], c["J_range"], c["K"], c["r"], c["seed"])
    kw = dict(parafac2=True, non_negative=True, n_iter_max=50, return_errors=True, return_admm_vars=True)
    plain = dec.cmf_aoadmm_multistart(mats, 16, range(3), method="fused", **kw)
    ones = rs.cmf_aoadmm_resample(mats, 16, np.ones((3, len(mats))), range(3), method="fused", **kw)
    assert all(_bits(a) == _bits(b) for a, b in zip(plain, ones))


def test_job_alone_equals_job_among_64_of_other_weights_and_runs_repeat():
    mats, _, _ = _ragged(seed=2)
    I = len(mats)
    kw = dict(parafac2=True, non_negative=True, n_iter_max=300, return_errors=True, return_admm_vars=True)
    weights = rs.resampling_weights(I, "bootstrap", 64, random_state=0)
    batch = rs.cmf_aoadmm_resample(mats, 3, weights, range(64), method="fused", **kw)
    again = rs.cmf_aoadmm_resample(mats, 3, weights, range(64), method="fused", **kw)
    assert all(_bits(a) == _bits(b) for a, b in zip(batch, again))
    others = rs.resampling_weights(I, "bootstrap", 64, random_state=1)
    for j in (0, 17, 63):
        alone = rs.cmf_aoadmm_resample(mats, 3, weights[j: j + 1], [j], method="fused", **kw)[0]
        assert _bits(alone) == _bits(batch[j])
        others[j] = weights[j]
    moved = rs.cmf_aoadmm_resample(mats, 3, others, range(64), method="fused", **kw)
    assert all(_bits(moved[j]) == _bits(batch[j]) for j in (0, 17, 63))


@pytest.mark.parametrize("dtype", ["bfloat16", "float16"])
def test_x16_equals_upcast(dtype):
    mats, _, _ = _ragged(seed=3)
    m16 = [torch.tensor(m, dtype=getattr(torch, dtype), device="cuda") for m in mats]
    m32 = [m.float() for m in m16]
    kw = dict(non_negative=True, l1_penalty={2: 0.05}, n_iter_max=50, return_errors=True, return_admm_vars=True)
    a = rs.cmf_aoadmm_resample(m16, 3, PARITY_WEIGHTS, range(4), method="fused", **kw)
    b = rs.cmf_aoadmm_resample(m32, 3, PARITY_WEIGHTS, range(4), method="fused", **kw)
    for (ca, _, da), (cb, _, db) in zip(a, b):
        assert da.regularized_loss == db.regularized_loss and da.rec_errors == db.rec_errors
        assert da.feasibility_gaps == db.feasibility_gaps
        for x, y in zip([ca[1][0], *ca[1][1], ca[1][2]], [cb[1][0], *cb[1][1], cb[1][2]]):
            assert x.dtype == getattr(torch, dtype) and torch.equal(x, y.to(x.dtype))


def test_a_fitted_model_as_the_start_and_the_scores_of_the_left_out():
    mats, X, row_ptr = _ragged(seed=4)
    I = len(mats)
    kw = dict(non_negative=[True, False, True], n_iter_max=400)
    model = dec.parafac2_aoadmm(mats, 3, random_state=0, **kw)
    weights = rs.resampling_weights(I, "kfold", 3, random_state=0)
    reps = rs.parafac2_aoadmm_resample(mats, 3, weights, range(3), method="fused", init=model, **kw)
    summary = rs.cmf_resample_summary(reps, model, weights)
    assert np.isfinite(summary.fms).all() and summary.C.mean.shape == np.asarray(model[1][2]).shape
    assert all(sorted(p) == [0, 1, 2] for p in summary.permutations.tolist())
    held = rs.parafac2_aoadmm_heldout_sse(mats, reps, weights)
    assert sorted(int(i) for h in held for i in h.indices) == list(range(I))
    assert all((h.slab_sse >= 0).all() and (h.slab_sse < h.slab_norm).all() for h in held)


# ---- the stopping rule with the default tolerances ----------------------------------------------------------------------------
# weighted fixtures whose relative loss change crosses tol = 1e-8 with a 10 % margin on both sides in the restatement (found on
# the CPU; tests/test_cmf_resampling_host.py::test_the_stopping_fixtures_have_their_margin checks it): the constrained one stops
# at iteration 154 with a change of 7.6e-9, the unconstrained one at 17 with 5.1e-9
STOP_WEIGHTS = [[2, 0, 1, 3, 0.5, 1], [0, 1, 1, 2, 3, 0.5]]
STOP = {
    "parafac2_nn": dict(problem_seed=3, noise=0.2, weights=STOP_WEIGHTS[1], seed=0, kw=dict(parafac2=True, non_negative=True)),
    "unconstrained": dict(problem_seed=0, noise=0.05, weights=STOP_WEIGHTS[0], seed=1, kw=dict()),
}
STOP_N_ITER_MAX = 400


def stop_problem(name):
    S = STOP[name]
    J = np.random.RandomState(S["problem_seed"]).randint(5, 12, size=6)
    X, row_ptr = orc.synthetic_problem(6, J, 9, 3, seed=S["problem_seed"], noise=S["noise"], dtype=np.float32)
    return [X[row_ptr[i]: row_ptr[i + 1]].astype(np.float64) for i in range(6)], X, row_ptr


@pytest.mark.parametrize("name", sorted(STOP))
def test_default_tolerances_stop_at_the_restatement_s_iteration(name):
    S = STOP[name]
    mats, X, row_ptr = stop_problem(name)
    kw = dict(S["kw"], n_iter_max=STOP_N_ITER_MAX)
    (cmf, diag), = rs.cmf_aoadmm_resample(mats, 3, [S["weights"]], [S["seed"]], method="fused", return_errors=True, **kw)
    res = orc.run(W.weighted_state(mats, X, row_ptr, 3, S["seed"], kw, S["weights"]), STOP_N_ITER_MAX)
    print(diag.n_iter, res["n_iter"], diag.message)
    assert 1 < res["n_iter"] < STOP_N_ITER_MAX
    assert diag.n_iter == res["n_iter"] and diag.message == res["message"]
    assert diag.satisfied_stopping_condition == res["satisfied_stopping_condition"]


# ---- resources and rate ---------------------------------------------------------------------------------------------------------
def test_no_scratch_in_the_weighted_kernel():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import kernel_resources

    ms = [k for k in kernel_resources.resources() if k["kernel"].startswith("k_multistart_weighted<")]
    assert len(ms) == 48, [k["kernel"] for k in ms]  # ranks 1..16 x {fp32, bf16, fp16}
    spilled = [(k["kernel"], k["scratch_bytes"], k["vgpr_spill"]) for k in ms if k["scratch_bytes"] or k["vgpr_spill"]]
    assert not spilled, spilled


# profiles/cmf_resample_rate.txt: at the examples' shape (10 x 15 x 20, rank 3, NN PARAFAC2, 200 iterations, tol=None) 64 fused
# bootstrap jobs take 46.8 ms against 3.09 s for 64 sequential ones (4 timed, scaled): RATE_MEASURED.  The guard asks for twice
# that ratio (DESIGN.md sections 11a and 17)
RATE_MEASURED = 0.0151
RATE_JOBS = 64


def test_rate_guard_examples_size():
    from tests.test_gpu_multistart import _example_problem

    mats = _example_problem(10, 15, 20, 3, 0.2, False)
    weights = rs.resampling_weights(len(mats), "bootstrap", RATE_JOBS, random_state=0)
    kw = dict(non_negative=True, n_iter_max=200, tol=None)
    rs.parafac2_aoadmm_resample(mats, 3, weights, range(RATE_JOBS), method="fused", **kw)  # warm-up
    rs.parafac2_aoadmm_resample(mats, 3, weights[:2], range(2), method="sequential", **kw)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rs.parafac2_aoadmm_resample(mats, 3, weights, range(RATE_JOBS), method="fused", **kw)
    torch.cuda.synchronize()
    t_fused = time.perf_counter() - t0
    t0 = time.perf_counter()
    rs.parafac2_aoadmm_resample(mats, 3, weights[:4], range(4), method="sequential", **kw)
    torch.cuda.synchronize()
    t_seq = (time.perf_counter() - t0) * RATE_JOBS / 4
    print(f"fused {t_fused * 1e3:.1f} ms, sequential {t_seq * 1e3:.1f} ms (4 timed, scaled), ratio {t_fused / t_seq:.4f}")
    assert t_fused <= 2 * RATE_MEASURED * t_seq, (t_fused, t_seq)
