"""GPU: cmf_aoadmm_missing / parafac2_aoadmm_missing (matcouply_amd/missing.py, csrc/multistart.hip: k_multistart_missing) -
parity per job with the fp64 restatement (tests/missing_aoadmm_restatement.py), values at missing entries that are never used,
bitwise independence of the batch, 16-bit X, the complete-data kernel on an all-true mask, the stopping rule, recovery of
held-out entries, element-wise K-fold cross-validation over the rank, the kernels' resources and the rate."""
import functools
import time

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from matcouply_amd import decomposition as dec  # noqa: E402
from matcouply_amd import missing  # noqa: E402
from matcouply_amd.coupled_matrices import CoupledMatrixFactorization  # noqa: E402
from tests import kernel_edge_cases as E  # noqa: E402
from tests import missing_aoadmm_restatement as mr  # noqa: E402
from tests import test_gpu_multistart as G  # noqa: E402
from tests import test_missing_host as H  # noqa: E402
from tests.weighted_aoadmm_restatement import compare  # noqa: E402

pytestmark = pytest.mark.gpu


def designed_mask(shapes, seed, K):
    """30 % of the entries missing at random, and on top: one row without an observed entry, one column without one inside one
    matrix, one column without one in any matrix"""
    masks = H.random_mask(shapes, 0.3, seed)
    masks[0][1, :] = False
    masks[2][:, K // 2] = False
    for m in masks:
        m[:, K - 2] = False
    assert all(m.any() for m in masks)
    return masks


def with_junk(mats, masks, junk=np.nan):
    return [np.where(o, m, junk) for m, o in zip(mats, masks)]


def fill_vector(fill, X, observed):
    return {"column_mean": lambda: mr.column_means(X, observed), "zero": lambda: np.zeros(X.shape[1]), "model": lambda: None}[fill]()


def _parity(mats, X, row_ptr, rank, stack, fill, per_job, n_jobs, n_iter=20, gap_bar=1e-5):
    shapes, K = [m.shape for m in mats], X.shape[1]
    job_masks = [designed_mask(shapes, 100 + s if per_job else 100, K) for s in range(n_jobs)]
    kw = dict(G.STACKS[stack], n_iter_max=n_iter, tol=None, return_errors=True)
    if per_job:
        got = missing.cmf_aoadmm_missing(mats, rank, job_masks, range(n_jobs), fill=fill, **kw)
    else:  # the shared mask once as NaN entries, found by the call itself
        got = missing.cmf_aoadmm_missing(with_junk(mats, job_masks[0]), rank, None, range(n_jobs), fill=fill, **kw)
    assert len(got) == n_jobs
    for s, (cmf, diag) in enumerate(got):
        observed = np.concatenate(job_masks[s])
        st = mr.missing_state(mats, np.where(observed, X, np.nan), row_ptr, rank, s, kw, observed, fill_vector(fill, X, observed))
        res = mr.run(st, n_iter, tol=None, absolute_tol=None)
        errs, gap, worst = compare(cmf, diag, st, res)
        assert diag.n_iter == n_iter and diag.satisfied_stopping_condition is False
        assert max(errs) < 1e-5, (stack, fill, s, errs)
        assert gap < gap_bar, (stack, fill, s, gap, "mode, device gap, restatement gap:", worst)


@pytest.mark.parametrize("stack,fill,per_job", [
    ("nn_l1C", "column_mean", False), ("nn_l1C", "model", True), ("box_l2ball", "zero", True), ("box_l2ball", "column_mean", False),
    ("parafac2_nn", "model", False), ("parafac2_nn", "column_mean", True), ("ridge_constant", "zero", False),
    ("ridge_constant", "column_mean", True)])
def test_restatement_parity_per_job(stack, fill, per_job):
    mats, X, row_ptr = G._ragged()
    _parity(mats, X.astype(np.float64), row_ptr, 3, stack, fill, per_job, 8)


@pytest.mark.parametrize("case,stack,fill", [
    ("r1", "parafac2_nn", "column_mean"), ("r1", "ridge_constant", "model"), ("r16", "parafac2_nn", "model"),
    ("r16", "ridge_constant", "column_mean"), ("rows_reduce_r12", "nn_l1C", "column_mean")])
def test_restatement_parity_at_the_rank_edges(case, stack, fill):
    # k_multistart_missing<1>, <16> and rows_reduce's one-thread-per-entry form (<12>).  PARAFAC2 at rank 16: a gap
    # ||F - Z|| / ||F|| below the comparison's 1e-3 floor carries the factors' relative difference as an absolute error, the
    # argument of tests/test_gpu_multistart.py::test_oracle_parity_every_rank and its bar
    c = E.MS_CASES[case]
    mats, X, row_ptr = E.ms_problem(c["I"], c["J_range"], c["K"], c["r"], c["seed"])
    _parity(mats, X.astype(np.float64), row_ptr, c["r"], stack, fill, True, 2,
            gap_bar=6e-5 if case == "r16" and stack == "parafac2_nn" else 1e-5)


def _bits(res):
    return G._bits(res) + [np.array(res[2].rec_errors).tobytes(), repr(res[2].feasibility_gaps)]


@pytest.mark.parametrize("fill", ["column_mean", "model"])
def test_values_at_missing_entries_are_never_used(fill):
    mats, _, _ = G._ragged(seed=1)
    masks = designed_mask([m.shape for m in mats], 5, 9)
    kw = dict(parafac2=True, non_negative=True, n_iter_max=30, return_errors=True, return_admm_vars=True)
    runs = [missing.cmf_aoadmm_missing(with_junk(mats, masks, junk), 3, masks, range(4), fill=fill, **kw) for junk in (np.nan, 1e30, 0.0)]
    for other in runs[1:]:
        assert all(_bits(a) == _bits(b) for a, b in zip(runs[0], other))
    assert all(np.isfinite(np.asarray(x)).all() for res in runs[0] for x in (res[0][1][0], res[0][1][2], res[2].rec_errors))


def test_job_alone_equals_job_in_a_batch_and_runs_repeat():
    mats, _, _ = G._ragged(seed=2)
    shapes = [m.shape for m in mats]
    job_masks = [designed_mask(shapes, s, 9) for s in range(64)]
    kw = dict(parafac2=True, non_negative=True, n_iter_max=100, return_errors=True, return_admm_vars=True)
    batch = missing.cmf_aoadmm_missing(mats, 3, job_masks, range(64), **kw)
    again = missing.cmf_aoadmm_missing(mats, 3, job_masks, range(64), **kw)
    for s in (0, 17, 63):
        alone = missing.cmf_aoadmm_missing(mats, 3, [job_masks[s]], [s], **kw)[0]
        assert _bits(alone) == _bits(batch[s])
    assert all(_bits(a) == _bits(b) for a, b in zip(batch, again))
    # ... and under one shared mask, with the model fill
    shared = missing.cmf_aoadmm_missing(mats, 3, job_masks[0], range(64), fill="model", **kw)
    assert _bits(missing.cmf_aoadmm_missing(mats, 3, job_masks[0], [41], fill="model", **kw)[0]) == _bits(shared[41])


@pytest.mark.parametrize("dtype", ["bfloat16", "float16"])
def test_x16_equals_upcast(dtype):
    mats, _, _ = G._ragged(seed=3)
    masks = designed_mask([m.shape for m in mats], 3, 9)
    m16 = [torch.tensor(m, dtype=getattr(torch, dtype), device="cuda") for m in with_junk(mats, masks)]
    m32 = [m.float() for m in m16]
    kw = dict(non_negative=True, l1_penalty={2: 0.05}, n_iter_max=50, return_errors=True, return_admm_vars=True)
    a = missing.cmf_aoadmm_missing(m16, 3, None, range(4), **kw)
    b = missing.cmf_aoadmm_missing(m32, 3, None, range(4), **kw)
    for (ca, _, da), (cb, _, db) in zip(a, b):
        assert da.regularized_loss == db.regularized_loss and da.rec_errors == db.rec_errors
        assert da.feasibility_gaps == db.feasibility_gaps and np.isfinite(da.rec_errors).all()
        for x, y in zip([ca[1][0], *ca[1][1], ca[1][2]], [cb[1][0], *cb[1][1], cb[1][2]]):
            assert x.dtype == getattr(torch, dtype) and x.is_cuda and torch.equal(x, y.to(x.dtype))


@pytest.mark.parametrize("stack", ["parafac2_nn", "nn_l1C"])
def test_all_true_mask_is_the_complete_data_fit(stack):
    mats, _, _ = G._ragged(seed=4)
    kw = dict(G.STACKS[stack], n_iter_max=40, tol=None, return_errors=True)
    full = [np.ones(m.shape, dtype=bool) for m in mats]
    got = missing.cmf_aoadmm_missing(mats, 3, full, range(4), fill="zero", **kw)
    want = dec.cmf_aoadmm_multistart(mats, 3, range(4), method="fused", **kw)
    for (cg, dg), (cw, dw) in zip(got, want):
        for x, y in zip([cg[1][0], *cg[1][1], cg[1][2]], [cw[1][0], *cw[1][1], cw[1][2]]):
            assert np.linalg.norm(x - y) <= 1e-10 * np.linalg.norm(y)
        np.testing.assert_allclose(dg.rec_errors, dw.rec_errors, rtol=1e-9)
        assert dg.n_iter == dw.n_iter == 40


# ---- the examples' problem: 10 x 15 x 20, rank 3, non-negative PARAFAC2 -------------------------------------------------------------
PF2 = dict(parafac2=True, non_negative=True, l2_penalty=0, return_errors=True)


@functools.lru_cache(maxsize=None)
def _example(noise_level):
    clean, mats = H.example_problem(noise_level=noise_level)
    mats = [m.astype(np.float32).astype(np.float64) for m in mats]  # what the device holds: X is packed in fp32
    shapes = [m.shape for m in mats]
    masks = H.random_mask(shapes, 0.3, seed=0)
    return clean, mats, masks, np.concatenate(mats), np.concatenate([[0], np.cumsum([s[0] for s in shapes])])


def _restated(noise_level, rank, seed, n_iter, observed=None, impute=True, **rule):
    _, mats, masks, X, row_ptr = _example(noise_level)
    observed = np.concatenate(masks) if observed is None else observed
    st = mr.missing_state(mats, X, row_ptr, rank, seed, dict(PF2, n_iter_max=n_iter, **rule), observed, mr.column_means(X, observed), impute)
    return st, mr.run(st, n_iter, **({"tol": None, "absolute_tol": None} if "tol" in rule else {}))


# Default tolerances at the examples' noise level 0.2.  The relative loss change falls by 1 - 3 % per iteration near tol = 1e-8,
# so a start's margin |change - tol| at the iteration that decides is 1e-10 at best.  Seeds 0 .. 9 of the restatement: margins
# 1.6e-12, 9.0e-11, 9.1e-11, 5.4e-11, 1.1e-10, 5.4e-11, 8.8e-12, 6.6e-11, 7.8e-11, 3.0e-11 (they stop after 274 .. 834
# iterations).  The five widest are taken: seeds 0 and 6 sit on the edge of tol, 3, 5 and 9 are the next narrowest.  The device's
# loss differs from the restatement's by a relative 2e-14 .. 3e-13 on these seeds, its change from one iteration to the next
# by 1e-14
STOP_SEEDS = (1, 2, 4, 7, 8)


def test_stopping_rule_follows_the_restatement():
    _, mats, masks, _, _ = _example(0.2)
    got = missing.parafac2_aoadmm_missing(with_junk(mats, masks), 3, None, STOP_SEEDS, non_negative=True, n_iter_max=1000,
                                          return_errors=True)
    for seed, (_, diag) in zip(STOP_SEEDS, got):
        _, res = _restated(0.2, 3, seed, 1000)
        L = np.array(res["losses"])
        change = np.abs(L[:-1] - L[1:]) / L[:-1]
        margin = np.min(np.abs(change - 1e-8))
        n = min(len(L), len(diag.regularized_loss))
        off = np.max(np.abs(np.array(diag.regularized_loss[:n]) - L[:n]) / L[:n])
        print(f"seed {seed}: n_iter {diag.n_iter} / {res['n_iter']}, margin {margin:.2e}, device - restatement loss {off:.2e}")
        assert res["satisfied_stopping_condition"] and res["n_iter"] < 1000
        assert margin >= 10 * off, (seed, margin, off, "this seed sits on the edge of tol: choose another")
        assert (diag.n_iter, diag.satisfied_stopping_condition, diag.message) == (
            res["n_iter"], res["satisfied_stopping_condition"], res["message"])
        assert diag.satisfied_feasibility_condition == res["satisfied_feasibility_condition"]


def _heldout_relative(imputed, clean, masks):
    held = ~np.concatenate(masks)
    return np.linalg.norm((np.concatenate(imputed) - np.concatenate(clean))[held]) / np.linalg.norm(np.concatenate(clean)[held])


def test_recovery_of_the_missing_entries():
    # noise-free, 30 % removed, 400 iterations, best of 3 starts by final loss.  The restatement: held-out relative error 1.27e-3
    # with imputation; 0.398 with the column-mean fill never updated.  The bars: 0.05 and 0.2
    clean, mats, masks, X, row_ptr = _example(0.0)
    holed = with_junk(mats, masks)
    got = missing.parafac2_aoadmm_missing(holed, 3, None, range(3), non_negative=True, n_iter_max=400, tol=None, return_errors=True)
    cmf, diag = min(got, key=lambda r: r[1].regularized_loss[-1])
    err_device = _heldout_relative(missing.impute(holed, cmf), clean, masks)
    restated = {}
    for on in (True, False):
        runs = [_restated(0.0, 3, s, 400, impute=on, tol=None) for s in range(3)]
        st, res = min(runs, key=lambda r: r[1]["losses"][-1])
        model = CoupledMatrixFactorization((None, (st.A, [st.B[row_ptr[i]: row_ptr[i + 1]] for i in range(len(mats))], st.C)))
        restated[on] = _heldout_relative(missing.impute(holed, model), clean, masks)
        if on:
            assert abs(diag.regularized_loss[-1] - res["losses"][-1]) <= 2e-5 * res["losses"][-1]  # (0.5 rec^2: twice the flat bar)
    print(f"held-out relative error: device {err_device:.3e}, restatement {restated[True]:.3e}, without imputation {restated[False]:.3e}")
    assert err_device < 0.05 and restated[True] < 0.05
    assert restated[False] > 0.2
    assert all(np.array_equal(np.asarray(i)[o], m[o]) for i, m, o in zip(missing.impute(holed, cmf), mats, masks))


def test_entrywise_kfold_prefers_the_true_rank():
    # 5 % noise, 5 folds of the entries, one start per fold, 300 iterations.  The restatement's cross-validated mean squared
    # error: rank 2 3.34e-2, rank 3 6.45e-4, rank 4 7.50e-4 - rank 2 over rank 3 by a factor of 52, so that is asserted (the
    # issue asks for a factor of 2 to spare); rank 4 is reported only
    _, mats, _, X, _ = _example(0.05)
    folds = missing.entry_kfold(mats, 5, random_state=0)
    mse, mse_restated = {}, {}
    for rank in (2, 3, 4):
        got = missing.parafac2_aoadmm_missing(mats, rank, folds, [0] * 5, non_negative=True, n_iter_max=300, tol=None)
        sse, count = missing.heldout_entry_sse(mats, got, folds)
        assert count.sum() == X.size and count.max() - count.min() <= 1
        mse[rank] = sse.sum() / count.sum()
        if rank < 4:
            total = 0.0
            for f in folds:
                observed = np.concatenate(f)
                st, _ = _restated(0.05, rank, 0, 300, observed=observed, tol=None)
                total += np.sum((st.model() - X)[~observed] ** 2)
            mse_restated[rank] = total / X.size
            # models that agree to the flat bar 1e-5 move a held-out residual of 3 % of the data (rank 3; more at rank 2) by
            # 1e-5 / 0.03, and its square by twice that: 7e-4
            assert abs(mse[rank] - mse_restated[rank]) <= 1e-3 * mse_restated[rank]
    print("cross-validated MSE, device:", mse, "restatement:", mse_restated)
    assert mse_restated[2] > 2 * mse_restated[3]
    assert mse[2] > mse[3]


def test_resources_of_the_three_kernel_families():
    import os
    import sys

    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import kernel_resources

    rows = kernel_resources.resources()
    for prefix, count in (("k_multistart_missing<", 16), ("k_multistart<", 48), ("k_multistart_weighted<", 48)):
        ms = [k for k in rows if k["kernel"].startswith(prefix)]
        assert len(ms) == count, (prefix, [k["kernel"] for k in ms])
        spilled = [(k["kernel"], k["scratch_bytes"], k["vgpr_spill"]) for k in ms if k["scratch_bytes"] or k["vgpr_spill"]]
        assert not spilled, spilled


# profiles/missing_rate.txt: at the examples' shape (10 x 15 x 20, rank 3, NN PARAFAC2, 200 iterations, tol=None, 30 % missing)
# missing / fused-complete is MEASURED_RATIO at 64 jobs.  The guard allows 1.5 x that: the headroom covers the run-to-run noise
# of a ~50 ms measurement on a shared machine
MEASURED_RATIO = 1.0355  # 47.2 ms against 45.6 ms (at 1024 jobs: 0.90, 361 ms against 400 ms)
RATE_GUARD = 1.5 * MEASURED_RATIO


def test_rate_guard_examples_size():
    _, mats, masks, _, _ = _example(0.0)
    holed = with_junk(mats, masks)
    kw = dict(non_negative=True, n_iter_max=200, tol=None)
    missing.parafac2_aoadmm_missing(holed, 3, None, range(64), **kw)  # warm-up (library load, code objects)
    dec.parafac2_aoadmm_multistart(mats, 3, range(64), method="fused", **kw)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    missing.parafac2_aoadmm_missing(holed, 3, None, range(64), **kw)
    torch.cuda.synchronize()
    t_missing = time.perf_counter() - t0
    t0 = time.perf_counter()
    dec.parafac2_aoadmm_multistart(mats, 3, range(64), method="fused", **kw)
    torch.cuda.synchronize()
    t_complete = time.perf_counter() - t0
    print(f"missing {t_missing * 1e3:.1f} ms, fused on complete data {t_complete * 1e3:.1f} ms, ratio {t_missing / t_complete:.3f}")
    assert t_missing <= RATE_GUARD * t_complete, (t_missing, t_complete)
