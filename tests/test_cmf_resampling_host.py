"""CPU: cmf_aoadmm_resample and its companions (matcouply_amd/resampling.py) without a device.  The fp64
restatement of the weighted AO-ADMM run (tests/weighted_aoadmm_restatement.py) is pinned to the oracle by three identities; every
refusal happens before the device is touched; the sequential method is checked through the calls it makes; the summary and the
held-out scores run on synthetic replicates; the exports and the C entry's own refusals."""
import ctypes
import inspect

import numpy as np
import pytest

import matcouply_amd
from matcouply_amd import _engine
from matcouply_amd import decomposition as dec
from matcouply_amd import multistart as ms
from matcouply_amd import resampling as rs
from oracle import aoadmm_oracle as orc
from tests import weighted_aoadmm_restatement as W

RANK, N_ITER = 3, 20
# the parity stacks of tests/test_gpu_cmf_resample.py (kept equal by test_the_gpu_parity_stacks_are_pinned_here) and the issue's
STACKS = {
    "nn_l1C": dict(non_negative={0: True, 1: True}, l1_penalty={2: 0.05}),
    "box_l2ball": dict(lower_bound={1: -0.5}, upper_bound={1: 2.0}, l2_norm_bound={0: 3.0, 2: 2.0},
                       constant_feasibility_penalty=True),
    "parafac2_nn": dict(parafac2=True, non_negative=True),
    "ridge_constant": dict(l2_penalty=[0.1, 0.2, 0.05], non_negative={2: True}, constant_feasibility_penalty=True),
    "l1_on_A": dict(l1_penalty={0: 0.05}, non_negative={1: True}),
    "box_B_positive_lower": dict(lower_bound={1: 0.1}, upper_bound={1: 2.0}, non_negative={0: True}),
    "ridge_BC": dict(l2_penalty=[0, 0.2, 0.05]),
}
# where the fit of sqrt(w_i) X_i is the weighted fit: penalties on A none or NonNegativity, no l2 on A, no constant penalty on A
SCALING_HOLDS = ["nn_l1C", "parafac2_nn", "box_B_positive_lower", "ridge_BC"]
BAR = 1e-9  # measured: 0 (a), 2.6e-15 (b), 1.7e-14 (c)


def _problem(seed=0, I=6, K=9):
    rng = np.random.RandomState(seed)
    J = rng.randint(5, 11, size=I)
    X, row_ptr = orc.synthetic_problem(I, J, K, RANK, seed=seed, dtype=np.float32)
    return [X[row_ptr[i]: row_ptr[i + 1]].astype(np.float64) for i in range(I)], X, row_ptr


def _run(state):
    return orc.run(state, N_ITER, tol=None, absolute_tol=None)


def _difference(st, res, ref, ref_res, keep, row_ptr):
    rows = np.concatenate([np.arange(row_ptr[i], row_ptr[i + 1]) for i in keep])
    d = [np.abs(st.A[keep] - ref.A).max(), np.abs(st.B[rows] - ref.B).max(), np.abs(st.C - ref.C).max(),
         np.abs(np.array(res["losses"]) - ref_res["losses"]).max(), np.abs(np.array(res["rec_errors"]) - ref_res["rec_errors"]).max()]
    for g, h in zip(res["gaps"], ref_res["gaps"]):
        d += [np.abs(np.array(g[m]) - h[m]).max() for m in range(3) if len(g[m])]
    return max(d)


@pytest.fixture(scope="module")
def problem():
    return _problem()


@pytest.mark.parametrize("stack", sorted(STACKS))
def test_a_all_weights_one_is_the_oracle(problem, stack):
    mats, X, row_ptr = problem
    kw = dict(STACKS[stack], n_iter_max=N_ITER, tol=None)
    st = W.weighted_state(mats, X, row_ptr, RANK, 0, kw, np.ones(6))
    ref = W.oracle_state(mats, X, row_ptr, RANK, 0, kw)
    assert _difference(st, _run(st), ref, _run(ref), np.arange(6), row_ptr) <= BAR


@pytest.mark.parametrize("stack", sorted(STACKS))
def test_b_zero_weights_are_the_oracle_on_the_shortened_list(problem, stack):
    mats, X, row_ptr = problem
    kw = dict(STACKS[stack], n_iter_max=N_ITER, tol=None)
    w = np.array([1, 0, 1, 1, 0, 1.0])
    keep = np.flatnonzero(w > 0)
    st = W.weighted_state(mats, X, row_ptr, RANK, 0, kw, w)
    ref = W.shortened(W.start_of(mats, RANK, 0, kw), X, row_ptr, keep)
    assert _difference(st, _run(st), ref, _run(ref), keep, row_ptr) <= BAR
    dead_rows = np.repeat(w == 0, np.diff(row_ptr))
    assert not st.A[w == 0].any() and not st.B[dead_rows].any()  # exact zeros
    for mode, dead in ((0, w == 0), (1, dead_rows)):
        for z, u in zip(st.aux[mode], st.dual[mode]):
            assert not (z[0] if isinstance(z, tuple) else z)[dead].any() and not u[dead].any()


def _scaled_fit_difference(problem, stack):
    mats, X, row_ptr = problem
    kw = dict(STACKS[stack], n_iter_max=N_ITER, tol=None)
    w = np.array([0.5, 2, 1, 3, 0.25, 1.5])
    st = W.weighted_state(mats, X, row_ptr, RANK, 0, kw, w)
    res = _run(st)
    ref = W.shortened(W.start_of(mats, RANK, 0, kw), X, row_ptr, np.arange(6), scale=np.sqrt(w))
    ref_res = _run(ref)
    ref.A = ref.A / np.sqrt(w)[:, None]
    return max(np.abs(st.A - ref.A).max(), np.abs(st.B - ref.B).max(), np.abs(st.C - ref.C).max(),
               np.abs(np.array(res["rec_errors"]) - ref_res["rec_errors"]).max())


@pytest.mark.parametrize("stack", SCALING_HOLDS)
def test_c_homogeneous_penalties_on_A_are_the_oracle_on_the_scaled_matrices(problem, stack):
    assert _scaled_fit_difference(problem, stack) <= BAR


@pytest.mark.parametrize("stack", ["l1_on_A", "box_l2ball", "ridge_constant"])
def test_d_the_scaling_route_fails_where_A_sees_its_scale(problem, stack):
    # the reason the weights are applied in the algorithm (measured: 0.21, 0.18, 0.34)
    assert _scaled_fit_difference(problem, stack) > 1e-3


def test_the_gpu_parity_stacks_are_pinned_here():
    from tests import test_gpu_cmf_resample as G

    assert all(STACKS[name] == kw for name, kw in G.STACKS.items())


def test_the_stopping_fixtures_have_their_margin():
    """tests/test_gpu_cmf_resample.py::test_default_tolerances_stop_at_the_restatement_s_iteration: the run stops on the relative
    criterion with a change below 0.9 tol on an iterate whose worst gap is below 0.9 feasibility_tol, and every iterate before it
    could not have stopped with a 10 % margin: its change is above 1.1 tol or its worst gap above 1.1 feasibility_tol"""
    from tests import test_gpu_cmf_resample as G

    for name, S in G.STOP.items():
        mats, X, row_ptr = G.stop_problem(name)
        kw = dict(S["kw"], n_iter_max=G.STOP_N_ITER_MAX)
        res = orc.run(W.weighted_state(mats, X, row_ptr, 3, S["seed"], kw, S["weights"]), G.STOP_N_ITER_MAX)
        n, losses = res["n_iter"], np.array(res["losses"])
        change = np.abs(losses[:-1] - losses[1:]) / losses[:-1]
        worst = [max([g for mode in gaps for g in mode], default=0.0) for gaps in res["gaps"]]
        assert 1 < n < G.STOP_N_ITER_MAX and res["message"].startswith("FEASIBILITY GAP CRITERION AND RELATIVE"), name
        assert change[n - 1] < 0.9e-8 and worst[n] < 0.9e-4 and losses[n] > 1.1e-10, name
        assert all(change[t] > 1.1e-8 or worst[t + 1] > 1.1e-4 for t in range(n - 1)), name


# ---- refusals, all without a device ----------------------------------------------------------------------------------------------
@pytest.fixture
def no_device(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the device was touched")

    monkeypatch.setattr(dec, "_device", boom)
    monkeypatch.setattr(dec, "_pack", boom)
    monkeypatch.setattr(_engine, "multistart_run_weighted", boom)


def test_refusals_before_the_device(problem, no_device):
    mats = problem[0]
    ones = np.ones((2, 6))
    with pytest.raises(ValueError, match="method must be"):
        rs.cmf_aoadmm_resample(mats, 3, ones, [0, 1], method="gpu")
    with pytest.raises(TypeError, match="random_states, not random_state"):
        rs.cmf_aoadmm_resample(mats, 3, ones, [0, 1], random_state=0)
    with pytest.raises(ValueError, match='init="random" or a fitted model'):
        rs.cmf_aoadmm_resample(mats, 3, ones, [0, 1], init="svd")
    with pytest.raises(TypeError, match="fitted model"):
        rs.cmf_aoadmm_resample(mats, 3, ones, [0, 1], init=3.5)
    with pytest.raises(TypeError):
        rs.cmf_aoadmm_resample(mats, 3, ones, [0, 1], no_such_keyword=1)
    for bad, match in ((np.ones((2, 5)), "shape"), (-ones, ">= 0"), (ones * np.nan, "finite"), (ones * np.inf, "finite"),
                       (np.array([[1.0] * 6, [0.0] * 6]), "job 1 has no positive weight"), ("weights", "real array|shape")):
        with pytest.raises(ValueError, match=match):
            rs.cmf_aoadmm_resample(mats, 3, bad, [0, 1], method="fused")
    with pytest.raises(ValueError, match="3 states for 2 jobs"):
        rs.cmf_aoadmm_resample(mats, 3, ones, [0, 1, 2])
    with pytest.raises(TypeError, match="parafac2"):
        rs.parafac2_aoadmm_resample(mats, 3, ones, [0, 1], parafac2=True)


@pytest.mark.parametrize("kw,reason", [
    (dict(unimodal={1: True}), "Unimodality on mode 1 is not served"),
    (dict(tv_penalty={1: 0.1}), "is not served"),
    (dict(verbose=True), "verbose"),
    (dict(arithmetic="exact"), "arithmetic"),
    (dict(l2_norm_bound={0: 1.0}), "L2Ball on mode 0 needs constant_feasibility_penalty"),
    (dict(parafac2=True, _rank=12), "Parafac2 is served on mode 1 with every J_i >= rank"),
    (dict(_rank=17), "rank 17 is above 16"),
])
def test_fused_serves_what_the_multistart_kernel_serves(problem, no_device, kw, reason):
    mats = problem[0]
    kw = dict(kw)
    rank = kw.pop("_rank", 3)
    assert reason in ms._multistart_unfused_reason(mats, rank, dec._cmf_kwargs(kw))
    with pytest.raises(NotImplementedError, match=r'cmf_aoadmm_resample\(method="fused"\)'):
        rs.cmf_aoadmm_resample(mats, rank, np.ones((2, 6)), [0, 1], method="fused", **kw)


# ---- the sequential method, through the calls it makes ------------------------------------------------------------------------
@pytest.fixture
def recorded(monkeypatch):
    calls = []

    def fake(matrices, rank, **kw):
        calls.append((matrices, rank, kw))
        I = len(matrices)
        A = np.arange(1.0, I * rank + 1).reshape(I, rank)
        B_is = [np.full((m.shape[0], rank), 1.0 + i) for i, m in enumerate(matrices)]
        cmf = dec.CoupledMatrixFactorization((None, (A, B_is, np.ones((matrices[0].shape[1], rank)))))
        out = [cmf]
        if kw.get("return_admm_vars"):
            out.append(dec.ADMMVars(([A * 2], [[b * 3 for b in B_is]], []), ([A * 4], [[b * 5 for b in B_is]], [])))
        if kw.get("return_errors"):
            out.append("diagnostics")
        return out[0] if len(out) == 1 else tuple(out)

    fake.__signature__ = inspect.signature(dec.cmf_aoadmm)  # _cmf_kwargs completes the keywords from the signature
    monkeypatch.setattr(dec, "cmf_aoadmm", fake)
    return calls


def test_sequential_fits_the_scaled_positive_weight_matrices(problem, recorded, no_device):
    mats = problem[0]
    w = np.array([[4.0, 0, 1, 0.25, 0, 1], [1, 1, 0, 1, 1, 1]])
    out = rs.cmf_aoadmm_resample(mats, 3, w, [7, 8], method="sequential", non_negative=True, n_iter_max=5, return_errors=True,
                                 return_admm_vars=True)
    assert len(recorded) == 2 and [c[2]["random_state"] for c in recorded] == [7, 8]
    keep = [0, 2, 3, 5]
    got, rank, kw = recorded[0]
    assert rank == 3 and kw["non_negative"] is True and kw["n_iter_max"] == 5 and "init" not in kw
    for m, i, f in zip(got, keep, [2.0, 1.0, 0.5, 1.0]):
        np.testing.assert_array_equal(m, mats[i] * f)
    assert recorded[0][0][1] is mats[2]  # weight 1: the matrix itself
    assert [m is mats[i] for m, i in zip(recorded[1][0], [0, 1, 3, 4, 5])] == [True] * 5
    cmf, admm, diag = out[0]
    A, B_is, C = cmf[1]
    fake_A = np.arange(1.0, 13).reshape(4, 3)
    np.testing.assert_array_equal(A[keep], fake_A / np.array([2.0, 1.0, 0.5, 1.0])[:, None])  # row i divided back by sqrt(w_i)
    assert not A[[1, 4]].any() and A.shape == (6, 3)
    assert [b.shape for b in B_is] == [(m.shape[0], 3) for m in mats] and not B_is[1].any() and not B_is[4].any()
    assert (B_is[3] == 3.0).all() and diag == "diagnostics"
    np.testing.assert_array_equal(admm.auxes[0][0][keep], 2 * fake_A / np.array([2.0, 1.0, 0.5, 1.0])[:, None])
    assert not admm.duals[0][0][[1, 4]].any() and not admm.auxes[1][0][4].any() and (admm.duals[1][0][5] == 20.0).all()


def test_sequential_starts_from_the_model_restricted_and_scaled(problem, recorded, no_device):
    mats = problem[0]
    model = (None, (np.ones((6, 3)), [np.full((m.shape[0], 3), 2.0) for m in mats], np.full((9, 3), 3.0)))
    rs.cmf_aoadmm_resample(mats, 3, [[4.0, 0, 1, 1, 1, 1]], [0], method="sequential", init=model)
    _, (A0, B0, C0) = recorded[0][2]["init"]
    np.testing.assert_array_equal(A0, np.array([2.0, 1, 1, 1, 1])[:, None] * np.ones((5, 3)))
    assert len(B0) == 5 and (np.asarray(C0) == 3.0).all()


@pytest.mark.parametrize("kw,reason", [(dict(l1_penalty={0: 0.1}), "other than NonNegativity"),
                                       (dict(l2_penalty=[0.1, 0, 0]), "l2_penalty on A"),
                                       (dict(non_negative=True, constant_feasibility_penalty=True), "constant feasibility penalty on A")])
def test_sequential_refuses_where_the_scaling_identity_fails(problem, recorded, no_device, kw, reason):
    mats = problem[0]
    with pytest.raises(NotImplementedError, match=reason):
        rs.cmf_aoadmm_resample(mats, 3, [[2.0, 0, 1, 1, 1, 1]], [0], method="sequential", **kw)
    assert not recorded
    rs.cmf_aoadmm_resample(mats, 3, [[1.0, 0, 1, 1, 0, 1]], [0], method="sequential", **kw)  # weights 0 / 1: nothing is scaled
    assert len(recorded) == 1 and len(recorded[0][0]) == 4


def test_auto_follows_the_multistart_rule(problem, monkeypatch):
    mats = problem[0]
    seen = []
    monkeypatch.setattr(ms, "_multistart_fused", lambda *a, **k: seen.append(("fused", k["zero_weights"].shape)) or [])
    one = lambda m, r, **k: seen.append("call") or dec.CoupledMatrixFactorization(
        (None, (np.ones((len(m), r)), [np.ones((x.shape[0], r)) for x in m], np.ones((9, r)))))
    one.__signature__ = inspect.signature(dec.cmf_aoadmm)
    monkeypatch.setattr(dec, "cmf_aoadmm", one)
    rs.cmf_aoadmm_resample(mats, 3, np.ones((2, 6)), [0, 1])  # small: fused from the first job
    rs.cmf_aoadmm_resample(mats, 3, np.ones((2, 6)), [0, 1], unimodal={1: True})  # not served: one by one
    big = [np.ones((200, 50))] * 6
    rs.cmf_aoadmm_resample(big, 3, np.ones((2, 6)), [0, 1])  # large and few: one by one
    assert seen == [("fused", (2, 6)), "call", "call", "call", "call"]


# ---- the zero-weight part of a state slice ---------------------------------------------------------------------------------------
def test_zero_weight_mask_follows_the_state_layout():
    row_ptr = np.array([0, 2, 5, 6])
    K, r = 4, 2
    kinds = [[_engine.PEN_NN], [_engine.PEN_PARAFAC2, _engine.PEN_NN], [_engine.PEN_L1]]
    mask = ms._StateLayout(row_ptr, K, r, kinds).zero_weight_mask(np.array([1.0, 0.0, 2.0]))
    assert mask.size == _engine.multistart_state_len(3, 6, K, r, kinds)
    A = [False] * 2 + [True] * 2 + [False] * 2
    B = [False] * 4 + [True] * 6 + [False] * 2
    C = [False] * 8
    expect = A + B + C + A + A + B + [False] * 4 + B + B + B + C + C
    assert mask.tolist() == expect


# ---- summary and held-out scores on synthetic replicates ---------------------------------------------------------------------
def _replicates(rng, n=5, I=4, J=6, K=5, r=2):
    A = rng.uniform(0.5, 1.5, (I, r))
    Delta = np.linalg.qr(rng.standard_normal((r, r)))[0] * 2.0
    P = [np.linalg.qr(rng.standard_normal((J, r)))[0] for _ in range(I)]
    C = rng.standard_normal((K, r))
    ref = dec.CoupledMatrixFactorization((None, (A, [p @ Delta for p in P], C)))
    weights = np.ones((n, I))
    reps = []
    for j in range(n):
        perm = rng.permutation(r)
        sA, sC = rng.choice([-1.0, 1.0], r), rng.choice([-1.0, 1.0], r)
        weights[j, j % I] = 0.0
        Aj = (A + 0.01 * rng.standard_normal(A.shape)) * sA
        Aj[j % I] = 0.0
        B_is = [(p @ Delta) * (sA * sC) if i != j % I else np.zeros((J, r)) for i, p in enumerate(P)]
        reps.append(dec.CoupledMatrixFactorization((None, (Aj[:, perm], [b[:, perm] for b in B_is], (C * sC)[:, perm]))))
    return ref, reps, weights, (A, P, Delta, C)


def test_summary_lines_the_replicates_up():
    ref, reps, weights, (A, P, Delta, C) = _replicates(np.random.RandomState(0))
    s = rs.cmf_resample_summary(reps, ref, weights, quantiles=(0.25, 0.5, 0.75))
    np.testing.assert_allclose(s.C.mean, C, atol=1e-12)
    np.testing.assert_allclose(s.C.std, 0, atol=1e-12)
    assert len(s.B_is) == 4 and s.C.quantiles.shape == (3, 5, 2) and s.fms.shape == (5,) and s.permutations.shape == (5, 2)
    for i in range(4):
        np.testing.assert_allclose(s.B_is[i].mean, P[i] @ Delta, atol=1e-12)  # over the replicates that held matrix i
    np.testing.assert_allclose(s.A.mean, A, atol=0.02)
    assert (s.A.std > 0).all() and (s.A.std < 0.05).all()
    # the row statistics skip the replicates that left the row out: matrix 0 was out in replicates 0 and 4
    held = [k for k in range(5) if weights[k, 0] > 0]
    lined = [np.sort(np.abs(np.asarray(reps[k][1][0])[0])) for k in held]  # the columns come permuted and with signs
    np.testing.assert_allclose(np.sort(s.A.mean[0]), np.sort(np.mean(lined, 0)), atol=1e-12)
    with pytest.raises(ValueError, match="rows for 5 replicates"):
        rs.cmf_resample_summary(reps, ref, weights[:3])
    with pytest.raises(ValueError, match="at least one"):
        rs.cmf_resample_summary([], ref, weights)


def test_heldout_scores_project_on_the_model_of_the_kept_matrices(monkeypatch):
    ref, reps, weights, (A, P, Delta, C) = _replicates(np.random.RandomState(1))
    rng = np.random.RandomState(2)
    mats = [(p @ Delta * a) @ C.T + 0.01 * rng.standard_normal((6, 5)) for p, a in zip(P, A)]
    seen = []

    class Proj:
        slab_sse, slab_norm = np.array([0.5]), np.array([2.0])

    def fake(matrices, model, **kw):
        seen.append((matrices, model, kw))
        return Proj

    import matcouply_amd.projection as projection

    monkeypatch.setattr(projection, "parafac2_project", fake)
    out = rs.parafac2_aoadmm_heldout_sse(mats, reps, weights, n_iter_max=7)
    assert [h.indices.tolist() for h in out] == [[0], [1], [2], [3], [0]] and out[0].slab_sse[0] == 0.5
    matrices, model, kw = seen[1]
    assert matrices[0] is mats[1] and kw == dict(n_iter_max=7)
    assert model[0] is None and model[1][0].shape == (3, 2) and len(model[1][1]) == 3 and model[1][0].all()  # no zero rows
    # a result whose B_i^T B_i differ is not a PARAFAC2 fit
    loose = dec.CoupledMatrixFactorization((None, (A, [rng.standard_normal((6, 2)) for _ in range(4)], C)))
    with pytest.raises(ValueError, match="does not come from a PARAFAC2 fit"):
        rs.parafac2_aoadmm_heldout_sse(mats, [loose], np.array([[1.0, 1, 0, 1]]))
    with pytest.raises(ValueError, match="rows for 5 replicates"):
        rs.parafac2_aoadmm_heldout_sse(mats, reps, weights[:2])


def test_heldout_scores_on_the_host_projection():
    ref, reps, weights, (A, P, Delta, C) = _replicates(np.random.RandomState(3))
    mats = [((p @ Delta) * a) @ C.T for p, a in zip(P, A)]
    out = rs.parafac2_aoadmm_heldout_sse(mats, reps, weights, method="host")
    for h in out:  # noise-free data of the very model: the left-out matrix is reproduced
        assert (h.slab_sse <= 1e-6 * h.slab_norm).all() and len(h.indices) == 1


# ---- exports and the C entry -------------------------------------------------------------------------------------------------
def test_exports():
    for name in ("cmf_aoadmm_resample", "parafac2_aoadmm_resample", "cmf_resample_summary", "parafac2_aoadmm_heldout_sse"):
        assert name in rs.__all__ and getattr(matcouply_amd, name) is getattr(rs, name)
    for name in ("mcl_multistart_weighted_workspace_bytes", "mcl_multistart_run_weighted"):
        assert name in _engine.EXPORTED_SYMBOLS and hasattr(_engine.load_library(), name)
    assert _engine.load_library().mcl_version() == 410


def _weighted_call(weights, n_jobs=2, I=3, null_weights=False):
    lib = _engine.load_library()
    row_ptr = np.array([0, 4, 9, 12], dtype=np.int64)
    rp = row_ptr.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
    opt = _engine.MultistartOptions()
    opt.n_iter_max, opt.inner_n_iter_max, opt.update_A, opt.update_B, opt.update_C = 3, 5, 1, 1, 1
    w = np.ascontiguousarray(weights, dtype=np.float64)
    fake = ctypes.c_void_p(256)  # never dereferenced: every refusal comes before any device call
    rc = lib.mcl_multistart_run_weighted(fake, 0, rp, I, 5, 2, ctypes.byref(opt), n_jobs, None if null_weights else w.ctypes.data,
                                         fake, fake, fake, fake, fake, 0, None)
    return rc, lib.mcl_multistart_last_error().decode()


def test_the_c_entry_refuses_bad_weights_before_any_launch():
    ones = np.ones((2, 3))
    for bad, text in ((None, "NULL slab_weights"), (-ones, "negative or not finite"), (ones * np.nan, "negative or not finite"),
                      (ones * np.inf, "negative or not finite"), (np.array([[1.0, 0, 2], [0, 0, 0]]), "job 1 has no positive weight")):
        rc, msg = _weighted_call(ones if bad is None else bad, null_weights=bad is None)
        assert rc != 0 and msg.startswith("mcl_multistart_run_weighted: ") and text in msg, msg
    rc, msg = _weighted_call(ones)  # good weights: the next refusal is the workspace's
    assert rc != 0 and "mcl_multistart_weighted_workspace_bytes" in msg
    lib = _engine.load_library()
    row_ptr = np.array([0, 4, 9, 12], dtype=np.int64)
    rp = row_ptr.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
    opt = _engine.MultistartOptions()
    plain = lib.mcl_multistart_workspace_bytes(rp, 3, 5, 2, ctypes.byref(opt), 2)
    assert lib.mcl_multistart_weighted_workspace_bytes(rp, 3, 5, 2, ctypes.byref(opt), 2) == plain + 256
    assert lib.mcl_multistart_weighted_workspace_bytes(rp, 3, 5, 17, ctypes.byref(opt), 2) == -1
