"""GeneralizedL2Penalty and UnitSimplex against golden vectors of the reference
(tests/golden/more_penalties.npz, oracle/tools/gen_golden.py --only more): the oracle's restatement, the product's
host prox methods on NumPy arrays and torch tensors, and (-m gpu) a 10-iteration trajectory through the solver, where
both penalties are evaluated on device tensors between the library's solve steps."""
import json

import numpy as np
import pytest

from oracle import aoadmm_oracle as orc
from tests.helpers import load_npz, rel_err, split_rows


def _descs(arrs):
    out = []
    for d in json.loads(str(arrs["manifest"])):
        d = dict(d)
        if d["kind"] == "gl2":
            d["norm_matrix"] = arrs[d["norm_matrix"]]
        out.append(d)
    return out


def _make(d, **kw):
    from matcouply_amd import penalties as pen

    return pen.GeneralizedL2Penalty(d["norm_matrix"], **kw) if d["kind"] == "gl2" else pen.UnitSimplex(**kw)


def test_oracle_prox_matches_reference():
    arrs = load_npz("more_penalties.npz")
    Y, row_ptr, rhos = arrs["Y"], arrs["row_ptr"], arrs["rhos"]
    J = int(row_ptr[1])
    for ci, d in enumerate(_descs(arrs)):
        tol = 1e-9 if d["kind"] == "simplex" else 1e-12  # the reference's bisection stops at ~1e-12 of the multiplier
        assert rel_err(orc.prox_matrix(d, Y[:J].copy(), 10.0), arrs[f"p{ci}_single_rho10"]) < tol, d["kind"]
        out = np.concatenate([orc.prox_matrix(d, Y[row_ptr[i]:row_ptr[i + 1]].copy(), rhos[i]) for i in range(len(rhos))])
        assert rel_err(out, arrs[f"p{ci}_list"]) < tol
        assert abs(orc.penalty_value(d, Y[:J]) - float(arrs[f"p{ci}_penalty"])) < 1e-10
        assert abs(orc.penalty_value(d, Y) - float(arrs[f"p{ci}_penalty_list"])) < 1e-10


@pytest.mark.parametrize("backend", ["numpy", "torch"])
def test_host_prox_matches_reference(backend):
    import torch

    arrs = load_npz("more_penalties.npz")
    Y, row_ptr, rhos = arrs["Y"], arrs["row_ptr"], arrs["rhos"]
    J = int(row_ptr[1])
    cast = (lambda a: torch.as_tensor(np.array(a))) if backend == "torch" else (lambda a: np.array(a))
    back = (lambda a: a.numpy()) if backend == "torch" else (lambda a: np.asarray(a))
    for ci, d in enumerate(_descs(arrs)):
        p = _make(d)
        tol = 1e-9 if d["kind"] == "simplex" else 1e-12
        assert rel_err(back(p.factor_matrix_update(cast(Y[:J]), 10.0, None)), arrs[f"p{ci}_single_rho10"]) < tol
        out = p.factor_matrices_update([cast(m) for m in split_rows(Y, row_ptr)], list(rhos), [None] * len(rhos))
        assert rel_err(np.concatenate([back(m) for m in out]), arrs[f"p{ci}_list"]) < tol
        assert abs(float(p.penalty(cast(Y[:J]))) - float(arrs[f"p{ci}_penalty"])) < 1e-10
        assert abs(float(p.penalty([cast(m) for m in split_rows(Y, row_ptr)])) - float(arrs[f"p{ci}_penalty_list"])) < 1e-10
        if d["kind"] == "simplex":
            x = back(p.factor_matrix_update(cast(Y[:J]), 1.0, None))
            assert x.min() >= 0 and np.allclose(x.sum(axis=0), 1.0, atol=1e-12)


def test_generalized_l2_validation():
    from matcouply_amd import penalties as pen

    M = np.array([[2.0, -1.0], [-1.0, 2.0]])
    pen.GeneralizedL2Penalty(M)
    with pytest.raises(ValueError):
        pen.GeneralizedL2Penalty(np.array([[1.0, 0.5], [0.0, 1.0]]))   # not symmetric
    with pytest.raises(ValueError):
        pen.GeneralizedL2Penalty(np.array([[1.0, 2.0], [2.0, 1.0]]))   # indefinite
    pen.GeneralizedL2Penalty(np.array([[1.0, 2.0], [2.0, 1.0]]), validate=False)
    # M = I is the ridge penalty: prox = rho / (rho + 2) x
    x = np.random.RandomState(0).standard_normal((4, 3))
    assert np.allclose(pen.GeneralizedL2Penalty(np.eye(4)).factor_matrix_update(x, 3.0, None), 3.0 / 5.0 * x)


def _traj_state(arrs):
    spec = json.loads(str(arrs["t_spec"]))
    regs = [[dict(d, norm_matrix=arrs[d["norm_matrix"]]) if d["kind"] == "gl2" else d for d in spec["regs"][m]]
            for m in range(3)]
    c1 = load_npz("c1_data.npz")
    aux = [[arrs[f"t_aux_in_m{m}_{s}"] for s in range(len(regs[m]))] for m in range(3)]
    dual = [[arrs[f"t_dual_in_m{m}_{s}"] for s in range(len(regs[m]))] for m in range(3)]
    return orc.OracleState(c1["X"], c1["row_ptr"], arrs["t_A0"], arrs["t_B0"], arrs["t_C0"], regs, aux, dual), spec, regs


def test_oracle_trajectory_matches_reference():
    arrs = load_npz("more_penalties.npz")
    st, spec, regs = _traj_state(arrs)
    res = orc.run(st, spec["n_iter_max"], tol=None, absolute_tol=None)
    assert rel_err(st.A, arrs["t_A"]) < 1e-8 and rel_err(st.B, arrs["t_B"]) < 1e-8 and rel_err(st.C, arrs["t_C"]) < 1e-8
    np.testing.assert_allclose(res["rec_errors"], arrs["t_rec_errors"], rtol=1e-9)
    np.testing.assert_allclose(res["losses"], arrs["t_regularized_loss"], rtol=1e-9)
    for m in range(3):
        for s in range(len(regs[m])):
            assert rel_err(st.aux[m][s], arrs[f"t_aux_m{m}_{s}"]) < 1e-8
            assert rel_err(st.dual[m][s], arrs[f"t_dual_m{m}_{s}"]) < 1e-8


def _forbid_host_prox(monkeypatch):
    """the two penalties must run in their NATIVE kernels (MCL_PEN_GL2 / MCL_PEN_SIMPLEX): their Python prox raises"""
    from matcouply_amd import penalties as pen

    def boom(self, *a, **kw):
        raise AssertionError(f"{type(self).__name__}: the host prox was called - the native kernel did not take the penalty")

    monkeypatch.setattr(pen.GeneralizedL2Penalty, "factor_matrix_update", boom)
    monkeypatch.setattr(pen.UnitSimplex, "factor_matrix_update", boom)
    monkeypatch.setattr(pen.GeneralizedL2Penalty, "_penalty", boom)  # ... and the value comes from mcl_penalty_value


@pytest.mark.gpu
def test_solver_trajectory_matches_reference(kernel_paths, monkeypatch):
    """GeneralizedL2Penalty on the B_i and UnitSimplex on C through cmf_aoadmm on the GPU - native kernels (k_gl2_pass,
    k_slab_simplex; VERDICT r4 #6: no per-slab Python loop, no BLAS call on the solver path), on both arithmetic paths of a
    small problem - vs the reference's own 10-iteration trajectory."""
    from matcouply_amd import decomposition as dec, penalties as pen

    _forbid_host_prox(monkeypatch)

    arrs = load_npz("more_penalties.npz")
    c1 = load_npz("c1_data.npz")
    X, row_ptr = c1["X"], c1["row_ptr"]
    spec = json.loads(str(arrs["t_spec"]))

    def mk(d, m, s):
        aux, dual = arrs[f"t_aux_in_m{m}_{s}"], arrs[f"t_dual_in_m{m}_{s}"]
        kw = dict(aux_init=split_rows(aux, row_ptr) if m == 1 else aux.copy(),
                  dual_init=split_rows(dual, row_ptr) if m == 1 else dual.copy())
        if d["kind"] == "gl2":
            return pen.GeneralizedL2Penalty(arrs[d["norm_matrix"]], **kw)
        if d["kind"] == "simplex":
            return pen.UnitSimplex(**kw)
        return pen.NonNegativity(**kw)

    regs = [[mk(d, m, s) for s, d in enumerate(spec["regs"][m])] for m in range(3)]
    cmf, admm, diag = dec.cmf_aoadmm(
        split_rows(X, row_ptr), spec["rank"], init=(None, (arrs["t_A0"].copy(), split_rows(arrs["t_B0"], row_ptr), arrs["t_C0"].copy())),
        regs=regs, n_iter_max=spec["n_iter_max"], tol=None, absolute_tol=None, return_errors=True, return_admm_vars=True)
    tol = 1e-5  # fp32 engine vs fp64 reference over 10 outer iterations
    assert rel_err(cmf[1][0], arrs["t_A"]) < tol and rel_err(cmf[1][2], arrs["t_C"]) < tol
    assert rel_err(np.concatenate(cmf[1][1]), arrs["t_B"]) < tol
    np.testing.assert_allclose(diag.rec_errors, arrs["t_rec_errors"], rtol=1e-5)
    np.testing.assert_allclose(diag.regularized_loss, arrs["t_regularized_loss"], rtol=4e-5)
    assert rel_err(admm.auxes[2][0], arrs["t_aux_m2_0"]) < tol
    assert np.allclose(np.sum(admm.auxes[2][0], axis=0), 1.0, atol=1e-5) and np.min(admm.auxes[2][0]) >= 0


@pytest.mark.gpu
@pytest.mark.parametrize("where", ["gl2_on_C_simplex_on_B", "gl2_on_A_simplex_on_A_constant", "simplex_on_C_big_rank"])
def test_native_gl2_and_simplex_on_every_mode(where, kernel_paths, monkeypatch):
    """the native GeneralizedL2 / UnitSimplex kernels on modes 0 (constant feasibility penalty), 1 and 2, two outer iterations
    against the oracle at the flat 1e-5 (both arithmetic paths)"""
    from tests.test_gpu_end_to_end import _compare, _run_both

    _forbid_host_prox(monkeypatch)
    rng = np.random.RandomState(3)
    lap = lambda n: (2 * np.eye(n) - np.eye(n, k=1) - np.eye(n, k=-1)) * 0.3 + 0.05 * np.eye(n)
    if where == "gl2_on_C_simplex_on_B":
        I, J, K, r, kw = 5, np.full(5, 37), 40, 4, {}
        regs = [[{"kind": "nn"}], [{"kind": "simplex"}], [{"kind": "gl2", "norm_matrix": lap(K)}, {"kind": "nn"}]]
    elif where == "gl2_on_A_simplex_on_A_constant":
        I, J, K, r = 9, rng.randint(20, 60, 9), 33, 3
        kw = dict(constant_A=True, constant_B=True)
        regs = [[{"kind": "gl2", "norm_matrix": lap(I)}, {"kind": "simplex"}], [{"kind": "nn"}],
                [{"kind": "l1", "reg_strength": 0.02}]]
    else:
        I, J, K, r, kw = 3, np.array([70, 130, 45]), 200, 24, {}
        regs = [[{"kind": "nn"}], [{"kind": "nn"}], [{"kind": "simplex"}]]
    X, row_ptr = orc.synthetic_problem(I, J, K, r, seed=2, dtype=np.float64)
    X = X.astype(np.float32).astype(np.float64)
    st = orc.random_state_for(X, row_ptr, r, regs, seed=5, **kw)
    cmf, admm, diag, res = _run_both(st, 2)
    errs = _compare(cmf, admm, diag, st, res, 1e-5, 1e-5)
    print(where, kernel_paths, {k: f"{v:.1e}" for k, v in errs.items()})


@pytest.mark.gpu
def test_generalized_l2_keyword():
    from matcouply_amd import decomposition as dec
    from matcouply_amd import penalties as pen

    c1 = load_npz("c1_data.npz")
    mats = split_rows(c1["X"], c1["row_ptr"])
    K = mats[0].shape[1]
    M = 2 * np.eye(K) - np.eye(K, k=1) - np.eye(K, k=-1)
    cmf, diag = dec.cmf_aoadmm(mats, 3, generalized_l2_penalty={2: 0.1 * M}, non_negative={0: True}, n_iter_max=5,
                               tol=None, absolute_tol=None, return_errors=True, random_state=0)
    assert np.isfinite(diag.regularized_loss).all() and diag.rec_errors[-1] < diag.rec_errors[0]
    with pytest.raises(ValueError):
        pen.GeneralizedL2Penalty(np.ones((3, 4)))


# ---- TotalVariationPenalty: the reference's prox lives in the absent GPL package condat_tv, so the anchor is the
# ---- optimality system of the problem itself (plus a brute-force dual solver on small inputs)
from tests.prox_cases import _tv_kkt  # noqa: E402  (the dual-variable system; shared with the prox-kernel tests)


def _tv_brute(x, lam, iters=20000):
    D = np.diff(np.eye(len(x)), axis=0)
    s = np.zeros(len(x) - 1)
    for _ in range(iters):
        s = np.clip(s + 0.25 * (D @ (x - D.T @ s)), -lam, lam)
    return x - D.T @ s


@pytest.mark.parametrize("impl", ["oracle", "product"])
def test_tv_denoise_is_optimal(impl):
    from matcouply_amd import penalties as pen

    f = orc.tv_denoise_1d if impl == "oracle" else pen.tv_denoise
    rng = np.random.RandomState(0)
    for n in (1, 2, 3, 5, 8, 13, 40, 100):
        for lam in (0.01, 0.1, 0.5, 2.0, 50.0):
            for rep in range(5):
                x = rng.standard_normal(n) * rng.choice([0.1, 1, 5])
                if rep == 0:
                    x = np.round(x)  # ties
                y = f(x, lam)
                if n == 1:
                    assert abs(y[0] - x[0]) < 1e-12
                    continue
                _tv_kkt(x, y, lam)
                if n <= 8 and rep < 2:
                    assert np.abs(y - _tv_brute(x, lam)).max() < 1e-9


def test_tv_penalty_host_methods():
    from matcouply_amd import penalties as pen

    rng = np.random.RandomState(1)
    Y = rng.standard_normal((30, 4))
    d = {"kind": "tv", "reg_strength": 0.3, "l1_strength": 0.1}
    p = pen.TotalVariationPenalty(0.3, l1_strength=0.1)
    assert rel_err(p.factor_matrix_update(Y, 2.5, None), orc.prox_matrix(d, Y, 2.5)) < 1e-13
    assert abs(float(p.penalty(Y)) - orc.penalty_value(d, Y)) < 1e-12
    out = p.factor_matrix_update(Y, 1e-3, None)            # huge lam: every column collapses to its mean, then shrinks
    assert np.allclose(out, out[0:1]) and np.all(np.abs(out) <= np.abs(Y.mean(axis=0)) + 1e-12)
    with pytest.raises(ValueError):
        pen.TotalVariationPenalty(0.0)
    with pytest.raises(ValueError):
        pen.TotalVariationPenalty(1.0, l1_strength=-1)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [1, 2, 0])
def test_tv_phase_vs_oracle(mode):
    """the native TV kernel (one lane per slab column) inside one phase against the oracle"""
    import copy
    import torch
    from tests.helpers import engine_from_oracle_state, to_np

    J = np.array([40, 7, 130, 1, 64, 33])
    X, row_ptr = orc.synthetic_problem(len(J), J, 24, 4, seed=3, dtype=np.float64)
    X = X.astype(np.float32).astype(np.float64)
    tv = {"kind": "tv", "reg_strength": 0.05, "l1_strength": 0.02 if mode == 2 else 0.0}
    regs = [[{"kind": "nn"}], [{"kind": "nn"}], [{"kind": "nn"}]]
    regs[mode] = [tv, {"kind": "nn"}] if mode == 1 else [tv]
    st = orc.random_state_for(X, row_ptr, 4, regs, seed=5)
    st.constant_A = (mode == 0)
    ref = copy.deepcopy(st)
    eng = engine_from_oracle_state(st)
    if mode == 1:
        eng.update_B(); ref.update_B()
        got, want = eng.B, ref.B
    elif mode == 2:
        eng.update_C_local(); eng.update_C_finish(); ref.update_C()
        got, want = eng.C, ref.C
    else:
        eng.update_A(); ref.update_A()
        got, want = eng.A, ref.A
    torch.cuda.synchronize()
    assert rel_err(to_np(got), want) < 1e-5
    assert rel_err(to_np(eng.regs[mode][0].aux), ref.aux[mode][0]) < 1e-5
    assert np.linalg.norm(to_np(eng.regs[mode][0].dual) - ref.dual[mode][0]) / max(np.linalg.norm(ref.dual[mode][0]),
                                                                                 np.linalg.norm(want)) < 1e-5
    eng.close()


@pytest.mark.gpu
def test_tv_trajectory_and_keyword():
    from matcouply_amd import decomposition as dec
    from tests.test_gpu_end_to_end import _compare, _run_both

    J = np.array([60, 25, 90, 41])
    X, row_ptr = orc.synthetic_problem(len(J), J, 32, 3, seed=8, dtype=np.float64)
    X = X.astype(np.float32).astype(np.float64)
    regs = [[{"kind": "nn"}], [{"kind": "tv", "reg_strength": 0.02, "l1_strength": 0.0}, {"kind": "nn"}],
            [{"kind": "tv", "reg_strength": 0.01, "l1_strength": 0.005}]]
    st = orc.random_state_for(X, row_ptr, 3, regs, seed=2)
    cmf, admm, diag, res = _run_both(st, 6)
    _compare(cmf, admm, diag, st, res, 1e-5, tol_rec=1e-5)
    cmf2, d2 = dec.cmf_aoadmm(split_rows(X, row_ptr), 3, tv_penalty={2: 0.01}, l1_penalty={2: 0.005}, non_negative={0: True},
                              n_iter_max=4, tol=None, absolute_tol=None, return_errors=True, random_state=0)
    assert np.isfinite(d2.regularized_loss).all() and d2.rec_errors[-1] < d2.rec_errors[0]


# ---- inner_tol: early exit of the inner ADMM loops (decomposition.py:90-117)
def _inner_tol_state(arrs):
    spec = json.loads(str(arrs["it_spec"]))
    c1 = load_npz("c1_data.npz")
    regs = spec["regs"]
    aux = [[arrs[f"it_aux_in_m{m}_{s}"] for s in range(len(regs[m]))] for m in range(3)]
    dual = [[arrs[f"it_dual_in_m{m}_{s}"] for s in range(len(regs[m]))] for m in range(3)]
    st = orc.OracleState(c1["X"], c1["row_ptr"], arrs["t_A0"], arrs["t_B0"], arrs["t_C0"], regs, aux, dual,
                         inner_n_iter_max=spec["inner_n_iter_max"])
    st.inner_tol = spec["inner_tol"]
    return st, spec


def test_oracle_inner_tol_matches_reference():
    arrs = load_npz("more_penalties.npz")
    st, spec = _inner_tol_state(arrs)
    res = orc.run(st, spec["n_iter_max"], tol=None, absolute_tol=None)
    assert max(st.inner_iters) < spec["inner_n_iter_max"]  # the early exit is actually taken
    assert rel_err(st.A, arrs["it_A"]) < 1e-10 and rel_err(st.B, arrs["it_B"]) < 1e-10 and rel_err(st.C, arrs["it_C"]) < 1e-10
    np.testing.assert_allclose(res["rec_errors"], arrs["it_rec_errors"], rtol=1e-10)
    np.testing.assert_allclose(res["losses"], arrs["it_regularized_loss"], rtol=1e-10)


@pytest.mark.gpu
def test_solver_inner_tol_matches_reference(kernel_paths, monkeypatch):
    """inner_tol > 0 through cmf_aoadmm vs the reference's trajectory: the inner stopping test runs ON THE DEVICE
    (mcl_options.inner_tol: k_inner_check sets a flag the remaining inner launches test) - the host-driven step
    calls are forbidden here, so no inner iteration synchronises with the host.  The exit decisions compare quantities far
    from their thresholds on this problem, so fp32 takes the same exits."""
    from matcouply_amd import _engine, decomposition as dec
    from tests.test_host_api import make_penalty

    def boom(self, *a, **kw):
        raise AssertionError("a host-driven step call was made: the inner stopping test did not run on the device")

    for name in ("B_solve", "A_solve", "C_solve", "B_prox_local"):
        monkeypatch.setattr(_engine.HipEngine, name, boom)

    arrs = load_npz("more_penalties.npz")
    spec = json.loads(str(arrs["it_spec"]))
    c1 = load_npz("c1_data.npz")
    X, rp = c1["X"], c1["row_ptr"]
    regs = [[make_penalty(d, aux_init=(split_rows(arrs[f"it_aux_in_m{m}_{s}"], rp) if m == 1 else arrs[f"it_aux_in_m{m}_{s}"].copy()),
                          dual_init=(split_rows(arrs[f"it_dual_in_m{m}_{s}"], rp) if m == 1 else arrs[f"it_dual_in_m{m}_{s}"].copy()))
             for s, d in enumerate(spec["regs"][m])] for m in range(3)]
    cmf, admm, diag = dec.cmf_aoadmm(
        split_rows(X, rp), spec["rank"], init=(None, (arrs["t_A0"].copy(), split_rows(arrs["t_B0"], rp), arrs["t_C0"].copy())),
        regs=regs, n_iter_max=spec["n_iter_max"], tol=None, absolute_tol=None, inner_tol=spec["inner_tol"],
        inner_n_iter_max=spec["inner_n_iter_max"], return_errors=True, return_admm_vars=True)
    tol = 1e-5
    assert rel_err(cmf[1][0], arrs["it_A"]) < tol and rel_err(cmf[1][2], arrs["it_C"]) < tol
    assert rel_err(np.concatenate(cmf[1][1]), arrs["it_B"]) < tol
    np.testing.assert_allclose(diag.rec_errors, arrs["it_rec_errors"], rtol=1e-5)
    np.testing.assert_allclose(diag.regularized_loss, arrs["it_regularized_loss"], rtol=2e-5)


@pytest.mark.gpu
@pytest.mark.parametrize("stack", ["pf2_ball", "uni_tv_constant", "rowsep", "stale_partials"])
def test_device_inner_tol_on_generic_stacks(stack, kernel_paths):
    """the device-side inner stopping test with slab-wise penalties in the loop (PARAFAC2 + L2 ball; unimodality + total
    variation with matrix penalties on A under a constant feasibility penalty; row-separable stacks with per-row rho on A):
    three outer iterations against the oracle, which takes the reference's exits (decomposition.py:90-117)"""
    from tests.test_gpu_end_to_end import _compare, _run_both

    rng = np.random.RandomState(11)
    if stack == "pf2_ball":
        I, J, K, r, kw = 6, rng.randint(30, 80, 6), 48, 4, {}
        regs = [[{"kind": "nn"}], [{"kind": "parafac2"}, {"kind": "l2ball", "norm_bound": 1.5}], [{"kind": "l1", "reg_strength": 0.02}]]
    elif stack == "uni_tv_constant":
        I, J, K, r, kw = 8, rng.randint(30, 80, 8), 40, 3, dict(constant_A=True, constant_B=True)
        regs = [[{"kind": "l2ball", "norm_bound": 2.0, "non_negativity": True}], [{"kind": "unimodal", "non_negativity": True}],
                [{"kind": "tv", "reg_strength": 0.01, "l1_strength": 0.0}]]
    elif stack == "stale_partials":
        # tiles of fewer than 64 rows leave row-less workgroups in the fp64 solve pass, whose entries of the shared
        # table of ||x - x_old||^2 partials used to keep another phase's values.  K = 37 and J_i <= 60 (no multiple of 64),
        # rank 4 (16 rows per workgroup) and B on 1e3 times the scale of C: a stale B-phase partial in the C-phase's sum would
        # keep the C loop running where the reference (decomposition.py:100-107) stops.
        I, J, K, r, kw = 5, np.array([60, 23, 37, 5, 49]), 37, 4, {}
        regs = [[{"kind": "nn"}], [{"kind": "l2ball", "norm_bound": 40.0}], [{"kind": "l2ball", "norm_bound": 0.5}]]
    else:
        I, J, K, r, kw = 7, rng.randint(30, 80, 7), 64, 5, {}
        regs = [[{"kind": "l1", "reg_strength": 0.05}, {"kind": "nn"}], [{"kind": "nn"}], [{"kind": "box", "min_val": 0.0, "max_val": 0.9}]]
    X, row_ptr = orc.synthetic_problem(I, J, K, r, seed=4, dtype=np.float64)
    X = X.astype(np.float32).astype(np.float64)
    st = orc.random_state_for(X, row_ptr, r, regs, seed=8, inner_n_iter_max=15, **kw)
    if stack == "stale_partials":
        st.B *= 30.0
        st.aux[1][0] *= 30.0
        st.C *= 0.03
        st.aux[2][0] *= 0.03
    st.inner_tol = 5e-2
    cmf, admm, diag, res = _run_both(st, 3, inner_tol=5e-2)
    assert min(st.inner_iters) < 15, st.inner_iters  # an early exit is actually taken somewhere
    errs = _compare(cmf, admm, diag, st, res, 1e-5, 1e-5)
    print(stack, kernel_paths, "inner iterations taken (oracle):", st.inner_iters, {k: f"{v:.1e}" for k, v in errs.items()})
