"""CPU: parafac2_project with method="host" against the restatement of tests/projection_restatement.py on every fixture of the
GPU tests, exact recovery without noise, the well-posedness of those fixtures under the float32 rounding of W, the forms of
`model`, the weights, the argument checks, the refusals of the device form (no device call is made here) and its C ABI."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch

import matcouply_amd
from matcouply_amd import _engine, projection as pj
from matcouply_amd.coupled_matrices import CoupledMatrixFactorization
from tests import projection_restatement as R
from tests.test_evaluation_host import no_device  # noqa: F401  (the fixture)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-9
MODES = {"three": dict(n_iter_max=3, tol=0.0), "converged": {}}
CASES = [(rank, K) for rank in R.RANKS for K in R.columns_of(rank, device=True)]  # the fixtures of the GPU tests
K_BELOW_RANK = [(rank, K) for rank in R.RANKS for K in R.columns_of(rank) if K < rank]


@pytest.fixture
def no_projection_device(no_device, monkeypatch):  # noqa: F811
    def refuse(*args, **kwargs):
        raise AssertionError("the device was touched")

    monkeypatch.setattr(_engine, "pf2_project", refuse)
    monkeypatch.setattr(pj, "_device_present", lambda: True)  # "auto" would take the device where it serves the call


def _rel(got, want):
    return np.linalg.norm(np.asarray(got, dtype=np.float64) - want) / max(np.linalg.norm(want), 1e-300)


@functools.lru_cache(maxsize=None)
def _reference(rank, K, noise, mode):
    f = R.parity_fixture(rank, K, noise)
    return f, R.project(f["Xs"], f["Delta"], f["C"], np.ones(rank), **MODES[mode])


def _assert_equals_reference(got, want, tol, n_iter=True):
    A, B_is = got.cmf[1][0], got.cmf[1][1]
    for i, w in enumerate(want):
        assert _rel(A[i], w["a"]) <= tol and _rel(B_is[i], w["B"]) <= tol and _rel(got.projections[i], w["P"]) <= tol, i
        assert abs(got.slab_sse[i] - w["sse"]) <= tol * w["nx"] and abs(got.slab_norm[i] - w["nx"]) <= tol * w["nx"], i
        k = w["n_iter"] if n_iter else min(w["n_iter"], got.n_iter[i])  # (not n_iter: the common part of the e2 sequences)
        assert np.abs(got.errors[i, :k] - w["errors"][:k]).max() <= tol and np.isnan(got.errors[i, got.n_iter[i]:]).all(), i
        if n_iter:
            assert got.n_iter[i] == k, i


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("rank,K", CASES)
def test_host_against_the_restatement(rank, K, mode):
    f, want = _reference(rank, K, 0.3, mode)
    got = pj.parafac2_project(f["Xs"], (f["Delta"], f["C"]), a_init=np.ones(rank), method="host", return_errors=True, **MODES[mode])
    assert got._fields == ("cmf", "projections", "slab_sse", "slab_norm", "n_iter", "errors")
    assert isinstance(got.cmf, CoupledMatrixFactorization) and got.errors.shape == (len(f["Xs"]), MODES[mode].get("n_iter_max", 100))
    # (at rank 1 the first iteration is already the minimiser, and with tol = 0 the stop at t = 2 hangs on the last bit of e2)
    _assert_equals_reference(got, want, TOL, n_iter=not (rank == 1 and mode == "three"))
    for P_i in got.projections:
        assert np.abs(P_i.T @ P_i - np.eye(rank)).max() <= 1e-12


@pytest.mark.parametrize("rank,K", K_BELOW_RANK)
def test_host_with_K_below_the_rank_returns_the_partial_isometry(rank, K):
    # W = X C has rank K: Q loses rank - K eigenvalues, P^T P is a projector of rank K, a is still determined.  Three iterations:
    # these are not fixtures of the GPU tests (the device refuses K < rank), and over a long run the under-determined polar step
    # amplifies the last bits (rank 32, K 9 to the default stop: 100 iterations, 3.7e-8 between the two routes)
    f, want = _reference(rank, K, 0.3, "three")
    assert K_BELOW_RANK == [(16, 9), (17, 9), (17, 16), (32, 9), (32, 16)]
    got = pj.parafac2_project(f["Xs"], (f["Delta"], f["C"]), a_init=np.ones(rank), method="host", return_errors=True, **MODES["three"])
    _assert_equals_reference(got, want, TOL)  # (slab_sse against the residual itself)
    for P_i in got.projections:
        sv = np.linalg.svd(P_i, compute_uv=False)
        assert np.abs(sv[:K] - 1.0).max() <= 1e-9 and sv[K:].max() <= 1e-9


@pytest.mark.parametrize("tol", sorted(R.STOP_SEEDS))
def test_host_against_the_restatement_on_the_stopping_fixtures(tol):
    f = R.stopping_fixture(tol)
    want = R.project(f["Xs"], f["Delta"], f["C"], np.ones(3), tol=tol)
    assert len({w["n_iter"] for w in want}) >= 4  # the matrices stop at different iterations
    for w in want:  # ... each at least 10 % away from the tolerance on both sides
        assert w["criteria"][-1] <= 0.9 * tol and (w["n_iter"] == 2 or w["criteria"][-2] >= 1.1 * tol) and w["n_iter"] < 100
    got = pj.parafac2_project(f["Xs"], (f["Delta"], f["C"]), a_init=np.ones(3), tol=tol, method="host", return_errors=True)
    _assert_equals_reference(got, want, TOL)


@pytest.mark.parametrize("rank,K", CASES)
def test_exact_recovery_without_noise_from_ones(rank, K):
    f = R.parity_fixture(rank, K, 0.0)
    got = pj.parafac2_project(f["Xs"], (f["Delta"], f["C"]), a_init=np.ones(rank), method="host")
    assert not hasattr(got, "errors") and isinstance(got, pj.Projection)
    for i, B_i in enumerate(got.cmf[1][1]):
        assert _rel(got.cmf[1][0][i], f["a_true"][i]) < 1e-5 and _rel(B_i, f["P_true"][i] @ f["Delta"]) < 1e-5, i
    assert got.n_iter.max() <= 21 and (got.slab_sse <= 1e-12 * got.slab_norm).all()


def _fixtures_of_the_gpu_tests():
    for rank, K in CASES:
        for mode in sorted(MODES):
            yield R.parity_fixture(rank, K, 0.3), rank, MODES[mode]
    for tol in sorted(R.STOP_SEEDS):
        yield R.stopping_fixture(tol), 3, dict(tol=tol)


def test_the_gpu_fixtures_are_well_posed_under_the_float32_rounding_of_W():
    worst = 0.0
    for f, rank, options in _fixtures_of_the_gpu_tests():
        model, data = pj._FixedModel((f["Delta"], f["C"])), pj._Data(f["Xs"])
        args = (model, data, pj._start(np.ones(rank), model, data.I), options.get("n_iter_max", 100), options.get("tol", 1e-8), 1e-13)
        A64, B64, _, sse64, nx, _, _ = pj._host_project(*args)
        A32, B32, _, sse32, _, _, _ = pj._host_project(*args, w_dtype=np.float32)
        for i in range(data.I):
            lo, hi = data.row_ptr[i], data.row_ptr[i + 1]
            worst = max(worst, _rel(A32[i], A64[i]), _rel(B32[lo:hi], B64[lo:hi]), abs(sse32[i] - sse64[i]) / nx[i])
    print(f"largest change of a, B_new, e2 under the rounding: {worst:.2e}")
    assert worst < 1e-6


def _model_forms(rank=3, K=9, seed=4):
    """one Delta-invariant model in the three forms of `model`, and new matrices"""
    f = R.fixture(seed, [5, 7, 12, 30], K, rank)
    rng = np.random.RandomState(seed)
    A = rng.uniform(0.5, 1.5, (6, rank))
    P_fit = [np.linalg.qr(rng.standard_normal((rank + 2 + i, rank)))[0] for i in range(6)]
    als = (None, (A, f["Delta"], f["C"]), P_fit)
    aoadmm = (None, (A, [P_i @ f["Delta"] for P_i in P_fit], f["C"]))
    tall = np.linalg.qr(rng.standard_normal((rank + 5, rank)))[0] @ f["Delta"]
    return f, A, [als, aoadmm, CoupledMatrixFactorization(aoadmm), (f["Delta"], f["C"]), (tall, f["C"])]


def test_the_forms_of_model_give_the_same_result():
    f, A, forms = _model_forms()
    outs = [pj.parafac2_project(f["Xs"], m, a_init=A.mean(0), method="host", return_errors=True) for m in forms]
    # another square root of Delta^T Delta turns P, nothing else; every root is rounded to float32 on its own (6e-8 relative),
    # which the conditioning of the fixture (kappa 2 for Delta and C, a in [0.5, 1.5]) amplifies by less than 100
    for out in outs[1:]:
        assert _rel(out.cmf[1][0], outs[0].cmf[1][0]) <= 6e-6
        assert all(_rel(B_i, B_0) <= 6e-6 for B_i, B_0 in zip(out.cmf[1][1], outs[0].cmf[1][1]))
        assert np.abs(out.slab_sse - outs[0].slab_sse).max() <= 6e-6 * out.slab_norm.max()
    # the default start: the column means of A for the models that have one, ones for the pairs
    for m, start in zip(forms, [A.mean(0)] * 3 + [np.ones(3)] * 2):
        got, want = pj.parafac2_project(f["Xs"], m, method="host"), pj.parafac2_project(f["Xs"], m, a_init=start, method="host")
        assert np.array_equal(got.cmf[1][0], want.cmf[1][0])
    # Delta of the first form is used as it is, in float32; a list of torch tensors gives torch tensors of its dtype
    got = pj.parafac2_project([torch.from_numpy(X).float() for X in f["Xs"]], forms[0], method="host")
    assert all(t.dtype == torch.float32 for t in [got.cmf[1][0], got.cmf[1][2]] + got.cmf[1][1] + got.projections)
    assert _rel(got.cmf[1][0].numpy(), outs[0].cmf[1][0]) <= 1e-6 and got.slab_sse.dtype == np.float64
    with pytest.raises(ValueError, match="not positive definite"):
        pj.parafac2_project(f["Xs"], (None, (A, [np.ones((4, 3))] * 6, f["C"])), method="host")
    with pytest.raises(TypeError):
        pj.parafac2_project(f["Xs"], 3, method="host")


def test_weights_fold_into_the_start_only():
    f, A, forms = _model_forms()
    w = np.array([2.0, 0.5, 3.0])
    _, factors, P_fit = forms[0]
    weighted, folded = (w, factors, P_fit), (None, (A * w, factors[1], factors[2]), P_fit)
    a, b = pj.parafac2_project(f["Xs"], weighted, method="host"), pj.parafac2_project(f["Xs"], folded, method="host")
    assert np.array_equal(a.cmf[1][0], b.cmf[1][0]) and all(np.array_equal(x, y) for x, y in zip(a.projections, b.projections))
    start = np.full((4, 3), 0.7)
    a, b = (pj.parafac2_project(f["Xs"], m, a_init=start, method="host") for m in (weighted, forms[0]))
    assert np.array_equal(a.cmf[1][0], b.cmf[1][0]) and a.cmf.weights is None


def test_argument_checks():
    f, A, forms = _model_forms()
    model, Xs = forms[3], f["Xs"]
    with pytest.raises(ValueError, match="method"):
        pj.parafac2_project(Xs, model, method="gpu")
    for bad in (0, -1, 2.5, True):
        with pytest.raises(ValueError, match="n_iter_max"):
            pj.parafac2_project(Xs, model, n_iter_max=bad, method="host")
    with pytest.raises(ValueError, match="negative"):
        pj.parafac2_project(Xs, model, tol=-1e-8, method="host")
    with pytest.raises(ValueError, match="negative"):
        pj.parafac2_project(Xs, model, absolute_tol=-1.0, method="host")
    with pytest.raises(ValueError, match="shape mismatch"):
        pj.parafac2_project([X[:, :-1] for X in Xs], model, method="host")
    with pytest.raises(ValueError, match="same number of columns"):
        pj.parafac2_project([Xs[0][:, :-1]] + Xs[1:], model, method="host")
    with pytest.raises(ValueError, match="shape mismatch"):
        pj.parafac2_project(Xs, model, a_init=np.ones(4), method="host")
    with pytest.raises(ValueError, match="shape mismatch"):
        pj.parafac2_project(Xs, model, a_init=np.ones((3, 3)), method="host")
    with pytest.raises(ValueError, match="shape mismatch"):
        pj.parafac2_project(Xs, (np.ones((2, 3)), f["C"]), method="host")
    with pytest.raises(ValueError, match="fewer than the rank"):
        pj.parafac2_project([Xs[0][:2]] + Xs[1:], model, method="host")
    with pytest.raises(ValueError, match="no matrix"):
        pj.parafac2_project([], model, method="host")


def test_device_refusals_touch_no_device(no_projection_device):
    wide = R.fixture(0, [40, 41], 35, 33)
    with pytest.raises(NotImplementedError, match="rank 33"):
        pj.parafac2_project(wide["Xs"], (wide["Delta"], wide["C"]), method="device")
    f, A, forms = _model_forms()
    model, Xs = forms[3], f["Xs"]
    with pytest.raises(NotImplementedError, match="fewer than the rank"):
        pj.parafac2_project([Xs[0][:2]] + Xs[1:], model, method="device")
    with pytest.raises(NotImplementedError, match="int64"):
        pj.parafac2_project([X.astype(np.int64) for X in Xs], model, method="device")
    low, want_low = _reference(16, 9, 0.3, "three")
    with pytest.raises(NotImplementedError, match="K = 9 is below the rank 16"):
        pj.parafac2_project(low["Xs"], (low["Delta"], low["C"]), method="device")
    got = pj.parafac2_project(low["Xs"] * 2, (low["Delta"], low["C"]), a_init=np.ones(16), **MODES["three"])  # "auto": the host
    assert all(_rel(got.cmf[1][0][i], w["a"]) <= TOL for i, w in enumerate(want_low))
    monkeypatch_rows = pj._Data(Xs)
    monkeypatch_rows.N = _engine.PROJECT_MAX_ROWS  # (a shape only: no such data is built)
    assert "packed rows" in pj._unserved_reason(pj._FixedModel(model), monkeypatch_rows, np.ones((4, 3)))
    for name, bad in (("Delta", (np.where(np.eye(3) > 0, np.inf, f["Delta"]), f["C"])), ("C", (f["Delta"], np.where(f["C"] > 9, 0, np.nan)))):
        with pytest.raises(NotImplementedError, match=name + " holds a non-finite"):
            pj.parafac2_project(Xs, bad, method="device")
    with pytest.raises(NotImplementedError, match="a_init holds a non-finite"):
        pj.parafac2_project(Xs, model, a_init=np.array([1.0, np.inf, 1.0]), method="device")
    # "auto" takes the host for what the device does not serve
    got = pj.parafac2_project(wide["Xs"], (wide["Delta"], wide["C"]), a_init=np.ones(33), n_iter_max=2)
    want = R.project(wide["Xs"], wide["Delta"], wide["C"], np.ones(33), n_iter_max=2)
    assert all(_rel(got.cmf[1][0][i], w["a"]) <= TOL for i, w in enumerate(want))
    with pytest.raises(ValueError, match="fewer than the rank"):  # ... and the host has no P for these either
        pj.parafac2_project([Xs[0][:2]] + Xs[1:], model)


def test_auto_takes_the_host_without_a_device(monkeypatch):
    def refuse(*args, **kwargs):
        raise AssertionError("the device was touched")

    monkeypatch.setattr(pj, "_device_present", lambda: False)
    monkeypatch.setattr(_engine, "pf2_project", refuse)
    f, want = _reference(3, 9, 0.3, "three")
    got = pj.parafac2_project(f["Xs"], (f["Delta"], f["C"]), a_init=np.ones(3), return_errors=True, **MODES["three"])
    _assert_equals_reference(got, want, TOL)


def test_names_are_exported_from_the_package():
    for name in ("parafac2_project", "Projection"):
        assert getattr(matcouply_amd, name) is getattr(pj, name) and name in pj.__all__
    assert matcouply_amd.projection is pj


# ---- the C ABI of the device form: header, binding and library agree -------------------------------------------------------
SYMBOLS = ("mcl_pf2_project_workspace_bytes", "mcl_pf2_project_typed", "mcl_pf2_project_last_error")
CTYPE_OF = {"int64_t": "c_long", "int32_t": "c_int", "int": "c_int", "double": "c_double", "const double *": "c_void_p",
            "double *": "c_void_p", "float *": "c_void_p", "int32_t *": "c_void_p", "void *": "c_void_p", "const void *": "c_void_p",
            "const int64_t *": "LP_c_long", "const char *": "c_char_p"}


def _declaration(name):
    text = open(os.path.join(REPO, "include", "matcouply_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"([\w ]+?\*?)\s*\b" + name + r"\s*\(([^)]*)\)\s*;", text)
    assert m, f"{name} is not declared in include/matcouply_hip.h"
    args = [] if m.group(2).strip() == "void" else [re.sub(r"\s*\w+$", "", a.strip()).strip() for a in m.group(2).split(",")]
    return m.group(1).strip(), args


@pytest.mark.parametrize("name", SYMBOLS)
def test_header_binding_and_library_agree_on_the_projection_symbols(name):
    assert name in _engine.EXPORTED_SYMBOLS
    fn = getattr(_engine.load_library(), name)
    result, args = _declaration(name)
    assert CTYPE_OF[result] == fn.restype.__name__
    assert [CTYPE_OF[a] for a in args] == [t.__name__ for t in fn.argtypes]


def test_projection_argument_lists_are_the_documented_ones():
    assert _declaration("mcl_pf2_project_workspace_bytes") == ("int64_t", ["const int64_t *", "int64_t", "int64_t", "int32_t"])
    assert _declaration("mcl_pf2_project_typed") == ("int", [
        "const void *", "int32_t", "const int64_t *", "int64_t", "int64_t", "int32_t", "const double *", "const double *", "const double *",
        "int32_t", "double", "double", "double *", "float *", "float *", "double *", "int32_t *", "double *", "void *", "int64_t", "void *"])
    assert _declaration("mcl_pf2_project_last_error") == ("const char *", [])
    assert _engine.MCL_ABI_VERSION == 410 and _engine.load_library().mcl_version() == 410 and _engine.PROJECT_MAX_RANK == 32


def test_projection_entry_refuses_bad_arguments_without_a_device():
    # these checks come before any HIP call, so they are the same on a machine without a device
    lib = _engine.load_library()
    rp = lambda a: np.ascontiguousarray(a, dtype=np.int64).ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
    good = rp([0, 3, 70, 75])
    size = lib.mcl_pf2_project_workspace_bytes
    assert size(good, 3, 5, 0) == -1 and size(good, 3, 5, 33) == -1 and size(good, 3, 5, 4) == -1 and size(rp([1, 3, 70, 75]), 3, 5, 3) == -1
    assert size(good, 3, 2, 3) == -1  # K < rank
    assert size(good, 0, 5, 3) == -1 and size(good, 3, 0, 3) == -1 and size(None, 3, 5, 3) == -1
    # 4 segments (3 + 64 + 3 + 5 rows), the fragments of one 64-column chunk at rank <= 16, H, Delta, W [75, 3] fp32 and T, T Delta
    # [3, 2, 3, 3] fp64; every part rounded up to 256 bytes
    al = lambda b: (b + 255) // 256 * 256
    want = al(4 * 16) + al(4 * 4) + al(4 * 64 * 4 * 4) + 2 * al(9 * 8) + al(75 * 3 * 4) + al(3 * 2 * 9 * 8)
    assert size(good, 3, 5, 3) == want
    fake = 256  # never dereferenced: every call below is refused first
    good_args = dict(X=fake, xt=0, rp=good, I=3, K=5, r=3, Delta=fake, C=fake, a_init=fake, n_iter_max=10, tol=1e-8, absolute_tol=1e-13,
                     A=fake, B=fake, P=fake, stats=fake, n_iter=fake, errors=None, ws=fake, ws_bytes=want, stream=None)
    call = lambda **kw: lib.mcl_pf2_project_typed(*{**good_args, **kw}.values())
    for change, message in [(dict(r=0), b"rank 0"), (dict(r=33), b"rank 33"), (dict(r=4), b"at least rank rows"), (dict(I=0), b"I >= 1"),
                            (dict(K=2), b"rank 3 exceeds K = 2"),
                            (dict(rp=rp([1, 3, 70, 75])), b"row_ptr[0]"), (dict(xt=7), b"x_type"), (dict(n_iter_max=0), b"n_iter_max >= 1"),
                            (dict(tol=-1.0), b"tol >= 0"), (dict(tol=float("nan")), b"tol >= 0"), (dict(absolute_tol=-1.0), b"absolute_tol >= 0"),
                            (dict(ws_bytes=want - 1), b"workspace too small"), (dict(ws=fake + 8), b"aligned")] + [
                               (dict([(name, None)]), b"NULL") for name in ("X", "Delta", "C", "a_init", "A", "B", "P", "stats", "n_iter", "ws")]:
        assert call(**change) != 0, change
        assert message in lib.mcl_pf2_project_last_error(), (change, lib.mcl_pf2_project_last_error())
        assert lib.mcl_pf2_project_last_error().startswith(b"mcl_pf2_project: ")


def test_auto_takes_the_host_for_a_few_matrices_on_the_host(no_projection_device):
    f, A, forms = _model_forms()  # four matrices, a device "present": below the measured crossover of eight
    assert len(f["Xs"]) < pj._AUTO_MIN_MATRICES == 8
    got, want = pj.parafac2_project(f["Xs"], forms[3]), pj.parafac2_project(f["Xs"], forms[3], method="host")
    assert np.array_equal(got.cmf[1][0], want.cmf[1][0])
    with pytest.raises(AssertionError, match="the device was touched"):  # eight matrices go to the device
        pj.parafac2_project(f["Xs"] * 2, forms[3])
