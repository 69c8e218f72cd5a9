"""CPU: resampling over the matrices of a PARAFAC2-ALS fit (matcouply_amd/resampling.py) - the weights of the schemes, the
scaling identity the fused kernel rests on (in the fp64 restatement), every refusal of parafac2_als_resample before anything
touches a device, the sequential path's packing, resample_summary on constructed replicates, and the layout of the scale array."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from matcouply_amd import _engine, decomposition as dec, resampling as rs  # noqa: E402
from tests import parafac2_als_restatement as R  # noqa: E402
from tests.oracle_engine import OracleEngineFactory  # noqa: E402


@pytest.fixture
def no_device(monkeypatch):
    def refuse(*args, **kwargs):
        raise AssertionError("the device was touched")

    monkeypatch.setattr(dec, "_device", refuse)
    monkeypatch.setattr(_engine, "pf2als_multistart_run_weighted", refuse)
    monkeypatch.setattr(_engine, "pf2als_multistart_run", refuse)
    monkeypatch.setattr(_engine, "parafac2_als", refuse)


def _mats(shapes=((5, 10), (8, 10), (6, 10)), seed=0):
    rng = np.random.RandomState(seed)
    return [rng.random_sample(s) for s in shapes]


def test_exported():
    import matcouply_amd

    for name in ("resampling_weights", "parafac2_als_resample", "resample_summary", "resample_heldout_sse"):
        assert name in rs.__all__ and getattr(matcouply_amd, name) is getattr(rs, name)


# ---- resampling_weights --------------------------------------------------------------------------------------------------------
def test_bootstrap_rows_are_counts_that_sum_to_I():
    w = rs.resampling_weights(11, "bootstrap", n=40, random_state=3)
    assert w.dtype == np.float64 and w.shape == (40, 11)
    assert np.array_equal(w, np.round(w)) and (w >= 0).all()
    assert np.array_equal(w.sum(1), np.full(40, 11.0))
    assert len({tuple(row) for row in w}) > 30  # the draws differ
    draws = np.random.RandomState(3).randint(0, 11, size=11)  # the first job: the first I draws of the state
    assert np.array_equal(w[0], np.bincount(draws, minlength=11))


def test_jackknife_rows():
    assert np.array_equal(rs.resampling_weights(4, "jackknife"), np.ones((4, 4)) - np.eye(4))


@pytest.mark.parametrize("I, n", [(10, 5), (11, 3), (7, 7), (9, 2)])
def test_every_index_is_left_out_exactly_once_over_the_folds(I, n):
    w = rs.resampling_weights(I, "kfold", n=n, random_state=0)
    assert w.shape == (n, I) and set(np.unique(w)) == {0.0, 1.0}
    assert np.array_equal((w == 0).sum(0), np.ones(I))
    sizes = (w == 0).sum(1)
    assert sizes.max() - sizes.min() <= 1 and sizes.min() >= 1


@pytest.mark.parametrize("scheme, n", [("bootstrap", 6), ("kfold", 4)])
def test_weights_are_reproducible_from_the_random_state(scheme, n):
    a = rs.resampling_weights(12, scheme, n=n, random_state=5)
    assert np.array_equal(a, rs.resampling_weights(12, scheme, n=n, random_state=5))
    assert np.array_equal(a, rs.resampling_weights(12, scheme, n=n, random_state=np.random.RandomState(5)))
    assert not np.array_equal(a, rs.resampling_weights(12, scheme, n=n, random_state=6))


@pytest.mark.parametrize("args, kw", [
    ((0, "bootstrap"), dict(n=3)), ((2.5, "bootstrap"), dict(n=3)), ((True, "jackknife"), {}),
    ((5, "bootstrap"), {}), ((5, "bootstrap"), dict(n=0)), ((5, "bootstrap"), dict(n=2.0)),
    ((5, "kfold"), {}), ((5, "kfold"), dict(n=6)), ((5, "kfold"), dict(n=0)),
    ((5, "kfold"), dict(n=1)),  # the one fold leaves every matrix out: a row of zeros
    ((1, "jackknife"), {}),     # the one job leaves the one matrix out
    ((5, "jackknife"), dict(n=5)), ((5, "loo"), {}), ((5, None), {}),
])
def test_bad_weight_arguments_are_refused(args, kw):
    with pytest.raises(ValueError):
        rs.resampling_weights(*args, **kw)


# ---- the identity, in the restatement -------------------------------------------------------------------------------------------
COUNTS = np.array([4, 2, 0, 6, 1, 2])  # twice the weights [2, 1, 0, 3, 0.5, 1]: what a list can hold


@pytest.mark.parametrize("n_iter", [3, 50])
@pytest.mark.parametrize("nn_modes", [None, [0], [0, 2]], ids=["als", "nn0", "nn02"])
def test_scaled_matrices_fit_like_the_duplicated_list(nn_modes, n_iter):
    mats = [m.astype(np.float64) for m in R.parafac2_problem(6, (8, 20), 12, 3, seed=2, noise=0.2)[0]]
    A0, B0, C0 = R.start(mats, 3, "random", 0)
    kw = dict(n_iter_max=n_iter, tol=1e-300, absolute_tol=0, nn_modes=nn_modes)
    owner = np.repeat(np.arange(6), COUNTS)  # the list with matrices duplicated, tripled and dropped
    dup = R.parafac2_als([mats[i] for i in owner], 3, factors=(A0[owner], B0, C0), **kw)
    worst = 0.0
    for w in (COUNTS.astype(np.float64), COUNTS / 2.0):  # the counts, and the same problem with every weight halved
        s = np.sqrt(w)
        A, B, C, P, errors, _ = R.parafac2_als([si * m for si, m in zip(s, mats)], 3, factors=(A0 * s[:, None], B0, C0), **kw)
        assert np.array_equal(A[2], np.zeros(3)) and np.array_equal(P[2], np.zeros_like(P[2]))  # exact zeros, no NaN
        assert all(np.isfinite(F).all() for F in (A, B, C, *P, errors))
        keep = s > 0
        A_back = A[keep] / s[keep][:, None]  # halving every weight changes neither the rows divided back nor e_t
        first = [int(np.flatnonzero(owner == i)[0]) for i in np.flatnonzero(keep)]
        diffs = [np.abs(A_back - dup[0][first]).max(), np.abs(B - dup[1]).max(), np.abs(C - dup[2]).max(),
                 max(np.abs(P[i] - dup[3][f]).max() for i, f in zip(np.flatnonzero(keep), first)), np.abs(errors - dup[4]).max()]
        for i in np.flatnonzero(keep):  # every copy of a matrix holds the same row of A
            assert np.ptp(dup[0][owner == i], axis=0).max() < 1e-9
        worst = max(worst, max(diffs))
    print(f"{nn_modes} {n_iter} iterations: scaled against duplicated {worst:.1e}")
    assert worst < 1e-9, worst


# ---- parafac2_als_resample: refusals --------------------------------------------------------------------------------------------
W3 = [[1.0, 2.0, 0.0], [0.5, 1.0, 1.0]]


@pytest.mark.parametrize("method", ["auto", "fused", "sequential"])
@pytest.mark.parametrize("weights, match", [
    ([[1.0, np.nan, 1.0]], "finite"), ([[1.0, np.inf, 1.0]], "finite"), ([[1.0, -0.5, 1.0]], ">= 0"),
    ([1.0, 1.0, 1.0], "shape"), ([[1.0, 1.0]], "shape"), ([[[1.0, 1.0, 1.0]]], "shape"),
    ([[1.0, 1.0, 1.0], [0.0, 0.0, 0.0]], "job 1 has no positive weight"), ([["a", "b", "c"]], "real array"),
])
def test_bad_weights_raise_before_the_device(no_device, method, weights, match):
    with pytest.raises(ValueError, match=match):
        rs.parafac2_als_resample(_mats(), 2, weights, starts=[0] * len(weights), method=method)


@pytest.mark.parametrize("method", ["auto", "fused", "sequential"])
def test_bad_arguments(no_device, method):
    with pytest.raises(TypeError, match="starts"):
        rs.parafac2_als_resample(_mats(), 2, W3, method=method)
    with pytest.raises(TypeError, match="random_state"):
        rs.parafac2_als_resample(_mats(), 2, W3, starts=[0, 1], method=method, random_state=0)
    with pytest.raises(TypeError, match="init"):
        rs.parafac2_als_resample(_mats(), 2, W3, starts=[0, 1], method=method, init="svd")
    with pytest.raises(TypeError, match="n_iter"):
        rs.parafac2_als_resample(_mats(), 2, W3, starts=[0, 1], method=method, n_iter=3)
    with pytest.raises(ValueError, match="3 random states for 2 jobs"):
        rs.parafac2_als_resample(_mats(), 2, W3, starts=[0, 1, 2], method=method)
    with pytest.raises(TypeError, match="starts"):
        rs.parafac2_als_resample(_mats(), 2, W3, starts=7, method=method)
    rng = np.random.RandomState(0)
    with pytest.raises(ValueError, match="start model"):  # A of another problem
        rs.parafac2_als_resample(_mats(), 2, W3, starts=(rng.rand(4, 2), rng.rand(2, 2), rng.rand(10, 2)), method=method)
    with pytest.raises(ValueError, match="non-finite"):
        rs.parafac2_als_resample(_mats(), 2, W3, starts=(np.full((3, 2), np.nan), rng.rand(2, 2), rng.rand(10, 2)), method=method)


def test_bad_method(no_device):
    with pytest.raises(ValueError, match="method"):
        rs.parafac2_als_resample(_mats(), 2, W3, starts=[0, 1], method="parallel")


@pytest.mark.parametrize("method", ["auto", "fused", "sequential"])
@pytest.mark.parametrize("kw, rank, shapes, match", [
    (dict(nn_modes=[1]), 2, None, "mode 1"),
    (dict(svd="randomized_svd"), 2, None, "svd"),
    (dict(normalize_factors=True), 2, None, "normalize_factors"),
    (dict(), 33, ((40, 40), (40, 40), (40, 40)), "32"),
    (dict(), 6, None, "J_i >= rank"),
    (dict(), 4, ((20, 3), (30, 3), (20, 3)), "K >= rank"),
])
def test_parafac2_als_refusals_raise_for_every_method(no_device, method, kw, rank, shapes, match):
    mats = _mats(shapes) if shapes else _mats()
    with pytest.raises(NotImplementedError, match=match):
        rs.parafac2_als_resample(mats, rank, W3, starts=[0, 1], method=method, **kw)


@pytest.mark.parametrize("method", ["auto", "fused", "sequential"])
@pytest.mark.parametrize("kw", [dict(nn_modes=[3]), dict(n_iter_max=0), dict(n_iter_parafac=0)])
def test_bad_values_raise_for_every_method(no_device, method, kw):
    with pytest.raises(ValueError):
        rs.parafac2_als_resample(_mats(), 2, W3, starts=[0, 1], method=method, **kw)


@pytest.mark.parametrize("rank, shapes, match", [
    (17, ((40, 20), (40, 20)), "rank 17"),
    (2, ((600, 500),), "elements"),
])
def test_fused_names_what_its_kernel_does_not_serve(no_device, rank, shapes, match):
    with pytest.raises(NotImplementedError, match=match):
        rs.parafac2_als_resample(_mats(shapes), rank, np.ones((3, len(shapes))), starts=[0, 1, 2], method="fused")


def test_fused_refuses_under_a_substitute_engine(no_device, monkeypatch):
    monkeypatch.setattr(dec, "_ENGINE_FACTORY", OracleEngineFactory())
    with pytest.raises(NotImplementedError, match="substitute"):
        rs.parafac2_als_resample(_mats(), 2, W3, starts=[0, 1], method="fused")


def test_the_servable_call_reaches_the_device(no_device):
    for method in ("auto", "fused", "sequential"):
        with pytest.raises(AssertionError, match="device was touched"):
            rs.parafac2_als_resample(_mats(), 2, W3, starts=[0, 1], method=method)


# ---- the sequential path ---------------------------------------------------------------------------------------------------------
class _FakeSequential:
    """stands in for _engine.parafac2_als: records what it is given and returns the start as the fit"""

    def __init__(self):
        self.calls = []

    def __call__(self, X, row_ptr, rank, start, n_iter_max, n_iter_parafac, tol, absolute_tol, nn_modes):
        self.calls.append(dict(X=X.clone(), row_ptr=np.array(row_ptr), rank=rank, start=start, options=(n_iter_max, n_iter_parafac,
                                                                                                         tol, absolute_tol, nn_modes)))
        A, B, C = (torch.as_tensor(np.asarray(F), dtype=torch.float32) for F in start)
        P = torch.arange(1, X.shape[0] * rank + 1, dtype=torch.float32).reshape(X.shape[0], rank)
        return A, B, C, P, torch.tensor([0.5, 0.25], dtype=torch.float64)


@pytest.mark.parametrize("method", ["auto", "sequential"])
def test_sequential_is_one_fit_per_job_of_the_positive_weight_matrices(monkeypatch, method):
    # rank 17 is above the fused kernel's bound: "auto" takes the sequential path
    fake = _FakeSequential()
    monkeypatch.setattr(dec, "_device", lambda: torch.device("cpu"))
    monkeypatch.setattr(_engine, "parafac2_als", fake)
    monkeypatch.setattr(_engine, "pf2als_multistart_run_weighted", lambda *a, **k: pytest.fail("the fused kernel was called"))
    rank, shapes = 17, ((20, 18), (17, 18), (25, 18), (19, 18))
    mats = _mats(shapes)
    weights = np.array([[2.0, 0.0, 1.0, 0.5], [0.0, 0.0, 3.0, 0.0], [1.0, 1.0, 1.0, 1.0]])
    seeds = [3, 7, 11]
    got = rs.parafac2_als_resample(mats, rank, weights, starts=seeds, method=method, n_iter_max=7, tol=1e-6, nn_modes=[0, 2],
                                   n_iter_parafac=2, return_errors=True)
    assert len(fake.calls) == 3 and len(got) == 3
    for call, w, seed, (result, errors) in zip(fake.calls, weights, seeds, got):
        keep = np.flatnonzero(w > 0)
        assert np.array_equal(call["row_ptr"], np.concatenate([[0], np.cumsum([shapes[i][0] for i in keep])]))
        want = np.concatenate([np.sqrt(w[i]) * mats[i] for i in keep]).astype(np.float32)  # the dropped matrices are not packed
        assert call["X"].dtype == torch.float32 and tuple(call["X"].shape) == want.shape
        np.testing.assert_allclose(call["X"].numpy(), want, rtol=3e-7)
        A0, B0, C0 = dec._pf2als_random_start(4, 18, rank, seed)
        np.testing.assert_array_equal(call["start"][0], A0[keep] * np.sqrt(w[keep])[:, None])
        np.testing.assert_array_equal(call["start"][1], B0)
        np.testing.assert_array_equal(call["start"][2], C0)
        assert call["rank"] == rank and call["options"] == (7, 2, 1e-6, 1e-13, [0, 2])
        (weights_out, (A, B, C), P) = result
        assert weights_out is None and errors == [0.5, 0.25]
        assert A.dtype == np.float64 and A.shape == (4, rank) and [p.shape for p in P] == [(s[0], rank) for s in shapes]
        np.testing.assert_allclose(A[keep], A0[keep], rtol=3e-7)  # the scale is divided back out
        for i in np.flatnonzero(w == 0):  # and the dropped matrices come back as exact zeros
            assert not A[i].any() and not P[i].any()
        np.testing.assert_array_equal(np.concatenate([P[i] for i in keep]).ravel(), np.arange(1, sum(shapes[i][0] for i in keep) * rank + 1))


def test_a_fitted_model_starts_every_job(monkeypatch):
    fake = _FakeSequential()
    monkeypatch.setattr(dec, "_device", lambda: torch.device("cpu"))
    monkeypatch.setattr(_engine, "parafac2_als", fake)
    mats = _mats()
    rng = np.random.RandomState(1)
    A, B, C = rng.rand(3, 2), rng.rand(2, 2), rng.rand(10, 2)
    fitted = (None, (A, B, C), [rng.rand(m.shape[0], 2) for m in mats])
    for model in ((A, B, C), fitted, (fitted, [0.3, 0.2])):
        fake.calls.clear()
        rs.parafac2_als_resample(mats, 2, W3, starts=model, method="sequential")
        assert len(fake.calls) == 2
        np.testing.assert_array_equal(fake.calls[0]["start"][0], A[:2] * np.sqrt([[1.0], [2.0]]))
        np.testing.assert_array_equal(fake.calls[1]["start"][0], A * np.sqrt([[0.5], [1.0], [1.0]]))
        for call in fake.calls:
            np.testing.assert_array_equal(call["start"][1], B)
            np.testing.assert_array_equal(call["start"][2], C)


# ---- resample_summary ------------------------------------------------------------------------------------------------------------
def _model(seed=0, I=7, r=3, K=9, rows=(5, 6, 4, 8, 5, 7, 6)):
    rng = np.random.RandomState(seed)
    A, B, C = rng.uniform(0.5, 1.5, (I, r)), np.eye(r) + 0.3 * rng.rand(r, r), rng.standard_normal((K, r))
    P = [np.linalg.qr(rng.standard_normal((J, r)))[0] for J in rows]
    return None, (A, B, C), P


def _disguise(model, perm, s_A, s_C, dC=None, weights=None):
    """the same X_i models with the columns permuted and the signs of (A, B) / (C, B) flipped; dC is added to C first"""
    _, (A, B, C), P = model
    s_A, s_C = np.asarray(s_A, dtype=np.float64), np.asarray(s_C, dtype=np.float64)
    C = C if dC is None else C + dC
    A2, B2, C2 = (A * s_A)[:, perm], (B * (s_A * s_C))[:, perm], (C * s_C)[:, perm]
    P2 = [p.copy() for p in P]
    if weights is not None:
        A2[weights == 0] = 0.0
        for i in np.flatnonzero(weights == 0):
            P2[i] = np.zeros_like(P2[i])
    return None, (A2, B2, C2), P2


PERMS = [[0, 1, 2], [2, 0, 1], [1, 0, 2], [2, 1, 0], [1, 2, 0]]
SIGNS = [([1, 1, 1], [1, 1, 1]), ([-1, 1, 1], [1, -1, 1]), ([1, -1, -1], [-1, -1, 1]), ([-1, -1, -1], [1, 1, -1]), ([1, 1, -1], [-1, 1, -1])]


@pytest.mark.parametrize("reference_form", ["result", "triple", "with_errors"])
def test_summary_returns_the_model_and_no_spread_for_disguised_copies(reference_form):
    model = _model()
    weights = np.ones((5, 7))
    weights[1, 2] = weights[3, 2] = weights[3, 6] = 0.0
    reps = [_disguise(model, p, sa, sc, weights=w) for p, (sa, sc), w in zip(PERMS, SIGNS, weights)]
    reps[2] = (reps[2], [0.4, 0.3])  # a result with its errors
    reference = {"result": model, "triple": model[1], "with_errors": (model, [0.1])}[reference_form]
    got = rs.resample_summary(reps, reference, weights)
    for name, F in zip("ABC", model[1]):
        s = getattr(got, name)
        np.testing.assert_allclose(s.mean, F, rtol=0, atol=1e-14)
        assert s.std.shape == F.shape and np.abs(s.std).max() < 1e-14
        assert s.quantiles.shape == (2,) + F.shape
        np.testing.assert_allclose(s.quantiles, np.broadcast_to(F, (2,) + F.shape), rtol=0, atol=1e-14)
    assert got.fms.shape == (5,) and got.permutations.shape == (5, 3)
    for perm, found in zip(PERMS, got.permutations):
        assert np.array_equal(np.asarray(perm)[found], [0, 1, 2])  # the permutation found undoes the one applied
    assert ((got.fms > 0) & (got.fms <= 1 + 1e-12)).all()  # the rows of A left out cost score, not the matching
    assert got.fms[0] == pytest.approx(1.0, abs=1e-12)


def test_summary_of_a_known_perturbation():
    model = _model()
    A, B, C = model[1]
    n = 9
    t = np.linspace(-1.0, 1.0, n)  # replicate j holds C + t_j E: mean C, and the quantiles of t times E
    E = 0.01 * np.random.RandomState(5).standard_normal(C.shape)
    order = np.random.RandomState(6).permutation(n)
    reps = [_disguise(model, PERMS[j % 5], *SIGNS[(j + 2) % 5], dC=t[j] * E) for j in order]
    q = (0.025, 0.25, 0.975)
    got = rs.resample_summary(reps, model, quantiles=q)
    np.testing.assert_allclose(got.C.mean, C, rtol=0, atol=1e-14)
    np.testing.assert_allclose(got.C.std, np.abs(E) * np.std(t, ddof=1), rtol=1e-12, atol=1e-15)
    want = np.stack([np.where(E >= 0, np.quantile(t, qi), np.quantile(-t, qi)) * np.abs(E) + C for qi in q])
    np.testing.assert_allclose(got.C.quantiles, want, rtol=0, atol=1e-14)
    assert np.abs(got.A.std).max() < 1e-14 and np.abs(got.B.std).max() < 1e-14
    np.testing.assert_allclose(got.A.mean, A, rtol=0, atol=1e-14)
    assert ((got.fms > 0.99) & (got.fms <= 1.0 + 1e-12)).all()


def test_summary_of_A_runs_over_the_replicates_that_held_the_row():
    model = _model()
    A = model[1][0]
    weights = np.ones((4, 7))
    weights[0, 1] = weights[2, 1] = 0.0
    weights[:, 5] = 0.0  # never held
    weights[:3, 4] = 0.0  # held once
    reps = []
    for j, w in enumerate(weights):
        m = _disguise(model, PERMS[j], *SIGNS[j], weights=w)
        m[1][0][1] *= (1.0 + 0.1 * j)  # row 1 of A differs between the replicates (zero where it was left out)
        reps.append(m)
    got = rs.resample_summary(reps, model, weights)
    np.testing.assert_allclose(got.A.mean[1], A[1] * np.mean([1.1, 1.3]), rtol=1e-13)
    np.testing.assert_allclose(got.A.std[1], np.abs(A[1]) * np.std([1.1, 1.3], ddof=1), rtol=1e-12)
    assert np.isnan(got.A.mean[5]).all() and np.isnan(got.A.std[5]).all() and np.isnan(got.A.quantiles[:, 5]).all()
    np.testing.assert_allclose(got.A.mean[4], A[4], rtol=1e-13)
    assert not got.A.std[4].any()
    np.testing.assert_allclose(got.A.mean[[0, 2, 3, 6]], A[[0, 2, 3, 6]], rtol=1e-13)


def test_summary_refusals():
    model = _model()
    with pytest.raises(ValueError, match="at least one"):
        rs.resample_summary([], model)
    with pytest.raises(TypeError, match="reference"):
        rs.resample_summary([model], "best")
    with pytest.raises(ValueError, match="2 rows for 1 replicates"):
        rs.resample_summary([model], model, np.ones((2, 7)))
    with pytest.raises(ValueError, match="quantiles"):
        rs.resample_summary([model], model, quantiles=(0.5, 1.5))


# ---- layout -----------------------------------------------------------------------------------------------------------------------
def test_scale_layout_is_jobs_by_matrices():
    I, jobs = 5, 3
    scale = np.arange(jobs * I, dtype=np.float64).reshape(jobs, I)
    for s in range(jobs):
        for i in range(I):
            assert scale.ravel()[_engine.pf2als_slab_scale_offset(I, s, i)] == scale[s, i]
    assert _engine.pf2als_slab_scale_offset(I, jobs, 0) == scale.size  # no padding between or after the jobs


@pytest.mark.parametrize("I, J, K, rank, n_jobs", [(3, (5, 9, 6), 10, 2, 1), (108, None, 21, 2, 64), (1, (16,), 16, 16, 3)])
def test_the_weighted_entry_shares_the_workspace_and_refuses_a_missing_scale(I, J, K, rank, n_jobs):
    rng = np.random.RandomState(0)
    J = np.asarray(J if J is not None else rng.randint(rank, 3 * rank + 20, size=I), dtype=np.int64)
    row_ptr = np.concatenate([[0], np.cumsum(J)]).astype(np.int64)
    lib = _engine.load_library()
    rp = row_ptr.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
    nbytes = lib.mcl_pf2als_multistart_workspace_bytes(rp, I, K, rank, n_jobs)
    assert nbytes == _engine.pf2als_multistart_workspace_bytes(I, int(row_ptr[-1]), K, rank, n_jobs)  # no bytes for the scales
    rc = lib.mcl_pf2als_multistart_run_weighted(None, 0, rp, I, K, rank, n_jobs, None, 1, 1, 0.0, 0.0, 0, None, None, None, None, None,
                                                0, None)
    assert rc != 0
    message = lib.mcl_pf2als_multistart_last_error().decode()
    assert "mcl_pf2als_multistart_run_weighted" in message and "slab_scale" in message
    rc = lib.mcl_pf2als_multistart_run_weighted(None, 0, rp, I, K, 17, n_jobs, None, 1, 1, 0.0, 0.0, 0, None, None, None, None, None,
                                                0, None)
    assert rc != 0 and "rank" in lib.mcl_pf2als_multistart_last_error().decode()  # the shape checks of the unweighted entry
    assert lib.mcl_version() == 410
