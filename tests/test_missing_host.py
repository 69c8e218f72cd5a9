"""CPU: the missing-entry fit's host side (matcouply_amd/missing.py) and its restatement (tests/missing_aoadmm_restatement.py) -
the restatement against the oracle itself, its monotone observed-entry error, the parsing of masks and fills, every refusal
before the device is touched, the folds of entry_kfold, impute and heldout_entry_sse on a hand-made case, and the refusals of
the C entry mcl_multistart_run_missing in the manner of tests/test_entry_refusals_host.py."""
import numpy as np
import pytest
import torch

from matcouply_amd import _engine, decomposition as dec, missing, multistart as ms
from matcouply_amd.coupled_matrices import CoupledMatrixFactorization
from oracle import aoadmm_oracle as orc
from tests import missing_aoadmm_restatement as mr
from tests import test_entry_refusals_host as T
from tests.weighted_aoadmm_restatement import oracle_state


def _ragged(seed=0, I=6, K=9, r=3):
    rng = np.random.RandomState(seed)
    J = rng.randint(5, 12, size=I)
    X, row_ptr = orc.synthetic_problem(I, J, K, r, seed=seed, dtype=np.float32)
    return [X[row_ptr[i]: row_ptr[i + 1]].astype(np.float64) for i in range(I)], X.astype(np.float64), row_ptr


def _truncated_normal(rng, size):
    x = rng.standard_normal(size=size)
    x[x < 0] = 0
    return x


def example_problem(I=10, J=15, K=20, rank=3, noise_level=0.0, seed=0):
    """the simulated non-negative PARAFAC2 data of the reference's examples (tests/test_gpu_multistart.py: _example_problem)"""
    rng = np.random.default_rng(seed)
    A = rng.uniform(size=(I, rank)) + 0.1
    blueprint = _truncated_normal(rng, (J, rank))
    C = _truncated_normal(rng, (K, rank))
    clean = [(np.roll(blueprint, i, axis=0) * A[i]) @ C.T for i in range(I)]
    noise = [rng.uniform(size=M.shape) for M in clean]
    return clean, [M + N * noise_level * np.linalg.norm(M) / np.linalg.norm(N) for M, N in zip(clean, noise)]


def random_mask(shapes, fraction, seed):
    rng = np.random.RandomState(seed)
    return [rng.uniform(size=s) >= fraction for s in shapes]


# ---- the restatement -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stack", [dict(non_negative={0: True, 1: True}, l1_penalty={2: 0.05}), dict(parafac2=True, non_negative=True)],
                         ids=["nn_l1C", "parafac2_nn"])
@pytest.mark.parametrize("fill", ["mean", "model"])
def test_all_observed_restatement_is_the_oracle(stack, fill):
    mats, X, row_ptr = _ragged()
    kw = dict(stack, n_iter_max=15, tol=None, return_errors=True)
    st = oracle_state(mats, X, row_ptr, 3, 1, kw)
    res = orc.run(st, 15, tol=None, absolute_tol=None)
    observed = np.ones(X.shape, dtype=bool)
    ms = mr.missing_state(mats, X, row_ptr, 3, 1, kw, observed, None if fill == "model" else mr.column_means(X, observed))
    got = mr.run(ms, 15, tol=None, absolute_tol=None)
    for a, b in ((ms.A, st.A), (ms.B, st.B), (ms.C, st.C)):
        assert np.linalg.norm(a - b) <= 1e-12 * np.linalg.norm(b)
    np.testing.assert_array_equal(ms.X, X)
    # (another formula for the same number: |X - M| directly, not |X|^2 - 2 <X, M> + |M|^2)
    np.testing.assert_allclose(got["rec_errors"], res["rec_errors"], rtol=1e-9)
    np.testing.assert_allclose(got["losses"], res["losses"], rtol=1e-9)
    assert got["gaps"] == res["gaps"] and got["n_iter"] == res["n_iter"] == 15


def test_restatement_stops_where_the_oracle_stops_on_complete_data():
    _, mats = example_problem(noise_level=0.2)
    X, row_ptr = np.concatenate(mats), np.concatenate([[0], np.cumsum([m.shape[0] for m in mats])])
    kw = dict(parafac2=True, non_negative=True, l2_penalty=0, n_iter_max=400, return_errors=True)
    res = orc.run(oracle_state(mats, X, row_ptr, 3, 2, kw), 400)
    got = mr.run(mr.missing_state(mats, X, row_ptr, 3, 2, kw, np.ones(X.shape, dtype=bool), np.zeros(X.shape[1])), 400)
    assert res["n_iter"] < 400 and res["satisfied_stopping_condition"]  # (default tolerances: after 262 iterations)
    assert (got["n_iter"], got["message"], got["satisfied_stopping_condition"]) == (
        res["n_iter"], res["message"], res["satisfied_stopping_condition"])


def test_observed_error_does_not_increase_after_iteration_50():
    _, mats = example_problem()
    shapes = [m.shape for m in mats]
    X, row_ptr = np.concatenate(mats), np.concatenate([[0], np.cumsum([s[0] for s in shapes])])
    observed = np.concatenate(random_mask(shapes, 0.3, seed=0))
    garbage = np.where(observed, X, np.nan)
    kw = dict(parafac2=True, non_negative=True, l2_penalty=0, n_iter_max=200, tol=None, return_errors=True)
    st = mr.missing_state(mats, garbage, row_ptr, 3, 0, kw, observed, mr.column_means(X, observed))
    rec = np.array(mr.run(st, 200, tol=None, absolute_tol=None)["rec_errors"])
    assert len(rec) == 201 and np.isfinite(rec).all() and np.isfinite(st.X).all()
    assert (np.diff(rec[50:]) <= 0).all(), np.diff(rec[50:]).max()
    assert rec[-1] < 0.05 * rec[0]


def test_restatement_never_uses_the_values_at_missing_entries():
    mats, X, row_ptr = _ragged(seed=1)
    observed = np.concatenate(random_mask([m.shape for m in mats], 0.3, seed=1))
    kw = dict(non_negative=True, n_iter_max=5, tol=None)
    runs = []
    for junk in (np.nan, 1e30, 0.0):
        st = mr.missing_state(mats, np.where(observed, X, junk), row_ptr, 3, 0, kw, observed)
        runs.append((mr.run(st, 5, tol=None, absolute_tol=None)["rec_errors"], st.A.tobytes()))
    assert runs[0] == runs[1] == runs[2]


# ---- masks and fills ---------------------------------------------------------------------------------------------------------------
def _small():
    rng = np.random.RandomState(3)
    mats = [rng.uniform(size=(4, 5)), rng.uniform(size=(3, 5)), rng.uniform(size=(6, 5))]
    return mats, [m.shape for m in mats]


def test_nan_entries_are_the_missing_ones():
    mats, shapes = _small()
    mats[0][1, 2] = mats[2][5, 4] = np.nan
    masks, X, row_ptr = missing.observed_masks(mats, None, 4)
    assert masks.shape == (1, 13, 5) and masks.dtype == bool and list(row_ptr) == [0, 4, 7, 13]
    want = np.ones((13, 5), dtype=bool)
    want[1, 2] = want[12, 4] = False
    np.testing.assert_array_equal(masks[0], want)
    np.testing.assert_array_equal(X[want], np.concatenate(mats)[want])


def test_shared_and_per_job_masks():
    mats, shapes = _small()
    shared = random_mask(shapes, 0.3, seed=0)
    masks, _, _ = missing.observed_masks(mats, shared, 3)
    assert masks.shape == (1, 13, 5)
    np.testing.assert_array_equal(masks[0], np.concatenate(shared))
    per_job = [random_mask(shapes, 0.3, seed=s) for s in range(3)]
    masks, _, _ = missing.observed_masks(mats, per_job, 3)
    assert masks.shape == (3, 13, 5)
    for s in range(3):
        np.testing.assert_array_equal(masks[s], np.concatenate(per_job[s]))
    # I masks for I jobs of I matrices are still one shared mask: arrays, not lists
    assert missing.observed_masks(mats, shared, len(mats))[0].shape[0] == 1


def test_column_means_against_a_direct_computation():
    mats, shapes = _small()
    per_job = [random_mask(shapes, 0.4, seed=s) for s in range(2)]
    for m in per_job[1]:
        m[:, 3] = False  # a column without an observed entry in job 1
    masks, X, _ = missing.observed_masks(mats, per_job, 2)
    got = missing.column_means(X, masks)
    assert got.shape == (2, 5) and got.dtype == np.float64
    for s in range(2):
        np.testing.assert_allclose(got[s], mr.column_means(X, masks[s]), rtol=1e-14)
    assert got[1, 3] == 0.0 and got[0, 3] != 0.0
    # NaN at the missing entries does not reach the means
    np.testing.assert_array_equal(missing.column_means(np.where(masks[0], X, np.nan), masks[:1]), got[:1])


# ---- refusals, before the device is touched ----------------------------------------------------------------------------------------
@pytest.fixture
def no_device(monkeypatch):
    def refuse(*args, **kwargs):
        raise AssertionError("the device was touched")

    monkeypatch.setattr(dec, "_device", refuse)
    monkeypatch.setattr(ms, "_multistart_fused", refuse)
    monkeypatch.setattr(_engine, "multistart_run_missing", refuse)


def test_value_errors_touch_no_device(no_device):
    mats, shapes = _small()
    good = random_mask(shapes, 0.2, seed=0)
    for m in good:
        m[0, 0] = True
    with pytest.raises(ValueError, match=r"observed\[1\] has shape \(2, 5\), its matrix \(3, 5\)"):
        missing.cmf_aoadmm_missing(mats, 2, [good[0], good[1][:2], good[2]], range(2))
    with pytest.raises(ValueError, match="observed holds 2 arrays for 3 matrices"):
        missing.cmf_aoadmm_missing(mats, 2, good[:2], range(2))
    with pytest.raises(ValueError, match="observed holds 3 masks for 2 jobs"):
        missing.cmf_aoadmm_missing(mats, 2, [good, good, good], range(2))
    empty = [m.copy() for m in good]
    empty[1][:] = False
    with pytest.raises(ValueError, match="mask 1: matrix 1 has no observed entry"):
        missing.cmf_aoadmm_missing(mats, 2, [good, empty], range(2))
    holed = [m.copy() for m in mats]
    holed[2][0, 0] = np.nan
    with pytest.raises(ValueError, match="mask 0: NaN at an observed entry"):
        missing.cmf_aoadmm_missing(holed, 2, good, range(2))
    all_nan = [m.copy() for m in mats]
    all_nan[0][:] = np.nan
    with pytest.raises(ValueError, match="mask 0: matrix 0 has no observed entry"):
        missing.cmf_aoadmm_missing(all_nan, 2, None, range(2))
    with pytest.raises(ValueError, match='needs init="random"'):
        missing.cmf_aoadmm_missing(mats, 2, good, range(2), init="svd")
    with pytest.raises(ValueError, match="fill must be one of"):
        missing.cmf_aoadmm_missing(mats, 2, good, range(2), fill="median")
    with pytest.raises(TypeError, match="takes random_states"):
        missing.cmf_aoadmm_missing(mats, 2, good, range(2), random_state=0)
    with pytest.raises(TypeError, match="unexpected keyword argument 'parafac2'"):
        missing.parafac2_aoadmm_missing(mats, 2, good, range(2), parafac2=True)


@pytest.mark.parametrize("kwargs,rank,sentence", [
    (dict(), 17, "rank 17 is above 16"),
    (dict(unimodal={1: True}), 2, "Unimodality on mode 1 is not served"),
    (dict(tv_penalty={1: 0.1}), 2, "TotalVariationPenalty on mode 1 is not served"),
    (dict(verbose=True), 2, "verbose output is not produced by the fused kernel"),
    (dict(arithmetic="fp64"), 2, "arithmetic='fp64' is not served"),
    (dict(l2_norm_bound={0: 1.0}), 2, "an L2Ball on mode 0 needs constant_feasibility_penalty"),
    (dict(parafac2=True), 4, "Parafac2 is served on mode 1 with every J_i >= rank"),
])
def test_what_the_fused_kernel_does_not_serve_is_not_implemented(no_device, kwargs, rank, sentence):
    mats, shapes = _small()
    with pytest.raises(NotImplementedError) as e:
        missing.cmf_aoadmm_missing(mats, rank, random_mask(shapes, 0.1, seed=0), range(2), **kwargs)
    assert str(e.value).startswith("cmf_aoadmm_missing: ") and sentence in str(e.value)
    assert str(e.value) == "cmf_aoadmm_missing: " + ms._multistart_unfused_reason(mats, rank, dec._cmf_kwargs(kwargs))


def test_too_many_elements_is_not_implemented(no_device):
    mats = [np.zeros((600, 500))]
    with pytest.raises(NotImplementedError, match="above the fused bound"):
        missing.cmf_aoadmm_missing(mats, 2, None, range(2))


def test_the_launch_gets_masks_fills_and_keywords(monkeypatch):
    mats, shapes = _small()
    seen = {}

    def fused(matrices, rank, random_states, kws, run):
        seen.update(rank=rank, states=list(random_states), kws=kws)
        run("X", "row_ptr", rank, ["the options of job 0"], torch.zeros(1))  # the launch the caller names, here on the host
        return ["result"] * len(random_states)

    def run_missing(X, row_ptr, rank, options, observed, fill_values, state):
        assert (X, row_ptr, options) == ("X", "row_ptr", "the options of job 0")
        seen["missing"] = (observed.numpy(), None if fill_values is None else fill_values.numpy())

    monkeypatch.setattr(ms, "_multistart_fused", fused)
    monkeypatch.setattr(_engine, "multistart_run_missing", run_missing)
    per_job = [random_mask(shapes, 0.3, seed=s) for s in range(2)]
    assert missing.cmf_aoadmm_missing(mats, 2, per_job, [5, 6], non_negative=True) == ["result"] * 2
    observed, fill = seen["missing"]
    assert observed.dtype == np.uint8 and observed.shape == (2, 13, 5) and seen["states"] == [5, 6] and seen["rank"] == 2
    np.testing.assert_array_equal(fill, missing.column_means(np.concatenate(mats), observed.astype(bool)))
    assert seen["kws"][0]["non_negative"] is True and len(seen["kws"]) == 1
    missing.cmf_aoadmm_missing(mats, 2, per_job[0], [5, 6], fill="zero")
    assert seen["missing"][0].shape == (1, 13, 5) and seen["missing"][1].shape == (1, 5) and not seen["missing"][1].any()
    missing.parafac2_aoadmm_missing(mats, 2, per_job[0], [5, 6], fill="model")
    assert seen["missing"][1] is None and seen["kws"][0]["parafac2"] is True and seen["kws"][0]["l2_penalty"] == 0
    assert missing.cmf_aoadmm_missing(mats, 2, per_job[0], []) == []


# ---- entry_kfold, impute, heldout_entry_sse ---------------------------------------------------------------------------------------
def test_entry_kfold_partitions_the_observed_entries():
    mats, shapes = _small()
    mats[1][2, 2] = np.nan
    data = ~np.isnan(np.concatenate(mats))
    folds = missing.entry_kfold(mats, 4, random_state=7)
    assert len(folds) == 4 and all(len(f) == 3 and [m.shape for m in f] == shapes for f in folds)
    held = np.stack([data & ~np.concatenate(f) for f in folds])
    assert (held.sum(axis=0) == data).all()  # every observed entry is held out of exactly one job, no other entry of any
    assert not np.stack([np.concatenate(f) for f in folds])[:, ~data].any()
    sizes = held.sum(axis=(1, 2))
    assert sizes.sum() == data.sum() == 64 and sizes.max() - sizes.min() <= 1
    again = missing.entry_kfold(mats, 4, random_state=7)
    other = missing.entry_kfold(mats, 4, random_state=8)
    assert all(np.array_equal(a, b) for f, g in zip(folds, again) for a, b in zip(f, g))
    assert not all(np.array_equal(a, b) for f, g in zip(folds, other) for a, b in zip(f, g))
    # under a mask of its own
    own = random_mask(shapes, 0.5, seed=1)
    folds = missing.entry_kfold(mats, 3, random_state=0, observed=[o & ~np.isnan(m) for o, m in zip(own, mats)])
    held = np.stack([np.concatenate(own) & data & ~np.concatenate(f) for f in folds])
    assert (held.sum(axis=0) == (np.concatenate(own) & data)).all()
    with pytest.raises(ValueError, match="need 2 <= n_folds"):
        missing.entry_kfold(mats, 1)


def _hand_made():
    # 2 x (3 x 4), rank 1: B_i D_i C^T = a_i b_i c^T
    A = np.array([[2.0], [3.0]])
    B_is = [np.array([[1.0], [2.0], [3.0]]), np.array([[1.0], [0.0], [-1.0]])]
    C = np.array([[1.0], [10.0], [100.0], [1000.0]])
    model = [np.array([[2.0, 20, 200, 2000], [4, 40, 400, 4000], [6, 60, 600, 6000]]),
             np.array([[3.0, 30, 300, 3000], [0, 0, 0, 0], [-3, -30, -300, -3000]])]
    return CoupledMatrixFactorization((None, (A, B_is, C))), model


def test_impute_on_a_hand_made_case():
    cmf, model = _hand_made()
    mats = [np.full((3, 4), 7.0), np.full((3, 4), -7.0)]
    mats[0][0, 1] = mats[0][2, 3] = mats[1][1, 0] = np.nan
    got = missing.impute(mats, cmf)
    want = [m.copy() for m in mats]
    want[0][0, 1], want[0][2, 3], want[1][1, 0] = 20.0, 6000.0, 0.0
    for g, w in zip(got, want):
        assert isinstance(g, np.ndarray) and g.dtype == np.float64
        np.testing.assert_array_equal(g, w)
    # an explicit mask; a result tuple led by the model; float32 in, float32 out
    mask = [np.ones((3, 4), dtype=bool), np.ones((3, 4), dtype=bool)]
    mask[1][2, 2] = False
    got = missing.impute([m.astype(np.float32) for m in want], (cmf, "diagnostics"), observed=mask)
    assert got[1][2, 2] == -300.0 and got[1].dtype == np.float32 and got[0][0, 1] == 20.0
    got[1][2, 2] = -7.0
    np.testing.assert_array_equal(got[1], want[1].astype(np.float32))


def test_heldout_entry_sse_on_a_hand_made_case():
    cmf, model = _hand_made()
    mats = [m + 1.0 for m in model]  # every entry is off by one ...
    mats[1][0, 0] += 2.0             # ... and one by three
    mats[0][1, 1] = np.nan           # not observed in the data: never counted
    full = [np.ones((3, 4), dtype=bool) for _ in range(2)]
    job0 = [f.copy() for f in full]
    job0[0][0, 0] = job0[0][1, 1] = job0[1][0, 0] = False  # held out: (0; 0, 0) and (1; 0, 0); (0; 1, 1) is missing anyway
    job1 = [f.copy() for f in full]
    job1[1][2, :] = False
    sse, count = missing.heldout_entry_sse(mats, [cmf, (cmf, None)], [job0, job1])
    assert sse.dtype == np.float64 and count.dtype == np.int64
    np.testing.assert_array_equal(count, [2, 4])
    np.testing.assert_allclose(sse, [1.0 + 9.0, 4.0], rtol=1e-12)
    with pytest.raises(ValueError, match="job_observed holds 1 masks for 2 results"):
        missing.heldout_entry_sse(mats, [cmf, cmf], [job0])


# ---- the C entry (tests/test_entry_refusals_host.py's table, one more entry) -----------------------------------------------------
MISSING_WANT = T.MS_WANT + T.al(2 * T.N * T.K * 8)
MISSING = T.Entry(
    "mcl_multistart_run_missing", T.SLOTS[3], "mcl_multistart_run_missing: ",
    T.ms_good(2, MISSING_WANT, observed=T.FAKE, n_masks=2, fill=None),
    T.ms_shape() + [(dict(opt=None), T.MS_HEAD), (dict(n=0), "need n_starts >= 1")]
    + [(dict(opt=T.options(1, **f)), m) for f, m in T.MS_OPTION_REFUSALS]
    + [(dict(opt=T.options(1, **T.PF2_ON_B), rank=4), "PARAFAC2 needs every J_i >= rank"),
       (dict(n_masks=0), "need n_masks = 1 or n_masks = n_jobs"), (dict(n_masks=3), "need n_masks = 1 or n_masks = n_jobs"),
       (dict(n_masks=-2), "need n_masks = 1 or n_masks = n_jobs"), (dict(observed=None), "NULL observed mask"),
       (dict(observed=None, n_masks=1), "NULL observed mask"), (dict(xt=7), T.x_type(7))]
    + T.workspace_refusals(MISSING_WANT, "mcl_multistart_missing_workspace_bytes"), T.MS_NOT_NULL)
MISSING_CASES = [(MISSING, change, message) for change, message in MISSING.refusals]


@pytest.mark.parametrize("case", MISSING_CASES, ids=T._case_id)
def test_c_entry_refusal_names_its_entry_in_its_own_slot(case):
    T.test_refusal_names_its_entry_in_its_own_slot(case)


def test_c_entry_sizer():
    lib = _engine.load_library()
    size = lib.mcl_multistart_missing_workspace_bytes
    one = T.options(1)
    assert size(T.GOOD, T.I, T.K, T.R, one, 2) == MISSING_WANT == _engine.multistart_missing_workspace_bytes(T.I, T.N, T.K, T.R, 2)
    # the X~ slices lie behind the plan of mcl_multistart_run, whose size and scratch formula stay what they were
    assert lib.mcl_multistart_workspace_bytes(T.GOOD, T.I, T.K, T.R, one, 2) == T.MS_WANT
    assert size(None, T.I, T.K, T.R, one, 2) == -1 and size(T.GOOD, T.I, T.K, 17, one, 2) == -1 and size(T.GOOD, T.I, T.K, T.R, one, 0) == -1
    assert size(T.GOOD, T.I, T.K, T.R, None, 2) == -1 and size(T.GOOD, T.I, T.K, T.R, T.options(1, **T.PF2_ON_B), 1) > 0
    assert size(T.rp([0, 2, 70, 75]), T.I, T.K, T.R, T.options(1, **T.PF2_ON_B), 1) == -1


def test_symbols_are_exported_and_the_abi_version_stays():
    lib = _engine.load_library()
    assert {"mcl_multistart_missing_workspace_bytes", "mcl_multistart_run_missing"} <= set(_engine.EXPORTED_SYMBOLS)
    assert hasattr(lib, "mcl_multistart_run_missing") and lib.mcl_version() == 410
