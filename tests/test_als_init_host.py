"""CPU: the CP initialisers (init="parafac_als" / "cp_als" / "parafac_hals" / "cp_hals") refuse what the device form does not
serve with NotImplementedError BEFORE anything touches a device; init="parafac2_als" keeps raising."""
import numpy as np
import pytest

from matcouply_amd import _engine, decomposition as dec

CP_NAMES = ["parafac_als", "cp_als", "parafac_hals", "cp_hals"]


@pytest.fixture(autouse=True)
def no_device(monkeypatch):
    def refuse(*args, **kwargs):
        raise AssertionError("the device was touched")

    monkeypatch.setattr(dec, "_device", refuse)
    monkeypatch.setattr(_engine, "als_init", refuse)


def _mats(shapes, seed=0):
    rng = np.random.RandomState(seed)
    return [rng.random_sample(s) for s in shapes]


@pytest.mark.parametrize("init", CP_NAMES)
@pytest.mark.parametrize("params", [{"normalize_factors": True}, {"svd": "truncated_svd"}, {"linesearch": True},
                                    {"n_iter_max": 5, "init": "random"}])
def test_unsupported_init_params(init, params):
    bad = sorted(set(params) - {"n_iter_max", "tol"})
    with pytest.raises(NotImplementedError, match=bad[0]):
        dec.initialize_cmf(_mats([(5, 10), (8, 10)]), 2, init, None, init_params=params)


@pytest.mark.parametrize("init", CP_NAMES)
def test_rank_above_min_of_longest_matrix_and_columns(init):
    with pytest.raises(NotImplementedError, match="rank"):
        dec.initialize_cmf(_mats([(4, 10), (6, 10)]), 7, init, None)  # max J_i = 6
    with pytest.raises(NotImplementedError, match="rank"):
        dec.initialize_cmf(_mats([(20, 5), (30, 5)]), 6, init, None)  # K = 5


@pytest.mark.parametrize("init", CP_NAMES)
def test_gram_bounds(init):
    with pytest.raises(NotImplementedError, match="2048"):
        dec.initialize_cmf(_mats([(3, 2049), (4, 2049)]), 2, init, None)
    with pytest.raises(NotImplementedError, match="2048"):
        dec.initialize_cmf(_mats([(2049, 3), (4, 3)]), 2, init, None)


@pytest.mark.parametrize("init", CP_NAMES)
def test_solver_refuses_cp_starts_under_group(init):
    with pytest.raises(NotImplementedError, match="group"):
        dec.cmf_aoadmm(_mats([(5, 10), (8, 10)]), 2, init=init, n_iter_max=1, group=object())


def test_parafac2_als_still_raises():
    with pytest.raises(NotImplementedError, match="parafac2_als"):
        dec.initialize_cmf(_mats([(5, 10), (8, 10)]), 2, "parafac2_als", None)


# ---- the fixtures of the GPU rank-bucket / load-path / ragged tests are well posed (tests/kernel_edge_cases.py) -------------------
from tests import als_restatement as R  # noqa: E402
from tests import kernel_edge_cases as E  # noqa: E402


@pytest.mark.parametrize("name", sorted(E.ALS_CASES))
def test_edge_fixture_is_well_posed(name, monkeypatch):
    mats, rank = E.als_problem(name)
    K, J_max = mats[0].shape[1], max(m.shape[0] for m in mats)
    assert rank <= min(K, J_max)
    for G in E.als_start_grams(mats):
        gap, tail = E.gram_gaps(G, rank)
        assert gap >= E.GAP_MIN and tail <= E.TAIL_RATIO_MAX, (name, gap, tail)
    rec = E.StepRecorder(monkeypatch, R)
    R.cp_init(mats, rank, hals=False, n_iter_max=3, tol=0)
    assert rec.cholesky_failed == 0 and max(rec.kappa) < E.KAPPA_MAX, (name, rec.cholesky_failed, max(rec.kappa))
    A, B, C, _ = R.cp_init(mats, rank, hals=True, n_iter_max=3, tol=0)
    assert np.isfinite(A).all() and np.isfinite(C).all() and all(np.isfinite(b).all() for b in B)
