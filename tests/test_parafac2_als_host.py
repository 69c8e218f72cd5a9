"""CPU: parafac2_als refuses what the device form does not serve (NotImplementedError) and bad arguments (ValueError) BEFORE
anything touches a device; the fp64 restatement of its spec (tests/parafac2_als_restatement.py) recovers a planted model."""
import numpy as np
import pytest

from matcouply_amd import _engine, decomposition as dec
from tests import parafac2_als_restatement as R


@pytest.fixture(autouse=True)
def no_device(monkeypatch):
    def refuse(*args, **kwargs):
        raise AssertionError("the device was touched")

    monkeypatch.setattr(dec, "_device", refuse)
    monkeypatch.setattr(_engine, "parafac2_als", refuse)


def _mats(shapes, seed=0):
    rng = np.random.RandomState(seed)
    return [rng.random_sample(s) for s in shapes]


def test_exported():
    assert "parafac2_als" in dec.__all__


@pytest.mark.parametrize("modes", [[1], [0, 1], (1, 2), "all"])
def test_nonnegative_b_mode_is_refused_with_the_reason(modes):
    with pytest.raises(NotImplementedError, match="mode 1"):
        dec.parafac2_als(_mats([(5, 10), (8, 10)]), 2, nn_modes=modes)


@pytest.mark.parametrize("kw", [{"svd": "randomized_svd"}, {"normalize_factors": True}, {"linesearch": True}, {"verbose": True}])
def test_unserved_tensorly_options_name_the_keyword(kw):
    with pytest.raises(NotImplementedError, match=next(iter(kw))):
        dec.parafac2_als(_mats([(5, 10), (8, 10)]), 2, **kw)


def test_shape_and_rank_limits():
    with pytest.raises(NotImplementedError, match="rank"):
        dec.parafac2_als(_mats([(3, 10), (8, 10)]), 4)  # J_0 < rank
    with pytest.raises(NotImplementedError, match="rank"):
        dec.parafac2_als(_mats([(20, 3), (30, 3)]), 4)  # K < rank
    with pytest.raises(NotImplementedError, match="32"):
        dec.parafac2_als(_mats([(40, 40), (40, 40)]), 33)
    with pytest.raises(NotImplementedError, match="2048"):
        dec.parafac2_als(_mats([(3, 2049), (4, 2049)]), 2, init="svd")


@pytest.mark.parametrize("kw", [{"init": "parafac2_als"}, {"init": None}, {"nn_modes": [3]}, {"nn_modes": "some"},
                                {"nn_modes": 0}, {"n_iter_max": 0}, {"n_iter_parafac": 0}])
def test_bad_values(kw):
    with pytest.raises(ValueError):
        dec.parafac2_als(_mats([(5, 10), (8, 10)]), 2, **kw)


def test_unknown_keyword():
    with pytest.raises(TypeError):
        dec.parafac2_als(_mats([(5, 10), (8, 10)]), 2, n_iter=3)


@pytest.mark.parametrize("init", ["svd", "random"])
def test_restatement_recovers_a_planted_model(init):
    mats, true = R.parafac2_problem(20, (10, 30), 15, 3, seed=0, noise=0.1)
    A, B, C, P, errors, _ = R.parafac2_als(mats, 3, init=init, random_state=0, n_iter_max=300)
    assert R.factor_match((A, B, C, P), true) > 0.95
    assert errors[-1] < 0.1
    assert np.all(np.diff(errors) <= 1e-12)


# ---- the fixtures of the GPU RMAX = 32 / load-path / boundary tests are well posed (tests/kernel_edge_cases.py) -------------------
from tests import kernel_edge_cases as E  # noqa: E402


@pytest.mark.parametrize("name", sorted(E.PF2_CASES))
def test_edge_fixture_is_well_posed(name, monkeypatch):
    mats, rank = E.pf2_problem(name)
    assert min(m.shape[0] for m in mats) >= rank and mats[0].shape[1] >= rank
    gap, tail = E.gram_gaps(sum(m.T.astype(np.float64) @ m for m in mats), rank)  # the stack Gram of init="svd"
    assert gap >= E.GAP_MIN and tail <= E.TAIL_RATIO_MAX, (name, gap, tail)
    rec = E.StepRecorder(monkeypatch, R)
    R.parafac2_als(mats, rank, n_iter_max=3, tol=1e-300, absolute_tol=0, init="svd")
    assert rec.cholesky_failed == 0 and max(rec.kappa) < E.KAPPA_MAX, (name, rec.cholesky_failed, max(rec.kappa))
