"""CPU: cmf_aoadmm_multistart / parafac2_aoadmm_multistart host logic with the checker engine - the sequential method is the
single call per start, and the fused method refuses what its kernel does not serve before anything touches a device."""
import numpy as np
import pytest

from matcouply_amd import _engine, decomposition as dec, multistart as ms
from matcouply_amd import penalties as pen
from matcouply_amd.coupled_matrices import CoupledMatrixFactorization
from tests.oracle_engine import OracleEngineFactory


@pytest.fixture
def checker_engine(monkeypatch):
    monkeypatch.setattr(dec, "_ENGINE_FACTORY", OracleEngineFactory())


@pytest.fixture
def no_device(monkeypatch):
    def refuse(*args, **kwargs):
        raise AssertionError("the device was touched")

    monkeypatch.setattr(dec, "_device", refuse)
    monkeypatch.setattr(_engine, "multistart_run", refuse)


def _mats(shapes=((6, 8), (9, 8), (7, 8)), seed=0):
    rng = np.random.RandomState(seed)
    return [rng.uniform(size=s) for s in shapes]


def _same(a, b):
    if isinstance(a, CoupledMatrixFactorization):
        assert isinstance(b, CoupledMatrixFactorization)
        _same(a[0], b[0])
        _same(list(a[1]), list(b[1]))
    elif isinstance(a, (tuple, list)):
        assert type(a) is type(b) or (isinstance(a, tuple) and isinstance(b, tuple)), (type(a), type(b))
        assert len(a) == len(b)
        for x, y in zip(a, b):
            _same(x, y)
    elif isinstance(a, np.ndarray):
        assert a.dtype == b.dtype and a.shape == b.shape
        np.testing.assert_array_equal(a, b)
    else:
        assert a == b or (a is None and b is None), (a, b)


@pytest.mark.parametrize("kwargs", [
    dict(non_negative=True, n_iter_max=4, return_errors=True),
    dict(parafac2=True, l1_penalty={2: 0.1}, n_iter_max=3, tol=None, return_errors=True, return_admm_vars=True),
])
def test_sequential_is_the_single_call_per_start(checker_engine, kwargs):
    mats = _mats()
    seeds = [3, 7, np.random.RandomState(11)]
    got = dec.cmf_aoadmm_multistart(mats, 2, seeds, method="sequential", **kwargs)
    seeds_again = [3, 7, np.random.RandomState(11)]
    assert len(got) == 3
    for res, rs in zip(got, seeds_again):
        _same(res, dec.cmf_aoadmm(mats, 2, random_state=rs, **kwargs))


def test_parafac2_sequential_matches_parafac2_aoadmm(checker_engine):
    mats = _mats()
    got = dec.parafac2_aoadmm_multistart(mats, 2, range(2), method="sequential", n_iter_max=3, non_negative=True,
                                         return_errors=True)
    for s, res in enumerate(got):
        _same(res, dec.parafac2_aoadmm(mats, 2, random_state=s, n_iter_max=3, non_negative=True, return_errors=True))


def test_auto_falls_back_to_sequential_with_a_checker_engine(checker_engine):
    mats = _mats()
    got = dec.cmf_aoadmm_multistart(mats, 2, [0], n_iter_max=2, non_negative=True)
    _same(got[0], dec.cmf_aoadmm(mats, 2, random_state=0, n_iter_max=2, non_negative=True))


class _UserNN(pen.NonNegativity):
    def factor_matrix_row_update(self, factor_matrix_row, feasibility_penalty, aux_row):
        return super().factor_matrix_row_update(factor_matrix_row, feasibility_penalty, aux_row)


@pytest.mark.parametrize("kwargs, match", [
    (dict(rank=17), "rank"),
    (dict(unimodal={1: True}), "Unimodality"),
    (dict(tv_penalty={2: 0.1}), "TotalVariation"),
    (dict(generalized_l2_penalty={2: np.eye(8)}), "GeneralizedL2"),
    (dict(regs=[[], [], [pen.UnitSimplex()]]), "UnitSimplex"),
    (dict(regs=[[], [], [_UserNN()]]), "_UserNN"),
    (dict(verbose=True), "verbose"),
    (dict(group=object()), "group"),
    (dict(arithmetic="exact"), "arithmetic"),
    (dict(arithmetic="fast"), "arithmetic"),
    (dict(l2_norm_bound={0: 1.0}), "constant_feasibility_penalty"),
    (dict(parafac2=True, rank=7), "J_i >= rank"),
    (dict(regs=[[pen.NonNegativity()] * 5, [], []]), "more than"),
    (dict(shapes=((600, 500),)), "elements"),
])
def test_fused_refuses_out_of_scope_without_touching_the_device(no_device, kwargs, match):
    kwargs = dict(kwargs)
    rank = kwargs.pop("rank", 2)
    mats = _mats(kwargs.pop("shapes", ((6, 8), (9, 8), (7, 8))))
    with pytest.raises(NotImplementedError, match=match):
        dec.cmf_aoadmm_multistart(mats, rank, range(3), method="fused", n_iter_max=2, **kwargs)


def test_fused_refuses_under_a_checker_engine(checker_engine, no_device):
    with pytest.raises(NotImplementedError, match="substitute"):
        dec.cmf_aoadmm_multistart(_mats(), 2, range(2), method="fused", n_iter_max=2)


@pytest.mark.parametrize("init", ["svd", "threshold_svd", "parafac_als", (None, (np.ones((3, 2)), None, None))])
@pytest.mark.parametrize("method", ["auto", "fused", "sequential"])
def test_non_random_init_raises(no_device, init, method):
    with pytest.raises(ValueError, match="init"):
        dec.cmf_aoadmm_multistart(_mats(), 2, range(3), method=method, init=init)


def test_bad_method_and_random_state(no_device):
    with pytest.raises(ValueError, match="method"):
        dec.cmf_aoadmm_multistart(_mats(), 2, range(2), method="parallel")
    with pytest.raises(TypeError, match="random_states"):
        dec.cmf_aoadmm_multistart(_mats(), 2, range(2), random_state=0)
    with pytest.raises(TypeError):
        dec.cmf_aoadmm_multistart(_mats(), 2, range(2), method="fused", no_such_option=1)


# ---- the fixtures of the GPU every-rank / batch / stride tests are served by the fused kernel (tests/kernel_edge_cases.py) --------
from tests import kernel_edge_cases as E  # noqa: E402

@pytest.mark.parametrize("name", sorted(E.MS_RUNS))
def test_edge_fixture_is_served_fused(no_device, name):
    from tests.test_gpu_multistart import STACKS

    c = E.MS_CASES[name]
    mats, X, row_ptr = E.ms_problem(c["I"], c["J_range"], c["K"], c["r"], c["seed"])
    assert X.size <= ms._MULTISTART_MAX_ELEMENTS
    for stack in E.MS_RUNS[name]:
        reason = ms._multistart_unfused_reason(mats, c["r"], dec._cmf_kwargs(dict(STACKS[stack], n_iter_max=20, tol=None)))
        assert reason is None, (name, stack, reason)


@pytest.mark.parametrize("kwargs, match", [
    (dict(non_negative={0: True, 1: True}, l1_penalty={2: 0.05}), "mode-0 system singular"),  # rho_i = 0, no l2
    (dict(l2_penalty=[0.1, 0.0, 0.0], non_negative={1: True}), "mode-1 system singular"),
    (dict(l2_penalty=[0.1, 0.1, 0.0], parafac2=True), "J_i >= rank"),
])
def test_fused_refuses_an_empty_matrix_with_a_singular_system(no_device, kwargs, match):
    mats = _mats(((6, 8), (0, 8), (7, 8)))
    with pytest.raises(NotImplementedError, match=match):
        dec.cmf_aoadmm_multistart(mats, 2, range(2), method="fused", n_iter_max=2, **kwargs)


def test_oracle_sums_an_empty_slab_to_zero():
    # np.add.reduceat alone returns the next slab's first row for an empty segment: the oracle's A right-hand side gave the
    # empty slab a non-zero A row and a wrong by-product error (0 instead of the full error)
    from oracle import aoadmm_oracle as orc

    V = np.arange(12.0).reshape(6, 2)
    np.testing.assert_array_equal(orc.segment_sums(V, [0, 2, 2, 5, 6, 6]), [[2, 4], [0, 0], [18, 21], [10, 11], [0, 0]])
    c = E.MS_CASES["empty_r3"]
    _, X, row_ptr = E.ms_problem(c["I"], c["J_range"], c["K"], c["r"], c["seed"])
    st = orc.random_state_for(X.astype(np.float64), row_ptr, 3, [[], [], []], l2=[0.1, 0.2, 0.05])
    orc.run(st, 3, tol=None, absolute_tol=None)
    assert np.all(st.A[1] == 0.0)
    assert abs(st.rec_error_from_A_byproducts() - st.rec_error_full()) < 1e-12
