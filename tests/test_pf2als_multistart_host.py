"""CPU: parafac2_als_multistart host logic - every refusal and bad argument raises before anything touches a device, the
sequential method is one parafac2_als call per start, and the Python restatement of the per-start workspace layout agrees with
the library's."""
import numpy as np
import pytest

from matcouply_amd import _engine, decomposition as dec, multistart as ms
from tests.oracle_engine import OracleEngineFactory


@pytest.fixture
def no_device(monkeypatch):
    def refuse(*args, **kwargs):
        raise AssertionError("the device was touched")

    monkeypatch.setattr(dec, "_device", refuse)
    monkeypatch.setattr(_engine, "pf2als_multistart_run", refuse)
    monkeypatch.setattr(_engine, "parafac2_als", refuse)


def _mats(shapes=((5, 10), (8, 10), (6, 10)), seed=0):
    rng = np.random.RandomState(seed)
    return [rng.random_sample(s) for s in shapes]


def test_exported():
    assert "parafac2_als_multistart" in dec.__all__


@pytest.mark.parametrize("method", ["auto", "fused", "sequential"])
def test_bad_arguments(no_device, method):
    with pytest.raises(TypeError, match="random_states"):
        dec.parafac2_als_multistart(_mats(), 2, range(2), method=method, random_state=0)
    with pytest.raises(TypeError, match="n_iter"):
        dec.parafac2_als_multistart(_mats(), 2, range(2), method=method, n_iter=3)
    for init in ("svd", None, "parafac2_als"):
        with pytest.raises(ValueError, match="init"):
            dec.parafac2_als_multistart(_mats(), 2, range(2), method=method, init=init)


def test_bad_method(no_device):
    with pytest.raises(ValueError, match="method"):
        dec.parafac2_als_multistart(_mats(), 2, range(2), method="parallel")


@pytest.mark.parametrize("method", ["auto", "fused", "sequential"])
@pytest.mark.parametrize("kw, rank, shapes, match", [
    (dict(nn_modes=[1]), 2, None, "mode 1"),
    (dict(nn_modes="all"), 2, None, "mode 1"),
    (dict(svd="randomized_svd"), 2, None, "svd"),
    (dict(normalize_factors=True), 2, None, "normalize_factors"),
    (dict(linesearch=True), 2, None, "linesearch"),
    (dict(verbose=True), 2, None, "verbose"),
    (dict(), 33, ((40, 40), (40, 40)), "32"),
    (dict(), 6, None, "J_i >= rank"),
    (dict(), 4, ((20, 3), (30, 3)), "K >= rank"),
])
def test_parafac2_als_refusals_raise_for_every_method(no_device, method, kw, rank, shapes, match):
    mats = _mats(shapes) if shapes else _mats()
    with pytest.raises(NotImplementedError, match=match):
        dec.parafac2_als_multistart(mats, rank, range(2), method=method, **kw)


@pytest.mark.parametrize("method", ["auto", "fused", "sequential"])
@pytest.mark.parametrize("kw", [dict(nn_modes=[3]), dict(n_iter_max=0), dict(n_iter_parafac=0)])
def test_bad_values_raise_for_every_method(no_device, method, kw):
    with pytest.raises(ValueError):
        dec.parafac2_als_multistart(_mats(), 2, range(2), method=method, **kw)


@pytest.mark.parametrize("rank, shapes, match", [
    (17, ((40, 20), (40, 20)), "rank 17"),
    (2, ((600, 500),), "elements"),
])
def test_fused_refuses_what_its_kernel_does_not_serve(no_device, rank, shapes, match):
    with pytest.raises(NotImplementedError, match=match):
        dec.parafac2_als_multistart(_mats(shapes), rank, range(3), method="fused")


def test_fused_refuses_under_a_substitute_engine(no_device, monkeypatch):
    monkeypatch.setattr(dec, "_ENGINE_FACTORY", OracleEngineFactory())
    with pytest.raises(NotImplementedError, match="substitute"):
        dec.parafac2_als_multistart(_mats(), 2, range(2), method="fused")


class _Recorder:
    def __init__(self):
        self.calls = []

    def __call__(self, matrices, rank, **kwargs):
        self.calls.append((matrices, rank, kwargs))
        return ("fit", len(self.calls))


@pytest.mark.parametrize("method", ["sequential", "auto"])
def test_sequential_is_one_parafac2_als_call_per_start(no_device, monkeypatch, method):
    rec = _Recorder()
    monkeypatch.setattr(dec, "parafac2_als", rec)
    if method == "auto":  # auto falls back to the loop when the fused kernel cannot serve the call
        monkeypatch.setattr(dec, "_ENGINE_FACTORY", OracleEngineFactory())
    mats = _mats()
    seeds = [3, 7, np.random.RandomState(11)]
    kw = dict(n_iter_max=7, tol=1e-6, nn_modes=[0, 2], n_iter_parafac=2, return_errors=True)
    got = dec.parafac2_als_multistart(mats, 2, seeds, method=method, **kw)
    assert got == [("fit", 1), ("fit", 2), ("fit", 3)]
    assert [c[2]["random_state"] for c in rec.calls] == seeds
    for m, r, kwargs in rec.calls:
        assert m is mats and r == 2
        assert {k: v for k, v in kwargs.items() if k != "random_state"} == kw


def test_no_starts_is_an_empty_list(no_device, monkeypatch):
    monkeypatch.setattr(dec, "parafac2_als", _Recorder())
    assert dec.parafac2_als_multistart(_mats(), 2, [], method="sequential") == []


def test_random_start_is_parafac2_als_draw():
    A, B, C = dec._pf2als_random_start(4, 6, 3, 5)
    rs = np.random.RandomState(5)
    for got, shape in zip((A, B, C), ((4, 3), (3, 3), (6, 3))):
        np.testing.assert_array_equal(got, rs.uniform(size=shape))


@pytest.mark.parametrize("I, J, K, rank, n_starts", [(3, (5, 9, 6), 10, 2, 1), (108, None, 21, 2, 64), (7, None, 33, 16, 5),
                                                     (1, (16,), 16, 16, 3)])
def test_workspace_layout_matches_the_library(I, J, K, rank, n_starts):
    rng = np.random.RandomState(0)
    J = np.asarray(J if J is not None else rng.randint(rank, 3 * rank + 20, size=I), dtype=np.int64)
    row_ptr = np.concatenate([[0], np.cumsum(J)]).astype(np.int64)
    N = int(row_ptr[-1])
    r = rank
    scratch = _engine.pf2als_multistart_scratch_len(I, N, K, r)
    assert scratch >= N * r + I * r * K + 3 * I * r * r + I * r + K * r
    assert scratch % 32 == 0
    import ctypes

    lib = _engine.load_library()
    rp = row_ptr.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
    assert lib.mcl_pf2als_multistart_workspace_bytes(rp, I, K, r, n_starts) == \
        _engine.pf2als_multistart_workspace_bytes(I, N, K, r, n_starts)
    assert lib.mcl_pf2als_multistart_workspace_bytes(rp, I, K, 17, n_starts) == -1
    assert lib.mcl_pf2als_multistart_workspace_bytes(rp, I, K, r, 0) == -1


def test_workspace_refuses_unserved_shapes():
    import ctypes

    lib = _engine.load_library()
    row_ptr = np.array([0, 3, 8], dtype=np.int64)  # J = 3, 5
    rp = row_ptr.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
    assert lib.mcl_pf2als_multistart_workspace_bytes(rp, 2, 6, 3, 1) > 0
    assert lib.mcl_pf2als_multistart_workspace_bytes(rp, 2, 6, 4, 1) == -1  # J_0 < rank
    assert lib.mcl_pf2als_multistart_workspace_bytes(rp, 2, 2, 3, 1) == -1  # K < rank


def test_auto_takes_the_loop_for_few_starts_of_a_large_problem(no_device, monkeypatch):
    # 64 x 64 x 64 at rank 8: one fused start is 5.1 x one call (profiles/pf2als_multistart_rate.txt)
    rec = _Recorder()
    monkeypatch.setattr(dec, "parafac2_als", rec)
    mats = _mats(((64, 64),) * 64)
    assert len(dec.parafac2_als_multistart(mats, 8, range(ms._PF2ALS_MS_AUTO_MIN_N - 1))) == ms._PF2ALS_MS_AUTO_MIN_N - 1
    with pytest.raises(AssertionError, match="device was touched"):  # from _PF2ALS_MS_AUTO_MIN_N starts: the fused kernel
        dec.parafac2_als_multistart(mats, 8, range(ms._PF2ALS_MS_AUTO_MIN_N))
    with pytest.raises(AssertionError, match="device was touched"):  # semiconductor-sized work: fused from the first start
        dec.parafac2_als_multistart(_mats(((110, 21),) * 108), 2, [0])
