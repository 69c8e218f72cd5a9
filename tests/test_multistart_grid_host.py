"""CPU: cmf_aoadmm_grid / parafac2_aoadmm_grid / best_start host logic with the checker engine - the sequential method is the
single call per grid point and start, every error comes before any work, and the fused method refuses what one launch cannot
hold (what its kernel does not serve, two state layouts in one grid, too much memory) before anything touches a device."""
import functools

import numpy as np
import pytest

import matcouply_amd
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
    monkeypatch.setattr(_engine, "multistart_run_grid", refuse)


@pytest.fixture
def no_fits(monkeypatch, no_device):
    @functools.wraps(dec.cmf_aoadmm)  # (the keyword parser reads cmf_aoadmm's signature)
    def refuse(*args, **kwargs):
        raise AssertionError("a fit was started")

    monkeypatch.setattr(dec, "cmf_aoadmm", refuse)


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


GRID = [dict(l1_penalty={2: 0.05}, l2_penalty=[0.1, 0.1, 0.0]), dict(l1_penalty={2: 0.2}, l2_penalty=[0.1, 0.3, 0.0]),
        dict(l1_penalty={2: 0.1}, l2_penalty=0.02)]


def test_exported():
    for name in ("cmf_aoadmm_grid", "parafac2_aoadmm_grid", "best_start"):
        assert name in dec.__all__ and getattr(matcouply_amd, name) is getattr(dec, name)


@pytest.mark.parametrize("common", [
    dict(non_negative={0: True, 1: True}, n_iter_max=4, return_errors=True),
    dict(non_negative=True, n_iter_max=3, tol=None, return_errors=True, return_admm_vars=True),
    dict(n_iter_max=2),
])
def test_sequential_is_the_single_call_per_point_and_start(checker_engine, common):
    mats = _mats()
    seeds = [3, 7, 11]
    got = dec.cmf_aoadmm_grid(mats, 2, GRID, seeds, method="sequential", **common)
    assert isinstance(got, list) and len(got) == len(GRID) and all(isinstance(g, list) and len(g) == 3 for g in got)
    for point, per_start in zip(GRID, got):
        for rs, res in zip(seeds, per_start):
            _same(res, dec.cmf_aoadmm(mats, 2, random_state=rs, **common, **point))


def test_parafac2_sequential_matches_parafac2_aoadmm(checker_engine):
    mats = _mats()
    grid = [dict(l1_penalty={2: 0.05}), dict(l1_penalty={2: 0.2}, l2_penalty=[0.1, 0.0, 0.1])]
    common = dict(n_iter_max=3, non_negative=True, return_errors=True)
    got = dec.parafac2_aoadmm_grid(mats, 2, grid, range(2), method="sequential", **common)
    assert len(got) == 2
    for point, per_start in zip(grid, got):
        for s, res in enumerate(per_start):
            _same(res, dec.parafac2_aoadmm(mats, 2, random_state=s, **common, **point))
    with pytest.raises(TypeError, match="parafac2"):
        dec.parafac2_aoadmm_grid(mats, 2, grid, range(2), parafac2=True)
    with pytest.raises(TypeError, match="parafac2"):
        dec.parafac2_aoadmm_grid(mats, 2, [dict(parafac2=True)], range(2))


def test_auto_falls_back_to_sequential_with_a_checker_engine(checker_engine, no_device):
    mats = _mats()
    got = dec.cmf_aoadmm_grid(mats, 2, GRID[:2], [0], n_iter_max=2, non_negative=True)
    for point, per_start in zip(GRID, got):
        _same(per_start[0], dec.cmf_aoadmm(mats, 2, random_state=0, n_iter_max=2, non_negative=True, **point))
    with pytest.raises(NotImplementedError, match="substitute"):
        dec.cmf_aoadmm_grid(mats, 2, GRID[:2], [0], method="fused", n_iter_max=2)


def test_empty_grid_and_no_starts(no_fits):
    assert dec.cmf_aoadmm_grid(_mats(), 2, [], range(3)) == []
    assert dec.parafac2_aoadmm_grid(_mats(), 2, [], range(3), method="fused") == []
    assert dec.cmf_aoadmm_grid(_mats(), 2, GRID, [], method="sequential") == [[], [], []]


class _UserNN(pen.NonNegativity):
    def factor_matrix_row_update(self, factor_matrix_row, feasibility_penalty, aux_row):
        return super().factor_matrix_row_update(factor_matrix_row, feasibility_penalty, aux_row)


@pytest.mark.parametrize("point, common, match", [
    (dict(unimodal={1: True}), {}, "grid point 1.*Unimodality"),
    (dict(tv_penalty={2: 0.1}), {}, "grid point 1.*TotalVariation"),
    (dict(generalized_l2_penalty={2: np.eye(8)}), {}, "grid point 1.*GeneralizedL2"),
    (dict(regs=[[], [], [pen.UnitSimplex()]]), {}, "grid point 1.*UnitSimplex"),
    (dict(regs=[[], [], [_UserNN()]]), {}, "grid point 1.*_UserNN"),
    (dict(arithmetic="exact"), {}, "grid point 1.*arithmetic"),
    (dict(l2_norm_bound={0: 1.0}), {}, "grid point 1.*constant_feasibility_penalty"),
    (dict(l1_penalty=0.2), dict(verbose=True), "grid point 0.*verbose"),
    (dict(l1_penalty=0.2), dict(group=object()), "grid point 0.*group"),
    (dict(l1_penalty=0.2), dict(rank=17), "grid point 0.*rank"),
    (dict(l1_penalty=0.2), dict(parafac2=True, rank=7), "J_i >= rank"),
    (dict(l1_penalty=0.2), dict(shapes=((600, 500),)), "elements"),
])
def test_fused_refuses_what_the_kernel_does_not_serve(no_fits, point, common, match):
    common = dict(common)
    rank = common.pop("rank", 2)
    mats = _mats(common.pop("shapes", ((6, 8), (9, 8), (7, 8))))
    with pytest.raises(NotImplementedError, match=match):
        dec.cmf_aoadmm_grid(mats, rank, [dict(l1_penalty=0.1), point], range(3), method="fused", n_iter_max=2, **common)


@pytest.mark.parametrize("grid, common, match", [
    ([dict(l1_penalty={2: 0.1}), dict(l1_penalty={2: 0.3}), dict(l1_penalty={2: 0})], {}, "grid point 2 .* mode 2"),
    ([dict(l1_penalty={2: 0.1}), dict(l1_penalty={2: None})], {}, "grid point 1 .* mode 2"),
    ([dict(l1_penalty=0.1), dict(l1_penalty=[0.1, 0, 0.1])], {}, "grid point 1 .* mode 1"),
    ([dict(l1_penalty=0.1), dict(l1_penalty=0.1, non_negative={0: True})], {}, "grid point 1 .* mode 0"),
    ([dict(lower_bound=0.0, upper_bound=1.0), dict(non_negative=True)], {}, "grid point 1 .* mode 0"),  # Box beside NonNegativity
    ([dict(regs=[[pen.NonNegativity(), pen.L1Penalty(0.1)], [], []]), dict(regs=[[pen.L1Penalty(0.1), pen.NonNegativity()], [], []])],
     {}, "grid point 1 .* mode 0"),  # the same penalties in another order
    ([dict(l2_norm_bound=1.0, constant_feasibility_penalty=True), dict(l2_norm_bound=2.0, constant_feasibility_penalty="A")],
     {}, "grid point 1 .*constant_feasibility_penalty"),
    ([dict(update_C=True), dict(update_C=False)], dict(non_negative=True), "grid point 1 .* mode 2"),
])
def test_fused_refuses_a_grid_of_two_layouts_and_auto_runs_it_sequentially(no_device, monkeypatch, grid, common, match):
    mats = _mats()
    with pytest.raises(NotImplementedError, match=match):
        dec.cmf_aoadmm_grid(mats, 2, grid, range(2), method="fused", n_iter_max=2, **common)
    calls = []
    monkeypatch.setattr(dec, "cmf_aoadmm", functools.wraps(dec.cmf_aoadmm)(lambda m, r, **kw: calls.append(kw) or len(calls)))
    got = dec.cmf_aoadmm_grid(mats, 2, grid, range(2), method="auto", n_iter_max=2, **common)
    assert got == [[2 * g + 1, 2 * g + 2] for g in range(len(grid))]
    assert calls == [dict(random_state=s, n_iter_max=2, **common, **point) for point in grid for s in range(2)]


def test_the_issue_s_mixed_layout_grid(no_fits):
    # l1_penalty 0 drops the penalty in the parser: not one layout with 0.1
    with pytest.raises(NotImplementedError, match=r"grid point 1 .*\[\].* mode 2.*\['L1Penalty'\]"):
        dec.cmf_aoadmm_grid(_mats(), 2, [dict(l1_penalty={2: 0.1}), dict(l1_penalty={2: 0})], range(2), method="fused")


def test_one_layout_is_not_refused_for_its_strengths(no_device):
    mats = _mats()
    kws = [dec._cmf_kwargs(dict(non_negative={0: True}, lower_bound={1: lo}, upper_bound={1: 2.0}, l1_penalty={2: l1},
                                l2_penalty=l2, feasibility_penalty_scale=sc, tol=tol, n_iter_max=n, inner_n_iter_max=inner,
                                inner_tol=itol, feasibility_tol=ftol, absolute_tol=atol))
           for lo, l1, l2, sc, tol, n, inner, itol, ftol, atol in [(-0.5, 0.1, None, 1, 1e-8, 10, 5, None, 1e-4, 1e-10),
                                                                    (0.0, 0.3, [0.1, 0.2, 0.3], 0.5, None, 50, 3, 1e-3, 1e-2, 1e-6),
                                                                    (-2.0, 1e-3, 0.7, 2, 1e-4, 0, 7, None, None, 1e-12)]]
    assert ms._grid_unfused_reason(mats, 2, kws, 4) is None


def test_fused_refuses_a_grid_beyond_the_memory_bound(no_fits, monkeypatch):
    mats = _mats()
    grid = [dict(l1_penalty=v) for v in (0.1, 0.2, 0.3)]
    kws = [dec._cmf_kwargs(dict(p, n_iter_max=9)) for p in grid]
    assert ms._grid_unfused_reason(mats, 2, kws, 2) is None
    # one job: state 2 * (3 + 22 + 8) doubles of factors + 2 x that of aux and dual, scratch, 10 rows of diagnostics, options
    I, N, K, r = 3, 22, 8, 2
    per_job = 8 * (3 * (I + N + K) * r + _engine.multistart_scratch_len(I, N, K, r) + 10 * _engine.MS_DIAG) + _engine.MS_OPTIONS_BYTES
    monkeypatch.setattr(ms, "_GRID_MAX_BYTES", 6 * per_job)
    assert ms._grid_unfused_reason(mats, 2, kws, 2) is None
    monkeypatch.setattr(ms, "_GRID_MAX_BYTES", 6 * per_job - 1)
    with pytest.raises(NotImplementedError, match="6 jobs of"):
        dec.cmf_aoadmm_grid(mats, 2, grid, range(2), method="fused", n_iter_max=9)
    assert ms._GRID_MAX_BYTES <= 1 << 33


def test_scratch_len_restates_the_kernel_s_plan():
    # ms_scratch of csrc/multistart.hip: every piece rounded up to 32 doubles
    al = lambda n: (n + 31) // 32 * 32
    I, N, K, r = 10, 150, 20, 3
    assert _engine.multistart_scratch_len(I, N, K, r) == 2 * al(N * r) + al(K * r) + 4 * al(I * r * r) + 2 * al(I) + 2 * al(I * r) \
        + al(8 * r * r + 64)
    assert _engine.MS_OPTIONS_BYTES == 16 + 3 * _engine.MCL_MAX_REGS * 24 + 24 + 5 * 8 + 8 * 4


def test_auto_counts_jobs_not_starts(no_device, monkeypatch):
    # above _MULTISTART_AUTO_ANY_N elements auto wants _MULTISTART_AUTO_MIN_N fits in the launch: 4 points x 2 starts are 8
    mats = _mats(((100, 100),))
    assert 100 * 100 > ms._MULTISTART_AUTO_ANY_N and ms._MULTISTART_AUTO_MIN_N == 8
    calls = []
    monkeypatch.setattr(ms, "_multistart_fused", lambda m, r, rs, kws, run: calls.append(  # the launch: options per job
        (len(kws), len(rs), run is _engine.multistart_run_grid)) or [("job", g, s) for g in range(len(kws)) for s in range(len(rs))])
    monkeypatch.setattr(dec, "cmf_aoadmm", functools.wraps(dec.cmf_aoadmm)(
        lambda m, r, random_state, **kw: ("call", kw["l1_penalty"], random_state)))
    grid = [dict(l1_penalty=v) for v in (0.1, 0.2, 0.3, 0.4)]
    assert dec.cmf_aoadmm_grid(mats, 2, grid, range(2), n_iter_max=2) == [[("job", g, s) for s in range(2)] for g in range(4)]
    assert calls == [(4, 2, True)]
    assert dec.cmf_aoadmm_grid(mats, 2, grid[:3], range(2), n_iter_max=2) == [[("call", v, s) for s in range(2)] for v in (0.1, 0.2, 0.3)]
    assert calls == [(4, 2, True)]


@pytest.mark.parametrize("method", ["auto", "fused", "sequential"])
def test_errors_before_any_work(no_fits, method):
    mats, grid = _mats(), [dict(l1_penalty=0.1), dict(l1_penalty=0.2)]
    run = lambda g, **kw: dec.cmf_aoadmm_grid(mats, 2, g, range(2), method=method, **kw)
    with pytest.raises(TypeError, match="random_states"):
        run(grid, random_state=0)
    with pytest.raises(TypeError, match=r"random_states.*param_grid\[1\]"):
        run([grid[0], dict(l1_penalty=0.2, random_state=1)])
    for init in ("svd", "parafac_als", (None, (np.ones((3, 2)), None, None))):
        with pytest.raises(ValueError, match="init"):
            run(grid, init=init)
        with pytest.raises(ValueError, match=r"(?s)init.*param_grid\[0\]"):
            run([dict(init=init), grid[1]])
    with pytest.raises(TypeError, match=r"'l1_penalty' both in param_grid\[0\]"):
        run(grid, l1_penalty=0.3)
    for key, value in (("return_errors", True), ("return_admm_vars", True), ("verbose", False), ("group", None)):
        with pytest.raises(ValueError, match=rf"'{key}' in param_grid\[1\]"):
            run([grid[0], dict(grid[1], **{key: value})])
    with pytest.raises(TypeError, match="no_such_option"):
        run([grid[0], dict(no_such_option=1)])
    with pytest.raises(TypeError, match=r"param_grid\[1\] is a float"):
        run([grid[0], 0.2])
    with pytest.raises(ValueError, match="method"):
        dec.cmf_aoadmm_grid(mats, 2, grid, range(2), method="parallel")


def _diag(loss, satisfied):
    return dec.DiagnosticMetrics(rec_errors=[1.0, loss], feasibility_gaps=[], regularized_loss=[2.0, loss],
                                 satisfied_stopping_condition=satisfied, satisfied_feasibility_condition=True, n_iter=1,
                                 message="")


def test_best_start():
    cmf = object()
    results = [(cmf, _diag(0.3, True)), (cmf, _diag(0.1, False)), (cmf, _diag(0.2, True)), (cmf, _diag(0.2, True)),
               (cmf, _diag(0.05, None))]
    assert dec.best_start(results) == 2
    assert dec.best_start(results[:2]) == 0
    assert dec.best_start([(cmf, _diag(0.1, False)), (cmf, _diag(0.2, None))]) is None
    assert dec.best_start([]) is None
    # with the ADMM variables in between, as return_admm_vars gives them
    assert dec.best_start([(cmf, dec.ADMMVars((), ()), _diag(0.3, True)), (cmf, dec.ADMMVars((), ()), _diag(0.2, True))]) == 1
    with pytest.raises(ValueError, match="return_errors"):
        dec.best_start([cmf, cmf])
    with pytest.raises(ValueError, match="return_errors"):
        dec.best_start([(cmf, dec.ADMMVars((), ()))])


# ---- the C entry point checks its jobs before it touches the device ----------------------------------------------------------
def _c_options(n):
    import ctypes

    kw = dec._cmf_kwargs(dict(n_iter_max=3))
    nn, l1 = (_engine.PEN_NN, False, 0.0, 0.0), (_engine.PEN_L1, False, 0.1, 0.0)
    array = (_engine.MultistartOptions * n)(*[ms._multistart_options(kw, [[nn], [], [l1]]) for _ in range(n)])
    row_ptr = np.array([0, 5, 9], dtype=np.int64)
    return ctypes, array, row_ptr, row_ptr.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))


def _c_run(array, rp, n):
    lib = _engine.load_library()
    rc = lib.mcl_multistart_run_grid(None, 0, rp, 2, 8, 3, array, n, None, None, None, None, None, 0, None)
    return rc, lib.mcl_multistart_last_error().decode()


def test_c_grid_workspace_holds_the_options_behind_the_plan_of_a_run():
    ctypes, array, row_ptr, rp = _c_options(5)
    lib = _engine.load_library()
    plain = lib.mcl_multistart_workspace_bytes(rp, 2, 8, 3, ctypes.byref(array[0]), 5)
    grid = lib.mcl_multistart_grid_workspace_bytes(rp, 2, 8, 3, array, 5)
    assert plain > 0 and grid == plain + (5 * _engine.MS_OPTIONS_BYTES + 255) // 256 * 256
    # strengths, tolerances and limits of their own are one layout
    array[3].regs[2][0].p0, array[3].l2_penalty[1], array[3].n_iter_max, array[3].tol = 0.7, 0.3, 50, 1e-5
    array[4].feasibility_penalty_scale, array[4].inner_n_iter_max, array[4].evaluate_loss_always = 2.0, 9, 1
    assert lib.mcl_multistart_grid_workspace_bytes(rp, 2, 8, 3, array, 5) == grid
    rc, message = _c_run(array, rp, 5)
    assert rc != 0 and "NULL argument" in message  # the checks passed; nothing to run on


@pytest.mark.parametrize("change", ["n_regs", "kind", "non_negativity", "constant_A", "constant_B", "update_A", "update_B", "update_C"])
def test_c_grid_refuses_jobs_of_two_layouts(change):
    ctypes, array, row_ptr, rp = _c_options(4)
    job = array[2]
    if change == "n_regs":
        job.n_regs[1] = 1
        job.regs[1][0].kind = _engine.PEN_NN
    elif change == "kind":
        job.regs[0][0].kind = _engine.PEN_BOX
    elif change == "non_negativity":
        job.regs[2][0].non_negativity = 1
    else:
        setattr(job, change, 0 if getattr(job, change) else 1)
    assert _engine.load_library().mcl_multistart_grid_workspace_bytes(rp, 2, 8, 3, array, 4) == -1
    rc, message = _c_run(array, rp, 4)
    assert rc != 0 and message.startswith("mcl_multistart_run_grid: job 2 differs from job 0")


def test_c_grid_checks_every_job():
    ctypes, array, row_ptr, rp = _c_options(3)
    for job in array:
        job.regs[0][0].kind = _engine.PEN_UNIMODAL  # the same layout in all jobs, and not served
    rc, message = _c_run(array, rp, 3)
    assert rc != 0 and "job 0: penalty kind 5 is not served" in message
    ctypes, array, row_ptr, rp = _c_options(3)
    array[1].n_iter_max = -1
    rc, message = _c_run(array, rp, 3)
    assert rc != 0 and "job 1: need inner_n_iter_max >= 0 and n_iter_max >= 0" in message
    assert _c_run(array, rp, 0)[0] != 0
