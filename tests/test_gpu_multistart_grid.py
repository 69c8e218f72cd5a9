"""GPU: cmf_aoadmm_grid / parafac2_aoadmm_grid with the fused kernel (csrc/multistart.hip, mcl_multistart_run_grid: options of
its own for every workgroup) - oracle parity per job, bitwise independence of a job from its grid, per-job stopping, 16-bit X
and the rate against one cmf_aoadmm_multistart call per grid point."""
import statistics
import time

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from matcouply_amd import decomposition as dec  # noqa: E402
from oracle import aoadmm_oracle as orc  # noqa: E402
from tests.test_gpu_multistart import STACKS, _example_problem, _oracle_state, _ragged  # noqa: E402

pytestmark = pytest.mark.gpu

# per stack of tests/test_gpu_multistart.py: (keywords common to the grid, grid points).  Every point sets the strengths of its
# stack and feasibility_penalty_scale in {0.5, 1, 2}; the first point is the stack itself
GRIDS = {
    "nn_l1C": (dict(non_negative={0: True, 1: True}),
               [dict(l1_penalty={2: 0.05}, feasibility_penalty_scale=1), dict(l1_penalty={2: 0.2}, feasibility_penalty_scale=0.5),
                dict(l1_penalty={2: 0.01}, feasibility_penalty_scale=2), dict(l1_penalty={2: 0.5}, feasibility_penalty_scale=2,
                                                                              inner_n_iter_max=3)]),
    "box_l2ball": (dict(constant_feasibility_penalty=True),
                   [dict(lower_bound={1: -0.5}, upper_bound={1: 2.0}, l2_norm_bound={0: 3.0, 2: 2.0}, feasibility_penalty_scale=1),
                    dict(lower_bound={1: -0.1}, upper_bound={1: 1.0}, l2_norm_bound={0: 2.0, 2: 1.0}, feasibility_penalty_scale=2),
                    dict(lower_bound={1: 0.0}, upper_bound={1: 0.8}, l2_norm_bound={0: 5.0, 2: 3.0}, feasibility_penalty_scale=0.5)]),
    "parafac2_nn": (dict(parafac2=True, non_negative=True),
                    [dict(feasibility_penalty_scale=1), dict(feasibility_penalty_scale=0.5, l2_penalty=[0.0, 0.0, 0.1]),
                     dict(feasibility_penalty_scale=2, l2_penalty=[0.05, 0.0, 0.0]), dict(feasibility_penalty_scale=2, l2_penalty=0.2)]),
    "ridge_constant": (dict(non_negative={2: True}, constant_feasibility_penalty=True),
                       [dict(l2_penalty=[0.1, 0.2, 0.05], feasibility_penalty_scale=1),
                        dict(l2_penalty=[1.0, 0.01, 0.3], feasibility_penalty_scale=0.5),
                        dict(l2_penalty=[0.01, 0.5, 0.0], feasibility_penalty_scale=2)]),
}


def test_the_grids_start_from_the_stacks():
    for stack, (common, grid) in GRIDS.items():
        first = dict(common, **grid[0])
        first.pop("feasibility_penalty_scale")
        assert first == STACKS[stack] and len(grid) >= 3
        assert {p["feasibility_penalty_scale"] for p in grid} == {0.5, 1, 2}


@pytest.mark.parametrize("stack", sorted(GRIDS))
def test_oracle_parity_per_job(stack):
    """every job of a grid of strengths x 4 starts against the fp64 oracle from the same start with that grid point's options, at
    the bar of test_oracle_parity_per_start: 1e-5 flat on factors, rec_errors, losses and (with the 1e-3 floor) gaps"""
    mats, X, row_ptr = _ragged()
    rank = 3
    common, grid = GRIDS[stack]
    run = dict(n_iter_max=20, tol=None, return_errors=True)
    got = dec.cmf_aoadmm_grid(mats, rank, grid, range(4), method="fused", **common, **run)
    assert len(got) == len(grid) and all(len(g) == 4 for g in got)
    rel = lambda a, b: np.linalg.norm(np.asarray(a) - b) / max(np.linalg.norm(b), 1e-300)
    worst = 0.0
    for g, point in enumerate(grid):
        kw = dict(common, **point, **run)
        for s, (cmf, diag) in enumerate(got[g]):
            st = _oracle_state(mats, X, row_ptr, rank, s, kw)
            res = orc.run(st, 20, tol=None, absolute_tol=None)
            _, (A, B_is, C) = cmf
            errs = [rel(A, st.A), rel(np.concatenate(B_is), st.B), rel(C, st.C),
                    np.max(np.abs(np.array(diag.rec_errors) - res["rec_errors"]) / np.array(res["rec_errors"])),
                    np.max(np.abs(np.array(diag.regularized_loss) - res["losses"]) / np.array(res["losses"]))]
            for g_got, g_ref in zip(diag.feasibility_gaps, res["gaps"]):
                for m in range(3):
                    if len(g_ref[m]):
                        errs.append(np.max(np.abs(np.array(g_got[m]) - g_ref[m]) / np.maximum(np.abs(g_ref[m]), 1e-3)))
            assert diag.n_iter == 20 and diag.satisfied_stopping_condition is False
            assert len(diag.feasibility_gaps) == 21 and len(diag.rec_errors) == 21
            worst = max(worst, max(errs))
            print(f"{stack} point {g} start {s}: worst relative difference {max(errs):.2e}")
            assert max(errs) < 1e-5, (stack, g, s, errs)
    print(f"{stack}: worst of all jobs {worst:.2e}")
    # the grid points are different problems: their fits differ
    assert all(got[0][0][1].regularized_loss[-1] != got[g][0][1].regularized_loss[-1] for g in range(1, len(grid)))


def _bits(res):
    """everything a fit returns with return_errors and return_admm_vars, as bytes / exact values"""
    cmf, admm, diag = res
    _, (A, B_is, C) = cmf
    flat = lambda x: [y for e in x for y in flat(e)] if isinstance(x, (list, tuple)) else [x]
    arrays = [A, *B_is, C] + flat(list(admm.auxes)) + flat(list(admm.duals))
    return [np.asarray(a).tobytes() for a in arrays] + [np.array(diag.regularized_loss).tobytes(), np.array(diag.rec_errors).tobytes(),
                                                        np.array(flat(diag.feasibility_gaps)).tobytes(), diag.n_iter, diag.message,
                                                        diag.satisfied_stopping_condition, diag.satisfied_feasibility_condition]


@pytest.mark.parametrize("stack", ["parafac2_nn", "box_l2ball"])
def test_one_point_grid_equals_multistart_bitwise(stack):
    # the options reach the kernel through device memory in a grid and through its arguments in cmf_aoadmm_multistart
    mats, _, _ = _ragged(seed=2)
    common, grid = GRIDS[stack]
    run = dict(n_iter_max=120, return_errors=True, return_admm_vars=True)
    point = grid[1]
    multi = dec.cmf_aoadmm_multistart(mats, 3, range(6), method="fused", **common, **point, **run)
    got = dec.cmf_aoadmm_grid(mats, 3, [point], range(6), method="fused", **common, **run)
    assert len(got) == 1 and len(got[0]) == 6
    for s in range(6):
        assert _bits(got[0][s]) == _bits(multi[s]), s
    # and with the point's keywords given as common ones
    again = dec.cmf_aoadmm_grid(mats, 3, [{}], range(6), method="fused", **common, **point, **run)
    assert all(_bits(a) == _bits(b) for a, b in zip(again[0], multi))


def test_job_alone_equals_job_in_a_grid_bitwise():
    # 9 points x 4 starts = 36 jobs whose points differ in strengths, tolerances, iteration limits and inner iterations
    mats, _, _ = _ragged(seed=2)
    common = dict(parafac2=True, non_negative={0: True, 2: True}, return_errors=True, return_admm_vars=True)
    grid = [dict(l1_penalty={1: l1}, l2_penalty=l2, feasibility_penalty_scale=sc, tol=tol, n_iter_max=n, inner_n_iter_max=inner,
                 feasibility_tol=ftol)
            for l1, l2, sc, tol, n, inner, ftol in [(0.01, 0, 1, 1e-8, 300, 5, 1e-4), (0.1, 0.1, 0.5, 1e-5, 200, 5, 1e-3),
                                                    (0.03, [0.1, 0, 0.2], 2, None, 40, 3, 1e-4), (0.3, 0.01, 1, 1e-3, 100, 8, 1e-2),
                                                    (0.02, 0, 4, 1e-8, 7, 5, 1e-4), (0.05, 0.5, 1, 1e-6, 150, 2, 1e-5),
                                                    (0.2, 0, 0.25, 1e-4, 0, 5, 1e-4), (0.15, 0.3, 1.5, None, 1, 5, None),
                                                    (0.07, 0.02, 1, 1e-7, 250, 6, 1e-4)]]
    seeds = [5, 6, 7, 8]
    batch = dec.cmf_aoadmm_grid(mats, 3, grid, seeds, method="fused", **common)
    again = dec.cmf_aoadmm_grid(mats, 3, grid, seeds, method="fused", **common)
    assert len(grid) * len(seeds) >= 32
    n_iters = {d.n_iter for per_start in batch for _, _, d in per_start}
    assert len(n_iters) > 4, n_iters  # the jobs do stop at different iterations
    for g, s in [(0, 0), (1, 3), (2, 1), (4, 2), (6, 0), (7, 3), (8, 3)]:
        alone = dec.cmf_aoadmm_grid(mats, 3, [grid[g]], [seeds[s]], method="fused", **common)[0][0]
        assert _bits(alone) == _bits(batch[g][s]), (g, s)
    # the same job beside other neighbours, at another place of the launch
    other = dec.cmf_aoadmm_grid(mats, 3, [grid[3], grid[1]], [seeds[3], seeds[0]], method="fused", **common)
    assert _bits(other[1][0]) == _bits(batch[1][3]) and _bits(other[0][1]) == _bits(batch[3][0])
    assert all(_bits(a) == _bits(b) for pa, pb in zip(batch, again) for a, b in zip(pa, pb))


def test_per_job_stopping_follows_the_oracle():
    """default-style tolerances on the simulated-nonnegative example: every job stops where the oracle stops with that grid
    point's tol and n_iter_max, with its verdict and message"""
    mats, rank = _example_problem(10, 15, 20, 3, 0.2, False), 3
    common = dict(non_negative=True, return_errors=True)
    grid = [dict(tol=1e-8, n_iter_max=1000), dict(tol=1e-5, n_iter_max=1000), dict(tol=1e-3, n_iter_max=400),
            dict(tol=1e-8, n_iter_max=25), dict(tol=1e-6, n_iter_max=120), dict(tol=None, n_iter_max=15)]
    got = dec.parafac2_aoadmm_grid(mats, rank, grid, range(3), method="fused", **common)
    X = np.concatenate(mats).astype(np.float32)
    row_ptr = np.concatenate([[0], np.cumsum([m.shape[0] for m in mats])])
    seen = set()
    for g, point in enumerate(grid):
        for s, (_, diag) in enumerate(got[g]):
            st = _oracle_state(mats, X, row_ptr, rank, s, dict(common, **point, parafac2=True, l2_penalty=0))
            res = orc.run(st, point["n_iter_max"], tol=point["tol"])
            print(f"point {g} {point} start {s}: n_iter {diag.n_iter} (oracle {res['n_iter']}), {diag.message}")
            assert diag.n_iter == res["n_iter"], (g, s)
            assert diag.satisfied_stopping_condition == res["satisfied_stopping_condition"], (g, s)
            assert diag.message == res["message"], (g, s)
            assert diag.satisfied_feasibility_condition == res["satisfied_feasibility_condition"], (g, s)
            assert len(diag.feasibility_gaps) == diag.n_iter + 1
            assert abs(diag.regularized_loss[-1] - res["losses"][-1]) <= 1e-8 * res["losses"][-1]
            seen.add((diag.n_iter, diag.message))
    assert len({m for _, m in seen}) >= 2 and len({n for n, _ in seen}) >= 4, seen  # stopped and exhausted jobs, many counts
    for g in (0, 1):
        best = dec.best_start(got[g])
        losses = [d.regularized_loss[-1] if d.satisfied_stopping_condition else np.inf for _, d in got[g]]
        assert best == (int(np.argmin(losses)) if np.isfinite(min(losses)) else None)
    assert dec.best_start(got[5]) is None  # tol=None: no stopping condition to satisfy


@pytest.mark.parametrize("dtype", ["bfloat16", "float16"])
def test_x16_equals_upcast(dtype):
    mats, _, _ = _ragged(seed=3)
    m16 = [torch.tensor(m, dtype=getattr(torch, dtype), device="cuda") for m in mats]
    m32 = [m.float() for m in m16]
    common, grid = GRIDS["nn_l1C"]
    run = dict(n_iter_max=50, return_errors=True, return_admm_vars=True)
    a = dec.cmf_aoadmm_grid(m16, 3, grid, range(3), method="fused", **common, **run)
    b = dec.cmf_aoadmm_grid(m32, 3, grid, range(3), method="fused", **common, **run)
    for pa, pb in zip(a, b):
        for (ca, _, da), (cb, _, db) in zip(pa, pb):
            # the fp64 diagnostics are bitwise equal; the factors come back in the input's dtype
            assert da.regularized_loss == db.regularized_loss and da.rec_errors == db.rec_errors
            assert da.feasibility_gaps == db.feasibility_gaps
            for x, y in zip([ca[1][0], *ca[1][1], ca[1][2]], [cb[1][0], *cb[1][1], cb[1][2]]):
                assert x.dtype == getattr(torch, dtype) and torch.equal(x, y.to(x.dtype))


def test_auto_takes_the_fused_grid_and_returns_the_single_call_s_types():
    mats, _, _ = _ragged(seed=4)
    common, grid = GRIDS["parafac2_nn"]
    run = dict(n_iter_max=5, return_errors=True, return_admm_vars=True)
    auto = dec.cmf_aoadmm_grid(mats, 3, grid, range(2), **common, **run)
    fused = dec.cmf_aoadmm_grid(mats, 3, grid, range(2), method="fused", **common, **run)
    assert all(_bits(a) == _bits(b) for pa, pb in zip(auto, fused) for a, b in zip(pa, pb))
    single = dec.cmf_aoadmm(mats, 3, random_state=1, **common, **grid[2], **run)

    def walk(a, b):
        assert type(a) is type(b), (type(a), type(b))
        if isinstance(a, (tuple, list)):
            assert len(a) == len(b)
            for x, y in zip(a, b):
                walk(x, y)
        elif isinstance(a, np.ndarray):
            assert a.dtype == b.dtype and a.shape == b.shape

    (cmf_f, admm_f, diag_f), (cmf_s, admm_s, diag_s) = fused[2][1], single
    walk(cmf_f[1], cmf_s[1])
    walk(admm_f.auxes, admm_s.auxes)
    walk(admm_f.duals, admm_s.duals)
    assert type(diag_f) is type(diag_s) and diag_f.n_iter == diag_s.n_iter
    assert len(diag_f.rec_errors) == len(diag_s.rec_errors) and len(diag_f.feasibility_gaps) == len(diag_s.feasibility_gaps)


# profiles/multistart_grid_rate.txt (tools/multistart_grid_rate.py): at the examples' shape (10 x 15 x 20, rank 3, NN PARAFAC2, 200
# iterations, tol=None) one fused grid of 16 points x 4 starts takes 65 ms against 472 ms for 16 cmf_aoadmm_multistart(
# method="fused") calls of 4 starts: a ratio of 0.137 (0.132 in this test's own first run; the repetitions of either way lie
# within 3 % of their median).  The guard is twice the measured ratio - small launches feel the host's noise, and machines differ
# by some 6 % - and far below 1: the grid must not lose to the loop it replaces
GRID_RATE_GUARD = 0.27


def rate_grid():
    return [dict(l2_penalty=l2, feasibility_penalty_scale=sc) for l2 in (0.0, 0.01, 0.1, 1.0) for sc in (0.5, 1, 2, 4)]


def test_rate_guard_examples_size():
    mats = _example_problem(10, 15, 20, 3, 0.2, False)
    common = dict(non_negative=True, n_iter_max=200, tol=None)
    grid = rate_grid()
    assert len(grid) == 16

    def fused_grid():
        return dec.parafac2_aoadmm_grid(mats, 3, grid, range(4), method="fused", **common)

    def loop():  # the way without the grid: one fused multi-start call per grid point
        return [dec.parafac2_aoadmm_multistart(mats, 3, range(4), method="fused", **common, **point) for point in grid]

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    a, b = fused_grid(), loop()  # warm-up of both (library load, code objects) and the same fits both ways
    for g in range(16):
        for s in range(4):
            np.testing.assert_array_equal(a[g][s][1][0], b[g][s][1][0])
    t_grid, t_loop = [], []
    for _ in range(7):  # alternating, so that a disturbance of the host meets both
        t_grid.append(timed(fused_grid))
        t_loop.append(timed(loop))
    m_grid, m_loop = statistics.median(t_grid), statistics.median(t_loop)
    print(f"grid {m_grid * 1e3:.1f} ms (min {min(t_grid) * 1e3:.1f}, max {max(t_grid) * 1e3:.1f}), 16 calls {m_loop * 1e3:.1f} ms "
          f"(min {min(t_loop) * 1e3:.1f}, max {max(t_loop) * 1e3:.1f}), ratio {m_grid / m_loop:.3f}")
    assert m_grid <= GRID_RATE_GUARD * m_loop, (m_grid, m_loop)
