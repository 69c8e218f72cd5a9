"""GPU: parafac2_als_resample with the fused kernel k_ms_pf2als_weighted (csrc/pf2als_multistart.hip)
against the fp64 NumPy restatement (tests/parafac2_als_restatement.py) run on sqrt(w_i) X_i from the start A0 sqrt(w), with its
A divided back: parity per job, the unweighted kernel's bits with all weights 1, bitwise independence of the batch, 16-bit X,
zero-weight matrices, every rank and the kernel's edges, the default stopping rule, the public surface, resources and rate."""
import os
import sys
import time

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from matcouply_amd import _engine  # noqa: E402
from matcouply_amd import decomposition as dec  # noqa: E402
from matcouply_amd import multistart as ms  # noqa: E402
from matcouply_amd import resampling as rs  # noqa: E402
from matcouply_amd.projection import parafac2_project  # noqa: E402
from tests import parafac2_als_restatement as R  # noqa: E402

pytestmark = pytest.mark.gpu

NOISE = 0.2
SMALL = dict(I=6, J_range=(8, 20), K=12, rank=3, seed=2)
# the bars of tests/test_gpu_pf2als_multistart.py for this kernel: the added arithmetic is one multiply
FAC_BAR, ERR_BAR = 5e-6, 1e-7
# weights from {0, 0.5, 1, 2, 3}, a zero first and a zero last, one row per job
SMALL_WEIGHTS = np.array([[0, 2, 0.5, 3, 1, 0], [0, 1, 1, 0.5, 2, 0], [0, 3, 0, 1, 0.5, 0], [0, 0.5, 2, 2, 3, 0]], dtype=np.float64)
SMALL_STARTS = [0, 1, 2, 3]


def problem(p, nonneg=False, J=None):
    """float64 copies of the float32 matrices: the results come back in float64, unrounded"""
    mats = R.parafac2_problem(p["I"], p.get("J_range"), p["K"], p["rank"], seed=p["seed"], noise=NOISE, nonneg=nonneg, J=J)[0]
    return [m.astype(np.float64) for m in mats]


def _packed(mats, dtype=torch.float32):
    row_ptr = np.concatenate([[0], np.cumsum([m.shape[0] for m in mats])]).astype(np.int64)
    X = torch.from_numpy(np.concatenate(mats, 0)).to("cuda").to(dtype).contiguous()
    return dec.PackedMatrices(X, row_ptr)


def _np(x):
    return np.asarray(x.cpu() if hasattr(x, "cpu") else x, dtype=np.float64)


def _rel(a, b):
    return np.linalg.norm(_np(a) - b) / np.linalg.norm(b)


def reference(mats, rank, w, start, drop=False, **kw):
    """the restatement of the problem weighted by w: run on sqrt(w_i) X_i from (A0 sqrt(w), B0, C0), A divided back, zeros in the
    row of A and the P_i of a zero-weight matrix.  drop: the zero-weight matrices are taken out of the list, not scaled to zero.
    -> (A, B, C, [P_i], e_t, e_t^2)"""
    w = np.asarray(w, dtype=np.float64)
    s = np.sqrt(w)
    A0, B0, C0 = start
    keep = np.flatnonzero(w > 0) if drop else np.arange(len(w))
    out = R.parafac2_als([s[i] * mats[i] for i in keep], rank, factors=(A0[keep] * s[keep][:, None], B0, C0), **kw)
    A = np.zeros((len(w), rank))
    P = [np.zeros((m.shape[0], rank)) for m in mats]
    for k, i in enumerate(keep):
        if w[i] > 0:
            A[i] = out[0][k] / s[i]
            P[i] = out[3][k]
        else:
            assert not out[0][k].any() and not out[3][k].any()  # the identity keeps them at exact zeros
    return (A, out[1], out[2], P, out[4], out[5])


def differences(res, ref):
    """relative differences of A, B, C and the stacked P_i B, and the largest difference of e_t"""
    (_, (A, B, C), P), errors = res
    rA, rB, rC, rP, rerr = ref[:5]
    PB = np.concatenate([_np(p) @ _np(B) for p in P])
    rPB = np.concatenate([p @ rB for p in rP])
    assert len(errors) == len(rerr), (len(errors), len(rerr))
    de = np.abs(np.asarray(errors) - rerr).max() if len(rerr) else 0.0
    return [_rel(A, rA), _rel(B, rB), _rel(C, rC), _rel(PB, rPB)], de


def _fused(data, rank, weights, starts, **kw):
    out = rs.parafac2_als_resample(data, rank, weights, starts=starts, method="fused", return_errors=True, **kw)
    torch.cuda.synchronize()
    return out


def _zero_rows_are_zero(res, w):
    (_, (A, _, _), P), _ = res
    for i in np.flatnonzero(np.asarray(w) == 0):
        assert not _np(A)[i].any() and not _np(P[i]).any(), i


# ---- parity -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_iter", [3, 50])
@pytest.mark.parametrize("nn_modes", [None, [0], [0, 2]], ids=["als", "nn0", "nn02"])
def test_parity_from_random_states(nn_modes, n_iter):
    mats = problem(SMALL)
    kw = dict(n_iter_max=n_iter, tol=1e-300, absolute_tol=0, nn_modes=nn_modes)
    got = _fused(mats, SMALL["rank"], SMALL_WEIGHTS, SMALL_STARTS, **kw)  # float64 lists: float64 results
    worst = [0.0, 0.0]
    for w, seed, res in zip(SMALL_WEIGHTS, SMALL_STARTS, got):
        ref = reference(mats, SMALL["rank"], w, R.start(mats, SMALL["rank"], "random", seed), **kw)
        assert len(res[1]) == n_iter
        errs, de = differences(res, ref)
        _zero_rows_are_zero(res, w)
        worst = [max(worst[0], max(errs)), max(worst[1], de)]
    print(f"random states {nn_modes} {n_iter} iterations: factors {worst[0]:.2e}, e_t {worst[1]:.2e}")
    assert worst[0] < FAC_BAR and worst[1] < ERR_BAR, worst


def converged_model(mats, rank, nn_modes):
    """the restatement's unweighted fit, far enough to sit in its basin: what a user passes as `starts`"""
    return R.parafac2_als(mats, rank, n_iter_max=300, tol=0, nn_modes=nn_modes, random_state=0)[:3]


# From a converged model the polar factors are well conditioned and nothing amplifies the rounding.  Measured (DESIGN.md section
# 17): the restatement's own sensitivity to a relative 1e-16 of the start is at most WARM_SENSITIVITY, the device differs from
# the restatement by at most WARM_MEASURED; the bars are ten times the larger figure of each pair.
WARM_SENSITIVITY = (6.5e-13, 2.0e-13)  # (factors, e_t)
WARM_MEASURED = (6.7e-13, 1.6e-13)
WARM_FAC_BAR, WARM_ERR_BAR = (10 * max(a, b) for a, b in zip(WARM_SENSITIVITY, WARM_MEASURED))


@pytest.mark.parametrize("n_iter", [3, 50])
@pytest.mark.parametrize("nn_modes", [None, [0], [0, 2]], ids=["als", "nn0", "nn02"])
def test_parity_from_a_converged_model(nn_modes, n_iter):
    mats = problem(SMALL)
    model = converged_model(mats, SMALL["rank"], nn_modes)
    kw = dict(n_iter_max=n_iter, tol=1e-300, absolute_tol=0, nn_modes=nn_modes)
    got = _fused(mats, SMALL["rank"], SMALL_WEIGHTS, model, **kw)
    worst = [0.0, 0.0]
    for w, res in zip(SMALL_WEIGHTS, got):
        errs, de = differences(res, reference(mats, SMALL["rank"], w, model, **kw))
        _zero_rows_are_zero(res, w)
        worst = [max(worst[0], max(errs)), max(worst[1], de)]
    print(f"converged model {nn_modes} {n_iter} iterations: factors {worst[0]:.2e}, e_t {worst[1]:.2e}")
    assert worst[0] < WARM_FAC_BAR and worst[1] < WARM_ERR_BAR, worst


@pytest.mark.parametrize("nn_modes", [None, [0], [0, 2]], ids=["als", "nn0", "nn02"])
def test_zero_weight_matrices_are_left_out(nn_modes):
    # exact zeros in their row of A and their P_i; B, C, the other rows and e_t are those of the list WITHOUT them
    mats = problem(SMALL)
    kw = dict(n_iter_max=20, tol=1e-300, absolute_tol=0, nn_modes=nn_modes)
    got = _fused(mats, SMALL["rank"], SMALL_WEIGHTS, SMALL_STARTS, **kw)
    for w, seed, res in zip(SMALL_WEIGHTS, SMALL_STARTS, got):
        (_, (A, _, _), P), _ = res
        for i in np.flatnonzero(w == 0):
            assert np.array_equal(A[i], np.zeros(SMALL["rank"])) and np.array_equal(P[i], np.zeros_like(P[i])), i
        assert all(np.isfinite(F).all() for F in (A, res[0][1][1], res[0][1][2], *P))
        ref = reference(mats, SMALL["rank"], w, R.start(mats, SMALL["rank"], "random", seed), drop=True, **kw)
        errs, de = differences(res, ref)
        print(f"zero weights {nn_modes} job {seed}: factors {max(errs):.2e}, e_t {de:.2e}")
        assert max(errs) < FAC_BAR and de < ERR_BAR, (seed, errs, de)


# ---- the engine entry: bits -------------------------------------------------------------------------------------------------------
def _start_factors(packed, rank, seeds, scale=None):
    I, K = len(packed), int(packed.X.shape[1])
    rows = []
    for j, s in enumerate(seeds):
        A0, B0, C0 = dec._pf2als_random_start(I, K, rank, s)
        if scale is not None:
            A0 = A0 * scale[j][:, None]
        rows.append(np.concatenate([np.ravel(F) for F in (A0, B0, C0)]))
    return torch.from_numpy(np.stack(rows)).cuda()


def _engine_run(packed, rank, seeds, weights, n_iter_max=30, tol=1e-300, nn_modes=(0,)):
    """-> [factors, P, errors, n_iter] of mcl_pf2als_multistart_run_weighted; weights None: of mcl_pf2als_multistart_run"""
    if weights is None:
        factors = _start_factors(packed, rank, seeds)
        P, errors, n_iter = _engine.pf2als_multistart_run(packed.X, packed.row_ptr, rank, factors, n_iter_max, 5, tol, 0.0, nn_modes)
    else:
        scale = np.sqrt(np.asarray(weights, dtype=np.float64))
        factors = _start_factors(packed, rank, seeds, scale)
        P, errors, n_iter = _engine.pf2als_multistart_run_weighted(packed.X, packed.row_ptr, rank, factors, torch.from_numpy(scale).cuda(),
                                                                   n_iter_max, 5, tol, 0.0, nn_modes)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in (factors, P, errors, n_iter)]


@pytest.mark.parametrize("tol", [1e-300, 1e-6])
@pytest.mark.parametrize("nn_modes", [(), (0, 2)], ids=["als", "nn02"])
def test_all_ones_is_the_unweighted_run_bit_for_bit(nn_modes, tol):
    packed = _packed(problem(SMALL))
    seeds = range(8)
    plain = _engine_run(packed, SMALL["rank"], seeds, None, tol=tol, nn_modes=nn_modes)
    ones = _engine_run(packed, SMALL["rank"], seeds, np.ones((8, SMALL["I"])), tol=tol, nn_modes=nn_modes)
    assert all(np.array_equal(a, b) for a, b in zip(plain, ones))
    assert plain[3].min() >= 2


def _batch_weights(n, I, seed=0):
    rng = np.random.RandomState(seed)
    w = rng.choice([0.0, 0.5, 1.0, 2.0, 3.0], size=(n, I))
    w[np.arange(n), rng.randint(0, I, size=n)] = 1.0  # every job keeps a matrix
    return w


def test_job_alone_equals_job_in_a_batch_and_runs_repeat():
    packed = _packed(problem(SMALL))
    w = _batch_weights(64, SMALL["I"])
    batch = _engine_run(packed, SMALL["rank"], range(64), w)
    again = _engine_run(packed, SMALL["rank"], range(64), w)
    assert all(np.array_equal(a, b) for a, b in zip(batch, again))
    other = _batch_weights(64, SMALL["I"], seed=1)  # the neighbours get other weights: nothing changes for the job
    for s in (0, 17, 63):
        alone = _engine_run(packed, SMALL["rank"], [s], w[s: s + 1])
        assert all(np.array_equal(a[0], b[s]) for a, b in zip(alone, batch)), s
        other[s] = w[s]
    mixed = _engine_run(packed, SMALL["rank"], range(64), other)
    for s in (0, 17, 63):
        assert all(np.array_equal(a[s], b[s]) for a, b in zip(mixed, batch)), s


MID = dict(I=24, J_range=(40, 100), K=64, rank=8, seed=0)


@pytest.mark.parametrize("dtype", ["bfloat16", "float16"])
def test_x16_is_the_run_of_the_upcast(dtype):
    p16 = _packed(problem(MID), getattr(torch, dtype))
    p32 = dec.PackedMatrices(p16.X.float().contiguous(), p16.row_ptr)
    w = _batch_weights(4, MID["I"])
    a = _engine_run(p16, MID["rank"], range(4), w, n_iter_max=10)
    b = _engine_run(p32, MID["rank"], range(4), w, n_iter_max=10)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


# ---- every rank, the kernel's edges -------------------------------------------------------------------------------------------------
# Start seeds are kept only where a relative 1e-16 of the start moves the restatement's own result by less than a fifth of the bars
# (DESIGN.md section 17): the seeds 0 and 1, except where one of them fails that rule
RANK_SEEDS = {3: [0, 2], 12: [0, 2], 13: [2, 1], 14: [0, 3]}


def rank_case(rank):
    """k_ms_pf2als_weighted<R, fp32>: I = 5, J_i in 16-30, K = 20, one zero weight"""
    mats = problem(dict(I=5, J_range=(16, 30), K=20, rank=rank, seed=rank))
    return mats, rank, np.array([[2.0, 1.0, 0.0, 0.5, 3.0], [1.0, 0.0, 3.0, 2.0, 0.5]]), RANK_SEEDS.get(rank, [0, 1])


@pytest.mark.parametrize("rank", range(1, 17))
def test_every_rank(rank):
    mats, rank, weights, seeds = rank_case(rank)
    kw = dict(n_iter_max=3, tol=1e-300, absolute_tol=0)
    got = _fused(mats, rank, weights, seeds, **kw)
    for w, s, res in zip(weights, seeds, got):
        errs, de = differences(res, reference(mats, rank, w, R.start(mats, rank, "random", s), **kw))
        _zero_rows_are_zero(res, w)
        print(f"rank {rank} job {s}: factors {max(errs):.2e}, e_t {de:.2e}")
        assert max(errs) < FAC_BAR and de < ERR_BAR, (rank, s, errs, de)


def _cycled(I, seed):
    """weights of I matrices from {0, 0.5, 1, 2, 3}, about a fifth of them zero"""
    return np.random.RandomState(seed).permutation(np.resize([2.0, 0.0, 1.0, 0.5, 3.0], I))[None]


# name -> (problem, weights [n_jobs, I], start seeds: the first that pass the rule of RANK_SEEDS).  The polar steps run in batches of nb = min(256, 40960 / (16 R^2)) slabs:
# nb = 10 at rank 16 and 256 at rank 2.
EDGES = {
    "polar_batch_rank16": (dict(I=11, J_range=(16, 24), K=18, rank=16, seed=1), _cycled(11, 0), [1]),  # I = nb + 1
    "polar_batch_rank2": (dict(I=257, K=3, rank=2, seed=0, J=[2] * 257), _cycled(257, 1), [0]),  # I = nb + 1, 2 x 3 matrices
    "below_a_block": (dict(I=3, J_range=(4, 6), K=5, rank=2, seed=0), np.array([[1.0, 0.0, 2.0], [0.5, 3.0, 1.0]]), [0, 2]),  # N, I K < 256
    "off_the_block": (dict(I=7, J_range=(38, 44), K=37, rank=3, seed=0), _cycled(7, 2), [0]),  # N = 286, I K = 259
    "rows_equal_rank": (dict(I=5, K=9, rank=4, seed=0, J=[4] * 5), np.array([[3.0, 1.0, 0.0, 0.5, 2.0]]), [0]),  # J_i == rank
    "one_matrix": (dict(I=1, J_range=(10, 10), K=8, rank=1, seed=0), np.array([[3.0]]), [0]),  # I = 1 with weight 3
    "one_positive_weight": (dict(I=5, J_range=(8, 12), K=8, rank=1, seed=0), np.array([[0.0, 0.0, 2.0, 0.0, 0.0]]), [0]),
}


def edge_case(name):
    p, weights, seeds = EDGES[name]
    return problem(p, J=p.get("J")), p["rank"], weights, seeds


@pytest.mark.parametrize("name", sorted(EDGES))
def test_kernel_edges(name):
    mats, rank, weights, seeds = edge_case(name)
    kw = dict(n_iter_max=3, tol=1e-300, absolute_tol=0)
    got = _fused(mats, rank, weights, seeds, **kw)
    for w, s, res in zip(weights, seeds, got):
        errs, de = differences(res, reference(mats, rank, w, R.start(mats, rank, "random", s), **kw))
        _zero_rows_are_zero(res, w)
        print(f"{name} job {s}: factors {max(errs):.2e}, e_t {de:.2e}")
        assert max(errs) < FAC_BAR and de < ERR_BAR, (name, s, errs, de)


# ---- stopping ---------------------------------------------------------------------------------------------------------------------
# A weighted fixture and starts on which the restatement's relative change of e^2 crosses the default tol = 1e-8 with at least a
# 10 % margin on both sides (asserted below): (rank, seed, I, J_range, K, weights, starts)
STOPPING = (1, 0, 8, (8, 20), 12, [2.0, 0.0, 1.0, 0.5, 3.0, 1.0, 0.0, 2.0], [0, 1, 2, 3])


def test_default_tol_stops_where_the_restatement_stops():
    rank, seed, I, J_range, K, w, seeds = STOPPING
    mats = [m.astype(np.float64) for m in R.parafac2_problem(I, J_range, K, rank, seed=seed, noise=NOISE)[0]]
    got = _fused(mats, rank, np.tile(w, (len(seeds), 1)), seeds)
    for s, res in zip(seeds, got):
        ref = reference(mats, rank, w, R.start(mats, rank, "random", s))
        rel = np.abs(np.diff(ref[5])) / ref[5][:-1]
        assert rel[-1] <= 0.9e-8 and rel[:-1].min() >= 1.1e-8, (s, rel[-1], rel[:-1].min())
        assert len(res[1]) == len(ref[4]), (s, len(res[1]), len(ref[4]))
        errs, de = differences(res, ref)
        assert de < ERR_BAR and max(errs) < FAC_BAR, (s, errs, de)


# ---- the public surface -----------------------------------------------------------------------------------------------------------
def test_fused_follows_sequential_on_a_fast_fixture():
    # the fixture of test_gpu_pf2als_multistart.test_fused_follows_sequential_on_a_fast_fixture, with weights
    mats = R.parafac2_problem(8, (8, 20), 12, 1, seed=0, noise=NOISE)[0]
    weights = np.array([[2.0, 0.0, 1.0, 0.5, 3.0, 1.0, 0.0, 2.0], [1.0] * 8, [0.0, 1.0, 1.0, 3.0, 0.5, 0.0, 2.0, 1.0], [3.0, 2.0, 0.5, 0.0, 0.0, 1.0, 1.0, 2.0]])
    kw = dict(tol=1e-5, return_errors=True)
    fused = rs.parafac2_als_resample(mats, 1, weights, starts=range(4), method="fused", **kw)
    seq = rs.parafac2_als_resample(mats, 1, weights, starts=range(4), method="sequential", **kw)
    for w, (f, ef), (q, eq) in zip(weights, fused, seq):
        assert len(ef) == len(eq), (len(ef), len(eq))
        for i, (a, b) in enumerate(zip([f[1][0], f[1][1], f[1][2], *f[2]], [q[1][0], q[1][1], q[1][2], *q[2]])):
            if i >= 3 and w[i - 3] == 0:
                assert not a.any() and not b.any()
            else:
                assert _rel(a, _np(b)) < 5e-5
        assert not f[1][0][w == 0].any() and not q[1][0][w == 0].any()


@pytest.mark.parametrize("method", ["fused", "sequential"])
@pytest.mark.parametrize("kind", ["numpy64", "numpy32", "torch_cpu", "torch_cuda", "packed"])
def test_return_types_match_parafac2_als(kind, method):
    mats = problem(SMALL)
    if kind == "numpy64":
        data = [m.astype(np.float64) for m in mats]
    elif kind == "numpy32":
        data = [m.astype(np.float32) for m in mats]
    elif kind == "torch_cpu":
        data = [torch.from_numpy(m) for m in mats]
    elif kind == "torch_cuda":
        data = [torch.from_numpy(m).cuda() for m in mats]
    else:
        data = _packed(mats)
    r = SMALL["rank"]
    for errors in (False, True):
        got = rs.parafac2_als_resample(data, r, SMALL_WEIGHTS[:1], starts=[0], method=method, n_iter_max=5, return_errors=errors)[0]
        single = dec.parafac2_als(data, r, random_state=0, n_iter_max=5, return_errors=errors)

        def walk(a, b):
            assert type(a) is type(b), (type(a), type(b))
            if isinstance(a, (tuple, list)):
                assert len(a) == len(b)
                for x, y in zip(a, b):
                    walk(x, y)
            elif isinstance(a, np.ndarray) or torch.is_tensor(a):
                assert a.dtype == b.dtype and tuple(a.shape) == tuple(b.shape)
                if torch.is_tensor(a):
                    assert a.device == b.device

        walk(got, single)


def test_kfold_heldout_sse_is_parafac2_project_by_hand():
    mats = problem(dict(I=9, J_range=(8, 20), K=12, rank=2, seed=4))
    weights = rs.resampling_weights(9, "kfold", n=3, random_state=0)
    reps = rs.parafac2_als_resample(mats, 2, weights, starts=[0, 1, 2], method="fused", n_iter_max=50)
    for method in ("host", "device"):
        held = rs.resample_heldout_sse(mats, reps, weights, method=method)
        assert sorted(int(i) for h in held for i in h.indices) == list(range(9))
        for h, rep, w in zip(held, reps, weights):
            assert np.array_equal(h.indices, np.flatnonzero(w == 0))
            by_hand = parafac2_project([mats[i] for i in h.indices], (rep[1][1], rep[1][2]), method=method)
            assert np.array_equal(h.slab_sse, by_hand.slab_sse) and np.array_equal(h.slab_norm, by_hand.slab_norm)
            np.testing.assert_allclose(h.slab_norm, [np.sum(mats[i] ** 2) for i in h.indices], rtol=1e-6)
            assert (h.slab_sse > 0).all() and (h.slab_sse < h.slab_norm).all()


def test_summary_of_a_bootstrap_from_the_fitted_model():
    # end to end: replicates started from the fitted model stay lined up with it; the summary's mean is near the model
    mats = problem(SMALL)
    model = dec.parafac2_als(mats, SMALL["rank"], random_state=0, n_iter_max=300, tol=0)
    weights = rs.resampling_weights(SMALL["I"], "bootstrap", n=16, random_state=0)
    reps = rs.parafac2_als_resample(mats, SMALL["rank"], weights, starts=model, method="fused", n_iter_max=100, tol=0)
    summary = rs.resample_summary(reps, model, weights)
    assert summary.C.mean.shape == model[1][2].shape and summary.C.quantiles.shape == (2,) + model[1][2].shape
    assert (summary.C.quantiles[0] <= summary.C.quantiles[1]).all() and np.isfinite(summary.C.std).all()
    assert (summary.fms > 0).all() and (summary.fms <= 1 + 1e-9).all()  # the rows of A and B_i a job left out cost score
    assert np.array_equal(summary.permutations, np.tile(np.arange(SMALL["rank"]), (16, 1)))  # the model's order is kept


# ---- resources, rate --------------------------------------------------------------------------------------------------------------
def test_no_scratch_in_the_weighted_kernel():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import kernel_resources

    ks = [k for k in kernel_resources.resources() if k["kernel"].startswith("k_ms_pf2als_weighted<")]
    assert len(ks) == 48, [k["kernel"] for k in ks]  # ranks 1..16 x {fp32, bf16, fp16}
    assert not any(kernel_resources.is_hot(k["kernel"]) for k in ks)
    spilled = [(k["kernel"], k["scratch_bytes"], k["vgpr_spill"]) for k in ks if k["scratch_bytes"] or k["vgpr_spill"]]
    assert not spilled, spilled


def semiconductor_problem():
    """the size of the reference's semiconductor example (tests/test_gpu_pf2als_multistart.semiconductor_problem)"""
    mats = R.parafac2_problem(108, (100, 120), 21, 2, seed=3, noise=NOISE)[0]
    assert sum(m.size for m in mats) <= ms._MULTISTART_MAX_ELEMENTS
    return mats


# 64 fused bootstrap jobs against 64 sequential ones (4 timed, scaled) at the semiconductor size, 200 iterations, tol = 0,
# nn_modes=[0]: measured 71.2 ms against 3.52 s, ratio 0.0202 (profiles/pf2als_resample_rate.txt); the guard is twice that, the
# headroom the other rate guards leave for the spread between boxes
RATE_MEASURED = 0.0202
RATE_GUARD = 2 * RATE_MEASURED


def test_rate_guard_semiconductor_size():
    mats = semiconductor_problem()
    weights = rs.resampling_weights(len(mats), "bootstrap", n=64, random_state=0)
    kw = dict(n_iter_max=200, tol=0, nn_modes=[0])
    rs.parafac2_als_resample(mats, 2, weights, starts=range(64), method="fused", **kw)  # warm-up
    rs.parafac2_als_resample(mats, 2, weights[:1], starts=range(1), method="sequential", **kw)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    t_fused = timed(lambda: rs.parafac2_als_resample(mats, 2, weights, starts=range(64), method="fused", **kw))
    t_seq = 16 * timed(lambda: rs.parafac2_als_resample(mats, 2, weights[:4], starts=range(4), method="sequential", **kw))
    print(f"64 jobs: fused {t_fused * 1e3:.1f} ms, sequential {t_seq * 1e3:.1f} ms, ratio {t_fused / t_seq:.4f}")
    assert t_fused <= RATE_GUARD * t_seq, (t_fused, t_seq)
