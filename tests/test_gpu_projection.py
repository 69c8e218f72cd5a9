"""GPU: parafac2_project with method="device" (csrc/projection.hip) against the float64 restatement of
tests/projection_restatement.py at every rank bucket, segment edge and column path, 16-bit X, the stop of every matrix, the bitwise
promises, a fitted parafac2_als model end to end, and the C-ABI refusals.  tests/test_projection_host.py shows on the CPU that
every fixture used here moves by less than 1e-6 under the float32 rounding of W."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from matcouply_amd import _engine, decomposition as dec, evaluation as ev, projection as pj
from tests import projection_restatement as R

pytestmark = pytest.mark.gpu

MODES = {"three": dict(n_iter_max=3, tol=0.0), "converged": {}}
BAR = {"three": 1e-5, "converged": 1e-4}  # relative, per matrix: the project's flat bar, and its bar for converged runs
E2_BAR = 1e-7  # absolute, on e2
CASES = [(rank, K) for rank in R.RANKS for K in R.columns_of(rank, device=True)]
K_BELOW_RANK = [(rank, K) for rank in R.RANKS for K in R.columns_of(rank) if K < rank]  # refused by the device, served by the host


def _rel(got, want):
    return np.linalg.norm(np.asarray(got, dtype=np.float64) - want) / max(np.linalg.norm(want), 1e-300)


@functools.lru_cache(maxsize=None)
def _reference(rank, K, mode):
    f = R.parity_fixture(rank, K)
    return f, R.project(f["Xs"], f["Delta"], f["C"], np.ones(rank), **MODES[mode])


def _f32(Xs):
    return [X.astype(np.float32) for X in Xs]


def _engine_run(Xs, f, a_init, dtype=torch.float32, n_iter_max=100, tol=1e-8, absolute_tol=1e-13):
    """the entry point alone on packed data: (A, B, P, stats, n_iter, errors) on the device"""
    row_ptr = np.concatenate([[0], np.cumsum([len(X) for X in Xs])]).astype(np.int64)
    X = torch.from_numpy(np.concatenate(Xs, 0)).to(dtype).cuda()
    up = lambda M: torch.from_numpy(np.ascontiguousarray(M, dtype=np.float64)).cuda()
    start = np.broadcast_to(a_init, (len(Xs), f["Delta"].shape[0]))
    return _engine.pf2_project(X, row_ptr, f["Delta"].shape[0], up(f["Delta"]), up(f["C"]), up(start), n_iter_max, tol, absolute_tol, True)


def _same(a, b):
    """bitwise, NaN = NaN"""
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(a.contiguous().reshape(-1).view(torch.uint8), b.contiguous().reshape(-1).view(torch.uint8)))


@functools.lru_cache(maxsize=None)
def _device_run(rank, K, mode):
    f, _ = _reference(rank, K, mode)
    return pj.parafac2_project(_f32(f["Xs"]), (f["Delta"], f["C"]), a_init=np.ones(rank), method="device", return_errors=True, **MODES[mode])


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("rank,K", CASES)
def test_parity_at_every_rank_bucket_row_edge_and_column_path(rank, K, mode):
    (f, want), got = _reference(rank, K, mode), _device_run(rank, K, mode)
    assert got.cmf[1][0].dtype == np.float32 and got.slab_sse.dtype == np.float64 and got.errors.shape == (6, MODES[mode].get("n_iter_max", 100))
    worst = np.zeros(3)
    for i, w in enumerate(want):
        assert np.isnan(got.errors[i, got.n_iter[i]:]).all() and np.isfinite(got.errors[i, :got.n_iter[i]]).all()
        worst = np.maximum(worst, [_rel(got.cmf[1][0][i], w["a"]), _rel(got.cmf[1][1][i], w["B"]), _rel(got.projections[i], w["P"])])
        assert abs(got.slab_norm[i] - w["nx"]) <= 1e-12 * w["nx"]
    print(f"rank {rank} K {K} {mode}: a {worst[0]:.2e} B_new {worst[1]:.2e} P {worst[2]:.2e}")
    assert worst.max() <= BAR[mode]


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("rank,K", CASES)
def test_e2_is_within_1e_7_of_the_residual_itself(rank, K, mode):
    """e2 of the formula (nx - 2 a^T d + a^T S a) / nx against the residual of the restatement, held to 1e-7 absolute.  From the
    fp32 W alone the matrices of one to four rows would miss it (4.8e-7 measured at rank 1, K 68, J 2: nothing averages the
    roundings of W out), so the kernel forms W in fp64 for the matrices with J r < 4 K; measured with that: 2.8e-8 at worst."""
    (f, want), got = _reference(rank, K, mode), _device_run(rank, K, mode)
    diff = np.empty(len(want))
    for i, w in enumerate(want):
        e2 = got.slab_sse[i] / got.slab_norm[i]
        assert abs(e2 - got.errors[i, got.n_iter[i] - 1]) <= 1e-14
        diff[i] = abs(e2 - w["errors"][-1])
    print(f"rank {rank} K {K} {mode}: e2 {diff.max():.2e} at J {len(f['Xs'][int(diff.argmax())])}")
    assert diff.max() <= E2_BAR


@pytest.mark.parametrize("rank,K", K_BELOW_RANK)
def test_K_below_the_rank_is_refused_by_the_device_and_served_by_the_host(rank, K):
    f = R.parity_fixture(rank, K)
    model, Xs = (f["Delta"], f["C"]), _f32(f["Xs"])
    with pytest.raises(NotImplementedError, match=f"K = {K} is below the rank {rank}"):
        pj.parafac2_project(Xs, model, method="device")
    with pytest.raises(_engine.EngineError, match=f"rank {rank} exceeds K = {K}"):  # the entry itself, before any launch
        _engine_run(f["Xs"], f, np.ones(rank))
    want = R.project(f["Xs"], f["Delta"], f["C"], np.ones(rank), **MODES["three"])
    got = pj.parafac2_project(f["Xs"] * 2, model, a_init=np.ones(rank), **MODES["three"])  # "auto", 12 matrices, a device present
    for i, w in enumerate(want):
        assert _rel(got.cmf[1][0][i], w["a"]) <= 1e-9 and abs(got.slab_sse[i] - w["sse"]) <= 1e-9 * w["nx"]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("rank,K", [(3, 9), (3, 16), (17, 33), (17, 68)])
def test_16_bit_X_is_the_float32_run_on_its_values_bit_for_bit(rank, K, dtype):
    f = R.parity_fixture(rank, K)
    Xs = [torch.from_numpy(X).to(dtype) for X in f["Xs"]]  # rounded once; both runs see these values
    as_16 = _engine_run([X.float().numpy() for X in Xs], f, np.ones(rank), dtype=dtype)
    as_32 = _engine_run([X.float().numpy() for X in Xs], f, np.ones(rank))
    assert all(_same(a, b) for a, b in zip(as_16, as_32))
    out = pj.parafac2_project(Xs, (f["Delta"], f["C"]), a_init=np.ones(rank), method="device")  # used as stored; results in its dtype
    assert out.cmf[1][0].dtype == dtype and out.projections[0].dtype == dtype
    assert np.array_equal(out.slab_sse, as_32[3][:, 0].cpu().numpy()) and np.array_equal(out.n_iter, as_32[4].cpu().numpy())


@pytest.mark.parametrize("tol", sorted(R.STOP_SEEDS))
def test_every_matrix_stops_where_the_restatement_stops(tol):
    f = R.stopping_fixture(tol)
    want = R.project(f["Xs"], f["Delta"], f["C"], np.ones(3), tol=tol)
    assert len({w["n_iter"] for w in want}) >= 4
    for w in want:  # at least 10 % away from the tolerance on both sides
        assert w["criteria"][-1] <= 0.9 * tol and (w["n_iter"] == 2 or w["criteria"][-2] >= 1.1 * tol) and w["n_iter"] < 100
    got = pj.parafac2_project(_f32(f["Xs"]), (f["Delta"], f["C"]), a_init=np.ones(3), tol=tol, method="device", return_errors=True)
    print("n_iter", got.n_iter.tolist(), "restatement", [w["n_iter"] for w in want])
    assert got.n_iter.tolist() == [w["n_iter"] for w in want]
    for i, w in enumerate(want):
        k = w["n_iter"]
        assert np.isfinite(got.errors[i, :k]).all() and np.isnan(got.errors[i, k:]).all()
        assert np.abs(got.errors[i, :k] - w["errors"]).max() <= E2_BAR and (np.diff(got.errors[i, :k]) <= 1e-7).all()
        assert _rel(got.cmf[1][0][i], w["a"]) <= 1e-4 and _rel(got.cmf[1][1][i], w["B"]) <= 1e-4


@pytest.fixture(scope="module")
def three_hundred():
    rows = [[5, 6, 20, 64, 65, 70][i % 6] for i in range(300)]
    f = R.fixture(7, rows, 12, 5)
    return f, _engine_run(f["Xs"], f, np.ones(5))


def test_a_matrix_does_not_depend_on_the_call_it_is_in(three_hundred):
    f, (A, B, P, stats, n_iter, errors) = three_hundred
    row_ptr = np.concatenate([[0], np.cumsum([len(X) for X in f["Xs"]])])
    assert len(set(n_iter.tolist())) > 1
    for i in (0, 137, 299):
        a, b, p, s, n, e = _engine_run(f["Xs"][i: i + 1], f, np.ones(5))
        lo, hi = row_ptr[i], row_ptr[i + 1]
        assert _same(a[0], A[i]) and _same(b, B[lo:hi]) and _same(p, P[lo:hi]) and _same(s[0], stats[i]) and _same(n[0], n_iter[i])
        assert _same(e[0], errors[i])


def test_two_runs_are_bitwise_equal(three_hundred):
    f, first = three_hundred
    assert all(_same(a, b) for a, b in zip(first, _engine_run(f["Xs"], f, np.ones(5))))


def test_a_fitted_parafac2_als_model_end_to_end():
    f = R.fixture(3, [10, 11, 12, 13, 14, 15, 16, 17], 12, 3)
    Xs = _f32(f["Xs"])
    fitted = dec.parafac2_als(Xs, 3, init="svd")
    out = pj.parafac2_project(Xs, fitted, a_init=fitted[1][0], method="device")
    fitted_sse = ev.slabwise_sse(fitted, Xs, method="device")
    print("projected sse - fitted sse, relative to |X_i|^2:", ((out.slab_sse - fitted_sse) / out.slab_norm).tolist(), "n_iter", out.n_iter.tolist())
    assert (out.slab_sse <= fitted_sse + 1e-6 * out.slab_norm).all()  # alternation cannot increase it
    assert (np.abs(ev.slabwise_sse(out.cmf, Xs, method="device") - out.slab_sse) <= 1e-6 * out.slab_norm).all()
    auto = pj.parafac2_project(Xs, fitted, a_init=fitted[1][0])  # "auto" with a device present is the device
    assert np.array_equal(auto.slab_sse, out.slab_sse) and auto.cmf[1][2].dtype == np.float32


def test_c_abi_refusals_launch_nothing_and_the_workspace_is_what_the_size_function_says():
    f = R.parity_fixture(3, 9)
    Xs, r, K, I = f["Xs"], 3, 9, 6
    lib = _engine.load_library()
    row_ptr = np.concatenate([[0], np.cumsum([len(X) for X in Xs])]).astype(np.int64)
    N, n_max = int(row_ptr[-1]), 7
    rp = lambda a: np.ascontiguousarray(a, dtype=np.int64).ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
    X = torch.from_numpy(np.concatenate(Xs, 0)).float().cuda()
    up = lambda M: torch.from_numpy(np.ascontiguousarray(M, dtype=np.float64)).cuda()
    Delta, C, a0 = up(f["Delta"]), up(f["C"]), up(np.ones((I, r)))
    nbytes = lib.mcl_pf2_project_workspace_bytes(rp(row_ptr), I, K, r)
    assert nbytes > 0
    guard = 4096
    buf = torch.full((nbytes + 2 * guard + 256,), 0xA5, dtype=torch.uint8, device="cuda")
    lo = guard + (-(buf.data_ptr() + guard)) % 256
    wp = buf.data_ptr() + lo
    filled = lambda dtype, *shape: torch.full(shape, -7, dtype=dtype, device="cuda")
    A, B, P = filled(torch.float64, I, r), filled(torch.float32, N, r), filled(torch.float32, N, r)
    stats, n_iter, errors = filled(torch.float64, I, 2), filled(torch.int32, I), filled(torch.float64, I, n_max)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    bad = {name: t.clone() for name, t in (("Delta", Delta), ("C", C), ("a_init", a0))}
    bad["Delta"][1, 2], bad["C"][4, 0], bad["a_init"][5, 1] = float("inf"), float("nan"), float("-inf")
    short = np.array(row_ptr)
    short[1:] -= 1  # the first matrix has rank - 1 rows
    good = dict(X=X.data_ptr(), xt=_engine.X_F32, rp=rp(row_ptr), I=I, K=K, r=r, Delta=Delta.data_ptr(), C=C.data_ptr(), a_init=a0.data_ptr(),
                n_iter_max=n_max, tol=1e-8, absolute_tol=1e-13, A=A.data_ptr(), B=B.data_ptr(), P=P.data_ptr(), stats=stats.data_ptr(),
                n_iter=n_iter.data_ptr(), errors=errors.data_ptr(), ws=wp, ws_bytes=nbytes, stream=stream)
    call = lambda **kw: lib.mcl_pf2_project_typed(*{**good, **kw}.values())
    for change, message in [(dict(r=0), b"rank 0"), (dict(r=33), b"rank 33"), (dict(rp=rp(short)), b"at least rank rows"), (dict(xt=7), b"x_type"),
                            (dict(n_iter_max=0), b"n_iter_max >= 1"), (dict(tol=-1.0), b"tol >= 0"), (dict(absolute_tol=-1.0), b"absolute_tol >= 0"),
                            (dict(ws_bytes=nbytes - 1), b"workspace too small"), (dict(ws=wp + 8), b"aligned"), (dict(X=None), b"NULL"),
                            (dict(stats=None), b"NULL"), (dict(Delta=bad["Delta"].data_ptr()), b"Delta holds a non-finite"),
                            (dict(C=bad["C"].data_ptr()), b"C holds a non-finite"), (dict(a_init=bad["a_init"].data_ptr()), b"a_init holds a non-finite")]:
        assert call(**change) != 0, change
        assert message in lib.mcl_pf2_project_last_error(), (change, lib.mcl_pf2_project_last_error())
    torch.cuda.synchronize()
    for t in (A, B, P, stats, n_iter, errors):
        assert bool((t == -7).all())  # nothing was launched
    assert bool((buf == 0xA5).all())
    assert call() == 0 and call(errors=None) == 0  # the errors are optional
    torch.cuda.synchronize()
    assert bool((buf[:lo] == 0xA5).all()) and bool((buf[lo + nbytes:] == 0xA5).all())  # the guard bytes around the workspace
    want = _engine_run(Xs, f, np.ones(r), n_iter_max=n_max)
    assert all(_same(a, b) for a, b in zip((A, B, P, stats, n_iter, errors), want))
