"""GPU: parafac2_als (mcl_parafac2_als) against the fp64 NumPy restatement of its spec (tests/parafac2_als_restatement.py):
factors, error trajectory, stopping rule, non-negativity, determinism, 16-bit X, array types, an end-to-end start of
parafac2_aoadmm, scratch-free kernels and the rate of an iteration at the config-3 shape."""
import time

import numpy as np
import pytest

from tests import parafac2_als_restatement as R

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SMALL = dict(I=6, J_range=(8, 20), K=12, rank=3, seed=2)
MID = dict(I=48, J_range=(40, 160), K=96, rank=8, seed=0)
NOISE = 0.2  # e_t ~ 0.2, as for the CP initialisers (the fp32 X passes perturb e_t by about eps / e_t)


def _problem(p, nonneg=False):
    return R.parafac2_problem(p["I"], p["J_range"], p["K"], p["rank"], seed=p["seed"], noise=NOISE, nonneg=nonneg)[0]


def _packed(mats, dtype=torch.float32):
    from matcouply_amd.decomposition import PackedMatrices

    row_ptr = np.concatenate([[0], np.cumsum([m.shape[0] for m in mats])]).astype(np.int64)
    X = torch.from_numpy(np.concatenate(mats, 0)).to("cuda").to(dtype).contiguous()
    return PackedMatrices(X, row_ptr)


def _run(data, rank, **kw):
    from matcouply_amd.decomposition import parafac2_als

    kw.setdefault("random_state", 0)
    (w, (A, B, C), P), errors = parafac2_als(data, rank, return_errors=True, **kw)
    torch.cuda.synchronize()
    return A, B, C, P, np.asarray(errors)


def _np(x):
    return np.asarray(x.cpu() if hasattr(x, "cpu") else x, dtype=np.float64)


def _rel(a, b):
    return np.linalg.norm(_np(a) - b) / np.linalg.norm(b)


def _compare(dev, ref):
    A, B, C, P, _ = dev
    rA, rB, rC, rP = ref[:4]
    Bi = np.concatenate([_np(p) @ _np(B) for p in P])
    rBi = np.concatenate([p @ rB for p in rP])
    return _rel(A, rA), _rel(Bi, rBi), _rel(C, rC)


@pytest.mark.parametrize("init", ["svd", "random"])
@pytest.mark.parametrize("nn_modes", [None, [0], [0, 2]], ids=["als", "nn0", "nn02"])
@pytest.mark.parametrize("size", ["small", "mid"])
def test_parity_over_three_iterations(size, nn_modes, init):
    p = SMALL if size == "small" else MID
    mats = _problem(p)
    dev = _run(_packed(mats), p["rank"], n_iter_max=3, tol=1e-300, absolute_tol=0, init=init, nn_modes=nn_modes)
    ref = R.parafac2_als(mats, p["rank"], n_iter_max=3, tol=1e-300, absolute_tol=0, init=init, nn_modes=nn_modes, random_state=0)
    assert len(dev[4]) == 3
    errs = _compare(dev, ref)
    # The random start is far from the model and its first polar factors are poorly conditioned: the fp32 W = X C is
    # amplified to ~1.5e-5 in B_i and ~2.4e-7 in e_t at the mid size; the svd start meets 1e-5 / 1e-7
    fac, err = (1e-5, 1e-7) if init == "svd" or size == "small" else (5e-5, 5e-7)
    assert max(errs) < fac, errs
    assert np.abs(dev[4] - ref[4]).max() < err, (dev[4], ref[4])


@pytest.mark.parametrize("init", ["svd", "random"])
@pytest.mark.parametrize("nn_modes", [None, [0, 2]], ids=["als", "nn02"])
def test_parity_over_fifty_iterations(nn_modes, init):
    mats = _problem(MID)
    dev = _run(_packed(mats), MID["rank"], n_iter_max=50, tol=1e-300, absolute_tol=0, init=init, nn_modes=nn_modes)
    ref = R.parafac2_als(mats, MID["rank"], n_iter_max=50, tol=1e-300, absolute_tol=0, init=init, nn_modes=nn_modes, random_state=0)
    errs = _compare(dev, ref)
    assert max(errs) < 1e-4, errs
    # (random start: 1.4e-7 measured for nn_modes [0, 2], see test_parity_over_three_iterations)
    assert np.abs(dev[4] - ref[4]).max() < (1e-7 if init == "svd" else 5e-7), np.abs(dev[4] - ref[4]).max()


@pytest.mark.parametrize("rank,seed,tol", [(1, 0, 1e-5), (1, 1, 1e-5), (1, 2, 1e-5), (2, 0, 1e-4), (2, 1, 1e-4), (3, 1, 1e-4)])
def test_stopping(rank, seed, tol):
    # Fixtures on which the restatement's relative criterion is >= 10 % from tol on both sides at its stop.  The default
    # tol = 1e-8 is not used: e^2 = (|X|^2 - 2 <M_C, C> + fit) / |X|^2 carries the fp32 rounding of the X passes, ~1e-7 |X|^2,
    # so its relative change cannot be resolved to 1e-8
    mats = R.parafac2_problem(8, (8, 20), 12, rank, seed=seed, noise=NOISE)[0]
    ref = R.parafac2_als(mats, rank, random_state=0, tol=tol)
    rel = np.abs(np.diff(ref[5])) / ref[5][:-1]
    assert rel[-1] <= 0.9 * tol and rel[:-1].min() >= 1.1 * tol, (rel[-1], rel[:-1].min())
    dev = _run(mats, rank, tol=tol)
    assert len(dev[4]) == len(ref[4]), (len(dev[4]), len(ref[4]))
    assert np.abs(dev[4] - ref[4]).max() < 1e-7


def test_nonnegative_modes_and_determinism():
    packed = _packed(_problem(MID, nonneg=True))
    for modes in ([0], [2], [0, 2]):
        r1 = _run(packed, MID["rank"], n_iter_max=20, tol=0, nn_modes=modes)
        r2 = _run(packed, MID["rank"], n_iter_max=20, tol=0, nn_modes=modes)
        for m in modes:
            assert float((r1[0] if m == 0 else r1[2]).min()) >= 0.0
        assert all(torch.equal(x, y) for x, y in zip(r1[:3], r2[:3])) and all(torch.equal(x, y) for x, y in zip(r1[3], r2[3]))


@pytest.mark.parametrize("dtype", ["bfloat16", "float16"])
def test_16bit_x_is_the_float32_run_of_the_upcast(dtype):
    from matcouply_amd.decomposition import PackedMatrices

    p16 = _packed(_problem(MID), getattr(torch, dtype))
    p32 = PackedMatrices(p16.X.float().contiguous(), p16.row_ptr)
    from matcouply_amd import _engine

    rng = np.random.RandomState(0)
    I, K, r = len(p16), p16.X.shape[1], MID["rank"]
    for start in (None, (rng.uniform(size=(I, r)), rng.uniform(size=(r, r)), rng.uniform(size=(K, r)))):
        # (the engine's fp32 results: the public function returns them in X's dtype)
        r16 = _engine.parafac2_als(p16.X, p16.row_ptr, r, start, 4, 5, 1e-300, 0.0, [0])
        r32 = _engine.parafac2_als(p32.X, p32.row_ptr, r, start, 4, 5, 1e-300, 0.0, [0])
        assert all(torch.equal(x, y) for x, y in zip(r16, r32))


def test_array_types():
    from matcouply_amd.decomposition import parafac2_als

    mats = _problem(SMALL)
    r = SMALL["rank"]
    for dt in (np.float64, np.float32):
        w, (A, B, C), P = parafac2_als([m.astype(dt) for m in mats], r, n_iter_max=5)
        assert w is None and all(isinstance(x, np.ndarray) and x.dtype == dt for x in [A, B, C, *P])
        assert B.shape == (r, r) and [p.shape for p in P] == [(m.shape[0], r) for m in mats]
    w, (A, B, C), P = parafac2_als([torch.from_numpy(m).cuda() for m in mats], r, n_iter_max=5)
    assert all(torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32 for x in [A, B, C, *P])
    packed = _packed(mats)
    w, (A, B, C), P = parafac2_als(packed, r, n_iter_max=5)
    assert all(torch.is_tensor(x) and x.is_cuda for x in [A, B, C, *P])
    base = P[0]._base if P[0]._base is not None else P[0]
    assert all(p._base is base or p is base for p in P[1:]) and base.shape == (packed.X.shape[0], r)


def test_projections_are_orthonormal():
    mats = _problem(MID)
    _, _, _, P, _ = _run(_packed(mats), MID["rank"], n_iter_max=10, tol=0)
    for p in P:
        g = _np(p).T @ _np(p)
        assert np.abs(g - np.eye(MID["rank"])).max() < 1e-4


def test_end_to_end_start_beats_random():
    from matcouply_amd import decomposition as dec
    from matcouply_amd.coupled_matrices import CoupledMatrixFactorization

    mats = [m.astype(np.float64) for m in _problem(SMALL)]
    pf2 = dec.parafac2_als(mats, SMALL["rank"], n_iter_max=100, init="svd")
    kw = dict(return_errors=True, n_iter_max=5, tol=None, absolute_tol=None, random_state=0)
    _, diag_p = dec.parafac2_aoadmm(mats, SMALL["rank"], init=CoupledMatrixFactorization.from_Parafac2Tensor(pf2), **kw)
    _, diag_r = dec.parafac2_aoadmm(mats, SMALL["rank"], init="random", **kw)
    assert np.isfinite(diag_p.rec_errors).all()
    assert diag_p.rec_errors[0] < diag_r.rec_errors[0], (diag_p.rec_errors[0], diag_r.rec_errors[0])


def test_no_scratch_in_the_new_kernels():
    import os
    import sys

    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import kernel_resources

    ks = [k for k in kernel_resources.resources() if k["kernel"].startswith("k_pf2als_")]
    assert len(ks) >= 12, [k["kernel"] for k in ks]
    assert not any(kernel_resources.is_hot(k["kernel"]) for k in ks)
    spilled = [(k["kernel"], k["scratch_bytes"], k["vgpr_spill"]) for k in ks if k["scratch_bytes"] or k["vgpr_spill"]]
    assert not spilled, spilled


def _config3_packed():
    from matcouply_amd.decomposition import PackedMatrices

    I, J, K, r = 1024, 512, 256, 16
    g = torch.Generator(device="cuda").manual_seed(0)
    A = torch.rand((I, r), device="cuda", generator=g)
    B = torch.rand((J, r), device="cuda", generator=g)
    C = torch.rand((K, r), device="cuda", generator=g)
    X = torch.einsum("jr,ir,kr->ijk", B, A, C).reshape(I * J, K)
    X += 0.01 * X.std() * torch.randn(X.shape, device="cuda", generator=g)
    return PackedMatrices(X.contiguous(), np.arange(I + 1, dtype=np.int64) * J), r


def iteration_time(packed, rank, n_iter_parafac=5, iterations=20, reps=3):
    """seconds per iteration: the difference of the median wall times of runs with 2 + iterations and 2 iterations (tol = 0)"""
    from matcouply_amd.decomposition import parafac2_als

    def med(n):
        ts = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            parafac2_als(packed, rank, n_iter_max=n, tol=0, init="svd", n_iter_parafac=n_iter_parafac)
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        return float(np.median(ts))

    med(2)  # warm-up
    return (med(2 + iterations) - med(2)) / iterations


# beyond two reads of X.  The issue's estimate was 250 us; measured on MI355X: 1701-1768 us (profiles/parafac2_als_rate.txt),
# most of it in the per-slab Jacobi of the polar step and the mode-A kernel.  ~20 % headroom.
RATE_GUARD_US = 2100.0


def test_rate_guard_config3():
    from matcouply_amd import _engine

    packed, r = _config3_packed()
    nbytes = packed.X.numel() * packed.X.element_size()
    read_s = nbytes / (_engine.read_bandwidth(packed.X) * 1e9)
    t = iteration_time(packed, r)
    print(f"config-3 shape, n_iter_parafac=5: {t * 1e6:.1f} us per iteration, {read_s * 1e6:.1f} us per read of X, "
          f"{(t - 2 * read_s) * 1e6:.1f} us beyond two reads")
    assert t <= 2 * read_s + RATE_GUARD_US * 1e-6, (t, read_s)


# ---- RMAX = 32, load paths and boundaries (fixtures: tests/kernel_edge_cases.py, checked on the CPU by
# tests/test_parafac2_als_host.py) -----------------------------------------------------------------------------------------------
from tests import kernel_edge_cases as E  # noqa: E402


def _case_parity(name, n_iter, nn_modes=None, fac=1e-5, err=1e-7, tol=1e-300, **kw):
    mats, rank = E.pf2_problem(name)
    dev = _run(_packed(mats), rank, n_iter_max=n_iter, tol=tol, absolute_tol=0, init="svd", nn_modes=nn_modes, **kw)
    ref = R.parafac2_als(mats, rank, n_iter_max=n_iter, tol=tol, absolute_tol=0, init="svd", nn_modes=nn_modes, random_state=0,
                         **kw)
    assert len(dev[4]) == len(ref[4]) == n_iter, (len(dev[4]), len(ref[4]))
    errs = _compare(dev, ref)
    assert max(errs) < fac, (name, errs)
    assert np.abs(dev[4] - ref[4]).max() < err, (dev[4], ref[4])
    return dev, ref


@pytest.mark.parametrize("nn_modes", [None, [0, 2]], ids=["als", "nn02"])
@pytest.mark.parametrize("name", ["r17", "r24", "r32"])
def test_rmax32_parity_over_three_iterations(name, nn_modes):
    # pf2als_run<XL, 32> (NB = 2): every k_pf2als_*<32> kernel.  HALS modes at ranks 24 and 32: 1.6e-5 and 2.7e-5 measured in
    # B_i (ALS: within 1e-5).  Not the fixture's conditioning: a rank-24 fixture with a 3x larger start-Gram gap measures
    # 1.6e-5 as well; the error grows over the iterations in the HALS modes only
    _case_parity(name, 3, nn_modes, fac=5e-5 if nn_modes and name != "r17" else 1e-5)


def test_rmax32_parity_over_fifty_iterations():
    _case_parity("r32", 50, None, fac=1e-4)


@pytest.mark.parametrize("name", ["k37", "k130"])
def test_scalar_loads(name):
    # K % 4 != 0: the VEC = false loads of k_pf2als_xc and k_pf2als_y (NB = 1 at K = 37, NB = 2 at K = 130)
    _case_parity(name, 3, [0])


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
def test_unaligned_base_is_bitwise_the_aligned_run(dtype):
    # K % 4 == 0, X at element offset 1 inside a larger buffer (in bounds): the VEC = false loads read the same values as the
    # aligned run's vector loads, same products, same order.  16-bit: an explicit start, compared with the aligned fp32 run of
    # the upcast values
    from matcouply_amd import _engine

    mats, rank = E.pf2_problem("unaligned")
    packed = _packed(mats, getattr(torch, dtype))
    X32 = packed.X.float().contiguous()
    buf = torch.zeros(packed.X.numel() + 1, dtype=packed.X.dtype, device="cuda")
    Xu = buf[1: 1 + packed.X.numel()].view(packed.X.shape)
    Xu.copy_(packed.X)
    assert Xu.is_contiguous() and Xu.data_ptr() % 16 != 0
    rng = np.random.RandomState(0)
    I, K = len(packed), packed.X.shape[1]
    starts = [(rng.uniform(size=(I, rank)), rng.uniform(size=(rank, rank)), rng.uniform(size=(K, rank)))]
    if dtype == "float32":
        starts.append(None)
    for start in starts:
        ref = _engine.parafac2_als(X32, packed.row_ptr, rank, start, 4, 5, 1e-300, 0.0, [0])
        got = _engine.parafac2_als(Xu, packed.row_ptr, rank, start, 4, 5, 1e-300, 0.0, [0])
        torch.cuda.synchronize()
        assert all(torch.equal(x, y) for x, y in zip(got, ref)), (dtype, start is None)


@pytest.mark.parametrize("name", ["j_is_rank", "k_is_rank", "seg_edges", "one_slab"])
def test_boundaries(name):
    # J_i == rank; K == rank; J_i at the PA_SEG = 64 segment edges; I = 1.  I = 1: 2.9e-7 measured in e_t (factors within
    # 1e-5): one slab's fp32 X passes are not averaged over slabs in |X|^2 - 2 <M_C, C> + fit
    err = 5e-7 if name == "one_slab" else 1e-7
    _case_parity(name, 3, None, err=err)
    _case_parity(name, 3, [0, 2], err=err)


def test_many_slabs_reduce_over_128_groups():
    # I = 1100 slabs: ngrp_ab = 128 (k_pf2als_ab / k_pf2als_fit partials, k_pf2als_err's reduction); tol > 0 so the error is
    # formed every iteration
    dev, ref = _case_parity("many_slabs", 10, None)
    assert np.all(np.isfinite(dev[4]))
