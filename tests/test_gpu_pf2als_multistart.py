"""GPU: parafac2_als_multistart with the fused kernel (csrc/pf2als_multistart.hip) against the fp64 NumPy restatement
(tests/parafac2_als_restatement.py) started from every start's own draw: parity per start, every rank, the default stopping
rule, the sequential method, bitwise independence of the batch, 16-bit X, return types, many slabs, resources and rate."""
import time

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from matcouply_amd import _engine  # noqa: E402
from matcouply_amd import decomposition as dec  # noqa: E402
from matcouply_amd import multistart as ms  # noqa: E402
from tests import parafac2_als_restatement as R  # noqa: E402

pytestmark = pytest.mark.gpu

NOISE = 0.2
SMALL = dict(I=6, J_range=(8, 20), K=12, rank=3, seed=2)
MID = dict(I=24, J_range=(40, 100), K=64, rank=8, seed=0)
NEAR_BOUND = dict(I=36, J_range=(100, 120), K=64, rank=4, seed=1)  # 253 k elements, just under the fused bound of 2^18
SIZES = {"small": SMALL, "mid": MID, "near_bound": NEAR_BOUND}


def _problem(p, nonneg=False):
    """float64 copies of the float32 matrices: the results come back in float64, unrounded"""
    mats = R.parafac2_problem(p["I"], p["J_range"], p["K"], p["rank"], seed=p["seed"], noise=NOISE, nonneg=nonneg)[0]
    return [m.astype(np.float64) for m in mats]


def _packed(mats, dtype=torch.float32):
    row_ptr = np.concatenate([[0], np.cumsum([m.shape[0] for m in mats])]).astype(np.int64)
    X = torch.from_numpy(np.concatenate(mats, 0)).to("cuda").to(dtype).contiguous()
    return dec.PackedMatrices(X, row_ptr)


def _np(x):
    return np.asarray(x.cpu() if hasattr(x, "cpu") else x, dtype=np.float64)


def _rel(a, b):
    return np.linalg.norm(_np(a) - b) / np.linalg.norm(b)


def _errs(res, ref):
    """relative differences of A, B, C and the stacked P_i B, and the largest difference of e_t"""
    (_, (A, B, C), P), errors = res
    rA, rB, rC, rP, rerr = ref[:5]
    PB = np.concatenate([_np(p) @ _np(B) for p in P])
    rPB = np.concatenate([p @ rB for p in rP])
    de = np.abs(np.asarray(errors) - rerr).max() if len(rerr) else 0.0
    assert len(errors) == len(rerr), (len(errors), len(rerr))
    return [_rel(A, rA), _rel(B, rB), _rel(C, rC), _rel(PB, rPB)], de


def _fused(data, rank, starts, **kw):
    out = dec.parafac2_als_multistart(data, rank, starts, method="fused", return_errors=True, **kw)
    torch.cuda.synchronize()
    return out


# fp64 against fp64 from the same start.  Not 1e-9 / 1e-7 with e_t to 1e-10: the random start's first polar factors amplify
# rounding about 1e9-fold - a relative perturbation of 1e-16 of the start moves the restatement's OWN factors by up to 6e-7 and
# its e_t by up to 1.7e-8 after three iterations (measured figures there)
FAC_BAR, ERR_BAR = 5e-6, 1e-7
BARS = {3: (FAC_BAR, ERR_BAR), 50: (FAC_BAR, ERR_BAR)}


@pytest.mark.parametrize("n_iter", [3, 50])
@pytest.mark.parametrize("nn_modes", [None, [0], [0, 2]], ids=["als", "nn0", "nn02"])
@pytest.mark.parametrize("size", ["small", "mid", "near_bound"])
def test_parity_per_start(size, nn_modes, n_iter):
    p = SIZES[size]
    mats = _problem(p)
    assert sum(m.size for m in mats) <= ms._MULTISTART_MAX_ELEMENTS
    starts = [0, 1, 2, 3]
    got = _fused(_packed(mats), p["rank"], starts, n_iter_max=n_iter, tol=1e-300, absolute_tol=0, nn_modes=nn_modes)
    fac, err = BARS[n_iter]
    worst = [0.0, 0.0]
    for s, res in zip(starts, got):
        ref = R.parafac2_als(mats, p["rank"], n_iter_max=n_iter, tol=1e-300, absolute_tol=0, nn_modes=nn_modes, random_state=s)
        assert len(res[1]) == n_iter
        errs, de = _errs(res, ref)
        worst = [max(worst[0], max(errs)), max(worst[1], de)]
    print(f"{size} {nn_modes} {n_iter} iterations: factors {worst[0]:.2e}, e_t {worst[1]:.2e}")
    assert worst[0] < fac and worst[1] < err, worst


@pytest.mark.parametrize("rank", range(1, 17))
def test_every_rank(rank):
    # k_ms_pf2als<R, fp32> for R = 1..16, three iterations
    mats = _problem(dict(I=5, J_range=(16, 30), K=20, rank=rank, seed=rank))
    got = _fused(mats, rank, [0, 1], n_iter_max=3, tol=1e-300, absolute_tol=0)
    for s, res in enumerate(got):
        ref = R.parafac2_als(mats, rank, n_iter_max=3, tol=1e-300, absolute_tol=0, random_state=s)
        errs, de = _errs(res, ref)
        print(f"rank {rank} start {s}: factors {max(errs):.2e}, e_t {de:.2e}")
        assert max(errs) < FAC_BAR and de < ERR_BAR, (rank, s, errs, de)


# Fixtures and starts on which the restatement's relative change of e^2 crosses the default tol = 1e-8 with at least a 10 %
# margin on both sides (checked below): (rank, seed, I, J_range, K, starts)
STOPPING = [(1, 0, 8, (8, 20), 12, [0, 1, 2, 3])]


@pytest.mark.parametrize("case", range(len(STOPPING)))
def test_default_tol_stops_where_the_restatement_stops(case):
    rank, seed, I, J_range, K, starts = STOPPING[case]
    mats = R.parafac2_problem(I, J_range, K, rank, seed=seed, noise=NOISE)[0]
    got = _fused(mats, rank, starts)
    for s, res in zip(starts, got):
        ref = R.parafac2_als(mats, rank, random_state=s)
        rel = np.abs(np.diff(ref[5])) / ref[5][:-1]
        assert rel[-1] <= 0.9e-8 and rel[:-1].min() >= 1.1e-8, (s, rel[-1], rel[:-1].min())
        assert len(res[1]) == len(ref[4]), (s, len(res[1]), len(ref[4]))
        errs, de = _errs(res, ref)
        assert de < 1e-10 and max(errs) < 1e-7, (s, errs, de)


def test_fused_follows_sequential_on_a_fast_fixture():
    mats = R.parafac2_problem(8, (8, 20), 12, 1, seed=0, noise=NOISE)[0]
    kw = dict(tol=1e-5, return_errors=True)
    fused = dec.parafac2_als_multistart(mats, 1, range(4), method="fused", **kw)
    seq = dec.parafac2_als_multistart(mats, 1, range(4), method="sequential", **kw)
    for (f, ef), (q, eq) in zip(fused, seq):
        assert len(ef) == len(eq), (len(ef), len(eq))
        for a, b in zip([f[1][0], f[1][1], f[1][2], *f[2]], [q[1][0], q[1][1], q[1][2], *q[2]]):
            assert _rel(a, _np(b)) < 5e-5


def _engine_run(packed, rank, starts, n_iter_max=30, tol=1e-300, nn_modes=(0,)):
    I, K = len(packed), int(packed.X.shape[1])
    f = np.stack([np.concatenate([np.ravel(F) for F in dec._pf2als_random_start(I, K, rank, s)]) for s in starts])
    factors = torch.from_numpy(f).cuda()
    P, errors, n_iter = _engine.pf2als_multistart_run(packed.X, packed.row_ptr, rank, factors, n_iter_max, 5, tol, 0.0, nn_modes)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in (factors, P, errors, n_iter)]


def test_start_alone_equals_start_in_a_batch_and_runs_repeat():
    packed = _packed(_problem(SMALL))
    batch = _engine_run(packed, SMALL["rank"], range(64))
    again = _engine_run(packed, SMALL["rank"], range(64))
    assert all(np.array_equal(a, b) for a, b in zip(batch, again))
    for s in (0, 17, 63):
        alone = _engine_run(packed, SMALL["rank"], [s])
        assert all(np.array_equal(a[0], b[s]) for a, b in zip(alone, batch)), s


@pytest.mark.parametrize("dtype", ["bfloat16", "float16"])
def test_x16_is_the_run_of_the_upcast(dtype):
    p16 = _packed(_problem(MID), getattr(torch, dtype))
    p32 = dec.PackedMatrices(p16.X.float().contiguous(), p16.row_ptr)
    a = _engine_run(p16, MID["rank"], range(4))
    b = _engine_run(p32, MID["rank"], range(4))
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("kind", ["numpy64", "numpy32", "torch_cpu", "torch_cuda", "packed"])
def test_return_types_match_parafac2_als(kind):
    mats = _problem(SMALL)
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
        fused = dec.parafac2_als_multistart(data, r, [0], method="fused", n_iter_max=5, return_errors=errors)[0]
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

        walk(fused, single)


def test_many_slabs():
    from tests import kernel_edge_cases as E

    mats, rank = E.pf2_problem("many_slabs")  # I = 1100
    mats = [m.astype(np.float64) for m in mats]
    got = _fused(mats, rank, [0, 1], n_iter_max=10, tol=1e-300, absolute_tol=0)
    for s, res in enumerate(got):
        ref = R.parafac2_als(mats, rank, n_iter_max=10, tol=1e-300, absolute_tol=0, random_state=s)
        errs, de = _errs(res, ref)
        print(f"many slabs start {s}: factors {max(errs):.2e}, e_t {de:.2e}")
        assert max(errs) < FAC_BAR and de < ERR_BAR, (s, errs, de)


def test_no_scratch_in_the_fused_kernel():
    import os
    import sys

    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import kernel_resources

    ks = [k for k in kernel_resources.resources() if k["kernel"].startswith("k_ms_pf2als<")]
    assert len(ks) == 48, [k["kernel"] for k in ks]  # ranks 1..16 x {fp32, bf16, fp16}
    assert not any(kernel_resources.is_hot(k["kernel"]) for k in ks)
    spilled = [(k["kernel"], k["scratch_bytes"], k["vgpr_spill"]) for k in ks if k["scratch_bytes"] or k["vgpr_spill"]]
    assert not spilled, spilled


def semiconductor_problem():
    """the size of the reference's semiconductor example: 108 matrices of 100-120 x 21, rank 2; this seed's draw of J_i keeps
    X under the fused bound of 2^18 elements"""
    mats = R.parafac2_problem(108, (100, 120), 21, 2, seed=3, noise=NOISE)[0]
    assert sum(m.size for m in mats) <= ms._MULTISTART_MAX_ELEMENTS
    return mats


# 64 fused starts against 64 sequential calls (4 timed, scaled) at the semiconductor size, 200 iterations, tol = 0, nn_modes=[0]:
# measured 70.5 ms against 4.11 s, ratio 0.0172 (profiles/pf2als_multistart_rate.txt: 0.0175); the guard leaves 2x headroom
RATE_GUARD = 0.035


def test_rate_guard_semiconductor_size():
    mats = semiconductor_problem()
    kw = dict(n_iter_max=200, tol=0, nn_modes=[0])
    dec.parafac2_als_multistart(mats, 2, range(64), method="fused", **kw)  # warm-up
    dec.parafac2_als_multistart(mats, 2, range(1), method="sequential", **kw)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    t_fused = timed(lambda: dec.parafac2_als_multistart(mats, 2, range(64), method="fused", **kw))
    t_seq = 16 * timed(lambda: dec.parafac2_als_multistart(mats, 2, range(4), method="sequential", **kw))
    print(f"64 starts: fused {t_fused * 1e3:.1f} ms, sequential {t_seq * 1e3:.1f} ms, ratio {t_fused / t_seq:.4f}")
    assert t_fused <= RATE_GUARD * t_seq, (t_fused, t_seq)
