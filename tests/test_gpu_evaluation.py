"""GPU: the model scores of csrc/evaluate.hip (method="device") against the dense float64 restatement of
tests/evaluation_restatement.py: the tables at every rank bucket, chunk tail and row edge and for every element type of X, the
SSE from the residual, the core pass on given tables, known core consistencies end to end, the bitwise promises, the C-ABI
refusals, and the starts of a fused multi-start fit."""
import ctypes

import numpy as np
import pytest
import torch

from matcouply_amd import _engine, decomposition as dec, evaluation as ev
from tests import evaluation_restatement as R

pytestmark = pytest.mark.gpu

TABLE_TOL = 1e-5  # relative (Frobenius) per matrix: the project's flat bar for fp32 products
SSE_TOL = 1e-3  # relative, per matrix, at a relative residual of 1e-3
CORE_TOL = 1e-9  # the core pass alone, fp64 on the same tables, condition numbers <= 100
CC_TOL = 1e-3  # core consistency (percent) for factors of condition number <= 3


def _rel(got, want):
    return np.linalg.norm(np.asarray(got) - want) / np.linalg.norm(want)


def _packed_models(cmfs):
    """float64 [n, (I + N + K) r] on the device, weights folded into A"""
    rows = []
    for w, (A, B_is, C) in cmfs:
        A = A * (1.0 if w is None else w)
        rows.append(np.concatenate([A.ravel(), np.concatenate(B_is, 0).ravel(), C.ravel()]))
    return torch.from_numpy(np.stack(rows)).cuda()


def _packed_data(Xs, dtype=torch.float32):
    row_ptr = np.concatenate([[0], np.cumsum([len(X) for X in Xs])]).astype(np.int64)
    return torch.from_numpy(np.concatenate(Xs, 0)).to(dtype).cuda(), row_ptr


def _as_seen(X):
    """the float64 values of the packed device matrix, split is done by the caller"""
    return X.to(torch.float64).cpu().numpy()


@pytest.mark.parametrize("K", [4, 37, 64, 130])
@pytest.mark.parametrize("rank", [1, 3, 16, 17, 32])
def test_tables_at_every_rank_chunk_tail_and_row_edge(rank, K):
    rows = R.RAGGED(rank)
    cmf, Xs = R.random_problem(np.random.RandomState(1000 * rank + K), rows, K, rank, noise=0.1)
    X, row_ptr = _packed_data(Xs)
    models = _packed_models([cmf])
    S, BtB, sse, norm = (t.cpu().numpy() for t in _engine.eval_tables(X, row_ptr, rank, models))
    A, B_is, C = cmf[1]
    want = R.tables(A, B_is, C, R.split(_as_seen(X), rows))
    for i, J in enumerate(rows):
        errs = (_rel(S[0, i], want[0][i]), _rel(BtB[0, i], want[1][i]), abs(norm[i] - want[3][i]) / want[3][i],
                abs(sse[0, i] - want[2][i]) / want[2][i])
        print(f"rank {rank} K {K} J {J}: S {errs[0]:.2e} BtB {errs[1]:.2e} norm {errs[2]:.2e} sse {errs[3]:.2e}")
        assert max(errs[:3]) <= TABLE_TOL
        assert errs[3] <= SSE_TOL  # (a relative residual of 0.1 here: far inside)
    # 16-bit X: bit for bit the fp32 run on the upcast matrix
    for dtype in (torch.bfloat16, torch.float16):
        X16 = X.to(dtype)
        narrow = _engine.eval_tables(X16, row_ptr, rank, models)
        wide = _engine.eval_tables(X16.float(), row_ptr, rank, models)
        assert all(torch.equal(a, b) for a, b in zip(narrow, wide)), dtype


def test_sse_comes_from_the_residual():
    """At a relative residual of 1e-3 the three-term form |X|^2 - 2 <X, M> + |M|^2 in fp32 is off by more than 1e-2, the residual
    form by 3e-5 at worst: the bar of 1e-3 tells them apart."""
    rank, K = 16, 130
    rows = R.RAGGED(rank)
    cmf, Xs = R.random_problem(np.random.RandomState(7), rows, K, rank, noise=1e-3)
    X, row_ptr = _packed_data(Xs)
    _, _, sse, norm = (t.cpu().numpy() for t in _engine.eval_tables(X, row_ptr, rank, _packed_models([cmf])))
    A, B_is, C = cmf[1]
    _, _, want, want_norm = R.tables(A, B_is, C, R.split(_as_seen(X), rows))
    assert np.allclose(np.sqrt(want / want_norm), 1e-3, rtol=1e-2)
    err = np.abs(sse[0] - want) / want
    print("relative error of sse_i:", err)
    assert err.max() <= SSE_TOL


@pytest.mark.parametrize("rank", [2, 5, 16, 17, 32])
def test_core_pass_alone_on_the_restatements_tables(rank):
    I, K = rank + 3, rank + 6
    rows = [rank + 1 + i for i in range(I)]
    cmfs, tabs = [], []
    for seed in range(3):
        cmf, Xs = R.random_problem(np.random.RandomState(100 * rank + seed), rows, K, rank, noise=0.3, kappa=100.0)
        A, B_is, C = cmf[1]
        assert max(np.linalg.cond(F) for F in [A, C] + B_is) <= 100.0 * (1 + 1e-9)
        cmfs.append(cmf)
        tabs.append(R.tables(A, B_is, C, Xs))
    S = torch.from_numpy(np.stack([t[0] for t in tabs])).cuda()
    BtB = torch.from_numpy(np.stack([t[1] for t in tabs])).cuda()
    core, cc, ccn = (t.cpu().numpy() for t in _engine.eval_core(_packed_models(cmfs), I, sum(rows), K, rank, S, BtB))
    for k, (cmf, t) in enumerate(zip(cmfs, tabs)):
        want = R.core_of_tables(cmf[1][0], cmf[1][2], t[0], t[1])
        print(f"rank {rank} model {k}: core {_rel(core[k], want):.2e}, cc {cc[k]!r} against {R.consistency(want)!r}")
        assert _rel(core[k], want) <= CORE_TOL
        scale = max(1.0, np.sum(want ** 2) / rank)  # the deviation is a sum of squares of the core's entries
        assert abs(cc[k] - R.consistency(want)) <= 100 * 4 * CORE_TOL * scale
        assert abs(ccn[k] - R.consistency(want, True)) <= 100 * 4 * CORE_TOL * scale


@pytest.mark.parametrize("kind", ["cp", "parafac2"])
@pytest.mark.parametrize("rank", [2, 5, 16])
def test_known_core_consistency_end_to_end(rank, kind):
    for deviation, answer in [(0.4, 60.0), (0.0, 100.0)]:
        cmf, Xs, G0 = R.known_core_problem(np.random.RandomState(10 * rank + (kind == "cp")), rank, kind, deviation)
        got = ev.core_consistency(cmf, Xs, method="device")
        normalised = ev.core_consistency(cmf, Xs, normalised=True, method="device")
        out = ev.multistart_evaluation(Xs, [cmf], method="device")
        print(f"rank {rank} {kind}: {got!r} for {answer}, normalised {normalised!r} for {R.consistency(G0, True)!r}, "
              f"core {_rel(out.core[0], G0):.2e}, fit {out.fit[0]!r}")
        assert abs(got - answer) <= CC_TOL
        assert abs(normalised - R.consistency(G0, True)) <= CC_TOL
        assert out.core_consistency[0] == got and out.core_consistency_normalised[0] == normalised
        assert abs(out.fit[0] - 1.0) <= 1e-5 if deviation == 0.0 else out.fit[0] < 1.0


@pytest.fixture(scope="module")
def five_models():
    rank, K, rows = 5, 37, [7, 64, 65, 5, 130, 16]
    rng = np.random.RandomState(3)
    cmf, Xs = R.random_problem(rng, rows, K, rank, noise=0.2)
    cmfs = [cmf] + [R.random_problem(rng, rows, K, rank)[0] for _ in range(4)]
    X, row_ptr = _packed_data(Xs)
    return cmfs, X, row_ptr, rank, K, rows


def _all_of(models, X, row_ptr, rank, K, rows):
    tables = _engine.eval_tables(X, row_ptr, rank, models)
    return tables + _engine.eval_core(models, len(rows), sum(rows), K, rank, tables[0], tables[1])


def test_a_model_does_not_depend_on_the_call_it_is_in(five_models):
    cmfs, X, *shape = five_models
    together = _all_of(_packed_models(cmfs), X, *shape)
    for k, cmf in enumerate(cmfs):
        alone = _all_of(_packed_models([cmf]), X, *shape)
        for name, a, b in zip(("S", "BtB", "sse", "norm", "core", "cc", "ccn"), alone, together):
            assert torch.equal(a[0] if name != "norm" else a, b[k] if name != "norm" else b), (k, name)


def test_two_runs_are_bitwise_equal(five_models):
    cmfs, X, *shape = five_models
    models = _packed_models(cmfs)
    first, second = _all_of(models, X, *shape), _all_of(models, X, *shape)
    assert all(torch.equal(a, b) for a, b in zip(first, second))


def test_c_abi_refusals_run_no_kernel(five_models):
    cmfs, X, row_ptr, r, K, rows = five_models
    lib = _engine.load_library()
    n, I, N = len(cmfs), len(rows), sum(rows)
    models = _packed_models(cmfs)
    rp = lambda a: np.ascontiguousarray(a, dtype=np.int64).ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
    nbytes = lib.mcl_eval_workspace_bytes(rp(row_ptr), I, K, r, n)
    assert nbytes > 0
    ws = torch.empty(nbytes + 256, dtype=torch.uint8, device="cuda")
    wp = ws.data_ptr() + (-ws.data_ptr()) % 256
    filled = lambda *shape: torch.full(shape, -7.0, dtype=torch.float64, device="cuda")
    S, BtB, sse, norm = filled(n, I, r, r), filled(n, I, r, r), filled(n, I), filled(I)
    core, cc, ccn = filled(n, r, r, r), filled(n), filled(n)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    bad_models = models.clone()
    bad_models[3, 11] = float("inf")
    flat = np.array(row_ptr)
    flat[2] = flat[1]
    down = np.array(row_ptr)
    down[3] = down[2] - 1
    good = dict(X=X.data_ptr(), xt=_engine.X_F32, rp=rp(row_ptr), I=I, K=K, r=r, models=models.data_ptr(), n=n, S=S.data_ptr(),
                BtB=BtB.data_ptr(), sse=sse.data_ptr(), norm=norm.data_ptr(), ws=wp, ws_bytes=nbytes, stream=stream)
    tables = lambda **kw: lib.mcl_eval_tables_typed(*{**good, **kw}.values())
    for change, message in [(dict(r=0), b"rank 0"), (dict(r=33), b"rank 33"), (dict(n=0), b"n_models"), (dict(n=-2), b"n_models"),
                            (dict(rp=rp(flat)), b"row_ptr must increase"), (dict(rp=rp(down)), b"row_ptr must increase"),
                            (dict(ws_bytes=nbytes - 1), b"workspace too small"), (dict(ws=wp + 8), b"aligned"),
                            (dict(models=bad_models.data_ptr()), b"model 3 holds a non-finite"), (dict(xt=7), b"x_type"),
                            (dict(X=None), b"NULL")]:
        assert tables(**change) != 0, change
        assert message in lib.mcl_eval_last_error(), (change, lib.mcl_eval_last_error())
    assert lib.mcl_eval_workspace_bytes(rp(row_ptr), I, K, 33, n) == -1 and lib.mcl_eval_workspace_bytes(rp(flat), I, K, r, n) == -1
    assert lib.mcl_eval_workspace_bytes(rp(row_ptr), I, K, r, 0) == -1
    good_core = dict(models=models.data_ptr(), n=n, I=I, N=N, K=K, r=r, S=S.data_ptr(), BtB=BtB.data_ptr(), core=core.data_ptr(),
                     cc=cc.data_ptr(), ccn=ccn.data_ptr(), stream=stream)
    core_call = lambda **kw: lib.mcl_eval_core(*{**good_core, **kw}.values())
    for change, message in [(dict(r=0), b"rank 0"), (dict(r=33), b"rank 33"), (dict(n=0), b"n_models"),
                            (dict(models=bad_models.data_ptr()), b"model 3 holds a non-finite"), (dict(core=None), b"NULL")]:
        assert core_call(**change) != 0, change
        assert message in lib.mcl_eval_last_error(), (change, lib.mcl_eval_last_error())
    torch.cuda.synchronize()
    for t in (S, BtB, sse, norm, core, cc, ccn):
        assert bool((t == -7.0).all())  # nothing was launched
    assert tables() == 0 and core_call() == 0
    torch.cuda.synchronize()
    want = _all_of(models, X, row_ptr, r, K, rows)
    assert all(torch.equal(a, b) for a, b in zip((S, BtB, sse, norm, core, cc, ccn), want))


def test_inputs_of_every_kind_and_the_refusal_of_non_finite_device_factors(five_models):
    cmfs, X, row_ptr, rank, K, rows = five_models
    Xs = R.split(X.cpu().numpy(), rows)
    want = ev.multistart_evaluation(Xs, cmfs[:2], method="device")
    on_device = lambda cmf: (None, (torch.from_numpy(cmf[1][0]).cuda(), [torch.from_numpy(B_i).cuda() for B_i in cmf[1][1]],
                                    torch.from_numpy(cmf[1][2]).cuda()))
    for data in ([torch.from_numpy(X_i) for X_i in Xs], [torch.from_numpy(X_i).cuda() for X_i in Xs], dec.PackedMatrices(X, row_ptr)):
        for models in (cmfs[:2], [on_device(c) for c in cmfs[:2]]):
            got = ev.multistart_evaluation(data, models)  # "auto" takes the device here
            assert all(np.array_equal(a, b) for a, b in zip(got, want))
    half = dec.PackedMatrices(X.bfloat16(), row_ptr)
    assert np.array_equal(ev.slabwise_sse(cmfs[0], half, method="device"),
                          ev.slabwise_sse(cmfs[0], dec.PackedMatrices(half.X.float(), row_ptr), method="device"))
    bad = on_device(cmfs[0])
    bad[1][2][0, 0] = float("nan")
    with pytest.raises(NotImplementedError, match="non-finite"):
        ev.fit(bad, Xs, method="device")


def _truncated_normal(rng, size):
    x = rng.standard_normal(size=size)
    x[x < 0] = 0
    return x


def _example_problem(I, J, K, rank, noise_level):
    """the simulated PARAFAC2 data of the reference's examples, as tests/test_gpu_multistart.py states it"""
    rng = np.random.default_rng(0)
    A = rng.uniform(size=(I, rank)) + 0.1
    B_blueprint = _truncated_normal(rng, (J, rank))
    B_is = [np.roll(B_blueprint, i, axis=0) for i in range(I)]
    C = _truncated_normal(rng, (K, rank))
    matrices = [(B_i * A[i]) @ C.T for i, B_i in enumerate(B_is)]
    noise = [rng.uniform(size=M.shape) for M in matrices]
    return [M + N * noise_level * np.linalg.norm(M) / np.linalg.norm(N) for M, N in zip(matrices, noise)]


def test_the_starts_of_a_fused_fit_end_to_end():
    mats = [M.astype(np.float32) for M in _example_problem(6, 20, 12, 3, 0.2)]
    results = dec.parafac2_aoadmm_multistart(mats, 3, range(8), method="fused", non_negative=True, n_iter_max=1000, return_errors=True)
    got = ev.multistart_evaluation(mats, results)  # method="auto": the device
    assert all(np.array_equal(a, b) for a, b in zip(got, ev.multistart_evaluation(mats, results, method="device")))
    host = ev.multistart_evaluation(mats, results, method="host")
    assert got.fit.shape == (8,) and got.slab_sse.shape == (8, 6) and got.core.shape == (8, 3, 3, 3)
    rec = np.array([diag.rec_errors[-1] for _, diag in results])
    print("fit", got.fit, "1 - rec_error^2", 1 - rec ** 2, "core consistency", got.core_consistency)
    assert np.abs(got.fit - (1 - rec ** 2)).max() <= 1e-5
    assert np.abs(got.fit - host.fit).max() <= 1e-5 and np.abs(got.relative_sse - host.relative_sse).max() <= 1e-5
    assert (np.abs(got.slab_sse - host.slab_sse) / host.slab_sse).max() <= SSE_TOL
    for s, (cmf, _) in enumerate(results):
        # a relative error d of S_i moves W_i = (B_i^T B_i)^+ S_i (C^T C)^+ by at most d cond(B_i)^2 cond(C)^2 of its norm, the
        # core by cond(A) times that; the consistency is 100 (1 - |G - T|^2 / r)
        A, B_is, C = (np.asarray(cmf[1][0], dtype=np.float64), [np.asarray(B_i, dtype=np.float64) for B_i in cmf[1][1]],
                      np.asarray(cmf[1][2], dtype=np.float64))
        bound = TABLE_TOL * np.linalg.cond(A) * max(np.linalg.cond(B_i) for B_i in B_is) ** 2 * np.linalg.cond(C) ** 2
        err = _rel(got.core[s], host.core[s])
        print(f"start {s}: core {err:.2e} (bound {bound:.2e}), cc {got.core_consistency[s]!r} host {host.core_consistency[s]!r}")
        assert err <= bound
        dG, G = np.linalg.norm(got.core[s] - host.core[s]), np.linalg.norm(host.core[s] - R.superdiagonal(3))
        assert abs(got.core_consistency[s] - host.core_consistency[s]) <= 100 * (2 * G * dG + dG ** 2) / 3 + 1e-9
