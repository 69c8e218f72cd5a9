"""GPU: the factor match scores of csrc/similarity.hip (method="device") against the restatement of
tests/similarity_restatement.py: every rank bucket and row tail, every option, one-vs-all / all-pairs / explicit pairs at several
model counts, the bitwise promises, the C-ABI refusals, and the starts of a fused multi-start fit end to end."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

from matcouply_amd import _engine, decomposition as dec, similarity as sim
from tests import similarity_restatement as R

pytestmark = pytest.mark.gpu

TOL = 1e-12  # scores: two summation orders over at most 600 rows differ by 600 * 3 * 1.1e-16 ~ 2e-13
MARGIN = 1e-6  # permutations are compared where the optimum is isolated by more than this


def _margin(M):
    return R.brute_force(M)[2] if len(M) <= 5 else R.margin(M)


def _check(score, perm, cmf1, cmf2, must_be_isolated, **options):
    """the three checks that hold without an isolated optimum; the permutation itself where it is isolated"""
    want, want_perm, M = R.fms(cmf1, cmf2, **options)
    rank = len(M)
    print(f"rank {rank}: score {score!r} restatement {want!r} difference {abs(score - want):.2e}")
    assert perm.dtype == np.int32 and sorted(perm.tolist()) == list(range(rank))
    assert abs(R.score_of(M, perm) - score) <= TOL
    assert abs(score - want) <= TOL
    if rank <= 5:
        assert abs(score - R.brute_force(M)[0]) <= TOL
    isolated = _margin(M) > MARGIN
    if must_be_isolated:
        assert isolated, "the seed gives no isolated optimum"
    if isolated:
        assert perm.tolist() == (R.brute_force(M)[1] if rank <= 5 else want_perm).tolist()


@pytest.mark.parametrize("rows", R.ROWS)
@pytest.mark.parametrize("rank", R.RANKS)
def test_parity_at_every_rank_and_row_tail(rank, rows):
    cmf1, cmf2 = R.parity_pair(rank, rows)
    score, perm = sim.factor_match_score(cmf1, cmf2, return_permutation=True, method="device")
    _check(score, perm, cmf1, cmf2, True)
    back, inverse = sim.factor_match_score(cmf2, cmf1, return_permutation=True, method="device")
    assert back == score and inverse.tolist() == np.argsort(perm).tolist()
    assert sim.factor_match_score(cmf1, cmf2, method="device") == score


@pytest.mark.parametrize("rank,rows", R.OPTION_CASES)
@pytest.mark.parametrize("weights", ["given", "none", "one side"])
def test_every_option(rank, rows, weights):
    cmf1, cmf2 = R.parity_pair(rank, rows)
    if weights == "none":
        cmf1, cmf2 = (None, cmf1[1]), (None, cmf2[1])
    elif weights == "one side":
        cmf2 = (None, cmf2[1])
    for consider_weights, absolute_value, skip_mode in itertools.product((True, False), (True, False), (None, 0, 1, 2)):
        options = dict(consider_weights=consider_weights, absolute_value=absolute_value, skip_mode=skip_mode)
        score, perm = sim.factor_match_score(cmf1, cmf2, return_permutation=True, method="device", **options)
        _check(score, perm, cmf1, cmf2, weights == "given", **options)


@pytest.fixture(scope="module")
def starts():
    """65 models of rank 3 and the restatement of all their pairs, computed once"""
    rng = np.random.RandomState(11)
    models = [R.random_model(rng, (3, 7, 5), 3, weights=bool(s % 3)) for s in range(65)]
    table = {(s, t): R.fms(models[s], models[t]) for s in range(65) for t in range(65)}
    return models, table


def _check_table(pairs, scores, perms, table):
    assert np.abs(scores - [table[s, t][0] for s, t in pairs]).max() <= TOL
    for (s, t), score, perm in zip(pairs, scores, perms):
        M = table[s, t][2]
        assert sorted(perm.tolist()) == [0, 1, 2] and abs(R.score_of(M, perm) - score) <= TOL
        best, best_perm, gap = R.brute_force(M)
        if gap > MARGIN:
            assert perm.tolist() == best_perm.tolist()


@pytest.mark.parametrize("n", [1, 2, 7, 65])
def test_one_vs_all_and_all_pairs(starts, n):
    models, table = starts
    models = models[:n]
    ref = n // 2
    scores, perms = sim.multistart_similarity(models, ref, return_permutations=True, method="device")
    assert scores.shape == (n,) and scores.dtype == np.float64 and perms.shape == (n, 3) and perms.dtype == np.int32
    _check_table([(ref, t) for t in range(n)], scores, perms, table)
    assert np.array_equal(sim.multistart_similarity(models, ref, method="device"), scores)
    matrix, perms = sim.multistart_similarity(models, all_pairs=True, return_permutations=True, method="device")
    assert matrix.shape == (n, n) and perms.shape == (n, n, 3) and np.array_equal(matrix, matrix.T)
    all_of = list(itertools.product(range(n), repeat=2))
    _check_table(all_of, matrix.reshape(-1), perms.reshape(-1, 3), table)
    assert np.abs(np.diag(matrix) - 1.0).max() <= TOL
    assert np.array_equal(matrix[ref], scores)  # the same pairs in another launch: the same bits
    outside = R.random_model(np.random.RandomState(12), (3, 7, 5), 3, weights=True)  # a reference that is not a start
    scores = sim.multistart_similarity(models, outside, method="device")
    assert np.abs(scores - [R.fms(outside, m)[0] for m in models]).max() <= TOL


def test_explicit_pairs_with_repeats(starts):
    models, table = starts
    pairs = [(3, 9), (9, 3), (3, 9), (5, 5), (64, 0), (0, 64), (5, 5), (17, 40)]
    scores, perms = sim.multistart_similarity(models, pairs=pairs, return_permutations=True, method="device")
    _check_table(pairs, scores, perms, table)
    assert scores[0] == scores[2] == scores[1] and scores[3] == scores[6] and scores[4] == scores[5]
    assert perms[0].tolist() == perms[2].tolist() and perms[1].tolist() == np.argsort(perms[0]).tolist()


def test_a_pair_does_not_depend_on_the_launch_it_is_in(starts):
    models, _ = starts
    matrix, perms = sim.multistart_similarity(models, all_pairs=True, return_permutations=True, method="device")  # 2145 pairs
    for s, t in [(0, 0), (0, 64), (13, 27), (63, 64), (31, 2)]:
        score, perm = sim.multistart_similarity(models, pairs=[(s, t)], return_permutations=True, method="device")
        assert score[0] == matrix[s, t] and perm[0].tolist() == perms[s, t].tolist()
        alone, perm = sim.factor_match_score(models[s], models[t], return_permutation=True, method="device")
        assert alone == matrix[s, t] and perm.tolist() == perms[s, t].tolist()
        assert sim.factor_match_score(models[t], models[s], method="device") == alone


@pytest.mark.parametrize("rank,rows", [(3, (3, 7, 5)), (16, (16, 64, 32))])
def test_zero_column(rank, rows):
    cmf1, cmf2 = R.parity_pair(rank, rows)
    for mode in range(3):
        a = [[np.array(B_i) for B_i in F] if isinstance(F, list) else F.copy() for F in cmf1[1]]
        for F in (a[mode] if mode == 1 else [a[mode]]):
            F[:, rank - 1] = 0.0
        one = (cmf1[0], tuple(a))
        for skip_mode, consider_weights in itertools.product((None, mode), (True, False)):
            score, perm = sim.factor_match_score(one, cmf2, return_permutation=True, skip_mode=skip_mode,
                                                 consider_weights=consider_weights, method="device")
            assert np.isfinite(score)
            _check(score, perm, one, cmf2, False, skip_mode=skip_mode, consider_weights=consider_weights)
    zero = (None, tuple([np.zeros_like(B_i) for B_i in F] if isinstance(F, list) else np.zeros_like(F) for F in cmf1[1]))
    assert sim.factor_match_score(zero, cmf2, method="device") == 0.0 and sim.factor_match_score(zero, zero, method="device") == 0.0


def test_float32_and_device_tensors_are_widened_exactly():
    cmf1, cmf2 = R.parity_pair(5, (10, 150, 20))
    cast = lambda cmf, f: (f(cmf[0]), (f(cmf[1][0]), [f(B_i) for B_i in cmf[1][1]], f(cmf[1][2])))
    f32 = [cast(c, lambda x: x.astype(np.float32)) for c in (cmf1, cmf2)]
    widened = [cast(c, lambda x: x.astype(np.float64)) for c in f32]
    want = sim.factor_match_score(*widened, return_permutation=True, method="device")
    _check(*want, *widened, False)
    on_device = lambda c: cast(c, lambda x: torch.from_numpy(x).cuda())
    for one, two in [f32, [on_device(c) for c in f32], [on_device(c) for c in widened], [on_device(f32[0]), widened[1]],
                     [f32[0], widened[1]]]:
        got = sim.factor_match_score(one, two, return_permutation=True, method="device")
        assert got[0] == want[0] and got[1].tolist() == want[1].tolist()
    assert sim.factor_match_score(*[on_device(c) for c in f32]) == want[0]  # "auto" takes the device here
    bad = on_device(widened[0])
    bad[1][2][0, 0] = float("nan")
    with pytest.raises(NotImplementedError, match="non-finite"):
        sim.factor_match_score(bad, widened[1], method="device")


def test_c_abi_refusals_run_no_kernel():
    lib = _engine.load_library()
    n, I, N, K, r = 4, 2, 3, 2, 3
    dev = torch.device("cuda")
    models = torch.randn(n, (I + N + K) * r, dtype=torch.float64, device=dev)
    score = torch.full((2,), -7.0, dtype=torch.float64, device=dev)
    perm = torch.full((2, r), -7, dtype=torch.int32, device=dev)
    ws = torch.empty(lib.mcl_fms_workspace_bytes(n, r) + 256, dtype=torch.uint8, device=dev)
    wp = ws.data_ptr() + (-ws.data_ptr()) % 256
    pairs = (ctypes.c_int32 * 4)(0, 1, 2, 3)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    good = dict(models=models.data_ptr(), n=n, I=I, N=N, K=K, r=r, weights=None, pairs=pairs, n_pairs=2, flags=3, skip=-1,
                score=score.data_ptr(), perm=perm.data_ptr(), ws=wp, stream=stream)
    call = lambda **kw: lib.mcl_fms_scores(*{**good, **kw}.values())
    for change, message in [(dict(r=0), b"rank 0"), (dict(r=17), b"rank 17"), (dict(n=0), b"n_models"), (dict(n=-4), b"n_models"),
                            (dict(I=-1), b"I >= 1"), (dict(N=0), b"N >= 1"), (dict(K=-2), b"K >= 1"), (dict(n_pairs=-1), b"n_pairs"),
                            (dict(pairs=(ctypes.c_int32 * 4)(0, 1, 2, 4)), b"names model 4"),
                            (dict(pairs=(ctypes.c_int32 * 4)(-1, 1, 2, 3)), b"names model -1"),
                            (dict(models=None), b"NULL"), (dict(pairs=None), b"NULL"), (dict(score=None), b"NULL"), (dict(ws=None), b"NULL"),
                            (dict(ws=wp + 8), b"aligned"), (dict(skip=3), b"skip_mode"), (dict(flags=8), b"flags")]:
        assert call(**change) != 0, change
        assert message in lib.mcl_fms_last_error(), (change, lib.mcl_fms_last_error())
    assert lib.mcl_fms_workspace_bytes(n, 0) == -1 and lib.mcl_fms_workspace_bytes(n, 17) == -1 and lib.mcl_fms_workspace_bytes(-1, 3) == -1
    torch.cuda.synchronize()
    assert bool((score == -7.0).all()) and bool((perm == -7).all())  # nothing was uploaded or launched
    assert call() == 0
    torch.cuda.synchronize()
    split = lambda m: (None, (m[: I * r].view(I, r).cpu().numpy(), m[I * r: (I + N) * r].view(N, r).cpu().numpy(),
                              m[(I + N) * r:].view(K, r).cpu().numpy()))
    for k, (s, t) in enumerate([(0, 1), (2, 3)]):
        _check(float(score[k]), perm[k].cpu().numpy(), split(models[s]), split(models[t]), False)
    assert call(n_pairs=0, pairs=None, score=None) == 0  # nothing to do is not an error


def _truncated_normal(rng, size):
    x = rng.standard_normal(size=size)
    x[x < 0] = 0
    return x


def _example_problem(I, J, K, rank, noise_level, c_normal):
    """the simulated PARAFAC2 data of the reference's examples, as tests/test_gpu_multistart.py states it"""
    rng = np.random.default_rng(0)
    A = rng.uniform(size=(I, rank)) + 0.1
    B_blueprint = _truncated_normal(rng, (J, rank))
    B_is = [np.roll(B_blueprint, i, axis=0) for i in range(I)]
    C = rng.standard_normal(size=(K, rank)) if c_normal else _truncated_normal(rng, (K, rank))
    matrices = [(B_i * A[i]) @ C.T for i, B_i in enumerate(B_is)]
    noise = [rng.uniform(size=M.shape) for M in matrices]
    return [M + N * noise_level * np.linalg.norm(M) / np.linalg.norm(N) for M, N in zip(matrices, noise)]


def test_the_starts_of_a_fused_fit_end_to_end():
    mats = _example_problem(10, 15, 20, 3, 0.2, False)
    results = dec.parafac2_aoadmm_multistart(mats, 3, range(8), method="fused", non_negative=True, n_iter_max=1000, return_errors=True)
    cmfs = [(np.asarray(c[0]) if c[0] is not None else None, (np.asarray(c[1][0]), [np.asarray(B_i) for B_i in c[1][1]], np.asarray(c[1][2])))
            for c, _ in results]
    best = dec.best_start(results)
    assert best is not None
    scores, perms = sim.multistart_similarity(results, return_permutations=True)  # reference="best", method="auto": the device
    want = [R.fms(cmfs[best], c) for c in cmfs]
    print("scores against the best start:", scores)
    assert np.abs(scores - [w[0] for w in want]).max() <= TOL
    for s in range(8):
        assert abs(R.score_of(want[s][2], perms[s]) - scores[s]) <= TOL
    assert np.array_equal(scores, sim.multistart_similarity(results, method="device"))
    matrix = sim.multistart_similarity(results, all_pairs=True)
    assert np.abs(matrix - [[R.fms(a, b)[0] for b in cmfs] for a in cmfs]).max() <= TOL and np.array_equal(matrix, matrix.T)
