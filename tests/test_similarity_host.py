"""CPU: factor_match_score / multistart_similarity / permute_cmf with method="host" against the restatement of
tests/similarity_restatement.py and a brute force over all permutations, every option, the refusals, and the C ABI of the device
form (no device call is made here)."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest
import torch

import matcouply_amd
from matcouply_amd import _engine, similarity as sim
from matcouply_amd.coupled_matrices import CoupledMatrixFactorization
from matcouply_amd.decomposition import DiagnosticMetrics
from tests import similarity_restatement as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-12  # scores: two summation orders over at most 600 rows differ by 600 * 3 * 1.1e-16 ~ 2e-13
MARGIN = 1e-6  # permutations are compared where the optimum is isolated by more than this


@pytest.fixture
def no_device(monkeypatch):
    def refuse(*args, **kwargs):
        raise AssertionError("the device was touched")

    monkeypatch.setattr(matcouply_amd.decomposition, "_device", refuse)
    monkeypatch.setattr(_engine, "fms_scores", refuse)
    monkeypatch.setattr(sim, "_device_present", lambda: True)  # "auto" would take the device where it serves the call


def _pair(rank, seed=0, weights=(True, True), rows=(4, 11, 6)):
    rng = np.random.RandomState(100 * rank + seed)
    return R.random_model(rng, rows, rank, weights=weights[0]), R.random_model(rng, rows, rank, weights=weights[1])


def _check(got, cmf1, cmf2, **options):
    """the checks that hold with or without an isolated optimum, then the permutation where it is isolated"""
    score, perm = got
    want, want_perm, M = R.fms(cmf1, cmf2, **options)
    rank = len(M)
    assert perm.dtype == np.int32 and sorted(perm.tolist()) == list(range(rank))
    assert abs(R.score_of(M, perm) - score) <= TOL
    assert abs(score - want) <= TOL
    if rank <= 5:
        best, best_perm, gap = R.brute_force(M)
        assert abs(score - best) <= TOL
        assert gap > MARGIN, "the seed gives no isolated optimum"
        assert perm.tolist() == best_perm.tolist()
    else:
        assert R.margin(M) > MARGIN, "the seed gives no isolated optimum"
        assert perm.tolist() == want_perm.tolist()


@pytest.mark.parametrize("rank", [1, 3, 5])
@pytest.mark.parametrize("weights", [(False, False), (True, True), (True, False)])
@pytest.mark.parametrize("skip_mode", [None, 0, 1, 2])
@pytest.mark.parametrize("absolute_value", [False, True])
@pytest.mark.parametrize("consider_weights", [False, True])
def test_host_matches_the_restatement_and_the_brute_force(rank, weights, skip_mode, absolute_value, consider_weights):
    cmf1, cmf2 = _pair(rank, weights=weights)
    options = dict(consider_weights=consider_weights, skip_mode=skip_mode, absolute_value=absolute_value)
    _check(sim.factor_match_score(cmf1, cmf2, return_permutation=True, method="host", **options), cmf1, cmf2, **options)
    score = sim.factor_match_score(cmf1, cmf2, method="host", **options)
    assert isinstance(score, float) and abs(score - R.fms(cmf1, cmf2, **options)[0]) <= TOL


def test_margin_agrees_with_the_brute_force():
    # the margin the GPU tests rely on above rank 5 is the brute-force one where both can be computed
    for rank in (2, 3, 4, 5):
        M = R.match_matrix(*_pair(rank, seed=3))
        assert abs(R.margin(M) - R.brute_force(M)[2]) <= 1e-12


@pytest.mark.parametrize("rows", R.ROWS)
@pytest.mark.parametrize("rank", R.RANKS)
def test_every_gpu_parity_case_has_an_isolated_optimum(rank, rows):
    # tests/test_gpu_similarity.py compares permutations on these models: the condition holds with the restatement alone
    cmf1, cmf2 = R.parity_pair(rank, rows)
    score, perm, M = R.fms(cmf1, cmf2)
    assert R.margin(M) > MARGIN
    if rank == 16:  # planted: every chosen entry is close to 1
        assert score > 0.99
    if (rank, rows) in R.OPTION_CASES:  # the cases at which every option is tried
        for consider_weights, absolute_value, skip_mode in itertools.product((True, False), (True, False), (None, 0, 1, 2)):
            assert R.margin(R.match_matrix(cmf1, cmf2, consider_weights=consider_weights, absolute_value=absolute_value,
                                           skip_mode=skip_mode)) > MARGIN


def test_planted_permutation_is_recovered():
    rng = np.random.RandomState(5)
    cmf1 = R.random_model(rng, (6, 40, 9), 16, weights=True)
    cmf2, p = R.planted_model(rng, cmf1)
    score, perm = sim.factor_match_score(cmf1, cmf2, return_permutation=True, method="host")
    assert score > 0.99 and np.argsort(p).tolist() == perm.tolist()  # cmf2[:, perm] ~ cmf1
    _check((score, perm), cmf1, cmf2)


@pytest.mark.parametrize("skip_mode", [None, 0, 1, 2])
def test_zero_column_scores_zero_without_nan(skip_mode):
    cmf1, cmf2 = _pair(3, seed=1, weights=(False, True))
    for mode, (c1, c2) in itertools.product(range(3), [(0, None), (None, 2), (1, 1)]):
        a, b = [[np.array(B_i) for B_i in F] if isinstance(F, list) else F.copy() for F in cmf1[1]], \
               [[np.array(B_i) for B_i in F] if isinstance(F, list) else F.copy() for F in cmf2[1]]
        for factors, col in ((a, c1), (b, c2)):
            if col is not None:
                for F in (factors[mode] if mode == 1 else [factors[mode]]):
                    F[:, col] = 0.0
        one, two = (cmf1[0], tuple(a)), (cmf2[0], tuple(b))
        for consider_weights in (False, True):
            score, perm = sim.factor_match_score(one, two, consider_weights=consider_weights, skip_mode=skip_mode,
                                                 return_permutation=True, method="host")
            M = R.match_matrix(one, two, consider_weights=consider_weights, skip_mode=skip_mode)
            assert np.isfinite(score) and np.isfinite(M).all()
            if c1 is not None and (mode != skip_mode or (consider_weights and c2 is None)):
                # congruence 0 with everything; where the mode is skipped, through the weight (two zero weights agree: factor 1)
                assert np.all(M[c1] == 0.0)
            assert abs(score - R.fms(one, two, consider_weights=consider_weights, skip_mode=skip_mode)[0]) <= TOL
            assert abs(R.score_of(M, perm) - score) <= TOL
    # a model that is all zeros: every score is 0, none is NaN
    zero = (None, tuple(np.zeros_like(F) if not isinstance(F, list) else [np.zeros_like(B_i) for B_i in F] for F in cmf1[1]))
    assert sim.factor_match_score(zero, cmf2, skip_mode=skip_mode, method="host") == 0.0
    assert sim.factor_match_score(zero, zero, skip_mode=skip_mode, method="host") == 0.0


def test_stacked_B_cmf_objects_and_torch_inputs_agree():
    cmf1, cmf2 = _pair(4, seed=2)
    want = sim.factor_match_score(cmf1, cmf2, return_permutation=True, method="host")
    stack = lambda cmf: (cmf[0], (cmf[1][0], np.concatenate(cmf[1][1]), cmf[1][2]))
    as_torch = lambda cmf: (torch.from_numpy(cmf[0]), (torch.from_numpy(cmf[1][0]), [torch.from_numpy(B_i) for B_i in cmf[1][1]],
                                                       torch.from_numpy(cmf[1][2])))
    for one, two in [(stack(cmf1), stack(cmf2)), (stack(cmf1), cmf2), (CoupledMatrixFactorization(cmf1), CoupledMatrixFactorization(cmf2)),
                     (as_torch(cmf1), as_torch(cmf2)), (as_torch(cmf1), cmf2)]:
        got = sim.factor_match_score(one, two, return_permutation=True, method="host")
        assert got[0] == want[0] and got[1].tolist() == want[1].tolist()
    # float32 factors are widened exactly
    f32 = lambda cmf: (cmf[0].astype(np.float32), (cmf[1][0].astype(np.float32), [B_i.astype(np.float32) for B_i in cmf[1][1]],
                                                   cmf[1][2].astype(np.float32)))
    f64 = lambda cmf: (cmf[0].astype(np.float64), (cmf[1][0].astype(np.float64), [B_i.astype(np.float64) for B_i in cmf[1][1]],
                                                   cmf[1][2].astype(np.float64)))
    assert sim.factor_match_score(f32(cmf1), f32(cmf2), method="host") == sim.factor_match_score(f64(f32(cmf1)), f64(f32(cmf2)), method="host")


@pytest.mark.parametrize("kind", ["tuple", "stacked", "object", "torch", "no weights"])
def test_permute_cmf_round_trip(kind):
    cmf1, cmf2 = _pair(5, seed=4)
    if kind == "stacked":
        cmf2 = (cmf2[0], (cmf2[1][0], np.concatenate(cmf2[1][1]), cmf2[1][2]))
    elif kind == "object":
        cmf2 = CoupledMatrixFactorization(cmf2)
    elif kind == "torch":
        cmf2 = (torch.from_numpy(cmf2[0]), (torch.from_numpy(cmf2[1][0]), [torch.from_numpy(B_i) for B_i in cmf2[1][1]],
                                            torch.from_numpy(cmf2[1][2])))
    elif kind == "no weights":
        cmf2 = (None, cmf2[1])
    score, perm = sim.factor_match_score(cmf1, cmf2, return_permutation=True, method="host")
    assert perm.tolist() != list(range(5))
    lined_up = sim.permute_cmf(cmf2, perm)
    assert type(lined_up) is type(cmf2)
    again, identity = sim.factor_match_score(cmf1, lined_up, return_permutation=True, method="host")
    assert identity.tolist() == list(range(5)) and abs(again - score) <= TOL
    if kind == "tuple":
        assert np.array_equal(lined_up[1][1][1], cmf2[1][1][1][:, perm]) and np.array_equal(lined_up[0], cmf2[0][perm])
    with pytest.raises(ValueError, match="permutation"):
        sim.permute_cmf(cmf2, [0, 0, 1, 2, 3])


def _diag(loss, satisfied):
    return DiagnosticMetrics(rec_errors=[1.0, loss], feasibility_gaps=[], regularized_loss=[2.0, loss], satisfied_stopping_condition=satisfied,
                             satisfied_feasibility_condition=True, n_iter=1, message="")


def _results(n=5, rank=3, seed=7):
    rng = np.random.RandomState(seed)
    return [R.random_model(rng, (4, 11, 6), rank, weights=bool(s % 2)) for s in range(n)]


def test_multistart_similarity_references():
    models = _results()
    losses = [0.5, 0.1, 0.3, 0.05, 0.4]
    with_diag = [(CoupledMatrixFactorization(m), _diag(l, s != 3)) for s, (m, l) in enumerate(zip(models, losses))]
    want = lambda ref: np.array([R.fms(ref, m)[0] for m in models])
    # best_start: the lowest loss among the starts that satisfied the stopping condition is start 1
    assert np.abs(sim.multistart_similarity(with_diag, method="host") - want(models[1])).max() <= TOL
    for results in (models, [(m,) for m in models], [(m, [0.1, 0.2]) for m in models]):
        with pytest.raises(ValueError, match="return_errors"):
            sim.multistart_similarity(results, method="host")
    with pytest.raises(ValueError, match="stopping condition"):
        sim.multistart_similarity([(m, _diag(0.1, False)) for m in models], method="host")
    scores = sim.multistart_similarity(models, 2, method="host")
    assert scores.dtype == np.float64 and scores.shape == (5,) and np.abs(scores - want(models[2])).max() <= TOL
    assert abs(scores[2] - 1.0) <= TOL
    assert np.array_equal(sim.multistart_similarity(models, -3, method="host"), scores)
    other = R.random_model(np.random.RandomState(8), (4, 11, 6), 3)
    scores, perms = sim.multistart_similarity(models, other, return_permutations=True, method="host", consider_weights=False)
    assert perms.dtype == np.int32 and perms.shape == (5, 3)
    for s, m in enumerate(models):
        _check((scores[s], perms[s]), other, m, consider_weights=False)
    got = sim.multistart_similarity(models, pairs=[(0, 1), (1, 0), (4, 4), (0, 1)], skip_mode=1, method="host")
    assert np.abs(got - [R.fms(models[s], models[t], skip_mode=1)[0] for s, t in [(0, 1), (1, 0), (4, 4), (0, 1)]]).max() <= TOL


def test_multistart_similarity_takes_parafac2_tensors():
    rng = np.random.RandomState(9)
    I, K, r = 3, 5, 2
    results = []
    for _ in range(3):
        P = [np.linalg.qr(rng.standard_normal((6, r)))[0] for _ in range(I)]
        results.append(((None, (rng.standard_normal((I, r)), rng.standard_normal((r, r)), rng.standard_normal((K, r))), P), [0.3, 0.2]))
    as_cmf = [(None, (t[1][0], [P_i @ t[1][1] for P_i in t[2]], t[1][2])) for t, _ in results]
    got = sim.multistart_similarity(results, 0, method="host")
    assert np.abs(got - [R.fms(as_cmf[0], m)[0] for m in as_cmf]).max() <= TOL


def test_all_pairs_is_exactly_symmetric():
    models = _results(6)
    scores, perms = sim.multistart_similarity(models, all_pairs=True, return_permutations=True, method="host")
    assert scores.shape == (6, 6) and perms.shape == (6, 6, 3) and perms.dtype == np.int32
    assert np.array_equal(scores, scores.T)
    assert np.abs(np.diag(scores) - 1.0).max() <= TOL
    for s, t in itertools.product(range(6), repeat=2):
        assert abs(scores[s, t] - R.fms(models[s], models[t])[0]) <= TOL
        M = R.match_matrix(models[s], models[t])
        assert sorted(perms[s, t].tolist()) == [0, 1, 2] and abs(R.score_of(M, perms[s, t]) - scores[s, t]) <= TOL
    assert np.array_equal(sim.multistart_similarity(models, all_pairs=True, method="host"), scores)


def test_value_errors(no_device):
    cmf1, cmf2 = _pair(3)
    rank4 = _pair(4)[0]
    taller = R.random_model(np.random.RandomState(0), (4, 12, 6), 3)
    for method in ("auto", "host", "device"):
        with pytest.raises(ValueError, match="rank"):
            sim.factor_match_score(cmf1, rank4, method=method)
        with pytest.raises(ValueError, match="shape"):
            sim.factor_match_score(cmf1, taller, method=method)
        with pytest.raises(ValueError, match="shape"):
            sim.factor_match_score(cmf1, taller, skip_mode=0, method=method)
        for skip_mode in (3, -1, "B", 1.0, True):
            with pytest.raises(ValueError, match="skip_mode"):
                sim.factor_match_score(cmf1, cmf2, skip_mode=skip_mode, method=method)
            with pytest.raises(ValueError, match="skip_mode"):
                sim.multistart_similarity([cmf1, cmf2], 0, skip_mode=skip_mode, method=method)
        with pytest.raises(ValueError, match="at least one"):
            sim.multistart_similarity([], 0, method=method)
        with pytest.raises(ValueError, match="rank"):
            sim.multistart_similarity([cmf1, rank4], 0, method=method)
        with pytest.raises(ValueError, match="shape"):
            sim.multistart_similarity([cmf1, taller], all_pairs=True, method=method)
        with pytest.raises(ValueError, match="outside"):
            sim.multistart_similarity([cmf1, cmf2], pairs=[(0, 2)], method=method)
        with pytest.raises(ValueError, match="outside"):
            sim.multistart_similarity([cmf1, cmf2], 2, method=method)
        with pytest.raises(ValueError, match="reference"):
            sim.multistart_similarity([cmf1, cmf2], "first", method=method)
        with pytest.raises(ValueError, match="either"):
            sim.multistart_similarity([cmf1, cmf2], pairs=[(0, 1)], all_pairs=True, method=method)
    with pytest.raises(ValueError, match="method"):
        sim.factor_match_score(cmf1, cmf2, method="fused")
    with pytest.raises(ValueError, match="rank"):
        sim.factor_match_score((np.ones(2), cmf1[1]), cmf2, method="host")
    with pytest.raises(TypeError, match="unexpected keyword"):
        sim.multistart_similarity([cmf1, cmf2], 0, weights=True)
    with pytest.raises(TypeError, match="model"):
        sim.multistart_similarity([cmf1, 3.0], 0, method="host")
    # a skipped mode may differ in its rows: the host serves it
    assert abs(sim.factor_match_score(cmf1, taller, skip_mode=1, method="host") - R.fms(cmf1, taller, skip_mode=1)[0]) <= TOL


def test_all_pairs_permutations_are_bounded(no_device, monkeypatch):
    models = _results(4)
    monkeypatch.setattr(sim, "_ALL_PAIRS_MAX_BYTES", 4 * 4 * 3 * 4 - 1)
    for method in ("auto", "host", "device"):
        with pytest.raises(ValueError, match="_ALL_PAIRS_MAX_BYTES"):
            sim.multistart_similarity(models, all_pairs=True, return_permutations=True, method=method)
    assert sim.multistart_similarity(models, all_pairs=True, method="host").shape == (4, 4)  # the scores alone are not bounded


def test_device_refusals_touch_no_device(no_device):
    rows = (4, 11, 6)
    rng = np.random.RandomState(0)
    rank17 = [R.random_model(rng, rows, 17) for _ in range(2)]
    with pytest.raises(NotImplementedError, match="rank 17"):
        sim.factor_match_score(*rank17, method="device")
    with pytest.raises(NotImplementedError, match="rank 17"):
        sim.multistart_similarity(rank17, 0, method="device")
    # mixed shapes: pairs that are each well formed, but not one shape for the whole launch
    mixed = [R.random_model(rng, rows, 3), R.random_model(rng, rows, 3), R.random_model(rng, (4, 12, 6), 3), R.random_model(rng, (4, 12, 6), 3)]
    with pytest.raises(NotImplementedError, match="one shape"):
        sim.multistart_similarity(mixed, pairs=[(0, 1), (2, 3)], method="device")
    with pytest.raises(NotImplementedError, match="one shape"):
        sim.factor_match_score(mixed[0], mixed[2], skip_mode=1, method="device")
    cmf1, cmf2 = _pair(3)
    half = (None, (cmf1[1][0].astype(np.float16), cmf1[1][1], cmf1[1][2]))
    with pytest.raises(NotImplementedError, match="float16"):
        sim.factor_match_score(half, cmf2, method="device")
    bad = (None, (cmf1[1][0].copy(), cmf1[1][1], cmf1[1][2]))
    bad[1][0][0, 0] = np.inf
    with pytest.raises(NotImplementedError, match="non-finite"):
        sim.factor_match_score(bad, cmf2, method="device")
    # "auto" falls back to the host for each of them
    assert abs(sim.factor_match_score(*rank17, method="auto") - R.fms(*rank17)[0]) <= TOL
    got = sim.multistart_similarity(mixed, pairs=[(0, 1), (2, 3)], method="auto")
    assert np.abs(got - [R.fms(mixed[0], mixed[1])[0], R.fms(mixed[2], mixed[3])[0]]).max() <= TOL
    assert abs(sim.factor_match_score(half, cmf2, method="auto") - R.fms(half, cmf2)[0]) <= TOL


def test_auto_takes_the_host_without_a_device(monkeypatch):
    def refuse(*args, **kwargs):
        raise AssertionError("the device was touched")

    monkeypatch.setattr(sim, "_device_present", lambda: False)
    monkeypatch.setattr(_engine, "fms_scores", refuse)
    cmf1, cmf2 = _pair(3)
    assert abs(sim.factor_match_score(cmf1, cmf2) - R.fms(cmf1, cmf2)[0]) <= TOL


def test_device_method_fails_loudly_without_a_device():
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible")
    with pytest.raises(_engine.EngineError, match="no HIP device"):
        sim.factor_match_score(*_pair(3), method="device")


def test_names_are_exported_from_the_package():
    for name in ("factor_match_score", "multistart_similarity", "permute_cmf"):
        assert getattr(matcouply_amd, name) is getattr(sim, name) and name in sim.__all__
    assert matcouply_amd.similarity is sim


# ---- the C ABI of the device form: header, binding and library agree -------------------------------------------------------
FMS_SYMBOLS = ("mcl_fms_workspace_bytes", "mcl_fms_scores", "mcl_fms_last_error")
CTYPE_OF = {"int64_t": "c_long", "int32_t": "c_int", "int": "c_int", "const double *": "c_void_p", "double *": "c_void_p",
            "int32_t *": "c_void_p", "void *": "c_void_p", "const int32_t *": "LP_c_int", "const char *": "c_char_p"}


def _declaration(name):
    text = open(os.path.join(REPO, "include", "matcouply_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"([\w ]+?\*?)\s*\b" + name + r"\s*\(([^)]*)\)\s*;", text)
    assert m, f"{name} is not declared in include/matcouply_hip.h"
    args = [] if m.group(2).strip() == "void" else [re.sub(r"\s*\w+$", "", a.strip()).strip() for a in m.group(2).split(",")]
    return m.group(1).strip(), args


@pytest.mark.parametrize("name", FMS_SYMBOLS)
def test_header_binding_and_library_agree_on_the_fms_symbols(name):
    assert name in _engine.EXPORTED_SYMBOLS
    fn = getattr(_engine.load_library(), name)
    result, args = _declaration(name)
    assert CTYPE_OF[result] == fn.restype.__name__
    assert [CTYPE_OF[a] for a in args] == [t.__name__ for t in fn.argtypes]


def test_fms_argument_list_is_the_documented_one():
    result, args = _declaration("mcl_fms_scores")
    assert result == "int" and args == ["const double *", "int64_t", "int64_t", "int64_t", "int64_t", "int32_t", "const double *",
                                        "const int32_t *", "int64_t", "int32_t", "int32_t", "double *", "int32_t *", "void *", "void *"]
    assert _declaration("mcl_fms_workspace_bytes") == ("int64_t", ["int64_t", "int32_t"])
    assert _declaration("mcl_fms_last_error") == ("const char *", [])
    assert _engine.MCL_ABI_VERSION == 410 and _engine.FMS_MAX_RANK == 16


def test_fms_entry_points_refuse_bad_arguments_without_a_device():
    # the checks come before any HIP call, so they are the same on a machine without a device
    lib = _engine.load_library()
    assert lib.mcl_fms_workspace_bytes(4, 0) == -1 and lib.mcl_fms_workspace_bytes(4, 17) == -1 and lib.mcl_fms_workspace_bytes(0, 3) == -1
    assert lib.mcl_fms_workspace_bytes(5, 3) == 5 * 512
    pairs = (ctypes.c_int32 * 2)(0, 4)
    fake = 256  # never dereferenced: every call below is refused first
    for args, message in [((fake, 4, 2, 3, 2, 0, None, pairs, 1, 3, -1, fake, None, fake, None), b"rank 0"),
                          ((fake, 4, 2, 3, 2, 17, None, pairs, 1, 3, -1, fake, None, fake, None), b"rank 17"),
                          ((fake, 4, 2, -3, 2, 3, None, pairs, 1, 3, -1, fake, None, fake, None), b"N >= 1"),
                          ((fake, 4, 2, 3, 2, 3, None, pairs, -1, 3, -1, fake, None, fake, None), b"n_pairs"),
                          ((fake, 4, 2, 3, 2, 3, None, pairs, 1, 3, 3, fake, None, fake, None), b"skip_mode"),
                          ((fake, 4, 2, 3, 2, 3, None, pairs, 1, 4, -1, fake, None, fake, None), b"flags"),
                          ((None, 4, 2, 3, 2, 3, None, pairs, 1, 3, -1, fake, None, fake, None), b"NULL"),
                          ((fake, 4, 2, 3, 2, 3, None, None, 1, 3, -1, fake, None, fake, None), b"NULL"),
                          ((fake, 4, 2, 3, 2, 3, None, pairs, 1, 3, -1, fake, None, fake + 8, None), b"aligned"),
                          ((fake, 4, 2, 3, 2, 3, None, pairs, 1, 3, -1, fake, None, fake, None), b"names model 4 of 4")]:
        assert lib.mcl_fms_scores(*args) != 0
        assert message in lib.mcl_fms_last_error(), (message, lib.mcl_fms_last_error())

