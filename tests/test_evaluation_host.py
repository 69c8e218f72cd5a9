"""CPU: core_consistency / slabwise_sse / relative_sse / fit / multistart_evaluation with method="host" against the dense
restatement of tests/evaluation_restatement.py (the pinv route against the Gram route of the package), the argument checks, the
refusal reasons of the device form, and its C ABI (no device call is made here)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import matcouply_amd
from matcouply_amd import _engine, evaluation as ev
from matcouply_amd.coupled_matrices import CoupledMatrixFactorization
from tests import evaluation_restatement as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-9  # the Gram route squares the condition number: 100^2 * 100 (three modes' worth) * 1.1e-16 ~ 1e-10


@pytest.fixture
def no_device(monkeypatch):
    def refuse(*args, **kwargs):
        raise AssertionError("the device was touched")

    monkeypatch.setattr(matcouply_amd.decomposition, "_device", refuse)
    monkeypatch.setattr(_engine, "eval_tables", refuse)
    monkeypatch.setattr(_engine, "eval_core", refuse)
    monkeypatch.setattr(ev, "_device_present", lambda: True)  # "auto" would take the device where it serves the call


def _problem(rank, seed=0, weights=False, kappa=100.0, rows=None, K=None):
    rows = rows or [rank + 2 + i for i in range(rank + 3)]
    cmf, Xs = R.random_problem(np.random.RandomState(100 * rank + seed), rows, K or rank + 4, rank, noise=0.3, kappa=kappa,
                               weights=weights)
    if kappa:
        assert max(np.linalg.cond(F) for F in [cmf[1][0], cmf[1][2]] + cmf[1][1]) <= kappa * (1 + 1e-9)
    return cmf, Xs


def _close(got, want):
    return np.linalg.norm(np.asarray(got) - want) <= TOL * max(np.linalg.norm(want), 1.0)


@pytest.mark.parametrize("weights", [False, True])
@pytest.mark.parametrize("rank", [1, 3, 8, 17])
def test_host_against_the_restatement(rank, weights):
    cmf, Xs = _problem(rank, weights=weights)
    want = R.evaluate(cmf, Xs)
    assert abs(ev.core_consistency(cmf, Xs, method="host") - want["core_consistency"]) <= 100 * TOL * max(1.0, np.sum(want["core"] ** 2))
    assert abs(ev.core_consistency(cmf, Xs, normalised=True, method="host") - want["core_consistency_normalised"]) <= 100 * TOL * max(
        1.0, np.sum(want["core"] ** 2))
    assert _close(ev.slabwise_sse(cmf, Xs, method="host"), want["slab_sse"])
    assert _close(ev.slabwise_sse(cmf, Xs, normalise=True, method="host"), want["slab_sse"] / want["slab_sse"].sum())
    assert abs(ev.relative_sse(cmf, Xs, method="host") - want["relative_sse"]) <= TOL
    assert abs(ev.fit(cmf, Xs, method="host") - want["fit"]) <= TOL
    out = ev.multistart_evaluation(Xs, [cmf], method="host")
    assert isinstance(out, ev.ModelEvaluation) and out._fields == ("fit", "relative_sse", "slab_sse", "core_consistency",
                                                                   "core_consistency_normalised", "core")
    assert _close(out.core[0], want["core"]) and out.core.shape == (1, rank, rank, rank)
    assert out.fit[0] == ev.fit(cmf, Xs, method="host") and out.core_consistency[0] == ev.core_consistency(cmf, Xs, method="host")


@pytest.mark.parametrize("kind", ["cp", "parafac2"])
@pytest.mark.parametrize("rank", [2, 5, 16])
def test_known_core_consistency(rank, kind):
    for deviation, answer in [(0.4, 60.0), (0.0, 100.0)]:
        cmf, Xs, G0 = R.known_core_problem(np.random.RandomState(rank), rank, kind, deviation)
        assert abs(ev.core_consistency(cmf, Xs, method="host") - answer) <= 1e-9
        assert _close(ev.multistart_evaluation(Xs, [cmf], method="host").core[0], G0)
        assert abs(ev.fit(cmf, Xs, method="host") - 1.0) <= 1e-9 if deviation == 0.0 else ev.fit(cmf, Xs, method="host") < 1.0


def test_every_kind_of_model_and_data():
    cmf, Xs = _problem(3, weights=True)
    w, (A, B_is, C) = cmf
    want = ev.multistart_evaluation(Xs, [cmf], method="host")
    same = [CoupledMatrixFactorization((w, (A, B_is, C))), (w, (A, np.concatenate(B_is, 0), C)), (None, (A * w, B_is, C)),
            (torch.from_numpy(w), (torch.from_numpy(A), [torch.from_numpy(B_i) for B_i in B_is], torch.from_numpy(C)))]
    for model in same:
        for data in (Xs, [torch.from_numpy(X) for X in Xs]):
            got = ev.multistart_evaluation(data, [model], method="host")
            assert all(np.allclose(a, b, rtol=1e-13, atol=1e-13) for a, b in zip(got, want))
    # a PARAFAC2 tensor (weights, (A, B, C), projections): B_i = P_i B
    rng = np.random.RandomState(5)
    P = [np.linalg.qr(rng.standard_normal((len(X), 3)))[0] for X in Xs]
    Delta = rng.standard_normal((3, 3))
    pf2, plain = (None, (A, Delta, C), P), (None, (A, [P_i @ Delta for P_i in P], C))
    assert ev.core_consistency(pf2, Xs, method="host") == ev.core_consistency(plain, Xs, method="host")


def test_multistart_evaluation_on_tuples_and_on_bare_models():
    rank = 3
    cmf, Xs = _problem(rank)
    rng = np.random.RandomState(1)
    cmfs = [cmf] + [(None, (cmf[1][0] + 0.1 * rng.standard_normal(cmf[1][0].shape), cmf[1][1], cmf[1][2])) for _ in range(3)]
    bare = ev.multistart_evaluation(Xs, cmfs, method="host")
    tuples = ev.multistart_evaluation(Xs, [(c, "diagnostics") for c in cmfs], method="host")
    assert all(np.array_equal(a, b) for a, b in zip(bare, tuples))
    assert bare.fit.shape == (4,) and bare.slab_sse.shape == (4, len(Xs)) and bare.core.shape == (4, rank, rank, rank)
    for k, c in enumerate(cmfs):
        want = R.evaluate(c, Xs)
        assert abs(bare.fit[k] - want["fit"]) <= TOL and _close(bare.slab_sse[k], want["slab_sse"]) and _close(bare.core[k], want["core"])
    with pytest.raises(ValueError, match="at least one"):
        ev.multistart_evaluation(Xs, [], method="host")
    with pytest.raises(TypeError):
        ev.multistart_evaluation(Xs, [3], method="host")


def test_rank_deficient_factors_take_the_pseudo_inverse():
    cmf, Xs = _problem(3, kappa=None, rows=[2, 5, 6, 7], K=6)  # a matrix with fewer rows than components
    want = R.evaluate(cmf, Xs)
    assert _close(ev.multistart_evaluation(Xs, [cmf], method="host").core[0], want["core"])


def test_argument_checks():
    cmf, Xs = _problem(3)
    w, (A, B_is, C) = cmf
    with pytest.raises(ValueError, match="method"):
        ev.fit(cmf, Xs, method="gpu")
    with pytest.raises(ValueError, match="shape mismatch"):
        ev.fit(cmf, Xs[:-1], method="host")
    with pytest.raises(ValueError, match="shape mismatch"):
        ev.core_consistency(cmf, [X[:, :-1] for X in Xs], method="host")
    with pytest.raises(ValueError, match="shape mismatch"):
        ev.slabwise_sse(cmf, [X[:-1] for X in Xs], method="host")
    swapped = Xs[:]  # the same total number of rows, in other matrices
    swapped[0], swapped[1] = Xs[1], Xs[0]
    with pytest.raises(ValueError, match="rows"):
        ev.relative_sse(cmf, swapped, method="host")
    with pytest.raises(ValueError, match="same number of columns"):
        ev.fit(cmf, [Xs[0][:, :-1]] + Xs[1:], method="host")
    with pytest.raises(ValueError, match="rank mismatch"):
        ev.multistart_evaluation(Xs, [cmf, _problem(4, rows=[len(X) for X in Xs], K=Xs[0].shape[1])[0]], method="host")
    with pytest.raises(TypeError):
        ev.fit(3, Xs, method="host")


def test_device_refusals_touch_no_device(no_device):
    rows = [40, 41]
    wide, Xw = _problem(33, kappa=None, rows=rows, K=35)
    with pytest.raises(NotImplementedError, match="rank 33"):
        ev.fit(wide, Xw, method="device")
    with pytest.raises(NotImplementedError, match="rank 33"):
        ev.multistart_evaluation(Xw, [wide], method="device")
    cmf, Xs = _problem(3)
    w, (A, B_is, C) = cmf
    with pytest.raises(NotImplementedError, match="float16"):
        ev.fit((None, (A.astype(np.float16), B_is, C)), Xs, method="device")
    bad = (None, (A.copy(), B_is, C))
    bad[1][0][0, 0] = np.inf
    with pytest.raises(NotImplementedError, match="non-finite"):
        ev.slabwise_sse(bad, Xs, method="device")
    with pytest.raises(NotImplementedError, match="int64"):
        ev.fit(cmf, [X.astype(np.int64) for X in Xs], method="device")
    with pytest.raises(NotImplementedError, match="one shape"):
        ev.multistart_evaluation(Xs, [cmf, _problem(4, rows=[len(X) for X in Xs], K=Xs[0].shape[1])[0]], method="device")
    short, Xshort = _problem(3, kappa=None, rows=[2, 5, 6, 7], K=6)
    with pytest.raises(NotImplementedError, match="fewer rows than components"):
        ev.core_consistency(short, Xshort, method="device")
    with pytest.raises(NotImplementedError, match="fewer rows than components"):
        ev.multistart_evaluation(Xshort, [short], method="device")
    # "auto" falls back to the host for each of them
    assert abs(ev.fit(wide, Xw) - R.evaluate(wide, Xw)["fit"]) <= TOL
    assert _close(ev.multistart_evaluation(Xshort, [short]).core[0], R.evaluate(short, Xshort)["core"])


def test_auto_takes_the_host_without_a_device(monkeypatch):
    def refuse(*args, **kwargs):
        raise AssertionError("the device was touched")

    monkeypatch.setattr(ev, "_device_present", lambda: False)
    monkeypatch.setattr(_engine, "eval_tables", refuse)
    cmf, Xs = _problem(3)
    assert abs(ev.fit(cmf, Xs) - R.evaluate(cmf, Xs)["fit"]) <= TOL


def test_names_are_exported_from_the_package():
    for name in ("core_consistency", "slabwise_sse", "relative_sse", "fit", "multistart_evaluation", "ModelEvaluation"):
        assert getattr(matcouply_amd, name) is getattr(ev, name) and name in ev.__all__
    assert matcouply_amd.evaluation is ev


# ---- the C ABI of the device form: header, binding and library agree -------------------------------------------------------
EVAL_SYMBOLS = ("mcl_eval_workspace_bytes", "mcl_eval_tables_typed", "mcl_eval_core", "mcl_eval_last_error")
CTYPE_OF = {"int64_t": "c_long", "int32_t": "c_int", "int": "c_int", "const double *": "c_void_p", "double *": "c_void_p",
            "void *": "c_void_p", "const void *": "c_void_p", "const int64_t *": "LP_c_long", "const char *": "c_char_p"}


def _declaration(name):
    text = open(os.path.join(REPO, "include", "matcouply_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"([\w ]+?\*?)\s*\b" + name + r"\s*\(([^)]*)\)\s*;", text)
    assert m, f"{name} is not declared in include/matcouply_hip.h"
    args = [] if m.group(2).strip() == "void" else [re.sub(r"\s*\w+$", "", a.strip()).strip() for a in m.group(2).split(",")]
    return m.group(1).strip(), args


@pytest.mark.parametrize("name", EVAL_SYMBOLS)
def test_header_binding_and_library_agree_on_the_eval_symbols(name):
    assert name in _engine.EXPORTED_SYMBOLS
    fn = getattr(_engine.load_library(), name)
    result, args = _declaration(name)
    assert CTYPE_OF[result] == fn.restype.__name__
    assert [CTYPE_OF[a] for a in args] == [t.__name__ for t in fn.argtypes]


def test_eval_argument_lists_are_the_documented_ones():
    assert _declaration("mcl_eval_workspace_bytes") == ("int64_t", ["const int64_t *", "int64_t", "int64_t", "int32_t", "int64_t"])
    assert _declaration("mcl_eval_tables_typed") == ("int", ["const void *", "int32_t", "const int64_t *", "int64_t", "int64_t", "int32_t",
                                                             "const double *", "int64_t", "double *", "double *", "double *", "double *",
                                                             "void *", "int64_t", "void *"])
    assert _declaration("mcl_eval_core") == ("int", ["const double *", "int64_t", "int64_t", "int64_t", "int64_t", "int32_t",
                                                     "const double *", "const double *", "double *", "double *", "double *", "void *"])
    assert _declaration("mcl_eval_last_error") == ("const char *", [])
    assert _engine.MCL_ABI_VERSION == 410 and _engine.load_library().mcl_version() == 410 and _engine.EVAL_MAX_RANK == 32


def test_eval_entry_points_refuse_bad_arguments_without_a_device():
    # these checks come before any HIP call, so they are the same on a machine without a device
    lib = _engine.load_library()
    rp = lambda a: np.ascontiguousarray(a, dtype=np.int64).ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
    good = rp([0, 3, 70, 71])
    assert lib.mcl_eval_workspace_bytes(good, 3, 5, 0, 2) == -1 and lib.mcl_eval_workspace_bytes(good, 3, 5, 33, 2) == -1
    assert lib.mcl_eval_workspace_bytes(good, 3, 5, 3, 0) == -1 and lib.mcl_eval_workspace_bytes(rp([0, 3, 3, 71]), 3, 5, 3, 2) == -1
    # 4 segments (3 + 64 + 3 + 1 rows), 3 matrices, one 64-column chunk at rank <= 16, 2 models; every part rounded up to 256 bytes
    al = lambda b: (b + 255) // 256 * 256
    want = al(4 * 16) + al(4 * 4) + 2 * al(2 * 64 * 16 * 4) + al(2 * 4 * (2 * 9 + 2) * 8)
    assert lib.mcl_eval_workspace_bytes(good, 3, 5, 3, 2) == want
    fake = 256  # never dereferenced: every call below is refused first
    tables = lambda rank=3, n=2, row_ptr=good, ws_bytes=want, ws=fake: lib.mcl_eval_tables_typed(
        fake, 0, row_ptr, 3, 5, rank, fake, n, fake, fake, fake, fake, ws, ws_bytes, None)
    for call, message in [(lambda: tables(rank=0), b"rank 0"), (lambda: tables(rank=33), b"rank 33"), (lambda: tables(n=0), b"n_models"),
                          (lambda: tables(row_ptr=rp([0, 3, 2, 71])), b"row_ptr must increase"),
                          (lambda: tables(ws_bytes=want - 1), b"workspace too small"), (lambda: tables(ws=fake + 8), b"aligned"),
                          (lambda: lib.mcl_eval_core(fake, 2, 3, 71, 5, 0, fake, fake, fake, fake, fake, None), b"rank 0"),
                          (lambda: lib.mcl_eval_core(fake, 0, 3, 71, 5, 3, fake, fake, fake, fake, fake, None), b"n_models"),
                          (lambda: lib.mcl_eval_core(fake, 2, 3, 71, 5, 3, fake, None, fake, fake, fake, None), b"NULL")]:
        assert call() != 0
        assert message in lib.mcl_eval_last_error(), (message, lib.mcl_eval_last_error())
