"""-m gpu: the software-pipelined chained B row pass (csrc/rowchain.hip: k_rows_chain_first / _mid / _last, nine stack signature x
(NBR, R64) forms each) at the stack, rank and tile edges of tests/kernel_edge_cases.py::ROWCHAIN_CASES.

  (a) one B-phase against the oracle, every case, and two outer iterations of one case per signature x bucket through the public
      call (the B-mode feasibility gaps k_rows_chain_last writes into its diagnostics tiles);
  (b) the pipelined kernels against the un-pipelined ones of rows.hip (MCL_NO_ROW_PREFETCH=1), bit for bit;
  (c) the fp32 NB = 1 forms (MCL_NO_ROWS64=1) and first + last in every inner iteration (MCL_NO_PASS_CHAIN=1);
  (d) stacks and shapes the chain does not serve, which must take other kernels and still meet the bars of (a).

The chain runs on the fast kernels only (MCL_EXACT=0).  Bars: a flat 1e-5 relative (BASELINE.json north_star); the fp32 B-phase
arithmetic is about 4e-7 per phase, while a wrong row, column, tile statistic or sink store is O(1e-2).
The orthogonal bases P_i are held to max(1e-5, 1e-8 x the oracle's worst cond(Y_i Delta^T)), as tests/test_gpu_end_to_end.py::
_compare holds them."""
import copy

import numpy as np
import pytest

from matcouply_amd import _engine as E
from tests import kernel_edge_cases as kec
from tests.helpers import native_regs, rel_err, to_np

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("fast_kernels")]  # the subject is a fast kernel

TOL = 1e-5
PIPELINED = "software-pipelined"
SWITCHES = ("MCL_NO_ROW_PREFETCH", "MCL_NO_ROWS64", "MCL_NO_PASS_CHAIN")


def _engine(st):
    """engine_from_oracle_state with the state's inner stopping tolerance passed on"""
    import torch

    t = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float32, device="cuda:0")
    regs = [native_regs(st.regs[m], st.aux[m], st.dual[m], "cuda:0") for m in range(3)]
    return E.HipEngine(t(st.X), st.row_ptr, st.A.shape[1], t(st.A), t(st.B), t(st.C), regs, l2_penalty=st.l2,
                       inner_n_iter_max=st.inner, feasibility_penalty_scale=st.scale, constant_A=st.constant_A,
                       constant_B=st.constant_B, inner_tol=st.inner_tol or 0.0)


def _device_b_phase(st, monkeypatch, switches=()):
    """one B-phase on the device from the state, with exactly `switches` of SWITCHES set -> (variant, {name: tensor})"""
    import torch

    for s in SWITCHES:
        if s in switches:
            monkeypatch.setenv(s, "1")
        else:
            monkeypatch.delenv(s, raising=False)
    eng = _engine(st)  # (the switches are read when the context is created)
    eng.update_B()
    out = {"B": eng.B.clone()}
    for k, (d, reg) in enumerate(zip(st.regs[1], eng.regs[1])):
        if d["kind"] == "parafac2":
            out[f"P{k}"], out[f"D{k}"] = reg.aux.clone(), reg.aux2.clone()
        else:
            out[f"aux{k}"] = reg.aux.clone()
        out[f"dual{k}"] = reg.dual.clone()
    out["diag"] = eng.diagnostics().clone()
    torch.cuda.synchronize()
    variant = eng.kernel_variant(E.PROF_ROWS_CHAIN)
    eng.close()
    for s in SWITCHES:
        monkeypatch.delenv(s, raising=False)
    return variant, out


def _oracle_errors(st, got):
    """the device's B-phase `got` against ref.update_B() from the same state -> (errors, bars)"""
    from oracle import aoadmm_oracle as orc

    ref = copy.deepcopy(st)
    orc.POLAR_COND["max"] = 1.0
    ref.update_B()
    p_tol = max(TOL, 1e-8 * orc.POLAR_COND["max"])
    errs, bars = {"B": rel_err(to_np(got["B"]), ref.B)}, {}
    for k, d in enumerate(ref.regs[1]):
        if d["kind"] == "parafac2":
            P, D = to_np(got[f"P{k}"]), to_np(got[f"D{k}"])
            P_ref, D_ref = ref.aux[1][k]
            errs[f"PD{k}"] = rel_err(P @ D, P_ref @ D_ref)
            errs[f"D{k}"] = rel_err(D, D_ref)
            errs[f"P{k}"] = rel_err(P, P_ref)
            bars[f"P{k}"] = p_tol
        else:
            errs[f"aux{k}"] = rel_err(to_np(got[f"aux{k}"]), ref.aux[1][k])
        # duals are ~0 where a constraint is inactive: measured against max(||dual||, ||B||) (test_gpu_sweep.py::_dual_err)
        want = ref.dual[1][k]
        errs[f"dual{k}"] = np.linalg.norm(to_np(got[f"dual{k}"]) - want) / max(np.linalg.norm(want), np.linalg.norm(ref.B))
    return errs, {k: bars.get(k, TOL) for k in errs}


def _check_oracle(name, st, got):
    errs, bars = _oracle_errors(st, got)
    worst = max(errs, key=lambda k: errs[k] / bars[k])
    print(f"{name}: worst {worst} {errs[worst]:.2e} (bar {bars[worst]:.0e});", {k: f"{v:.1e}" for k, v in errs.items()})
    bad = {k: (v, bars[k]) for k, v in errs.items() if not (v < bars[k])}
    assert not bad, (name, bad)


def _check_bitwise(name, a, b):
    import torch

    assert a.keys() == b.keys()
    differ = {}
    for k in a:
        if not torch.equal(a[k], b[k]):
            d = (a[k].double() - b[k].double()).abs()
            differ[k] = (int((d > 0).sum()), float(d.max()))
    assert not differ, (name, "pipelined != un-pipelined (elements that differ, largest difference)", differ)


def _pipelined(variant, r64):
    assert PIPELINED in variant, variant
    assert ("<R64>" in variant) == r64, variant


# ---- (a) + (b): every case, default path ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(kec.ROWCHAIN_CASES))
def test_b_phase_vs_oracle(name, monkeypatch):
    st = kec.rowchain_state(name)
    variant, got = _device_b_phase(st, monkeypatch)
    _pipelined(variant, st.A.shape[1] <= 16)
    _check_oracle(name, st, got)


@pytest.mark.parametrize("name", sorted(kec.ROWCHAIN_CASES))
def test_pipelined_equals_unpipelined_bitwise(name, monkeypatch):
    st = kec.rowchain_state(name)
    variant, got = _device_b_phase(st, monkeypatch)
    _pipelined(variant, st.A.shape[1] <= 16)
    variant0, got0 = _device_b_phase(st, monkeypatch, ("MCL_NO_ROW_PREFETCH",))
    assert PIPELINED not in variant0 and "k_rows_chain" not in variant0, variant0
    _check_bitwise(name, got, got0)


@pytest.mark.parametrize("name", kec.ROWCHAIN_TRAJECTORY_CASES)
def test_two_outer_iterations_vs_oracle(name):
    """B -> C -> A twice through cmf_aoadmm: factors, ADMM variables, losses and the feasibility gaps of every iteration (those
    of mode 1 come from the diagnostics tiles of k_rows_chain_last)"""
    from tests.test_gpu_end_to_end import _compare, _run_both

    st = kec.rowchain_state(name)
    cmf, admm, diag, res = _run_both(st, 2, arithmetic="fast")
    errs = _compare(cmf, admm, diag, st, res, TOL, tol_rec=TOL)
    print(name, {k: f"{v:.1e}" for k, v in errs.items()})


# ---- (c) the other two paths through the pipelined kernels ---------------------------------------------------------------------
@pytest.mark.parametrize("name", kec.ROWCHAIN_NB1_CASES)
def test_fp32_nb1_forms(name, monkeypatch):
    """k_rows_chain_*<1, false, SIG>: the fp32 forms at rank <= 16.  A PARAFAC2 stack of rank <= 16 takes the fp64 row algebra
    (R64) by default: these nine kernels are reachable only with MCL_NO_ROWS64=1."""
    st = kec.rowchain_state(name)
    assert st.A.shape[1] <= 16
    variant, got = _device_b_phase(st, monkeypatch, ("MCL_NO_ROWS64",))
    _pipelined(variant, False)
    _check_oracle(name, st, got)
    variant0, got0 = _device_b_phase(st, monkeypatch, ("MCL_NO_ROWS64", "MCL_NO_ROW_PREFETCH"))
    assert PIPELINED not in variant0 and "<R64>" not in variant0, variant0
    _check_bitwise(name, got, got0)


@pytest.mark.parametrize("name", sorted(kec.ROWCHAIN_NO_PASS_CHAIN_CASES))
def test_first_and_last_every_inner_iteration(name, monkeypatch):
    """MCL_NO_PASS_CHAIN=1: k_rows_chain_first -> k_rows_chain_last in every inner iteration, the last pass with want_diag = 0 in
    all but the final one"""
    st = kec.rowchain_state(name)
    st.inner = kec.ROWCHAIN_NO_PASS_CHAIN_CASES[name]
    assert st.inner >= 3
    variant, got = _device_b_phase(st, monkeypatch, ("MCL_NO_PASS_CHAIN",))
    _pipelined(variant, st.A.shape[1] <= 16)
    _check_oracle(name, st, got)
    variant0, got0 = _device_b_phase(st, monkeypatch, ("MCL_NO_PASS_CHAIN", "MCL_NO_ROW_PREFETCH"))
    assert PIPELINED not in variant0, variant0
    _check_bitwise(name, got, got0)


# ---- (d) stacks and shapes without a pipelined instantiation -------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(kec.ROWCHAIN_OTHER_CASES))
def test_stacks_without_a_chain_instantiation_take_other_kernels(name, monkeypatch):
    st = kec.rowchain_state(name)
    variant, got = _device_b_phase(st, monkeypatch)
    assert PIPELINED not in variant, (name, variant)
    _check_oracle(name, st, got)
