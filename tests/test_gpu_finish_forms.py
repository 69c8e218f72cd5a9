"""The A-phase and C-phase finish kernels (csrc/afinish.h, csrc/admm.hip), one case per form, each pinning the form that
ran (kernel_variant) and holding its outputs to the oracle.

Two rounds B -> C -> A through the C ABI, as tests/test_gpu_sweep.py::test_one_iteration_phase_by_phase: the second round
consumes the next B-phase's systems the first A finish built.  After every round: A with its auxiliary and dual variables,
C, rho_A, the reconstruction error from the A by-products and the mode-0 / mode-2 gap columns of diagnostics() against the
oracle at the project's flat 1e-5 relative.

The engine starts from the fp32 rounding of the state the (fp64) oracle starts from, so a part of every measured error is the
oracle's own sensitivity to that rounding.  test_problems_are_stable_under_fp32_inputs (no GPU) bounds it by a quarter of the
bar for every problem below - three quarters stay for the kernels' arithmetic; a problem that misses it is too ill-conditioned
for a 1e-5 comparison and has to be replaced, not excused.
"""
import copy

import numpy as np
import pytest

from tests.helpers import rel_err

TOL = 1e-5
NN = {"kind": "nn"}
# A feasibility gap ||z - F|| only has entries where the constraint is ACTIVE (elsewhere z = F + u with u = 0 after one step,
# and the fp32 residue of that is noise against the oracle's fp64 zero), and it is a difference of fp32-stored values: where
# z sits on a bound b the entry is b - F, and the factor's 5e-7 shows in the gap divided by gap / ||F||.  Non-negativity or
# a box touch few entries of these factors (medians 0.45 and 0.5) and two rounds pull those onto the bound: gaps of 1e-3 of
# the factor, which no fp32 kernel holds to 1e-5.  A strong L1 penalty does better: every entry below its threshold has z = 0
# EXACTLY in both implementations, so the gap there is |F| itself.  The default penalties of modes 0 and 2 are therefore L1
# with thresholds reg / rho of a few tenths: rho_i = tr(Q_i) / 2 is about 4 r K for the median slab of 70 rows, rho_C about
# r N / 18.
def l1(strength):
    return {"kind": "l1", "reg_strength": float(strength)}


def L1A(r, K):
    return l1(1.2 * r * K)


def L1C(r, N):
    return l1(0.016 * r * N)


def _problem(J, K, r, switches, a_form, c_form, regs0="l1", regs2="l1", l2=(0.0, 0.0, 0.0)):
    """a case; regs0 / regs2: "l1" (the default above) or an explicit penalty list of the mode"""
    N = int(np.sum(J))
    regs0 = [L1A(r, K)] if regs0 == "l1" else [L1A(r, K) if d == "l1" else d for d in regs0]
    regs2 = [L1C(r, N)] if regs2 == "l1" else [L1C(r, N) if d == "l1" else d for d in regs2]
    return (J, K, r, [regs0, [NN], regs2], switches, a_form, c_form, l2)


# Where mode 0 is not the subject of a case (the C-finish cases; rank 17, whose 16-row slab has a singular B_i^T B_i) it carries
# two boxes that cannot both hold, around the median 0.45 of A: the row settles between them and BOTH gaps stay at 0.2 of the
# factor for as many rounds as one likes, every auxiliary entry sitting exactly on a bound.
TWO_BOXES_A = [{"kind": "box", "min_val": 0.55, "max_val": 2.0}, {"kind": "box", "min_val": -1.0, "max_val": 0.35}]


J5 = [70, 33, 257, 16, 130]   # five slabs: not a multiple of the four slabs per workgroup; one of exactly 16 rows
J5L = [70, 133, 257, 96, 130]  # no short slab: un-shifted (penalty-free) A systems need J_i well above the rank
TWO_PASS = {"MCL_NO_SWEEP": "1"}

# name: (J_i, K, rank, penalties per mode, MCL_* switches, A-finish form or None, prefix of the C-finish form or None)
A_CASES = {
    # the column kernel: ranks <= 4 and > 32, on the two-pass path
    "cols_r3": _problem(J5, 128, 3, TWO_PASS, "k_A_finish", None),
    "cols_r33": _problem(J5, 64, 33, TWO_PASS, "k_A_finish", None),
    # the row-split kernel, one wave per slab (two-pass path: the right-hand sides arrive assembled)
    "rows_r5": _problem(J5, 128, 5, TWO_PASS, "k_A_finish_rows", None),
    "rows_r16": _problem(J5, 128, 16, TWO_PASS, "k_A_finish_rows", None),
    "rows_r17": _problem(J5, 128, 17, TWO_PASS, "k_A_finish_rows", None, regs0=TWO_BOXES_A),
    # behind the sweep: one workgroup per slab, three waves stream the partials of M
    "wide1_r8": _problem(J5, 192, 8, {}, "k_A_finish_rows_wide<SPB=1>", None),
    "wide1_r16": _problem(J5, 256, 16, {}, "k_A_finish_rows_wide<SPB=1>", None),
    "wide1_r20": _problem(J5, 256, 20, {}, "k_A_finish_rows_wide<SPB=1>", None),
    # more than 512 slabs with one partial each: two slabs per workgroup, the odd slab out
    "wide2_r8_515_slabs": _problem([64] * 515, 64, 8, {}, "k_A_finish_rows_wide<SPB=2>", None),
    # the only way to the column kernel's instantiations for ranks 5..32
    "cols_forced_r16": _problem(J5, 256, 16, {"MCL_A_FINISH_COLS": "1"}, "k_A_finish", None),
    # n = 0 and n = 2 penalties in the shared inner loop, in both layouts: the same two problems, the column layout forced
    # (at rank 3 the un-shifted 3 x 3 systems of nearly collinear columns, and the 15 entries of A, leave no margin at 1e-5)
    "cols_forced_r8_none": _problem(J5L, 256, 8, {"MCL_A_FINISH_COLS": "1"}, "k_A_finish", None, regs0=[]),
    "rows_r8_none": _problem(J5L, 256, 8, {}, "k_A_finish_rows_wide<SPB=1>", None, regs0=[]),
    "cols_forced_r16_nn_l1": _problem(J5, 256, 16, {"MCL_A_FINISH_COLS": "1"}, "k_A_finish", None, regs0=[NN, "l1"]),
    "rows_r16_nn_l1": _problem(J5, 256, 16, {}, "k_A_finish_rows_wide<SPB=1>", None, regs0=[NN, "l1"]),
}
# the exact-products mode small problems take by default, forced so that neither the size threshold nor the environment decides
# (no fast_kernels): the fp64 inner loop of the finish, both layouts
EXACT = {"MCL_EXACT": "1"}
EXACT_CASES = {
    "exact_cols_r3": _problem(J5, 128, 3, EXACT, "k_A_finish", None, regs0=[NN, "l1"]),
    "exact_rows_r16": _problem(J5, 128, 16, EXACT, "k_A_finish_rows", None, regs0=[NN, "l1"]),
}
C_CASES = {}
for _n, _regs in {0: [], 1: "l1", 2: [NN, "l1"]}.items():
    _kw = dict(regs0=TWO_BOXES_A, regs2=_regs)
    # K = 130: three workgroups, the last one with 2 rows
    C_CASES[f"multi_k130_r12_n{_n}"] = _problem(J5, 130, 12, {}, None, f"k_C_finish_multi<NREG={_n}>", **_kw)
    C_CASES[f"fused_nomulti_k130_r12_n{_n}"] = _problem(J5, 130, 12, {"MCL_NO_MULTI_C": "1"}, None, f"k_C_finish_fused<NBR=1,NREG={_n}>", **_kw)
    C_CASES[f"fused_k36_r12_n{_n}"] = _problem(J5, 36, 12, {}, None, f"k_C_finish_fused<NBR=1,NREG={_n}>", **_kw)
    if _n <= 1:  # (two column blocks: instantiated for 0 and 1 penalties)
        # penalty-free at rank 20: the un-shifted 20 x 20 G multiplies the fp32 rounding of B by its condition number; the
        # small l2 term keeps the penalty-free fp64 solve (its system is l2-shifted only) and leaves it a margin
        C_CASES[f"fused_k130_r20_n{_n}"] = _problem(J5, 130, 20, {}, None, f"k_C_finish_fused<NBR=2,NREG={_n}>",
                                                    l2=(0.0, 0.0, 30.0 if _n == 0 else 0.0), **_kw)
FAST_CASES = {**A_CASES, **C_CASES}
ALL_CASES = {**FAST_CASES, **EXACT_CASES}


def _state(case):
    from oracle import aoadmm_oracle as orc

    J, K, r, regs = case[:4]
    J = np.array(J)
    X, row_ptr = orc.synthetic_problem(len(J), J, K, r, seed=1, dtype=np.float64)
    X = X.astype(np.float32).astype(np.float64)
    return orc.random_state_for(X, row_ptr, r, regs, seed=2, l2=case[7])


def _gap_sq(st, mode):
    from oracle.aoadmm_oracle import aux_as_packed

    F = (st.A, st.B, st.C)[mode]
    return [float(np.sum((aux_as_packed(d, z) - F) ** 2)) for d, z in zip(st.regs[mode], st.aux[mode])]


def _oracle_round(st):
    """one B -> C -> A round of the oracle; what the test compares"""
    st.update_B()
    st.update_C()
    st.update_A()
    out = {"A": st.A.copy(), "C": st.C.copy(), "rhoA": np.array(st.rho_A), "rec": np.array(st.rec_error_from_A_byproducts())}
    for k in range(len(st.regs[0])):
        out[f"auxA{k}"], out[f"dualA{k}"] = st.aux[0][k].copy(), st.dual[0][k].copy()
    for m in (0, 2):
        for k, g in enumerate(_gap_sq(st, m)):
            out[f"gap{m}_{k}"] = np.array(g)
    return out


def _errors(got, want):
    errs = {}
    for key, w in want.items():
        if key.startswith("dualA"):  # (a dual is a difference of fp32-stored values of the factor's size: measured against it)
            errs[key] = np.linalg.norm(got[key] - w) / max(np.linalg.norm(w), np.linalg.norm(want["A"]))
        else:
            errs[key] = rel_err(got[key], w)
    return errs


@pytest.mark.parametrize("name", sorted(ALL_CASES))
def test_problems_are_stable_under_fp32_inputs(name):
    """The oracle alone, on the CPU: the same two rounds from the fp64 draw and from its fp32 rounding (what the engine is
    handed) agree to a quarter of the bar in every compared quantity."""
    ref = _state(ALL_CASES[name])
    f32 = copy.deepcopy(ref)
    rnd = lambda a: a.astype(np.float32).astype(np.float64)
    f32.A, f32.B, f32.C = rnd(f32.A), rnd(f32.B), rnd(f32.C)
    for m in range(3):
        f32.aux[m] = [rnd(z) for z in f32.aux[m]]
        f32.dual[m] = [rnd(u) for u in f32.dual[m]]
    for it in range(2):
        errs = _errors(_oracle_round(f32), _oracle_round(ref))
        worst = max(errs, key=errs.get)
        print(f"{name} round {it}: worst {worst} {errs[worst]:.1e}")
        assert errs[worst] < TOL / 4, (name, it, {k: f"{v:.1e}" for k, v in errs.items() if not v < TOL / 4})


def _run_case(case, monkeypatch):
    import torch

    from matcouply_amd import _engine as E
    from tests.helpers import engine_from_oracle_state, to_np

    switches, a_form, c_form = case[4:7]
    for key, val in switches.items():
        monkeypatch.setenv(key, val)  # (contexts read the MCL_* switches when they are created)
    st = _state(case)
    ref = copy.deepcopy(st)
    eng = engine_from_oracle_state(st)
    try:
        for it in range(2):
            eng.update_B()
            eng.update_C_local()
            eng.update_C_finish()
            c_ran = eng.kernel_variant(E.PROF_C_FINISH)
            eng.update_A()
            a_ran = eng.kernel_variant(E.PROF_A_FINISH)
            torch.cuda.synchronize()
            if a_form is not None:
                assert a_ran == a_form, (it, a_ran)
            if c_form is not None:
                assert c_ran.startswith(c_form), (it, c_ran)
            want = _oracle_round(ref)
            d = eng.diagnostics().cpu().numpy()
            rec = np.sqrt(max(0.0, d[E.DIAG_X_SQ] - 2 * d[E.DIAG_INNER] + d[E.DIAG_MODEL_SQ]) / d[E.DIAG_X_SQ])
            got = {"A": to_np(eng.A), "C": to_np(eng.C), "rhoA": to_np(eng.rho(0)), "rec": np.array(rec)}
            for k in range(len(st.regs[0])):
                got[f"auxA{k}"], got[f"dualA{k}"] = to_np(eng.regs[0][k].aux), to_np(eng.regs[0][k].dual)
            for m in (0, 2):
                for k in range(len(st.regs[m])):
                    got[f"gap{m}_{k}"] = np.array(d[E.DIAG_REG + (m * E.MCL_MAX_REGS + k) * 2])
            errs = _errors(got, want)
            print(f"round {it} [{a_ran} | {c_ran}]:", {k: f"{v:.1e}" for k, v in errs.items()})
            bad = {k: v for k, v in errs.items() if not (v < TOL)}
            assert not bad, (it, bad)
    finally:
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(FAST_CASES))
def test_finish_form(name, fast_kernels, monkeypatch):
    _run_case(FAST_CASES[name], monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(EXACT_CASES))
def test_finish_form_exact_products(name, monkeypatch):
    """small enough for the exact-products mode: the fp64 (`wide_inner`) inner loop of the finish"""
    _run_case(EXACT_CASES[name], monkeypatch)
