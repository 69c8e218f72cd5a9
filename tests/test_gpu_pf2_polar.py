"""-m gpu: the PARAFAC2 polar-factor kernels alone against the fp64 references of tests/polar_cases.py (checked on the CPU by
tests/test_polar_cases_host.py), slab by slab on designed spectra, at every rank bucket and route of csrc/pf2polar.hip.

(a) test_kernels_alone*, test_clamped_waves, test_stale_estimate, test_qr_not_launched: mode 1 through the step API without a
    solve (mcl_B_begin, mcl_B_factor, mcl_B_prox_local): the stack is not fused, so the call runs exactly k_pf2_gram<NB>,
    k_pf2_algebra_ns | k_pf2_algebra | k_pf2_polar_qr, k_pf2_apply and k_pf2_sum; mcl_B_prox_finish then runs k_pf2_delta and
    k_rows_pf2_dual.  aux, dual and aux2 live in sentinel buffers (rank "16u": one float into the buffer, the non-VEC row kernels).
      Gram      |S_i - Y_i^T Y_i| <= J_i 2^-52 |Y_i|^T |Y_i| elementwise (the products are exact in fp64, only the sums round)
      status    negative for a designed Newton-Schulz slab, exactly 2 for a QR slab where the QR kernel is launched, nothing
                where the encoding is ambiguous (0: Jacobi, or a Newton-Schulz run of no step)
      P_i       relative Frobenius error <= max(8 e32_i, 8 eG_i, 8 x 2^-24): e32 the error of fp32(Y_i) @ fp32(T_i) in float32,
                eG that of the Gram route in fp64 (only for the slabs a Gram route handles), both emulated on the CPU from the
                reference alone.  8: the device sums in another order, and Newton-Schulz stops at ||I - Z Y|| < 1e-8 at worst.
      Delta     |got - want| <= 4 x 2^-24 max(1, max |want|) + 8 x (the reference's Gram-route Delta - its SVD Delta)
      dual      1e-6 of max(1, max |Y| of the slab column) against B - (P Delta - U) of the values read back
    B must come back bit-identical, Delta unchanged by the local step, and nothing may be written outside the buffers.

(b) test_fp64_state: one inner iteration of a whole B-phase in the exact-products mode - k_wide_gram, mcl_launch_pf2_jacobi_wide,
    k_wide_pf2_apply, k_wide_pf2_delta, k_wide_pf2_dual (csrc/wide.hip).  With F1 the B read back: P_i = polar((F1_i + U0_i) Delta0^T),
    Delta_new = the weighted mean of P_i^T Y_i, dual = U0 + F1 - P Delta_new.  The test sees F1 rounded to fp32 where the kernel
    used fp64; the polar factor of a full-rank matrix is Lipschitz, ||dP||_F <= 2 ||dA||_F / (sigma_r + sigma_r-1) (Li 1995):
        ||P_i - want||_F <= 2 (2 x 2^-24 ||F1_i||_F ||Delta0||_2 / (sigma_r + sigma_r-1) + 2^-24 ||P_i||_F).
    A slab with J_i < r is compared on the projection P_i P_i^T A_i (d(P P^T A) = dP P^T A + P dP^T A: twice the bound with
    sigma_k for sigma_r, times ||A_i||_2).

Every test prints its worst error over its bar per route (DESIGN.md records them)."""
import os

import numpy as np
import pytest

from tests import polar_cases as pc
from tests.helpers import padded as _padded, untouched_outside as _untouched_outside

pytestmark = pytest.mark.gpu

HALF_ULP, BAR_DUAL = pc.HALF_ULP, 1e-6
SWITCHES = {"default": {}, "jacobi": {"MCL_PF2_JACOBI": "1"}, "plain": {"MCL_NS_PLAIN": "1"}}


def _f32(a, dev):
    import torch

    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float32, device=dev)


def _np64(t):
    return t.detach().cpu().numpy().astype(np.float64)


class _Switches:
    """set the MCL_* switches of a variant before the engine is created (contexts read them then), restore them afterwards"""

    def __init__(self, variant):
        self.want = dict({"MCL_PF2_JACOBI": None, "MCL_NS_PLAIN": None}, **SWITCHES[variant])

    def __enter__(self):
        self.saved = {k: os.environ.get(k) for k in self.want}
        for k, v in self.want.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)

    def __exit__(self, *exc):
        for k, v in self.saved.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


_REFERENCES = {}


def _reference(key, p, rho):
    """one fp64 reference (and its emulated errors) per (problem, rho)"""
    k = (key, rho.tobytes())
    if k not in _REFERENCES:
        ref = pc.reference(p["B"], p["U"], p["Delta"], p["row_ptr"], rho)
        _REFERENCES[k] = (ref, pc.emulated_error(ref, p["Delta"], p["row_ptr"]))
    return _REFERENCES[k]


class _Alone:
    """mode-1 engine on problem p with the single PARAFAC2 penalty; aux (zeros), dual (U) and aux2 (Delta) in padded buffers"""

    def __init__(self, p, rank, variant="default"):
        import torch

        from matcouply_amd._engine import KIND, HipEngine, NativeReg

        self.p, self.rank, self.r = p, rank, pc.rank_of(rank)
        dev = torch.device("cuda", 0)
        N, un = int(p["row_ptr"][-1]), rank == "16u"
        self.aux_buf, self.aux = _padded(np.zeros((N, self.r), dtype=np.float32), un, dev)
        self.dual_buf, self.dual = _padded(p["U"], un, dev)
        self.delta_buf, self.delta = _padded(p["Delta"], un, dev)
        reg = NativeReg(KIND["parafac2"], self.aux, self.dual, aux2=self.delta)
        with _Switches(variant):
            self.eng = HipEngine(_f32(p["X"], dev), p["row_ptr"], self.r, _f32(p["A"], dev), _f32(p["B"], dev), _f32(p["C"], dev),
                                 [[], [reg], []])
        try:
            self.eng.B_begin()
            self.eng.B_factor()
            torch.cuda.synchronize()
            self.rho = _np64(self.eng.rho(1))
            assert np.all(np.abs(self.rho - p["rho"]) <= 1e-5 * p["rho"]), (self.rho, p["rho"])
        except BaseException:
            self.eng.close()
            raise

    def local(self):
        """mcl_B_prox_local -> (P, status, S) read back"""
        import torch

        from matcouply_amd import _engine as E

        eng, I, r = self.eng, len(self.p["row_ptr"]) - 1, self.r
        eng.B_prox_local(0)
        torch.cuda.synchronize()
        status = eng.internal(E.BUF_PF2_STATUS).view(torch.int32).cpu().numpy()[:I].copy()
        S = eng.internal(E.BUF_PF2_GRAM).view(torch.float64).cpu().numpy()[: I * r * r].reshape(I, r, r).copy()
        return _np64(self.aux), status, S

    def finish(self):
        import torch

        self.eng.B_prox_finish(0)
        torch.cuda.synchronize()
        return _np64(self.delta), _np64(self.dual)

    def untouched(self):
        return (_untouched_outside(self.aux_buf, self.aux) and _untouched_outside(self.dual_buf, self.dual)
                and _untouched_outside(self.delta_buf, self.delta))

    def close(self):
        self.eng.close()


def _slab_errors(p, ref, got):
    return np.array([np.linalg.norm(got[s:e] - ref["P"][s:e]) / max(np.linalg.norm(ref["P"][s:e]), 1e-300)
                     for s, e in zip(p["row_ptr"][:-1], p["row_ptr"][1:])])


def _check_P(label, p, rank, variant, ref, emu, got, status, qr_launched=True):
    """every compared slab within its bar, the status of the unambiguous routes; prints the worst error / bar per route"""
    slabs, r = p["slabs"], pc.rank_of(rank)
    routes = [pc.route(rank, s, variant) for s in slabs]
    gram = np.array([rt in ("ns", "jacobi") for rt in routes])
    bar = pc.p_bar(emu, gram)
    err = _slab_errors(p, ref, got)
    compared = pc.compared(rank, slabs, variant, qr_launched)
    assert np.all(np.isfinite(got))
    worst = {}
    for i, rt in enumerate(routes):
        s, e = p["row_ptr"][i], p["row_ptr"][i + 1]
        if rt == "zero":
            assert not got[s:e].any(), (label, i, "P of an all-zero slab")
            continue
        if not compared[i]:
            continue
        worst[rt] = max(worst.get(rt, 0.0), err[i] / bar[i])
    rig = float(np.max(np.where(compared & (emu["rigorous"] > 0), err / np.maximum(emu["rigorous"], 1e-300), 0.0)))
    print(f"{label} rank {rank} {variant}: worst P error / bar " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(worst.items()))
          + f"; / rigorous componentwise bound {rig:.4f}")
    for i, rt in enumerate(routes):
        if compared[i] and rt != "zero":
            assert err[i] <= bar[i], (label, rank, variant, i, slabs[i], rt, err[i], bar[i], int(status[i]))
        if rt == "ns":
            assert status[i] < 0 or (r == 1 and status[i] == 0), (label, rank, variant, i, slabs[i], int(status[i]))
    return gram, compared


def _not_flagged(p, rank, variant, status):
    """the designed QR slabs (cond >= 1e6 or exactly rank-deficient, J_i >= r) whose status is not 2"""
    return [(i, s, int(status[i])) for i, s in enumerate(p["slabs"]) if pc.route(rank, s, variant) == "qr" and status[i] != 2]


def _check_gram(label, p, ref, S):
    for i, (s, e) in enumerate(zip(p["row_ptr"][:-1], p["row_ptr"][1:])):
        Ya = np.abs(ref["Y"][s:e])
        bound = (e - s) * 2.0 ** -52 * (Ya.T @ Ya)
        assert np.all(np.abs(S[i] - ref["S"][i]) <= bound), (label, i, float(np.abs(S[i] - ref["S"][i]).max()))


def _check_finish(label, p, ref, emu, rho, gram, B0, U0, P_got, D_got, dual_got, check_delta=True):
    assert np.all(np.isfinite(D_got)) and np.all(np.isfinite(dual_got))
    if check_delta:
        bar = pc.delta_bar(ref, emu, rho, p["row_ptr"], gram)
        worst = float(np.abs(D_got - ref["Delta_new"]).max()) / bar
    else:
        worst = float("nan")
    ref_dual = B0 - (P_got @ D_got - U0)  # U <- F - (P Delta - U)   (k_rows_pf2_dual)
    scale = np.concatenate([np.broadcast_to(np.maximum(np.abs(ref["Y"][s:e]).max(axis=0), 1.0), (e - s, ref["Y"].shape[1]))
                            for s, e in zip(p["row_ptr"][:-1], p["row_ptr"][1:])])
    worst_dual = float((np.abs(dual_got - ref_dual) / (BAR_DUAL * scale)).max())
    print(f"{label}: worst Delta error / bar {worst:.3f}, dual {worst_dual:.3f}")
    assert not check_delta or worst <= 1.0, (label, "Delta", worst)
    assert worst_dual <= 1.0, (label, "dual", worst_dual)


_SEEN = {}  # (problem, variant) -> (arithmetic path, P, Delta, dual): both paths must leave the same bits for I <= 64
_STATUS = {}  # (problem, rank, variant, arithmetic path) -> status of the run (test_qr_slabs_are_flagged)


def _run_alone(key, p, rank, variant, kernel_paths, label):
    import torch

    a = _Alone(p, rank, variant)
    try:
        ref, emu = _reference(key, p, a.rho)
        B0, U0, D0 = a.eng.B.clone(), a.dual.clone(), a.delta.clone()
        assert np.array_equal(_np64(B0) + _np64(U0), ref["Y"])
        P_got, status, S = a.local()
        _check_gram(label, p, ref, S)
        gram, _ = _check_P(label, p, rank, variant, ref, emu, P_got, status)
        _STATUS[(key, rank, variant, kernel_paths)] = status
        assert torch.equal(a.eng.B, B0) and torch.equal(a.dual, U0) and torch.equal(a.delta, D0), "the local step changed B, U or Delta"
        assert a.untouched(), "a store outside aux / dual / aux2"
        D_got, dual_got = a.finish()
        _check_finish(f"{label} rank {rank} {variant}", p, ref, emu, a.rho, gram, _np64(B0), _np64(U0), P_got, D_got, dual_got)
        assert torch.equal(a.eng.B, B0) and np.array_equal(_np64(a.aux), P_got), "the finish step changed B or P"
        assert a.untouched(), "a store outside aux / dual / aux2"
        seen = _SEEN.setdefault((key, rank, variant), (kernel_paths, P_got, D_got, dual_got))
        if seen[0] != kernel_paths:
            assert all(np.array_equal(x, y) for x, y in zip(seen[1:], (P_got, D_got, dual_got))), "the arithmetic paths differ"
        return P_got, D_got, dual_got, status
    finally:
        a.close()


@pytest.mark.parametrize("rank", pc.RANKS)
def test_kernels_alone(rank, kernel_paths):
    """the main engine of every rank: J in {1, r - 1, r, r + 1, 15, 16, 17, 63, 64, 65, 130, 257} x cond in {1, 10, 1e3, 1e4},
    two QR slabs (1e6, 1e7).  Rank <= 16: k_pf2_gram<1>, k_pf2_algebra_ns<1> with its in-kernel Jacobi; 17, 32: <2> + k_pf2_algebra
    behind the status; 33, 45 (NB = 3 -> 4) and 46 .. 64: k_pf2_gram<4>, Jacobi for every slab (odd ranks: the bye; 46+ / 52+:
    the dynamic-LDS attribute of k_pf2_algebra / k_pf2_polar_qr)"""
    _run_alone(("main", pc.rank_of(rank)), pc.main_problem(rank), rank, "default", kernel_paths, "main")


@pytest.mark.parametrize("rank", pc.JACOBI_RANKS)
def test_kernels_alone_jacobi_switch(rank, kernel_paths):
    """MCL_PF2_JACOBI=1: Jacobi for every slab on the data Newton-Schulz has at these ranks"""
    _run_alone(("main", pc.rank_of(rank)), pc.main_problem(rank), rank, "jacobi", kernel_paths, "main")


@pytest.mark.parametrize("rank", pc.PLAIN_RANKS)
def test_kernels_alone_plain_newton_schulz(rank, kernel_paths):
    """MCL_NS_PLAIN=1: the unscaled iteration (no carried estimate)"""
    _run_alone(("main", pc.rank_of(rank)), pc.main_problem(rank), rank, "plain", kernel_paths, "main")


@pytest.mark.parametrize("which", ["diag", "zero"])
@pytest.mark.parametrize("rank", pc.SPECIAL_RANKS)
def test_kernels_alone_deficient_and_zero_slabs(rank, which, kernel_paths):
    """diag: Delta a diagonal of powers of two and a slab with J >= r whose Y_i Delta^T is EXACTLY rank-deficient (two zero
    columns): flagged 2, the partial isometry from k_pf2_polar_qr - and a J = r - 1 slab of cond 1e6, the one slab whose kept
    rank the pseudo-inverse threshold of the Jacobi route decides (polar_cases.special_slabs).  zero: an all-zero slab - no reference; finite output, P_i = 0,
    its rho_i in the weight total of Delta, every other slab within its bar"""
    _run_alone((which, rank), pc.special_problem(rank, which), rank, "default", kernel_paths, which)


FLAG_CASES = ([("main", rank, "default") for rank in pc.RANKS if pc.rank_of(rank) > 1] + [("main", rank, "jacobi") for rank in pc.JACOBI_RANKS]
              + [("main", rank, "plain") for rank in pc.PLAIN_RANKS] + [("diag", rank, "default") for rank in pc.SPECIAL_RANKS])


@pytest.mark.parametrize("which,rank,variant", FLAG_CASES, ids=lambda v: str(v))
def test_qr_slabs_are_flagged(which, rank, variant, kernel_paths):
    """BUF_PF2_STATUS is exactly 2 for every designed QR slab (cond 1e6, 1e7 or exactly rank-deficient, J_i >= r) wherever
    k_pf2_polar_qr is launched - on the run of the test above where there was one (the P, Delta and dual of these slabs are held
    to their bars there, whatever the route).

    This check found a defect: Newton-Schulz "converges" by stagnation at its round-off floor on the cond-1e6 and cond-1e7 slabs
    (status -28 .. -33, -40 .. -46 with MCL_NS_PLAIN) and kept them on the Gram route at ranks 3, 16, 17, 32 and in the 65-slab
    rank-4 problem, which left Delta 7 to 30 times over its bar at ranks 3, 16 and 17; pf2_ill_conditioned (csrc/pf2polar.hip)
    now flags such a slab (2) for the QR kernel."""
    p = pc.main_problem(rank) if which == "main" else pc.special_problem(rank, which)
    key = ("main", pc.rank_of(rank)) if which == "main" else (which, rank)
    status = _STATUS.get((key, rank, variant, kernel_paths))
    if status is None:
        a = _Alone(p, rank, variant)
        try:
            _, status, _ = a.local()
        finally:
            a.close()
    missed = _not_flagged(p, rank, variant, status)
    print(f"{which} rank {rank} {variant}: status of the QR slabs "
          f"{[(s, int(status[i])) for i, s in enumerate(p['slabs']) if pc.route(rank, s, variant) == 'qr']}")
    assert not missed, missed


def test_qr_not_launched(kernel_paths):
    """rank 4, 65 slabs, one of cond 1e7: with the fast kernels the QR kernel is deliberately not launched (ink_qr of
    mcl_launch_pf2_polar) and that slab keeps its Gram-route factor - status 2, finite output, every other
    slab within its bar; the exact-products mode launches it and the slab is held to its bar like any other"""
    import torch

    from matcouply_amd import _engine as E

    p = pc.many_slabs_problem()
    launched = kernel_paths == "default"
    a = _Alone(p, 4)
    try:
        ref, emu = _reference(("many", 4), p, a.rho)
        B0, U0 = _np64(a.eng.B), _np64(a.dual)
        P_got, status, S = a.local()
        assert (a.eng.kernel_variant(E.VARIANT_EXACT_MODE) != "") == launched
        _check_gram("many", p, ref, S)
        gram, compared = _check_P("many", p, 4, "default", ref, emu, P_got, status, qr_launched=launched)
        assert int(np.sum(~compared)) == (0 if launched else 1)
        D_got, dual_got = a.finish()
        _check_finish(f"many rank 4 {kernel_paths}", p, ref, emu, a.rho, gram, B0, U0, P_got, D_got, dual_got, check_delta=launched)
        assert a.untouched() and torch.equal(a.eng.B, _f32(p["B"], a.eng.B.device))
        assert status[-1] == 2, ("the cond-1e7 slab", int(status[-1]))
    finally:
        a.close()


@pytest.mark.parametrize("last", ["ns", "short"])
@pytest.mark.parametrize("n_slabs", pc.CLAMP_I)
def test_clamped_waves(n_slabs, last, kernel_paths):
    """k_pf2_algebra_ns<1, .> runs four slabs per workgroup; at I % 4 != 0 the spare waves are clamped onto the last slab - once a
    Newton-Schulz slab, once a J < r slab for the in-kernel Jacobi.  Every slab within its bar, two runs bit-identical"""
    p = pc.clamp_problem(n_slabs, last)
    key = ("clamp", n_slabs, last)
    first = _run_alone(key, p, pc.CLAMP_RANK, "default", kernel_paths, f"clamp I={n_slabs} {last}")
    second = _run_alone(key, p, pc.CLAMP_RANK, "default", kernel_paths, f"clamp I={n_slabs} {last}")
    assert all(np.array_equal(x, y) for x, y in zip(first, second)), "two runs differ"


@pytest.mark.parametrize("rank", pc.STALE_RANKS)
def test_stale_estimate(rank, kernel_paths):
    """the starting estimate pf2_xmin carried from call to call: a call on a cond-1 problem leaves it at its largest, then B and
    the dual are overwritten in place with the cond-1e4 problem of the same shape - "a wrong estimate costs iterations, not
    convergence": status negative, P within the bar of a fresh engine on that data; a third call on unchanged data likewise"""
    import torch

    easy, hard = pc.stale_problems(rank)
    a = _Alone(easy, rank)
    try:
        ref_e, emu_e = _reference(("stale-easy", rank), easy, a.rho)
        P_got, status, _ = a.local()
        _check_P("stale (first call, cond 1)", easy, rank, "default", ref_e, emu_e, P_got, status)
        a.eng.B.copy_(_f32(hard["B"], a.eng.B.device))
        a.dual.copy_(_f32(hard["U"], a.eng.B.device))
        torch.cuda.synchronize()
        ref, emu = _reference(("stale-hard", rank), hard, a.rho)
        steps = []
        for call in ("stale estimate", "third call"):
            P_got, status, S = a.local()
            _check_gram("stale", hard, ref, S)
            _check_P(f"stale ({call}, cond 1e4)", hard, rank, "default", ref, emu, P_got, status)
            steps.append((-status).tolist())
        print(f"stale rank {rank}: Newton-Schulz steps with the stale estimate {steps[0]}, with its own {steps[1]}")
        assert a.untouched()
    finally:
        a.close()
    fresh = _Alone(hard, rank)
    try:
        P_fresh, status, _ = fresh.local()
        _check_P("stale (fresh engine, cond 1e4)", hard, rank, "default", ref, emu, P_fresh, status)
    finally:
        fresh.close()


# ---- (b) ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stack", ["pf2", "pf2+nn"])
@pytest.mark.parametrize("size,rank", pc.WIDE_CASES, ids=lambda v: str(v))
def test_fp64_state(size, rank, stack):
    """(b) of the module docstring"""
    import torch

    from matcouply_amd import _engine as E

    p = pc.wide_problem(size, rank)
    dev = torch.device("cuda", 0)
    row_ptr, N = p["row_ptr"], int(p["row_ptr"][-1])
    regs = [E.NativeReg(E.KIND["parafac2"], _f32(p["P0"], dev), _f32(p["dual0"], dev), aux2=_f32(p["Delta0"], dev))]
    dual_nn = -np.roll(p["dual0"], 1, axis=1)
    if stack == "pf2+nn":
        regs.append(E.NativeReg(E.KIND["nn"], _f32(np.maximum(p["B"], 0.0), dev), _f32(dual_nn, dev)))
    old = os.environ.pop("MCL_EXACT", None)
    try:
        eng = E.HipEngine(_f32(p["X"], dev), row_ptr, rank, _f32(p["A"], dev), _f32(p["B"], dev), _f32(p["C"], dev), [[], regs, []],
                          inner_n_iter_max=1)
    finally:
        if old is not None:
            os.environ["MCL_EXACT"] = old
    try:
        eng.update_B()
        torch.cuda.synchronize()
        assert eng.kernel_variant(E.VARIANT_EXACT_MODE) != ""
        assert eng.kernel_variant(E.PROF_ROWS_FUSED).startswith("k_wide_"), eng.kernel_variant(E.PROF_ROWS_FUSED)
        assert "on the fp64 state" in eng.kernel_variant(E.PROF_PF2), eng.kernel_variant(E.PROF_PF2)
        F1, rho = _np64(eng.B), _np64(eng.rho(1))
        P_got, D_got, dual_got = _np64(regs[0].aux), _np64(regs[0].aux2), _np64(regs[0].dual)
        assert np.all(np.isfinite(F1)) and np.all(rho > 0) and np.all(np.isfinite(P_got))
        U0, D0 = p["dual0"].astype(np.float64), p["Delta0"].astype(np.float64)
        ref = pc.reference(F1, U0, D0, row_ptr, rho)
        nD = np.linalg.norm(D0, 2)
        worst, worst_short, dbar = 0.0, 0.0, 0.0
        for i, (s, e) in enumerate(zip(row_ptr[:-1], row_ptr[1:])):
            sv, k = ref["sigma"][i], int(ref["kept"][i])
            assert k == min(e - s, rank), "a random slab lost rank"
            gap = sv[k - 1] + (sv[k - 2] if k > 1 else sv[k - 1])
            nF = np.linalg.norm(F1[s:e])
            bar = 2.0 * (2.0 * HALF_ULP * nF * nD / gap + HALF_ULP * np.linalg.norm(ref["P"][s:e]))
            if e - s >= rank:
                err = np.linalg.norm(P_got[s:e] - ref["P"][s:e])
                worst = max(worst, err / bar)
            else:
                A = ref["Y"][s:e] @ D0.T
                err = np.linalg.norm(P_got[s:e] @ (P_got[s:e].T @ A) - ref["P"][s:e] @ (ref["P"][s:e].T @ A))
                bar = 2.0 * sv[0] * bar
                worst_short = max(worst_short, err / bar)
            assert err <= bar, (size, rank, stack, i, int(e - s), err, bar, float(sv[0] / sv[k - 1]))
            # what the slab may add to Delta: dP^T Y + P^T dY, weighted
            dbar += rho[i] * (2.0 * (2.0 * HALF_ULP * nF * nD / gap) * np.linalg.norm(ref["Y"][s:e]) + HALF_ULP * nF)
        dbar = dbar / rho.sum() + 2.0 * HALF_ULP * max(1.0, float(np.abs(ref["Delta_new"]).max()))
        worst_delta = float(np.abs(D_got - ref["Delta_new"]).max()) / dbar
        ref_dual = U0 + F1 - P_got @ D_got
        scale = np.concatenate([np.broadcast_to(np.maximum(np.abs(ref["Y"][s:e]).max(axis=0), 1.0), (e - s, rank))
                                for s, e in zip(row_ptr[:-1], row_ptr[1:])])
        worst_dual = float((np.abs(dual_got - ref_dual) / (BAR_DUAL * scale)).max())
        print(f"fp64 state {size} rank {rank} {stack}: worst P error / bar {worst:.3f}, projection (J < r) {worst_short:.3f}, "
              f"Delta {worst_delta:.3f}, dual {worst_dual:.3f}")
        assert worst_delta <= 1.0 and worst_dual <= 1.0, (size, rank, stack, worst_delta, worst_dual)
        if stack == "pf2+nn":  # the second member of the stack: its own aux / dual, untouched by the PARAFAC2 addressing
            Ynn = F1 + dual_nn.astype(np.float64)
            Z = _np64(regs[1].aux)
            assert np.all(np.abs(Z - np.maximum(Ynn, 0.0)) <= 3.0 * HALF_ULP * np.maximum(1.0, np.abs(Ynn)))
            assert np.all(np.abs(_np64(regs[1].dual) - (dual_nn + F1 - Z)) <= BAR_DUAL * np.maximum(1.0, np.abs(Ynn)))
    finally:
        eng.close()
