"""-m gpu: what the context caches between entry points (X C, C^T C, the fragment image of C, the sweep's partials, the
A-phase tables, the next B-phase's systems, the diagnostics tables) and when it recomputes it.

Every case plays a SCRIPT - a sequence of entry points - on a HipEngine and on the fp64 checker engine built from the same
oracle state, and pins two things:
  (a) the factors, every ADMM variable and every diagnostics vector the script asked for against the checker (1e-5), and
  (b) the launches per profile slot after the script: the observable record of what was recomputed and what was served from
      the cache.  The expected vectors are literals, read off the library before the validity flags were gathered into
      csrc/byproducts.h; a by-product invalidated too eagerly shows as a launch more, one kept too long as a launch less (and,
      with luck, a wrong number in (a)).
Shape of tests/test_gpu_cabi_contract.py: I = 5, rows 70 / 33 / 128 / 65 / 90 (two 64-row tile edges, a partial last tile),
K = 48, rank 6.  Both arithmetic modes (the kernel_paths fixture): by default a problem of this size runs in the exact-products
mode; with it forced off the one-pass sweep and the two-pass contractions run."""
import ctypes

import numpy as np
import pytest

from matcouply_amd import _engine as E
from tests.helpers import engine_from_oracle_state, rel_err, to_np

pytestmark = pytest.mark.gpu

NN = {"kind": "nn"}
L1 = {"kind": "l1", "reg_strength": 0.05, "non_negativity": True}
PLAIN = [[NN], [NN], [L1]]
PF2 = [[NN], [{"kind": "parafac2"}, {"kind": "l2ball", "norm_bound": 1.0}], [NN]]

ROUND_PF2 = ["B_begin", "B_factor", "B_solve", ("B_prox_local", 0), ("B_prox_finish", 0), ("B_prox_local", 1), ("B_prox_finish", 1)]

# name: (penalties, script, keywords of the oracle state).  "update_C" is update_C_local + update_C_finish; the entries in
# capitals exist on the HIP engine only (they change nothing the checker knows of).  The step scripts of modes 0 and 2 make the
# solves of a host that evaluates the proxes itself and leave the ADMM variables alone, on both engines; mode 0 is stepped
# under a constant feasibility penalty, where mcl_A_begin assembles the per-matrix systems mcl_A_factor needs.
# deferred_across_two_sweeps runs two inner iterations per phase: two B-phases in a row are then 4 consecutive inner iterations
# on fixed A and C, fewer than the 5 of one ordinary phase.  With 5 each they are 10, the non-negativity constraint is all but
# met, and its dual variable - B - (Z - U), a difference of nearly equal numbers - is small against the fp32 rounding of its
# terms (measured on the library this file was written against: relative error 6.1e-5 of that dual, 9e-7 of B itself, the
# deferred vector right to 2e-8).  A relative bound on such a dual measures the script's conditioning, not the cache.
SCRIPTS = {
    "iterate2_diag_twice": (PLAIN, [("iterate", 2), "diagnostics", "LAUNCHES", "diagnostics"], {}),
    "A_then_B": (PLAIN, ["update_A", "update_B"], {}),
    "A_set_options_B": (PLAIN, ["update_A", "SET_OPTIONS", "update_B"], {}),
    "C_then_A": (PLAIN, ["update_C", "update_A"], {}),
    "C_set_factors_A": (PLAIN, ["update_C", "SET_FACTORS", "update_A"], {}),
    "step_B_round_C_A": (PF2, ROUND_PF2 + ["update_C", "update_A"], {}),
    "step_C_then_B": (PLAIN, ["update_C_local", "C_begin", "C_solve", "C_end", "update_B"], {}),
    "step_A_then_B": (PLAIN, ["A_begin", "A_factor", "A_solve", "A_end", "update_B"], dict(constant_A=True)),
    "deferred_across_one_sweep": (PLAIN, [("iterate", 1), "diagnostics_deferred", "update_B", "update_C", "update_A"], {}),
    "deferred_across_two_sweeps": (PLAIN, [("iterate", 1), "diagnostics_deferred", "update_B", "update_B", "update_C", "update_A"],
                                   dict(inner_n_iter_max=2)),
    "stopped_run_then_iterate": (PLAIN, ["RUN_STOPS_AT_0", "LAUNCHES", ("iterate", 1)], {}),
    "A_set_workspace_B": (PLAIN, ["update_A", "SET_WORKSPACE", "update_B"], {}),
}

# launches per slot (XC, XT, ROWS_FUSED, SWEEP, REDUCE, C_FINISH, A_FINISH, ROWS_CHAIN, UNIMODAL, PF2, DIAG, OTHER) after the
# script, less those at its LAUNCHES mark if it has one (iterate2_diag_twice: the second diagnostics call alone;
# stopped_run_then_iterate: the iteration after the run - how many iterations the host had enqueued when the device stopped is
# not determined, that the by-products are forgotten afterwards is)
EXPECTED = {
    ("iterate2_diag_twice", "default"): (0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0),
    ("A_then_B", "default"): (1, 0, 1, 0, 0, 0, 1, 0, 0, 0, 0, 2),
    ("A_set_options_B", "default"): (1, 0, 1, 0, 0, 0, 1, 0, 0, 0, 0, 3),
    ("C_then_A", "default"): (1, 1, 0, 0, 0, 1, 1, 0, 0, 0, 0, 2),
    ("C_set_factors_A", "default"): (1, 1, 0, 0, 0, 1, 1, 0, 0, 0, 0, 2),
    ("step_B_round_C_A", "default"): (2, 1, 0, 0, 0, 1, 1, 2, 0, 1, 0, 6),
    ("step_C_then_B", "default"): (1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 3),
    ("step_A_then_B", "default"): (1, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 5),
    ("stopped_run_then_iterate", "default"): (2, 1, 1, 0, 0, 1, 1, 0, 0, 0, 0, 4),
    ("iterate2_diag_twice", "fast-kernels"): (0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0),
    ("A_then_B", "fast-kernels"): (1, 0, 0, 1, 0, 0, 1, 0, 0, 0, 0, 3),
    ("A_set_options_B", "fast-kernels"): (1, 0, 0, 1, 0, 0, 1, 0, 0, 0, 0, 4),
    ("C_then_A", "fast-kernels"): (1, 1, 0, 0, 1, 1, 1, 0, 0, 0, 0, 1),
    ("C_set_factors_A", "fast-kernels"): (1, 1, 0, 0, 1, 1, 1, 0, 0, 0, 0, 3),
    ("step_B_round_C_A", "fast-kernels"): (2, 1, 0, 0, 1, 1, 1, 2, 0, 1, 0, 6),
    ("step_C_then_B", "fast-kernels"): (0, 1, 0, 1, 1, 0, 0, 0, 0, 0, 0, 4),
    ("step_A_then_B", "fast-kernels"): (1, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 6),
    ("stopped_run_then_iterate", "fast-kernels"): (0, 0, 0, 1, 1, 1, 1, 0, 0, 0, 0, 3),
    ("deferred_across_one_sweep", "fast-kernels"): (0, 0, 0, 2, 2, 2, 2, 0, 0, 0, 1, 4),
    ("deferred_across_two_sweeps", "fast-kernels"): (0, 0, 0, 3, 2, 2, 2, 0, 0, 0, 1, 5),
    # The one script that library got wrong: it kept "the next B-phase's systems are built" across mcl_set_workspace, so the
    # B solve read the zeroed rhoB / LinvB of the new buffer (B = 0, relative error 1.0) with (2, .., 3) and (1, .., 5)
    # launches.  Right is one launch more in OTHER: the B systems, built again like X C and C^T C.
    ("A_set_workspace_B", "default"): (2, 0, 1, 0, 0, 0, 1, 0, 0, 0, 0, 4),
    ("A_set_workspace_B", "fast-kernels"): (1, 0, 0, 1, 0, 0, 1, 0, 0, 0, 0, 6),
}


def _state(regs, seed=3, **kw):
    from oracle import aoadmm_oracle as orc

    J = np.array([70, 33, 128, 65, 90])
    X, row_ptr = orc.synthetic_problem(len(J), J, 48, 6, seed=seed, dtype=np.float64)
    X = X.astype(np.float32).astype(np.float64)
    return orc.random_state_for(X, row_ptr, 6, regs, seed=seed + 1, **kw)


def _checker(st):
    """the fp64 checker engine (tests/oracle_engine.py) on copies of the oracle state"""
    import torch
    from tests.oracle_engine import OracleEngine

    t = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float64)
    regs = []
    for m in range(3):
        regs.append([])
        for d, z, u in zip(st.regs[m], st.aux[m], st.dual[m]):
            kind = E.KIND[d["kind"]]
            if d["kind"] == "parafac2":
                regs[m].append(E.NativeReg(kind, t(z[0]), t(u), aux2=t(z[1])))
            else:
                regs[m].append(E.NativeReg(kind, t(z), t(u), non_negativity=d.get("non_negativity", False),
                                           p0=d.get("reg_strength", d.get("norm_bound", 0.0))))
    return OracleEngine(t(st.X), st.row_ptr, st.A.shape[1], t(st.A), t(st.B), t(st.C), regs, l2_penalty=st.l2,
                        inner_n_iter_max=st.inner, feasibility_penalty_scale=st.scale, constant_A=st.constant_A,
                        constant_B=st.constant_B)


def _launches(eng):
    return np.array([eng.profile_launches(s) for s in range(E.PROF_SLOTS)], dtype=np.int64)


def _engine_only(eng, op, keep):
    if op == "SET_OPTIONS":  # unchanged values
        eng._check(eng.lib.mcl_set_options(eng._h, ctypes.byref(eng._opt)))
    elif op == "SET_FACTORS":  # the same pointers
        eng._check(eng.lib.mcl_set_factors(eng._h, eng.A.data_ptr(), eng.B.data_ptr(), eng.C.data_ptr()))
    elif op == "SET_WORKSPACE":  # a second buffer; the first one stays allocated
        import torch

        nbytes = eng.lib.mcl_workspace_bytes(eng._h)
        ws2 = torch.empty(int(nbytes) + 256, dtype=torch.uint8, device=eng.device)
        off = (-ws2.data_ptr()) % 256
        eng._check(eng.lib.mcl_set_workspace(eng._h, ws2.data_ptr() + off, nbytes))
        keep.append(eng.workspace)
        eng.workspace, eng._ws_off = ws2, off


def play(name):
    """-> (launch vector, [(what, HIP engine's value, checker's value)])"""
    import torch

    regs, script, kw = SCRIPTS[name]
    st = _state(regs, **kw)
    eng, ora = engine_from_oracle_state(st), _checker(st)
    eng.profile_enable(8, stride=1 << 20)  # counts every launch, times (nearly) none
    mark, keep, vectors = 0, [], []
    for op in script:
        op, args = (op, ()) if isinstance(op, str) else (op[0], op[1:])
        if op == "LAUNCHES":
            mark = _launches(eng)
        elif op == "RUN_STOPS_AT_0":  # a rule that any loss satisfies: the device stops after the first iteration
            kw = dict(tol=10.0, absolute_tol=0.0, feasibility_tol=float("inf"), initial_loss=1.0,
                      penalty_weight=[[0.0], [0.0], [0.0]], evaluate_loss_always=True)
            n_e, code_e = eng.run(4, **kw)[:2]
            n_o, code_o = ora.run(4, **kw)[:2]
            assert (n_e, code_e) == (n_o, code_o) == (1, E.STOP_RELATIVE)
        elif op.isupper():
            _engine_only(eng, op, keep)
        elif op == "update_C":
            for e in (eng, ora):
                e.update_C_local()
                e.update_C_finish()
        elif op in ("diagnostics", "diagnostics_deferred"):
            out = torch.full((E.DIAG_LEN,), float("nan"), dtype=torch.float64, device=eng.device)
            getattr(eng, op)(out=out)
            vectors.append((f"{op} #{len(vectors)}", out, ora.diagnostics().numpy().copy()))
        else:
            getattr(eng, op)(*args)
            getattr(ora, op)(*args)
    eng.B_end()  # a deferred row pass / diagnostics reduction of the script's last call is issued (launches: counted)
    launches = _launches(eng) - mark
    torch.cuda.synchronize()
    got = [(w, to_np(a), b) for w, a, b in vectors]
    got += [("A", to_np(eng.A), ora.A.numpy()), ("B", to_np(eng.B), ora.B.numpy()), ("C", to_np(eng.C), ora.C.numpy())]
    for m in range(3):
        for k, (re_, ro) in enumerate(zip(eng.regs[m], ora.regs[m])):
            got.append((f"aux[{m}][{k}]", to_np(re_.aux), ro.aux.numpy()))
            got.append((f"dual[{m}][{k}]", to_np(re_.dual), ro.dual.numpy()))
            if re_.aux2 is not None:
                got.append((f"aux2[{m}][{k}]", to_np(re_.aux2), ro.aux2.numpy()))
    got.append(("final diagnostics", to_np(eng.diagnostics()), ora.diagnostics().numpy()))
    eng.close()
    return launches, got


def _check(name, path):
    launches, got = play(name)
    print(f"\nLAUNCHES {name!r} {path!r} {tuple(int(v) for v in launches)}")
    for what, a, b in got:
        err = rel_err(a, b)
        print(f"  {what}: {err:.2e}")
        assert np.isfinite(a).all() and err < 1e-5, (name, what, err)
    assert tuple(int(v) for v in launches) == EXPECTED[name, path], (name, path, tuple(int(v) for v in launches))


@pytest.mark.parametrize("name", [n for n in SCRIPTS if not n.startswith("deferred_")])
def test_script(name, kernel_paths):
    _check(name, kernel_paths)


@pytest.mark.parametrize("name", [n for n in SCRIPTS if n.startswith("deferred_")])
def test_deferred_vector_across_sweeps(name, fast_kernels):
    """the deferred reduction rides on the C-phase reduction behind ONE sweep; a second sweep would overwrite the table it
    recorded, so it is issued on its own first - either way the vector describes the iterate at the time of the call"""
    _check(name, "fast-kernels")


def test_what_the_cache_saves():
    """the pinned vectors say what the scripts are there to say"""
    other, diag = E.PROF_OTHER, E.PROF_DIAG
    for path in ("default", "fast-kernels"):
        second = np.array(EXPECTED["iterate2_diag_twice", path])
        assert second[diag] == 1 and second.sum() == 1                      # the second diagnostics call: its reduction only
        kept, rebuilt = np.array(EXPECTED["A_then_B", path]), np.array(EXPECTED["A_set_options_B", path])
        assert (rebuilt - kept).sum() == 1 and (rebuilt - kept)[other] == 1  # the B systems, and only they, are built again
        moved, stayed = np.array(EXPECTED["A_set_workspace_B", path]), np.array(EXPECTED["A_then_B", path])
        # a new workspace holds nothing: C^T C, the B systems and X C (the sweep: the fragment image of C) are made again
        assert (moved - stayed).sum() == 3 and (moved - stayed)[E.PROF_XC] == (1 if path == "default" else 0)
    # mcl_set_factors behind a C-phase: X C falls with C anyway; the fast finish had left C^T C and the fragment image (two
    # launches in OTHER), the fp64 finish of the exact-products mode leaves neither (nothing to lose)
    extra = {p: np.array(EXPECTED["C_set_factors_A", p]) - np.array(EXPECTED["C_then_A", p]) for p in ("default", "fast-kernels")}
    assert extra["default"].sum() == 0 and extra["fast-kernels"][other] == 2 and extra["fast-kernels"].sum() == 2
