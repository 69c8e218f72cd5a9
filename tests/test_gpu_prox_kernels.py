"""-m gpu: every native prox kernel alone against the fp64 references of tests/prox_cases.py (checked on the CPU by
tests/test_prox_cases_host.py), at the slab, rank and alignment edges of its tiling.

(a) test_kernel_alone_*: mode 1 through the step API without a solve (mcl_B_begin, mcl_B_factor, mcl_B_prox_local): the stack is not
    fused, so the call runs exactly k_rows_prox_rowsep (csrc/rows.hip) | k_slab_colsq + k_rows_l2ball | k_slab_tv + k_rows_dual |
    k_gl2_pass (both directions) | k_slab_simplex + k_rows_dual (csrc/slabprox.hip; k_rows_dual: rows.hip), on designed Y = B + U (exact in fp32 and fp64) at the
    feasibility penalties the device computed (eight decades over the eleven slabs).
    Bar on aux: |got - want| <= 2.4e-7 max(1, max |Y| of the slab column, threshold) - four half-units of fp32 (4 x 2^-24 =
    2.4e-7), the bar of tests/test_gpu_unimodal_kernels.py.  fp32 roundings between Y and the stored value, everything else
    being fp64 or exact:
        L2 ball        3: (float)sqrt(colsq), bound / fmaxf(nrm, bound), y * scale
        TV             3: (float)v, (float)(p1 / rho), the subtraction of the soft threshold - and the fp32 image of the strength
                          the fast kernels keep (RegSet::p0, half a unit of the threshold 2 alpha / rho)
        simplex, GL2   1: the rounding of an fp64 result
        row-separable  2: the fp32 threshold p0 / rho, one subtraction - and the fp32 image of p0 (L1) or of the box bounds
    `threshold` is the largest constant the prox adds to or compares with Y (2 alpha / rho and l1 / rho, reg / rho, the ball's
    bound, the box bounds): its rounding is half a unit of ITSELF, which at rho = 1e-4 is far above max |Y|.
    Bar on the dual: 1e-6 of the same scale against B - (Z - U) of the values read back.  B itself must be bit-identical, and
    nothing may be written behind row N of aux or dual (buffers three rows longer; rank "16u": one float into a larger buffer,
    4-byte aligned only, which takes the non-VEC row kernels at a rank divisible by 4).

(b) test_phase_postcondition: every form in every mode through ONE inner iteration of a whole phase (update_B, update_C_local +
    update_C_finish, update_A), under both arithmetic paths: by default the fp64 k_wide_* kernels of csrc/wide.hip and the double
    instantiations of k_gl2_pass / k_slab_simplex, with the fast kernels the generic loop on C and A (one slab of K or I rows) and
    the fused forms.  With F1 the factor read back: aux_k == prox_k(F1 + U_k0) at the phase's rho and dual_k == U_k0 + F1 - aux_k
    for every member k of the stack.  The test sees F1 rounded to fp32 where the wide kernels used the fp64 value (and the fast
    kernels that add in fp32 round the sum): |delta Y| <= 2^-24 |F1| elementwise, the prox is non-expansive in the 2-norm over its
    coupling set (n rows of a slab column; one element for the row-separable kinds), so
        |delta Z| <= (sqrt(n) + 2) 2^-24 max(1, max |Y| of that column, threshold)
    (+2: the output rounding and the threshold; `threshold` in the unit for the reason given under (a)).  Dual: 1e-6 as in (a).

Every test prints its worst observed error over its bar (DESIGN.md records them per kernel)."""
import numpy as np
import pytest

from tests import prox_cases as pc
from tests.helpers import padded as _padded, untouched_outside as _untouched_outside

pytestmark = pytest.mark.gpu

BAR_AUX, BAR_DUAL, HALF_ULP = 2.4e-7, 1e-6, 2.0 ** -24
FP32_SUM = ("tv", "l2ball", "nn", "box", "l1")  # kinds whose fast kernel forms Y = F + U in fp32 (simplex, GL2: in fp64)


def _f32(a, dev):
    import torch

    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float32, device=dev)


def _np64(t):
    return t.detach().cpu().numpy().astype(np.float64)


_REFERENCES = {}


def _reference(key, p, desc, rho):
    """one fp64 reference per (problem, parameters, rho) - the Python TV is the slowest part of this file"""
    k = (key, pc.desc_id(desc), rho.tobytes())
    if k not in _REFERENCES:
        _REFERENCES[k] = pc.reference(desc, p["Y"], p["row_ptr"], rho)
    return _REFERENCES[k]


def _engine_alone(p, rank, desc, dev):
    """mode-1 engine on problem p with the single penalty `desc`, aux (zeros) and dual (U) in padded buffers"""
    from matcouply_amd._engine import HipEngine
    from tests.helpers import native_regs

    r, N = pc.rank_of(rank), int(p["row_ptr"][-1])
    regs = native_regs([desc], [np.zeros((N, r))], [p["U"]], dev)
    aux_buf, aux = _padded(np.zeros((N, r), dtype=np.float32), rank == "16u", dev)
    dual_buf, dual = _padded(p["U"], rank == "16u", dev)
    regs[0].aux, regs[0].dual = aux, dual
    eng = HipEngine(_f32(p["X"], dev), p["row_ptr"], r, _f32(p["A"], dev), _f32(p["B"], dev), _f32(p["C"], dev), [[], regs, []])
    return eng, aux_buf, aux, dual_buf, dual


def _check_alone(p, key, rank, desc, label):
    import torch

    dev = torch.device("cuda", 0)
    eng, aux_buf, aux, dual_buf, dual = _engine_alone(p, rank, desc, dev)
    try:
        eng.B_begin()
        eng.B_factor()
        torch.cuda.synchronize()
        rho = _np64(eng.rho(1))
        assert np.all(np.abs(rho - p["rho"]) <= 1e-5 * p["rho"]), (rho, p["rho"])  # the regimes the host test found hold here
        B0, U0 = eng.B.clone(), dual.clone()
        Y = _np64(B0 + U0) if desc["kind"] in FP32_SUM else _np64(B0) + _np64(U0)  # as the kernel forms it
        assert np.array_equal(Y, p["Y"])
        want = _reference(key, p, desc, rho)
        eng.B_prox_local(0)
        torch.cuda.synchronize()
        got = _np64(aux)
        scale = pc.column_scale(desc, Y, p["row_ptr"], rho)
        worst = float((np.abs(got - want) / (BAR_AUX * scale)).max())
        ref_dual = _np64(B0) - (got - _np64(U0))  # U <- B - (Z - U)   (decomposition.py:282-285)
        worst_dual = float((np.abs(_np64(dual) - ref_dual) / (BAR_DUAL * scale)).max())
        print(f"{label} rank {rank} {pc.desc_id(desc)}: worst aux error / bar {worst:.3f}, dual {worst_dual:.3f}")
        j, c = np.unravel_index(np.argmax(np.abs(got - want) / scale), got.shape)
        assert worst <= 1.0, (label, rank, desc, int(j), int(c), got[j, c], want[j, c], scale[j, c])
        assert worst_dual <= 1.0, (label, rank, desc, "dual")
        assert torch.equal(eng.B, B0), "the prox step changed B"
        assert _untouched_outside(aux_buf, aux) and _untouched_outside(dual_buf, dual), "a store outside the N rows of aux / dual"
        return eng, got
    except BaseException:
        eng.close()
        raise


@pytest.mark.parametrize("rank", pc.RANKS["tv"])
@pytest.mark.parametrize("desc", pc.PARAMS["tv"], ids=pc.desc_id)
def test_kernel_alone_tv(rank, desc):
    """k_slab_tv (one lane per (slab, column), workgroups of 64: rank 17 = 187 lanes, three workgroups, the last partly filled)
    + k_rows_dual.  3 fp32 roundings (module docstring)."""
    eng, _ = _check_alone(pc.ragged_problem(rank), ("ragged", pc.rank_of(rank)), rank, desc, "k_slab_tv + k_rows_dual")
    eng.close()


@pytest.mark.parametrize("rank", pc.RANKS["simplex"])
def test_kernel_alone_simplex(rank):
    """k_slab_simplex<float> (one wave per (slab, column): one-row slabs, the strided loop at 64 / 65 rows, ties at the root,
    vertices) + k_rows_dual.  1 fp32 rounding."""
    eng, got = _check_alone(pc.ragged_problem(rank), ("ragged", pc.rank_of(rank)), rank, pc.PARAMS["simplex"][0],
                            "k_slab_simplex + k_rows_dual")
    eng.close()
    p = pc.ragged_problem(rank)
    sums = np.array([got[s:e].sum(axis=0) for s, e in zip(p["row_ptr"][:-1], p["row_ptr"][1:])])
    assert got.min() >= 0 and np.abs(sums - 1.0).max() <= 257 * HALF_ULP


@pytest.mark.parametrize("rank", pc.RANKS["l2ball"])
@pytest.mark.parametrize("desc", pc.PARAMS["l2ball"], ids=pc.desc_id)
def test_kernel_alone_l2ball(rank, desc):
    """k_slab_colsq + k_rows_l2ball.  3 fp32 roundings."""
    eng, _ = _check_alone(pc.ragged_problem(rank), ("ragged", pc.rank_of(rank)), rank, desc, "k_slab_colsq + k_rows_l2ball")
    eng.close()


@pytest.mark.parametrize("rank", pc.RANKS["rowsep"])
@pytest.mark.parametrize("desc", pc.PARAMS["rowsep"], ids=pc.desc_id)
def test_kernel_alone_rowsep(rank, desc):
    """k_rows_prox_rowsep.  2 fp32 roundings (+ the fp32 image of the parameter)."""
    eng, _ = _check_alone(pc.ragged_problem(rank), ("ragged", pc.rank_of(rank)), rank, desc, "k_rows_prox_rowsep")
    eng.close()


@pytest.mark.parametrize("n", pc.GL2_N)
@pytest.mark.parametrize("rank", pc.GL2_RANKS)
@pytest.mark.parametrize("which", ["laplacian", "random_psd"])
def test_kernel_alone_gl2_and_value(n, rank, which):
    """k_gl2_pass<float, false / true> (thread ty owns columns ty + 4 q: q > 0 from rank 5; a second 64-row tile of `a` and its
    tail from n = 65) - 1 fp32 rounding - and k_gl2_value (eig[e % n] over three slabs) against trace(F^T M F) in fp64.  Both are
    fp64 sums of at most 3 n r = 25 000 non-negative terms (25 000 x 1.1e-16 = 2.8e-12 of the value at the very worst) behind an
    eigen-decomposition that reproduces M to 1e-13 (tests/test_prox_cases_host.py): bar 1e-11 of max(1, value)."""
    import torch

    p = pc.gl2_problem(n, rank, which)
    eng, _ = _check_alone(p, ("gl2", n, rank, which), rank, {"kind": "gl2", "norm_matrix": p["M"]}, "k_gl2_pass x 2")
    try:
        val = float(eng.penalty_value(1, 0).cpu()[0])
        torch.cuda.synchronize()
        want = pc.gl2_value(p["B"], p["row_ptr"], p["M"])
        print(f"k_gl2_value n {n} rank {rank} {which}: error / bar {abs(val - want) / (1e-11 * max(1.0, abs(want))):.1e}")
        assert abs(val - want) <= 1e-11 * max(1.0, abs(want)), (val, want)
    finally:
        eng.close()


# ---- (b) ---------------------------------------------------------------------------------------------------------------------------
TV0, TV1 = pc.PARAMS["tv"]
BALL, BALL_NN = pc.PARAMS["l2ball"]
L1, L1_NN, BOX = pc.PARAMS["rowsep"][:3]
STACKS = {
    "tv": [TV0],
    "tv_l1+nn": [TV1, {"kind": "nn"}],  # two members: a mix-up of the penalty index in the aux / dual addressing shows here
    "simplex": [pc.PARAMS["simplex"][0]],
    "nn+simplex": [{"kind": "nn"}, pc.PARAMS["simplex"][0]],  # ... and the slab-wise kernels as member 1
    "l1+tv": [L1, TV0],
    "l2ball": [BALL],
    "l2ball_nn+box": [BALL_NN, BOX],
    "l1+box": [L1, BOX],
    "l1_nn": [L1_NN],
    "gl2": [{"kind": "gl2", "norm_matrix": "laplacian"}],
    "gl2_psd+nn": [{"kind": "gl2", "norm_matrix": "random_psd"}, {"kind": "nn"}],
}
ROWSEP_KINDS = ("nn", "box", "l1")
PHASES = ([(1, n, r) for n, r in pc.PHASE_B] + [(2, n, r) for n, r in pc.PHASE_SHAPES] + [(0, n, r) for n, r in pc.PHASE_SHAPES])
# (GeneralizedL2 needs slabs of one length: on mode 1 it takes the problems of three equal slabs, the other kinds the ragged ones)
PHASE_CASES = [(ph, st) for ph in PHASES for st in sorted(STACKS) if ph[0] != 1 or st.startswith("gl2") == (ph[1] is not None)]


def _phase_id(v):
    return "mode{}-n{}-r{}".format(*v)


@pytest.mark.parametrize("phase,stack", PHASE_CASES, ids=lambda v: v if isinstance(v, str) else _phase_id(v))
def test_phase_postcondition(phase, stack, kernel_paths):
    """(b) of the module docstring: one inner iteration of the phase of `phase` = (mode, rows, rank) under the stack `stack`"""
    import torch

    from matcouply_amd import _engine as E
    from tests.helpers import native_regs

    mode, size, rank = phase
    p = pc.phase_problem(mode, size, rank)
    slabs = p["slabs"]
    n_rows = int(slabs[-1])
    descs = [dict(d, norm_matrix=pc.norm_matrix(d["norm_matrix"], int(slabs[1]))) if d["kind"] == "gl2" else d for d in STACKS[stack]]
    rowsep = all(d["kind"] in ROWSEP_KINDS for d in descs)
    constant_A = mode == 0 and not rowsep  # the matrix kinds on A need the constant feasibility penalty
    dev = torch.device("cuda", 0)
    # member k starts from the designed columns shifted by k (so that two members do not start equal) and a small dual
    aux0 = [np.roll(p["aux0"], k, axis=1) for k in range(len(descs))]
    dual0 = [np.roll(p["dual0"], k, axis=1) * (1.0 if k % 2 == 0 else -1.0) for k in range(len(descs))]
    regs = [[], [], []]
    regs[mode] = native_regs(descs, aux0, dual0, dev)
    eng = E.HipEngine(_f32(p["X"], dev), p["row_ptr"], rank, _f32(p["A"], dev), _f32(p["B"], dev), _f32(p["C"], dev), regs,
                      inner_n_iter_max=1, constant_A=constant_A)
    try:
        if mode == 1:
            eng.update_B()
        elif mode == 2:
            eng.update_C_local()
            eng.update_C_finish()
        else:
            eng.update_A()
        torch.cuda.synchronize()
        exact = eng.kernel_variant(E.VARIANT_EXACT_MODE) != ""
        assert exact == (kernel_paths == "default")
        if mode != 0 or constant_A:  # (row-separable stacks on A stay in the A-finish kernel on both paths)
            assert eng.kernel_variant(E.PROF_ROWS_FUSED).startswith("k_wide_") == exact, eng.kernel_variant(E.PROF_ROWS_FUSED)
        F1 = _np64((eng.A, eng.B, eng.C)[mode])
        if mode == 1:
            rho = _np64(eng.rho(1))
        elif mode == 2:
            rho = _np64(eng.rho(2))[:1]
        else:
            rho = _np64(eng.A_rho_max())[:1] if constant_A else _np64(eng.rho(0))
        assert np.all(np.isfinite(F1)) and np.all(rho > 0)
        for k, d in enumerate(descs):
            # a row-separable kind couples nothing: every row is its own coupling set (and has its own rho on a non-constant A)
            ptr = np.arange(n_rows + 1) if d["kind"] in ROWSEP_KINDS else slabs
            per_slab = d["kind"] in ROWSEP_KINDS and len(rho) == len(slabs) - 1
            rho_k = rho[np.repeat(np.arange(len(slabs) - 1), np.diff(slabs))] if per_slab else rho
            Y = F1 + dual0[k].astype(np.float64)
            want = pc.reference(d, Y, ptr, rho_k)
            scale = pc.column_scale(d, Y, ptr, rho_k)
            n_couple = np.repeat(np.diff(ptr), np.diff(ptr)).astype(np.float64)[:, None]
            bar = (np.sqrt(n_couple) + 2.0) * HALF_ULP * scale
            got = _np64(eng.regs[mode][k].aux)
            worst = float((np.abs(got - want) / bar).max())
            ref_dual = dual0[k].astype(np.float64) + F1 - got
            worst_dual = float((np.abs(_np64(eng.regs[mode][k].dual) - ref_dual) / (BAR_DUAL * scale)).max())
            print(f"{_phase_id(phase)} {stack}[{k}] {d['kind']} {kernel_paths}: worst aux error / bar {worst:.3f}, dual {worst_dual:.3f}")
            j, c = np.unravel_index(np.argmax(np.abs(got - want) / bar), got.shape)
            assert worst <= 1.0, (phase, stack, k, kernel_paths, int(j), int(c), got[j, c], want[j, c], bar[j, c])
            assert worst_dual <= 1.0, (phase, stack, k, kernel_paths, "dual")
    finally:
        eng.close()
