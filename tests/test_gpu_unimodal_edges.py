"""-m gpu: the unimodal prox kernel (csrc/unimodal.hip) on the designed columns of tests/unimodal_cases.py - stacks of exactly RC,
RC + 1 and RC + NRF entries, collapses of RC - 1, RC, RC + 1, RC / 2 and all entries in one pooling loop, a falling flank that pops
one ring entry per element over a spilled stack, a pause of the pruned schedule over a spilled stack, exactly tied splits, every
batch edge of the sweeps, the split search and the emit loops, slabs of 1 and of 300 rows in one wave, lane counts of 64 k +- 1 -
in all eight forms: the pruned schedule with 4, 2 and 1 waves per workgroup, the unpruned sweeps, the two-launch latency form, and
the last three again without the cooperative ring refill (MCL_NO_UNI_COOP: the per-lane refill takes its blocking branch).

Same route as tests/test_gpu_unimodal_kernels.py (mcl_B_begin, mcl_B_factor, mcl_B_prox_local on a mode-1 engine whose only penalty
is the unimodal one) and the same bars: aux within 2.4e-7 max(1, max |want|) of the oracle's regression of Y (four half-units of
fp32), the dual within 1e-6 of the same scale of B - (aux - U).  The columns are multiples of 1 / 64 and B + U is exact in fp32
(tests/test_unimodal_cases_host.py), so a wrong pop, refill, tie or batch edge is an error of at least 1 / 64.  B must be
bit-identical after the call and nothing may be written outside the N rows of aux and dual (buffers three rows longer, filled with
a sentinel; some layouts start one float into the buffer).  The engine reports the kernel form of the launch (kernel_variant),
which must be the one asked for; it does not report whether the cooperative refill ran - for that switch the test can only
check that the library saw it (mcl_active_switches).

Every case prints its worst error over the bar per form (DESIGN.md records them)."""
import os

import numpy as np
import pytest

from tests import unimodal_cases as uc
from tests.helpers import padded, to_np, untouched_outside

pytestmark = pytest.mark.gpu

BAR_AUX, BAR_DUAL = 2.4e-7, 1e-6
SWITCHES = ("MCL_UNI_SPLIT", "MCL_UNI_NOPRUNE", "MCL_UNI_WPB", "MCL_NO_UNI_COOP")
PRUNED4, PRUNED2, PRUNED1 = "k_slab_unimodal_v4<3, WPB=4>", "k_slab_unimodal_v4<3, WPB=2>", "k_slab_unimodal_v4<3>"
UNPRUNED, LATENCY = "k_slab_unimodal_v4<0>", "k_slab_unimodal_v4<1> + k_slab_unimodal_v4<2>"
FORMS = (
    ("pruned", {"MCL_UNI_SPLIT": "0"}, PRUNED4),
    ("pruned-wpb2", {"MCL_UNI_SPLIT": "0", "MCL_UNI_WPB": "2"}, PRUNED2),
    ("pruned-wpb1", {"MCL_UNI_SPLIT": "0", "MCL_UNI_WPB": "1"}, PRUNED1),
    ("unpruned", {"MCL_UNI_SPLIT": "0", "MCL_UNI_NOPRUNE": "1"}, UNPRUNED),
    ("latency", {"MCL_UNI_SPLIT": "1"}, LATENCY),
    ("pruned-nocoop", {"MCL_UNI_SPLIT": "0", "MCL_NO_UNI_COOP": "1"}, PRUNED4),
    ("unpruned-nocoop", {"MCL_UNI_SPLIT": "0", "MCL_UNI_NOPRUNE": "1", "MCL_NO_UNI_COOP": "1"}, UNPRUNED),
    ("latency-nocoop", {"MCL_UNI_SPLIT": "1", "MCL_NO_UNI_COOP": "1"}, LATENCY),
)

_REFERENCES = {}


def _reference(fam, packing, nonneg):
    """one regression per (family, packing, nonneg), never written to"""
    key = (fam, packing, nonneg)
    if key not in _REFERENCES:
        want = uc.reference(uc.problem(fam, packing), nonneg)
        want.setflags(write=False)
        _REFERENCES[key] = want
    return _REFERENCES[key]


@pytest.mark.parametrize("nonneg", [False, True], ids=["free", "nonneg"])
@pytest.mark.parametrize("fam,packing", uc.cases())
def test_designed_columns_in_every_form(fam, packing, nonneg):
    import torch

    from matcouply_amd import _engine as E

    p = uc.problem(fam, packing)
    want = _reference(fam, packing, nonneg)
    scale = max(1.0, float(np.abs(want).max()))
    dev = torch.device("cuda", 0)
    f32 = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float32, device=dev)
    N, r = p["Y"].shape
    aux_buf, aux = padded(np.zeros((N, r), dtype=np.float32), p["unaligned"], dev)
    dual_buf, dual = padded(p["U"], p["unaligned"], dev)
    eng = E.HipEngine(f32(p["X"]), p["row_ptr"], r, f32(p["A"]), f32(p["B"]), f32(p["C"]),
                      [[], [E.NativeReg(E.PEN_UNIMODAL, aux, dual, non_negativity=nonneg)], []])
    saved = {k: os.environ.get(k) for k in SWITCHES}
    try:
        eng.B_begin()
        eng.B_factor()
        B0, U0 = eng.B.clone(), dual.clone()
        assert np.array_equal(to_np(B0 + U0), p["Y"])  # the fp32 sum the kernel forms is the designed column, exactly
        worst = {}
        for label, env, variant in FORMS:
            for k in SWITCHES:
                os.environ.pop(k, None)
            os.environ.update(env)
            eng.reload_switches()  # the library reads its switches once per context
            eng.B.copy_(B0)
            dual.copy_(U0)
            aux.zero_()
            eng.B_prox_local(0)
            torch.cuda.synchronize()
            assert eng.kernel_variant(E.PROF_UNIMODAL) == variant, (label, eng.kernel_variant(E.PROF_UNIMODAL))
            assert ("MCL_NO_UNI_COOP" in eng.lib.mcl_active_switches(eng._h).decode().split()) == ("MCL_NO_UNI_COOP" in env), label
            got = to_np(aux)
            err = np.abs(got - want)
            j, c = np.unravel_index(np.argmax(err), err.shape)
            slab = int(np.searchsorted(p["row_ptr"], j, side="right") - 1)
            worst[label] = float(err[j, c]) / (BAR_AUX * scale)
            assert worst[label] <= 1.0, (label, fam, packing, nonneg, p["names"][slab][c], int(j - p["row_ptr"][slab]), got[j, c], want[j, c])
            # the dual step of the penalty: U <- B - (Z - U)   (decomposition.py:282-285)
            ref_dual = to_np(B0) - (got - to_np(U0))
            assert np.abs(to_np(dual) - ref_dual).max() <= BAR_DUAL * scale, (label, "dual")
            assert torch.equal(eng.B, B0), (label, "the prox step changed B")
            assert untouched_outside(aux_buf, aux) and untouched_outside(dual_buf, dual), (label, "a store outside the N rows of aux / dual")
        print(f"unimodal {fam} {packing} nonneg={int(nonneg)}: worst aux error / bar " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
        eng.close()
