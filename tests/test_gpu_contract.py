"""-m gpu: the two passes over X - X C and [G | R] = [(B o a)^T (B o a) | X^T (B o a)] (csrc/contract.hip, csrc/xclds.hip) - kernel by
kernel against an fp64 NumPy reference, over tests/kernel_edge_cases.py::CONTRACT_CASES (tests/test_contract_cases.py proves on a
CPU which forms and edges the table reaches).

Every run takes its by-products from fresh contexts (no sweep by-product exists on one): B_begin gives X C in the plain form;
update_C_local gives [G | R]; update_A gives X C again from the form with the fused per-segment reductions, rhs_i and
(B_i^T B_i) o (C^T C).  The kernel_variant strings and the planner's tables on the device must be what tests/contract_dispatch.py
predicts.

Leg A, integer data: X, A, B, C hold small integers such that every sum of absolute products stays below 2^24 (asserted on the
CPU), so fp32 chains, fp64 sums and bf16 / fp16 storage are all exact and the results must EQUAL the reference - tolerance zero.
Leg B, real-valued data at fp32: elementwise a-priori bounds, one ulp per accumulation step and 8 for the roundings around the
chain: (n + 8) 2^-23 sum|products| with n = K for X C, n = 256 for G, R and B_i^T B_i (the fp32 chains end with their segment of
at most 256 rows; the sums over segments are fp64), n = K + 256 for the fused rhs_i (the chain through X C, then over the rows);
the exact-products forms: 8 2^-53 sum|products|, plus 2^-24 |value| where an fp32 image is stored.  Each case runs twice (bitwise
equal: fixed summation order), and its switch twins must agree bit for bit (leg C): MCL_X_NT_MB=1, MCL_XC_LDS_DEPTH=8 against 4,
MCL_XT_DEPTH=2 against 4, MCL_NO_SWEEP.  MCL_XC_DEPTH1 against k_contract_xc_256 is NO such pair: the first adds four fp32 chains
pairwise in fp32, the second eight chains as a tree in fp64 - by design; both are held by leg A and by the leg-B bound.

Worst error / bound per family, measured on an MI355X (printed by test_real_valued_bounds):
    X C      k_contract_xc 0.019, k_contract_xc_row 0.003, k_contract_xc_256 0.002, k_contract_xc_lds 0.001
    G, R     k_contract_xt 0.016, 0.003
    rhs_i    0.002 (both fused forms and k_slab_gram);  (B_i^T B_i) o (C^T C)  0.021 in fp32 chains, 0.002 in fp64
    exact    X C 0.997, rhs_i 0.91, Q 0.97 (all three the one fp32 rounding of the stored image); k_exact_gr G 0.81, R 0.13
354 tests, 6 s on an MI355X."""
import numpy as np
import pytest

from matcouply_amd import _engine as E
from tests import contract_dispatch as cd
from tests import kernel_edge_cases as kec

pytestmark = pytest.mark.gpu
CASES = kec.CONTRACT_CASES
U32, U64 = 2.0 ** -23, 2.0 ** -53


def _run(name, env, a_kind, xt, kind, monkeypatch):
    """the by-products of one run (numpy float64), the kernel variants and the planner's tables"""
    import torch

    c = CASES[name]
    for k in cd.SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    d = kec.contract_data(name, kind)
    dev = torch.device("cuda:0")
    N, K, r, I = d["X"].shape[0], c["K"], c["rank"], len(c["J"])
    t = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float32, device=dev)
    xdt = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}[xt]
    if c["unaligned"]:  # the data start one element past a 16-byte boundary
        buf = torch.zeros(N * K + 4, dtype=torch.float32, device=dev)
        X = buf[1:1 + N * K].view(N, K)
        X.copy_(t(d["X"]))
        assert X.data_ptr() % 16 == 4 and X.is_contiguous()
    else:
        X = t(d["X"]).to(xdt)
    zeros = lambda rows: torch.zeros((rows, r), dtype=torch.float32, device=dev)
    nn = lambda rows: E.NativeReg(E.KIND["nn"], zeros(rows), zeros(rows))
    out = {}

    def engine():
        regs = [[nn(I)] if a_kind == "nn" else [], [nn(N)], [nn(K)]]
        with pytest.warns(RuntimeWarning, match="MCL_"):
            return E.HipEngine(X, d["row_ptr"], r, t(d["A"]), t(d["B"]), t(d["C"]), regs,
                               l2_penalty=(0.0 if a_kind == "nn" else kec.CONTRACT_RIDGE, 0.0, 0.0))

    np64 = lambda x: x.detach().cpu().numpy().astype(np.float64)
    e1 = engine()
    e1.B_begin()
    out["XC"] = np64(e1.internal(E.BUF_XC)).reshape(N, r)
    out["variant_xc0"] = e1.kernel_variant(E.PROF_XC)
    ints = lambda which: e1.internal(which).view(torch.int32).cpu().numpy().tolist()
    out["segs"] = (ints(E.BUF_SEG_ROW0), ints(E.BUF_SEG_NROWS), ints(E.BUF_WAVE_SEG_PTR))
    e1.close()
    e2 = engine()
    gr = np64(e2.update_C_local())
    out["G"], out["R"] = gr[:r * r].reshape(r, r), gr[r * r:].reshape(K, r)
    out["variant_xt"] = e2.kernel_variant(E.PROF_XT)
    e2.update_A()
    out["XC_gram"] = np64(e2.internal(E.BUF_XC)).reshape(N, r)
    out["rhs"], out["Q"] = np64(e2.rhses()), np64(e2.cross_products())
    out["variant_xc1"] = e2.kernel_variant(E.PROF_XC)
    torch.cuda.synchronize()
    e2.close()
    return out


LEG_A = [(rn, n, env, a, xt) for rn, n, env, a in kec.contract_runs() for xt in kec.contract_x_types(CASES[n])]


@pytest.mark.parametrize("run,name,env,a_kind,xt", LEG_A, ids=[f"{rn}-{xt}" for rn, _, _, _, xt in LEG_A])
def test_integer_data_bit_for_bit(run, name, env, a_kind, xt, monkeypatch):
    c = CASES[name]
    got = _run(name, env, a_kind, xt, "int", monkeypatch)
    al = not c["unaligned"]
    x0 = cd.launch_xc(c["J"], c["K"], c["rank"], xt, al, env, 0)
    xa = cd.launch_xc(c["J"], c["K"], c["rank"], xt, al, env, 1 if a_kind == "nn" else 2)
    assert got["variant_xc0"] == x0["variant"] and got["variant_xc1"] == xa["variant"]
    assert got["variant_xt"] == cd.launch_xt(c["J"], c["K"], c["rank"], xt, al, env)["variant"]
    _, row0, nrows, ptr = cd.plan_segments(c["J"], env)
    assert got["segs"] == (row0, nrows, ptr)
    ref = kec.contract_reference(name, "int")
    for k, want in (("XC", ref["XC"]), ("XC_gram", ref["XC"]), ("G", ref["G"]), ("R", ref["R"]), ("rhs", ref["rhs"]), ("Q", ref["Q"])):
        bad = np.argwhere(got[k] != want)
        assert bad.size == 0, (run, xt, k, len(bad), bad[:4].tolist(), got[k][tuple(bad[0])], want[tuple(bad[0])])


def _bounds(name, exact):
    """elementwise bounds of the real-valued leg (module docstring)"""
    c, ref = CASES[name], kec.contract_reference(name, "real")
    K = c["K"]
    if exact:
        img = lambda k: 8 * U64 * ref[k + "_abs"] + 2.0 ** -24 * np.abs(ref[k])
        return dict(XC=img("XC"), XC_gram=img("XC"), G=8 * U64 * ref["G_abs"], R=8 * U64 * ref["R_abs"], rhs=img("rhs"), Q=img("Q"))
    b = lambda n, k: (n + 8) * U32 * ref[k + "_abs"]
    return dict(XC=b(K, "XC"), XC_gram=b(K, "XC"), G=b(256, "G"), R=b(256, "R"), rhs=b(K + 256, "rhs"), Q=b(256, "Q"))


LEG_B = [(rn, n, env, a) for rn, n, env, a in kec.contract_runs() if CASES[n]["legB"] and "MCL_X_NT_MB" not in env]
_REF_KEY = {"XC": "XC", "XC_gram": "XC", "G": "G", "R": "R", "rhs": "rhs", "Q": "Q"}


@pytest.mark.parametrize("run,name,env,a_kind", LEG_B, ids=[rn for rn, *_ in LEG_B])
def test_real_valued_bounds(run, name, env, a_kind, monkeypatch):
    c = CASES[name]
    got = _run(name, env, a_kind, "f32", "real", monkeypatch)
    ref, bound = kec.contract_reference(name, "real"), _bounds(name, env.get("MCL_EXACT") == "1")
    ratios = {k: float(np.max(np.abs(got[k] - ref[_REF_KEY[k]]) / np.maximum(bound[k], 1e-300), initial=0.0)) for k in _REF_KEY}
    fam = cd.launch_xc(c["J"], c["K"], c["rank"], "f32", not c["unaligned"], env, 1 if a_kind == "nn" else 2)
    print(f"\nleg B {run}: {fam['variant']} / {got['variant_xt']}: worst |error| / bound " + " ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    # fixed summation order: a second run, and every switch twin, gives the same bits
    again = [("again", env)] + [(str(t), {k: v for k, v in {**env, **t}.items() if v is not None}) for t in c["twins"]]
    if c["nt"]:
        again.append(("MCL_X_NT_MB=1", {**env, "MCL_X_NT_MB": "1"}))
    for label, env2 in again:
        other = _run(name, env2, a_kind, "f32", "real", monkeypatch)
        for k in _REF_KEY:
            assert np.array_equal(got[k], other[k]), (run, label, k, float(np.abs(got[k] - other[k]).max()))
    bad = {k: v for k, v in ratios.items() if not v <= 1.0}
    assert not bad, (run, bad)
