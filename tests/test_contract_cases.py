"""CPU: the case table of tests/test_gpu_contract.py (tests/kernel_edge_cases.py::CONTRACT_CASES) reaches every form and tile edge
of the two passes over X (csrc/contract.hip, csrc/xclds.hip), the integer data of its bit-for-bit leg stay exact in every number
format involved, and every instantiation of those kernels in the BUILT library is launched by a case or listed, with its reason,
in CONTRACT_UNREACHABLE.  The dispatch is restated in tests/contract_dispatch.py; the GPU test holds the device to the same
restatement (kernel_variant strings, the planner's tables), so what is proved here is proved about the library."""
import itertools
import os
import re
import sys

import numpy as np
import pytest

from tests import contract_dispatch as cd
from tests import kernel_edge_cases as kec

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = kec.CONTRACT_CASES
RUNS = kec.contract_runs()


def _runs_of(pred=lambda c, env, a: True):
    """(case, switches, A, xc launch of B_begin, xc launch of A_begin, xt launch, segments) of every fp32 run that satisfies pred"""
    out = []
    for _, n, env, a in RUNS:
        c = CASES[n]
        if not pred(c, env, a):
            continue
        al = not c["unaligned"]
        out.append((c, env, a, cd.launch_xc(c["J"], c["K"], c["rank"], "f32", al, env, 0),
                    cd.launch_xc(c["J"], c["K"], c["rank"], "f32", al, env, 1 if a == "nn" else 2),
                    cd.launch_xt(c["J"], c["K"], c["rank"], "f32", al, env), cd.plan_segments(c["J"], env)))
    return out


ALL = _runs_of()
FAST = [x for x in ALL if x[3]["family"] != "xc_f64"]


def test_cases_are_small_and_well_formed():
    for n, c in CASES.items():
        assert sum(c["J"]) <= 6000 and c["K"] <= 2048 and 1 <= c["rank"] <= 64, n
        assert set(c["env"]) <= set(cd.SWITCHES), n
        assert c["A"] in ("nn", "ridge", "both"), n
        if c["nt"]:  # the non-temporal twin needs more than MCL_X_NT_MB = 1 MiB of X, and the plain run less than the default 256
            assert cd.x_streams(sum(c["J"]), c["K"], {"MCL_X_NT_MB": "1"}) and not cd.x_streams(sum(c["J"]), c["K"], {}), n
        if c["unaligned"]:
            assert c["K"] % 4 == 0, n
        for t in c["twins"]:
            assert set(t) <= set(cd.SWITCHES), n


def test_ranks():
    assert {c["rank"] for c in CASES.values()} >= {1, 3, 5, 12, 16, 17, 20, 32, 33, 64}
    assert {c["rank"] for c in CASES.values()} & {40, 48}
    assert cd.nb_of(33) == cd.nb_of(48) == 4 and cd.nb_of(16) == 1 and cd.nb_of(17) == cd.nb_of(32) == 2


def test_contract_xc_forms():
    xc = [x for x in FAST if x[3]["family"] == "xc"]
    have = {(cd.nb_of(c["rank"]), 4 if (c["K"] % 4 == 0 and not c["unaligned"]) else 1, cd.xc_chunks(c["K"], cd.nb_of(c["rank"]))[1])
            for c, *_ in xc}
    assert have == {(nb, v, k) for nb, ks in ((1, (2, 4, 0)), (2, (2, 0)), (4, (0,))) for k in ks for v in (4, 1)}, have
    for nb, ks in ((1, (2, 4, 0)), (2, (2, 0)), (4, (0,))):  # VEC = 1 once from K % 4 != 0 and once from the unaligned view
        for k in ks:
            mine = [c for c, *_ in xc if cd.nb_of(c["rank"]) == nb and cd.xc_chunks(c["K"], nb)[1] == k]
            assert any(c["K"] % 4 for c in mine) and any(c["unaligned"] for c in mine), (nb, k)
    assert any((c["K"] + 63) // 64 == 5 and cd.xc_chunks(c["K"], 1)[0] == 8 for c, *_ in xc)  # a padded chunk count
    assert any(c["K"] == 256 and "MCL_XC_NOROW" in env and x0["kernels"][-1] == "k_contract_xc<1, 4, 4>" for c, env, _, x0, *_ in xc)
    part = [cd.xc_block_partition(sum(c["J"]), env) for c, env, *_ in xc]
    assert any(bpw >= 2 and nblk % bpw for nblk, bpw, _ in part)  # bpw >= 2 and a short last wave
    assert any(sum(c["J"]) % 16 and any(s % 16 for s in np.cumsum(c["J"])[:-1]) for c, *_ in xc)  # blocks straddle slab boundaries


def test_contract_xc_256_and_row_forms():
    k = lambda fam: {(c["K"], cd.nb_of(c["rank"]), xa["gram"], "MCL_X_NT_MB" in env) for c, env, _, x0, xa, *_ in FAST
                     for xa in (x0, xa) if xa["family"] == fam}
    assert {(g, nt) for K, nb, g, nt in k("xc_256")} == set(itertools.product((0, 1, 2), (False, True)))
    row = k("xc_row")
    for K, nb in ((256, 2), (256, 4), (768, 1), (768, 2), (768, 4), (1536, 2), (512, 4)):
        assert {g for K_, nb_, g, _ in row if (K_, nb_) == (K, nb)} == ({0, 1, 2} if nb < 4 else {0, 1}), (K, nb)
    assert any(c["K"] == 1024 and "MCL_NO_XC_LDS" in env and x0["family"] == "xc_row" for c, env, _, x0, *_ in FAST)
    creg = {xa["gram"] for c, env, _, x0, xa, *_ in FAST for xa in (x0, xa) if xa["family"] == "xc_row" and "MCL_XC_DEPTH1" in env}
    assert creg == {0, 1, 2}
    # NB = 4 with a penalty-free A: the plain X C form, then k_slab_gram<4>
    assert any(cd.nb_of(c["rank"]) == 4 and a == "ridge" and xa["family"] == "xc_row" and xa["gram"] == 0 and xa["slab_gram"]
               for c, _, a, _, xa, *_ in FAST)


def test_contract_xc_lds_forms():
    lds = [(c["K"], cd.nb_of(c["rank"]), x0["depth"], env.get("MCL_XC_LDS_DEPTH")) for c, env, _, x0, *_ in FAST if x0["family"] == "xc_lds"]
    assert {(K, nb) for K, nb, d, _ in lds if d == 4} >= {(512, 1), (1024, 1), (1536, 1), (2048, 1), (512, 2), (1024, 2)}
    assert {(K, nb) for K, nb, d, _ in lds if d == 8} == {(1024, 1), (2048, 1), (1024, 2)}
    assert {K for K, nb, d, want in lds if want == "8" and d == 4} == {512, 1536}  # the launcher falls back to four
    assert cd.xc_lds_depth([64], 2048, 2, True, {}, 1) == 0  # 256 KB of C fragments: over the 160 KB of a CU
    for c, env, _, x0, *_ in FAST:
        if x0.get("depth") == 8:
            assert c["f32_only"]


def test_contract_xt_forms():
    xt = [(c, env, t, seg) for c, env, _, _, _, t, seg in FAST]
    assert {(t["KB"], t["NB"]) for _, _, t, _ in xt} == {(1, 1), (2, 1), (4, 1), (1, 2), (2, 2), (1, 4)}
    for kbnb in ((1, 1), (2, 1), (4, 1), (1, 2), (2, 2), (1, 4)):
        mine = [(c, env, t) for c, env, t, _ in xt if (t["KB"], t["NB"]) == kbnb]
        assert {t["vec"] for _, _, t in mine} == {True, False}, kbnb
        assert any(t["vec"] and t["depth"] == 2 for _, _, t in mine) and any(t["depth"] == 4 for _, _, t in mine), kbnb
        assert any(c["K"] % 4 for c, _, t in mine), kbnb  # VEC = 1 for the 16-bit twins too
    assert any(t["NB"] == 4 and len(t["kernels"]) == 3 for _, _, t, _ in xt)  # both launches at NB = 4
    assert any(c["K"] < 64 * t["KB"] for c, _, t, _ in xt)  # K below one slice
    assert any(c["K"] % (64 * t["KB"]) and t["n_slices"] >= 2 for c, _, t, _ in xt)
    assert any(t["nb"] > 8 and t["nb"] % 8 for _, _, t, _ in xt)  # the XCD-padded grid has idle workgroups


def test_non_temporal_forms():
    fams = {x["family"] + ("_creg" if "CREG=1" in x["variant"] else "") for c, env, _, x0, xa, t, _ in FAST if "MCL_X_NT_MB" in env
            for x in (x0, xa, t) if any(k.endswith("true>") or ", true, " in k for k in x["kernels"])}
    assert fams >= {"xt", "xc_row", "xc_row_creg", "xc_256", "xc_lds"}, fams


def test_exact_forms():
    ex = [(c, t) for c, env, _, x0, _, t, _ in ALL if x0["family"] == "xc_f64"]
    assert all(c["env"].get("MCL_EXACT") == "1" for c, _ in ex)
    assert {cd.nb_of(c["rank"]) for c, _ in ex} == {1, 2, 4}
    assert {t["n_chunks"] for _, t in ex} == {1, 2, 8, 9}
    assert {sum(c["J"]) % 256 for c, _ in ex} >= {0, 1, 255}
    assert any(c["K"] % 16 for c, _ in ex)
    assert cd.exact_mode(4096, 256, {}) and not cd.exact_mode(4097, 256, {}) and not cd.exact_mode(16, 16, {"MCL_EXACT": "0"})


def test_planner_edges():
    assert {j for c in CASES.values() for j in c["J"]} >= {0, 1, 15, 16, 17, 255, 256, 257}
    assert any(len(c["J"]) == 1 for c in CASES.values())
    few = [(c, seg) for c, env, _, _, _, _, seg in FAST if "MCL_XC_WAVES" in env]
    segs_of_wave = lambda seg: [list(range(seg[3][w], seg[3][w + 1])) for w in range(len(seg[3]) - 1)]
    assert any(len(w) >= 3 for _, seg in few for w in segs_of_wave(seg))
    assert any(len({seg[0][s] for s in w}) >= 2 for _, seg in few for w in segs_of_wave(seg))
    waves_of_slab = lambda seg, i: {w for w, ss in enumerate(segs_of_wave(seg)) for s in ss if seg[0][s] == i}
    assert any(len(waves_of_slab(seg, i)) >= 3 for c, seg in few for i in range(len(c["J"])))
    # a segment cut mid-slab by the quota: it ends before its slab does, shorter than the 256-row cap
    ends = lambda c: set(np.cumsum(c["J"]))
    assert any(n < 256 and r0 + n not in ends(c) for c, seg in few for r0, n in zip(seg[1], seg[2]))
    assert any(n == 256 for _, seg in few for n in seg[2])
    assert {(len(seg[3]) - 1) % 4 for _, seg in few} == {0, 1, 2, 3}
    assert any(c["env"].get("MCL_SEG_ROWS") == "32" and max(seg[2]) == 32 for c, _, _, _, _, _, seg in FAST)
    # without MCL_XC_WAVES a small problem gets one 16-row block per wave: no segment longer than a block
    for c, env, _, _, _, _, seg in FAST:
        if "MCL_XC_WAVES" not in env and sum((j + 15) // 16 for j in c["J"]) <= 512:
            assert max(seg[2]) <= 16 and len(seg[3]) - 1 == len(seg[0])
    for c, env, _, _, _, _, seg in ALL:  # the segments tile the rows, slab by slab
        assert seg[1] == list(np.concatenate([[0], np.cumsum(seg[2])[:-1]])) and sum(seg[2]) == sum(c["J"])
        rp = np.concatenate([[0], np.cumsum(c["J"])])
        assert all(rp[i] <= r0 and r0 + n <= rp[i + 1] for i, r0, n in zip(*seg[:3]))


def test_sweep_planned_pair():
    a, b = CASES["xc_sweep_k128_r20"], CASES["xc_nosweep_k128_r20"]
    assert (a["J"], a["K"], a["rank"]) == (b["J"], b["K"], b["rank"]) and "MCL_NO_SWEEP" in b["env"] and {"MCL_NO_SWEEP": "1"} in a["twins"]
    nb = cd.nb_of(a["rank"])
    assert cd.sweep_planned(a["J"], a["K"], nb, a["env"]) and not cd.sweep_planned(b["J"], b["K"], nb, b["env"])
    assert cd.cfrag_chunks(a["J"], a["K"], nb, a["env"]) != cd.cfrag_chunks(b["J"], b["K"], nb, b["env"])  # the image is sized differently


def test_real_valued_leg_has_a_case_per_family_and_nb():
    have = set()
    for c, env, _, x0, xa, t, _ in ALL:
        if c["legB"]:
            have |= {(x0["family"], cd.nb_of(c["rank"])), (t["family"], cd.nb_of(c["rank"]))}
    want = {("xc", 1), ("xc", 2), ("xc", 4), ("xc_row", 1), ("xc_row", 2), ("xc_row", 4), ("xc_256", 1), ("xc_lds", 1), ("xc_lds", 2),
            ("xt", 1), ("xt", 2), ("xt", 4), ("xc_f64", 1), ("xc_f64", 2), ("xc_f64", 4), ("exact_gr", 1), ("exact_gr", 2), ("exact_gr", 4)}
    assert have >= want, want - have
    twins = [t for c in CASES.values() if c["legB"] for t in c["twins"]]
    assert {"MCL_XC_LDS_DEPTH": "8"} in twins and {"MCL_XT_DEPTH": "2"} in twins and {"MCL_NO_SWEEP": "1"} in twins
    assert any(c["legB"] and c["nt"] for c in CASES.values())


@pytest.mark.parametrize("name", sorted(CASES))
def test_integer_data_stay_exact(name):
    """leg A: every entry of X is an integer of at most 256 in magnitude (exact in bf16 and fp16), and every sum of absolute
    products - so every product, partial sum and output, in whatever order a kernel adds - is an integer below 2^24"""
    d, ref = kec.contract_data(name, "int"), kec.contract_reference(name, "int")
    for k in ("X", "A", "B", "C"):
        assert np.array_equal(d[k], np.round(d[k])), k
    assert np.abs(d["X"]).max() <= 256
    for k in ("XC_abs", "G_abs", "R_abs", "rhs_abs", "Q_abs"):
        assert ref[k].max(initial=0.0) < 2 ** 24, (k, ref[k].max())
    assert np.abs(d["X"]).max() >= 2 and np.abs(ref["XC"]).max() > 16  # and not trivially small


def claimed_instantiations():
    """every kernel of the two passes the GPU cases launch, over the element types of every run"""
    out = set()
    for _, n, env, a in RUNS:
        c = CASES[n]
        for xt in kec.contract_x_types(c):
            al = not c["unaligned"]
            x0 = cd.launch_xc(c["J"], c["K"], c["rank"], xt, al, env, 0)
            xa = cd.launch_xc(c["J"], c["K"], c["rank"], xt, al, env, 1 if a == "nn" else 2)
            out |= set(x0["kernels"]) | set(xa["kernels"]) | set(cd.launch_xt(c["J"], c["K"], c["rank"], xt, al, env)["kernels"])
            if xa["slab_gram"]:
                out.add(cd.slab_gram_kernel(c["rank"]))
    return out


PASS_KERNELS = r"k_contract_x|k_exact_gr|k_slab_gram<|k_reduce_partials$|k_build_cfrag$"


def _unreachable(kernel):
    return any(re.fullmatch(p, kernel) for p in kec.CONTRACT_UNREACHABLE)


def test_every_instantiation_is_claimed_or_listed_unreachable():
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import kernel_resources as kr

    if not os.path.exists(kr.LIB):
        pytest.skip(f"{kr.LIB} is not built (python -c 'import __graft_entry__ as g; g.build()')")
    built = {r["kernel"] for r in kr.resources() if re.match(PASS_KERNELS, r["kernel"])}
    assert len(built) >= 300, len(built)
    claimed = claimed_instantiations()
    listed = {k for k in built if _unreachable(k)}
    assert not claimed & listed, sorted(claimed & listed)
    unclaimed = built - claimed - listed
    assert not unclaimed, f"{len(unclaimed)} instantiations no case of CONTRACT_CASES runs: {sorted(unclaimed)}"
    assert not claimed - built, f"cases claim instantiations the library does not have: {sorted(claimed - built)}"
    for p in kec.CONTRACT_UNREACHABLE:
        assert any(re.fullmatch(p, k) for k in built), f"CONTRACT_UNREACHABLE lists nothing that is built: {p}"


def test_unreachable_table_agrees_with_the_dispatch():
    """no shape and no switch makes the restated dispatch choose a listed instantiation: K = 1 .. 4096, rank = 1 .. 64 (every NB and
    rank edge), aligned and not, every switch of the launchers on and off, the three element types"""
    ranks = (1, 16, 17, 32, 33, 48, 49, 64)
    switch_sets = [dict(zip(ks, vs)) for ks in [("MCL_X_NT_MB", "MCL_XC_NOROW", "MCL_XC_DEPTH1", "MCL_NO_XC_LDS", "MCL_XC_LDS_DEPTH", "MCL_XT_DEPTH")]
                   for vs in itertools.product(("1", None), ("1", None), ("1", None), ("1", None), ("8", None), ("2", None))]
    switch_sets = [{**{k: v for k, v in s.items() if v is not None}, "MCL_EXACT": "0"} for s in switch_sets]
    seen = set()
    J = [3000, 2000]  # more than 1 MiB from K = 53 on: MCL_X_NT_MB=1 streams
    for K in range(1, 4097):
        for r in ranks:
            for al in (True, False):
                for sw in switch_sets if K % 256 == 0 or K in (60, 100, 128, 200) else switch_sets[:1] + switch_sets[-1:]:
                    for xt in cd.X_TYPES:
                        if not al and xt != "f32":
                            continue
                        for g in (0, 1, 2):
                            seen.update(cd.launch_xc(J, K, r, xt, al, sw, g)["kernels"])
                        seen.update(cd.launch_xt(J, K, r, xt, al, sw)["kernels"])
    bad = sorted(k for k in seen if _unreachable(k))
    assert not bad, bad
    assert len(seen) > 250
    for nb in (1, 2, 4):  # and the two rules themselves
        kcts = {cd.xc_chunks(K, nb)[1] for K in range(1, 4097)}
        assert kcts == {1: {2, 4, 0}, 2: {2, 0}, 4: {0}}[nb]
