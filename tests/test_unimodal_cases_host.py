"""The designed columns and layouts of tests/unimodal_cases.py, checked without a GPU: the stack of every collapse and flank column
reaches its nominal depth and pops its nominal count at the designed element; every column either is a declared exact tie or
has its optimal fit separated from every other fit by a thousand times the kernel's pruning margin; the oracle's two forms
agree bit for bit and agree with the reference's regression (tests/golden/unimodal_edges.npz); the fp32 sums are exact; the
layouts have the lane counts, wave counts and length spreads the GPU test (tests/test_gpu_unimodal_edges.py) is meant to run; a
model of a lane's ring shows that the columns of the in-step layout take each refill path of the kernel."""
import numpy as np
import pytest

from oracle import aoadmm_oracle as orc
from tests import unimodal_cases as uc
from tests.helpers import load_npz

RC, NRF = uc.RC, uc.NRF
MARGIN = 1e-6  # x sum of squares: a thousand times the pruning margin of the kernel (1e-9 x the same sum)


def test_constants_are_the_kernels():
    import os
    import re

    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "matcouply_amd", "csrc", "unimodal.hip")).read()
    for name, want in (("MCL_UNI_RC", uc.RC), ("MCL_UNI_NRF", uc.NRF), ("MCL_UNI_UB", uc.UB)):
        assert int(re.search(r"#define %s (\d+)" % name, src).group(1)) == want
    for name, want in (("EB", uc.EB), ("SB", uc.SB)):
        assert int(re.search(r"constexpr int %s = (\d+);" % name, src).group(1)) == want


@pytest.mark.parametrize("L", uc.COLLAPSE_L)
def test_collapse_columns_reach_their_depth_and_pop_their_count(L):
    depths = uc.collapse_depths(L)
    assert {1, L - 1, L} <= set(depths) and all(d in depths for d in (RC // 2, RC - 1, RC, RC + 1, RC + NRF) if d <= L)
    fam = uc.family("collapse_short" if L <= 26 else "collapse_long")
    for d in depths:
        for name, direction in ((f"collapse-L{L}-d{d}", "left"), (f"collapse-L{L}-d{d}/mirror", "right")):
            y = fam[name]
            assert len(y) == L + 6
            depth, popped = uc.depth_profile(y, direction)
            assert np.array_equal(depth[:L], 1 + np.arange(L)) and not popped[:L].any()  # every element its own block
            assert popped[L] == d and depth[L] == L - d + 1                              # the dip: exactly d blocks
            assert not popped[L + 1: L + 4].any() and depth[L + 3] == L - d + 4          # the rise to the peak pools nothing
            # the peak is the largest element and the split that ends the left fit there is optimal: the pooled block is emitted
            z = y if direction == "left" else y[::-1]
            assert np.argmax(z) == L + 3
            for nonneg in (False, True):
                total, split, fit = uc.split_margin(z, nonneg)[0]
                assert split in (L + 3, L + 4) and total > 0
                pooled = fit[L - d: L + 1]  # d blocks of the ramp and the dip
                assert len(pooled) == d + 1 and np.all(pooled == pooled[0]) and np.all(np.diff(fit[:L + 4]) >= 0)
                assert pooled[0] < fit[L + 1] and (d == L or fit[L - d - 1] < pooled[0])


def test_pause_columns_put_the_dip_at_the_pause_over_a_spilled_stack():
    fam = uc.family("collapse_short")
    for d in (1, RC + 1, uc.DIP_L):
        for where in (-1, 0, 1):
            y = fam[f"pause-d{d}-at{where:+d}"]
            m = len(y) // 2
            depth, popped = uc.depth_profile(y)
            assert m + where == uc.DIP_L and popped[uc.DIP_L] == d and not popped[:uc.DIP_L].any()
            # the stack phase A writes out at the pause (after element m - 1); ring and cached blocks hold RC + 2 of them
            if where >= 0:
                assert depth[m - 1] == m > RC + 2 + NRF  # phase C resumes over more spilled entries than one refill brings back
            else:
                assert depth[m - 1] == uc.DIP_L - d + 1  # the collapse was phase A's last element
            ym = fam[f"pause-d{d}-at{where:+d}/mirror"]
            assert np.array_equal(ym, y[::-1]) and len(ym) // 2 == m


def test_flank_pops_one_ramp_block_per_element_over_a_spilled_stack():
    for name, direction in (("flank", "left"), ("flank/mirror", "right")):
        y = uc.family("flank")[name]
        depth, popped = uc.depth_profile(y, direction)
        a, b, c, e = uc.FLANK_RAMP, uc.FLANK_RAMP + uc.FLANK_FALL, uc.FLANK_RAMP + uc.FLANK_FALL + uc.FLANK_RISE2, len(y) - 5
        assert (a, b, c, e) == (80, 140, 164, 184)
        assert np.array_equal(depth[:a], 1 + np.arange(a)) and depth[a - 1] - 2 - RC == 62  # entries in the spill area
        # 60 elements: the flank's own block and exactly ONE block of the ramp each - the ring loses one entry per element
        assert np.all(popped[a:b] == 2) and np.array_equal(depth[a:b], a - 1 - np.arange(b - a)) and depth[b - 1] == 20
        assert not popped[b:c].any() and depth[c - 1] == 44 and depth[c - 1] - 2 - RC > NRF  # spills again: the prefetch is void
        assert np.all(popped[c:e] == 2) and depth[e - 1] == 24
        assert not popped[e:e + 3].any()
        z = y if direction == "left" else y[::-1]
        for nonneg in (False, True):
            _, split, fit = uc.split_margin(z, nonneg)[0]
            assert np.argmax(z) == e + 2 and split in (e + 2, e + 3) and np.all(np.diff(fit[:e + 3]) >= 0) and len(np.unique(fit[a - 25: e])) < 8


def _check_tie_or_margin(name, y, nonneg):
    ranked = uc.split_margin(y, nonneg)
    n, ss = len(y), float(np.sum(y * y))
    best_total, best_split, best_fit = ranked[0]
    got = orc.unimodal_columns(y, nonneg, force_python=True)
    assert np.array_equal(got, best_fit), name  # the smallest split among the minima is the oracle's
    by_split = {t: (tot, fit) for tot, t, fit in ranked}
    if uc.is_tie(name):
        assert np.array_equal(y, y[::-1]), name
        for t in range(n + 1):
            assert by_split[t][0] == by_split[n - t][0], (name, t)  # bit-equal
            assert np.array_equal(by_split[t][1], by_split[n - t][1][::-1]), (name, t)
        if uc.is_flat(name):
            assert all(np.array_equal(fit, best_fit) for _, _, fit in ranked), name
            return "flat"
        near = [(tot, t, fit) for tot, t, fit in ranked if tot <= best_total + MARGIN * ss]
        assert all(tot == best_total for tot, _, _ in near), name        # the candidates tie EXACTLY ...
        assert len(near) < len(ranked) or n < 6
        mirror = best_fit[::-1]
        assert np.abs(best_fit - mirror).max() >= 0.25, name             # ... on two fits that differ
        assert all(np.array_equal(fit, best_fit) or np.array_equal(fit, mirror) for _, _, fit in near), name
        assert any(np.array_equal(fit, mirror) for _, _, fit in near), name
        m = n // 2
        assert min(t for _, t, _ in near) <= m < max(t for _, t, _ in near), name  # minima on either side of the pause
        # every pooled block of either fit has a power-of-two count: level and error are exact in any arithmetic
        runs = np.diff(np.concatenate([[0], np.nonzero(np.diff(best_fit))[0] + 1, [n]]))
        assert all(int(c) & (int(c) - 1) == 0 for c in runs), (name, runs)
        return "tie"
    for tot, t, fit in ranked:
        if np.abs(fit - best_fit).max() > 1e-6:
            assert tot > best_total + MARGIN * ss, (name, nonneg, t, tot, best_total, ss)
    return "margin"


@pytest.mark.parametrize("fam", uc.ALL_FAMILIES)
def test_every_column_is_an_exact_tie_or_has_a_margin(fam):
    kinds = set()
    for name, y in uc.family(fam).items():
        for nonneg in (False, True):
            kinds.add(_check_tie_or_margin(name, y, nonneg))
    assert kinds == ({"tie", "flat", "margin"} if fam == "ties" else {"tie", "margin"} if fam == "wave_span" else {"margin"})


def test_tie_minima_lie_in_different_quarters_of_the_split_search():
    """<2> scans i = n - 1 - split in four quarters of (n + 3) / 4 and combines them in ascending order"""
    apart = 0
    for name, y in uc.family("ties").items():
        if uc.is_tie(name) and not uc.is_flat(name):
            n = len(y)
            ranked = uc.split_margin(y, False)
            q = {(n - 1 - t) // ((n + 3) >> 2) for tot, t, _ in ranked if tot == ranked[0][0] and t < n}
            apart += len(q) > 1
    assert apart >= 8
    assert {len(y) % 4 for name, y in uc.family("ties").items() if name.startswith("tie-")} == {0, 1, 3}


def test_edge_columns_have_their_optimum_at_the_ends():
    fam = uc.family("edges")
    assert {len(y) for y in fam.values()} == set(uc.EDGE_N)
    for n in uc.EDGE_N:
        if n < 3:
            continue
        for shape, splits in (("dec", {0, 1}), ("peak_first", {1, 2}), ("peak_last", {n - 2, n - 1}), ("inc", {n - 1, n})):
            y = fam[f"edge-n{n}-{shape}"]
            assert y.min() < 0 <= y.max()
            ranked = uc.split_margin(y, False)
            assert {t for tot, t, _ in ranked if tot == ranked[0][0]} == splits and ranked[0][0] == 0.0


def test_oracle_forms_agree_bit_for_bit():
    if orc._oracle_lib() is None:
        pytest.skip("oracle C library not built (run __graft_entry__.build())")
    for name, y in uc.all_columns().items():
        for nonneg in (False, True):
            assert np.array_equal(orc.unimodal_columns(y, nonneg), orc.unimodal_columns(y, nonneg, force_python=True)), name


@pytest.mark.parametrize("force_python", [True, False])
def test_oracle_agrees_with_the_reference(force_python):
    if not force_python and orc._oracle_lib() is None:
        pytest.skip("oracle C library not built (run __graft_entry__.build())")
    g = load_npz("unimodal_edges.npz")
    assert sorted(g) == ["out", "out_nn", "ptr", "y"]
    cols = list(uc.all_columns().values())
    ptr = g["ptr"]
    assert len(ptr) == len(cols) + 1 and np.array_equal(g["y"], np.concatenate(cols))  # the fixture is of THESE columns
    for i, y in enumerate(cols):
        for nonneg, key in ((False, "out"), (True, "out_nn")):
            got = orc.unimodal_columns(y, nonneg, force_python=force_python)
            np.testing.assert_allclose(got, g[key][ptr[i]: ptr[i + 1]], rtol=0, atol=1e-13)


@pytest.mark.parametrize("fam,packing", uc.cases())
def test_problems_are_exact_sums_within_the_size_budget(fam, packing):
    p = uc.problem(fam, packing)
    Y, B, U, rp, r = p["Y"], p["B"], p["U"], p["row_ptr"], p["r"]
    assert B.dtype == np.float32 and U.dtype == np.float32
    assert np.array_equal((B + U).astype(np.float64), Y) and np.array_equal(B.astype(np.float64) + U.astype(np.float64), Y)
    assert np.array_equal(np.round(U * 64.0), U * 64.0) and np.abs(U).max() <= 1.0 and np.abs(Y).max() < 2.0 ** 10
    assert np.diff(rp).max() <= uc.MAX_SLAB and rp[-1] <= uc.MAX_ROWS and np.diff(rp).min() >= 1
    cols = dict(uc.fillers())
    cols.update(uc.family(fam))
    used = {name for s in p["names"] for name in s}
    if packing in uc.PACKINGS:  # every column of the family, and short edge columns in the slabs that fill the layout up
        assert set(uc.family(fam)) <= used <= set(cols)
    else:
        assert used == {k for k in cols if k.startswith("span-" if packing == "span_r3" else "inphase")}
    for i, s in enumerate(p["names"]):
        for c, name in enumerate(s):
            assert np.array_equal(Y[rp[i]: rp[i + 1], c], cols[name])


def test_layouts_have_the_lane_and_wave_counts_they_are_named_for():
    for fam in uc.FAMILIES:
        lanes = {k: (len(uc.problem(fam, k)["row_ptr"]) - 1) * uc.problem(fam, k)["r"] for k in uc.PACKINGS}
        assert lanes["r1_64k+1"] % 64 == 1 and lanes["r1_64k-1"] % 64 == 63
        assert [-(-lanes[k] // 64) for k in ("r17_5waves", "r17_6waves", "r17_7waves")] == [5, 6, 7]
    assert {uc.problem(f, k)["r"] for f in uc.FAMILIES for k in uc.PACKINGS} == {1, 3, 17, 64}
    assert {uc.problem(f, k)["unaligned"] for f, k in uc.cases()} == {False, True}
    # one wave spans slabs of 1 and of 300 rows
    p = uc.problem("wave_span", "span_r3")
    assert tuple(np.diff(p["row_ptr"])) == uc.SPAN_J == (1, 300, 2, 65, 1, 130) and p["r"] == 3 and len(uc.SPAN_J) * 3 <= 64
    # all 64 lanes of a wave carry the same collapse column, depth above RC + NRF
    p = uc.problem("wave_span", "inphase_r64")
    assert p["r"] == 64 and all(len(set(s)) == 1 for s in p["names"]) and len(p["names"]) == 2 * len(uc.INPHASE)
    depth, popped = uc.depth_profile(p["Y"][: p["row_ptr"][1], 0])
    assert depth.max() == 100 and popped[100] == RC + NRF
    # every lane of a wave another (L, d): the r = 1 layout of the collapse columns
    p = uc.problem("collapse_short", "r1_64k+1")
    first_wave = [s[0] for s in p["names"][:64]]
    assert len(set(first_wave)) == 64 and len({len(uc.family("collapse_short")[k]) for k in first_wave}) >= 8


def test_in_step_waves_take_every_refill_path():
    """the ring of a wave whose 64 lanes carry the same column (layout inphase_r64), modelled by uc.ring_events: each of the three
    refill paths of the kernel - cooperative from prefetched registers, cooperative with a load, per-lane inside a pooling loop
    (with and without prefetched entries) - is taken, in both sweep directions, and the resumed phase C refills from the
    stack the pause wrote out"""
    cols = uc.family("wave_span")
    for mirror, direction in (("", "left"), ("/mirror", "right")):
        ev = uc.ring_events(cols["inphase-flank" + mirror], direction)
        assert ev["spill"] >= 62 and ev["coop_load"] >= 2 and ev["coop_prefetched"] >= 4, ev  # the load: the first refill and the one after the second rise
        ev = uc.ring_events(cols["inphase-flank" + mirror], direction, coop=False)
        assert ev["dry_load"] >= 62 // (RC // 2) and ev["coop_load"] == ev["coop_prefetched"] == ev["dry_prefetched"] == 0, ev
        ev = uc.ring_events(cols["inphase-flank-collapse" + mirror], direction)
        assert ev["dry_prefetched"] >= 1 and ev["coop_prefetched"] >= 4, ev
        ev = uc.ring_events(cols["inphase-collapse" + mirror], direction)
        assert ev["spill"] >= 100 - 2 - RC and ev["dry_load"] >= 1, ev  # RC + NRF pops out of a full ring of RC
    # the pruned schedule: the left-to-right sweep pauses before element m and resumes with everything in the spill area
    for name, y in uc.family("collapse_short").items():
        if name.startswith("pause-") and not name.endswith("/mirror"):
            m = len(y) // 2
            ev, ev_dry = uc.ring_events(y, pause=m), uc.ring_events(y, pause=m, coop=False)
            if m <= uc.DIP_L:  # the dip is phase C's: over a stack that is all spilled
                assert ev["coop_load"] >= 1 and (ev_dry["dry_load"] >= 1 or "-d1-" in name), (name, ev, ev_dry)  # (one pop: the pushed top)
    # the dip pushes the cached top before it pools: L - 1 pushes.  The ring is exactly full at L = RC + 1, spills its first entry at
    # RC + 2 and has spilled NRF at RC + 1 + NRF
    for L, spills in ((RC, 0), (RC + 1, 0), (RC + 2, 1), (RC + 1 + NRF, NRF), (RC + 2 + NRF, NRF + 1)):
        y = uc.collapse(L, L) if L not in uc.COLLAPSE_L else uc.family("collapse_short")[f"collapse-L{L}-d{L}"]
        assert uc.ring_events(y)["spill"] == spills, L
