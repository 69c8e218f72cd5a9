"""The fixtures and references of tests/polar_cases.py, checked without a GPU: every designed slab is well-posed (its achieved
conditioning is the designed one, no singular value sits where the routes' thresholds would make the expected route a matter
of rounding, the reference polar factor is a partial isometry, and the SVD reference agrees with the Gram route where the
latter is accurate), every route is met at every rank it exists at, and no slab but the ones named is left out of a comparison.
Prints the table of emulated errors the bars of tests/test_gpu_pf2_polar.py come from."""
import numpy as np
import pytest

from tests import polar_cases as pc

EPS = 2.0 ** -52


def _fixtures():
    out = [(f"main-{rank}", rank, pc.main_problem(rank)) for rank in pc.RANKS if rank != "16u"]
    out += [(f"{which}-{rank}", rank, pc.special_problem(rank, which)) for rank in pc.SPECIAL_RANKS for which in ("diag", "zero")]
    out += [(f"clamp-{n}-{last}", pc.CLAMP_RANK, pc.clamp_problem(n, last)) for n in pc.CLAMP_I for last in ("ns", "short")]
    out += [(f"stale-{rank}-{name}", rank, p) for rank in pc.STALE_RANKS for name, p in zip(("easy", "hard"), pc.stale_problems(rank))]
    out.append(("many-4", 4, pc.many_slabs_problem()))
    return out


FIXTURES = _fixtures()
_REF = {}


def _ref(name, p):
    if name not in _REF:
        ref = pc.reference(p["B"], p["U"], p["Delta"], p["row_ptr"], p["rho"])
        _REF[name] = (ref, pc.emulated_error(ref, p["Delta"], p["row_ptr"]))
    return _REF[name]


@pytest.mark.parametrize("name,rank,p", FIXTURES, ids=[f[0] for f in FIXTURES])
def test_fixture_is_well_posed(name, rank, p):
    r = pc.rank_of(rank)
    ref, emu = _ref(name, p)
    B, U, D = p["B"], p["U"], p["Delta"]
    assert B.dtype == U.dtype == D.dtype == np.float32 and np.all(p["rho"] > 0) and np.all(p["A"] > 0) and np.all(p["C"] > 0)
    assert p["X"].shape[1] == max(r, 8)
    sd = np.linalg.svd(D.astype(np.float64), compute_uv=False)
    assert 1.0 <= sd.min() and sd.max() <= 2.0, sd
    for i, ((J, cond, kind), s, e) in enumerate(zip(p["slabs"], p["row_ptr"][:-1], p["row_ptr"][1:])):
        assert e - s == J
        if kind == "zero":
            assert not ref["Y"][s:e].any() and ref["kept"][i] == 0 and not ref["P"][s:e].any()
            continue
        assert not (3e4 <= cond < 1e6), "a target at the route thresholds (1e5)"
        k = min(J, r) - (2 if kind == "deficient_tall" else 0)
        assert ref["kept"][i] == k, (name, i, ref["kept"][i], k)
        target = cond if k > 1 else 1.0  # (one singular value)
        assert target / 2.0 <= ref["cond"][i] <= 2.0 * target, (name, i, ref["cond"][i], cond)
        rel = ref["sigma"][i] / ref["sigma"][i][0]
        qr_full = cond >= 1e6 and kind == "full" and J >= r
        if J < r and cond >= 1e6:  # the slab of the pseudo-inverse threshold (polar_cases.special_slabs): a decade off either side
            assert name.startswith("diag") and rel.min() > 5e-7 and np.sum(rel < 1e-5) >= 1
        elif not qr_full:
            assert not np.any((rel > 1e-12) & (rel < 1e-5)), (name, i, rel)
        else:
            assert rel.min() > 1e-8  # full rank: above the pseudo-inverse threshold of k_pf2_polar_qr by six decades
        if kind == "deficient_tall":  # exactly rank-deficient: Y_i Delta^T has two zero columns
            assert J >= r and np.sum(~(ref["Y"][s:e] @ D.astype(np.float64).T).any(axis=0)) == 2
        sv = np.linalg.svd(ref["P"][s:e], compute_uv=False)
        assert np.abs(sv[:k] - 1.0).max() <= 1e-12 and (k == len(sv) or sv[k:].max() <= 1e-12)  # P_i^T P_i = a projector of rank k
        G = ref["P"][s:e].T @ ref["P"][s:e]
        assert np.abs(G @ G - G).max() <= 1e-12
        if cond <= 1e4:
            assert emu["eG"][i] <= 100.0 * EPS * max(ref["cond"][i], 1.0) ** 2, (name, i, emu["eG"][i])
        # the stored pair holds Y: B = fp32(Y), U = fp32(Y - B)
        assert np.array_equal(ref["Y"][s:e].astype(np.float32), B[s:e])


def test_every_route_is_met_and_no_slab_is_left_out():
    left_out = 0
    for name, rank, p in FIXTURES:
        for variant in ("default", "jacobi"):
            routes = [pc.route(rank, s, variant) for s in p["slabs"]]
            if name.startswith("main") and pc.rank_of(rank) > 1:
                conds = {(rt, s[1]) for rt, s in zip(routes, p["slabs"])}
                gram = "ns" if (pc.rank_of(rank) <= 32 and variant == "default") else "jacobi"
                assert (gram, 1e4) in conds and (gram, 1.0) in conds and ("qr", 1e6) in conds and ("qr", 1e7) in conds, (name, conds)
                assert any(rt == "jacobi" and s[0] < pc.rank_of(rank) and s[1] >= 1e3 for rt, s in zip(routes, p["slabs"]))
        left_out += int(np.sum(~pc.compared(rank, p["slabs"])))
    # ... and the cond-1e7 slab of the 65-slab rank-4 problem under the fast kernels
    many = pc.many_slabs_problem()
    assert len(many["slabs"]) == 65 and np.sum(~pc.compared(4, many["slabs"], qr_launched=False)) == 1
    assert left_out == len(pc.SPECIAL_RANKS)  # the all-zero slabs
    for rank in pc.RANKS:  # the J edges of k_pf2_gram at every rank
        Js = {s[0] for s in pc.slab_list(rank)}
        r = pc.rank_of(rank)
        assert set(pc.J_EDGES) <= Js and {1, r, r + 1} <= Js and (r <= 2 or r - 1 in Js)
        assert sum(s[0] for s in pc.slab_list(rank)) <= 1300
    for n in pc.CLAMP_I:  # the last slab: once Newton-Schulz, once the in-kernel Jacobi
        assert pc.route(pc.CLAMP_RANK, pc.clamp_problem(n, "ns")["slabs"][-1]) == "ns" and len(pc.clamp_problem(n, "ns")["slabs"]) == n
        assert pc.route(pc.CLAMP_RANK, pc.clamp_problem(n, "short")["slabs"][-1]) == "jacobi"


def test_emulated_error_table():
    """the table the bars come from (printed with -s): per fixture and target cond the range of e32 and eG, and the ratio of
    the rigorous componentwise bound to e32"""
    rows = {}
    for name, rank, p in FIXTURES:
        if not name.startswith("main"):
            continue
        ref, emu = _ref(name, p)
        for i, (J, cond, kind) in enumerate(p["slabs"]):
            print(f"rank {rank:>3} J {J:>3} cond {cond:7.0e}: e32 {emu['e32'][i]:.2e}  eG {emu['eG'][i]:.2e}  rigorous / e32 "
                  f"{emu['rigorous'][i] / max(emu['e32'][i], 1e-300):6.1f}")
            if min(J, pc.rank_of(rank)) > 1:
                rows.setdefault(cond, []).append((emu["e32"][i], emu["eG"][i]))
    for cond in sorted(rows):
        e32, eG = np.array(rows[cond]).T
        print(f"cond {cond:7.0e}: e32 {e32.min():.1e} .. {e32.max():.1e}   eG {eG.min():.1e} .. {eG.max():.1e}")
        # the fp32 storage of T_i in front of the conditioning: 2^-24 cond within a factor 30 either way
        assert e32.min() >= pc.HALF_ULP * cond / 30.0 and e32.max() <= 30.0 * pc.HALF_ULP * cond, (cond, e32.min(), e32.max())
    bar = pc.p_bar(dict(e32=np.array([1e-9]), eG=np.array([1.0])), np.array([False]))
    assert bar[0] == 8.0 * pc.HALF_ULP  # the floor, and eG does not count for a QR slab


def test_delta_and_dual_of_the_reference():
    """Delta_new is the weighted mean of P_i^T Y_i and symmetric positive semi-definite in the coordinates of Delta (P_i^T Y_i
    Delta^T = (A_i^T A_i)^1/2); the dual is what k_rows_pf2_dual forms"""
    for name, rank, p in FIXTURES[:6]:
        ref, emu = _ref(name, p)
        H = ref["Delta_new"] @ p["Delta"].astype(np.float64).T
        assert np.abs(H - H.T).max() <= 1e-9 * max(1.0, np.abs(H).max()) and np.linalg.eigvalsh(0.5 * (H + H.T)).min() >= -1e-9
        want = p["U"].astype(np.float64) + p["B"].astype(np.float64) - ref["P"] @ ref["Delta_new"]
        assert np.abs(ref["dual"] - want).max() <= 1e-13 * max(1.0, np.abs(want).max())
        gram = np.array([pc.route(rank, s) != "qr" for s in p["slabs"]])
        assert pc.delta_bar(ref, emu, p["rho"], p["row_ptr"], gram) < 1e-5  # the Gram term stays far below the data
