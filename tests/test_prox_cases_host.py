"""The inputs and references of tests/prox_cases.py, checked without a GPU: every reference the GPU tests compare a kernel with
satisfies the optimality conditions of ITS PROBLEM on exactly those inputs (never the restated algorithm), the product's host
prox methods agree with the references, and the inputs reach the regimes a green GPU run is meant to have covered - rho is
the fp64 value of the formula here; the GPU tests check the device's rho against it before they use it."""
import numpy as np
import pytest

from tests import prox_cases as pc

ALL_RANKS = sorted({pc.rank_of(r) for ranks in pc.RANKS.values() for r in ranks})


def _slabs(p):
    return list(zip(p["row_ptr"][:-1], p["row_ptr"][1:]))


def test_inputs_are_exact_float32_sums():
    for rank in ALL_RANKS:
        p = pc.ragged_problem(rank)
        B, U, Y = p["B"], p["U"], p["Y"]
        assert B.dtype == np.float32 and U.dtype == np.float32
        assert np.array_equal((B + U).astype(np.float64), Y) and np.array_equal(B.astype(np.float64) + U.astype(np.float64), Y)
        rho = p["rho"]
        assert rho.max() / rho.min() > 1e7 and len(rho) == len(pc.J_RAGGED) == 11 and p["row_ptr"][-1] == 633
        kinds = {pc.column_kind(i, c) for i in range(len(rho)) for c in range(rank)}
        assert kinds == set(pc.COLUMN_KINDS)


@pytest.mark.parametrize("rank", sorted({pc.rank_of(r) for r in pc.RANKS["tv"]}))
@pytest.mark.parametrize("desc", pc.PARAMS["tv"], ids=pc.desc_id)
def test_tv_reference_is_optimal_and_leaves_the_easy_regime(rank, desc):
    from matcouply_amd import penalties as pen

    p = pc.ragged_problem(rank)
    Y, rho = p["Y"], p["rho"]
    Z = pc.reference(desc, Y, p["row_ptr"], rho)
    host = pen.TotalVariationPenalty(desc["reg_strength"], l1_strength=desc["l1_strength"])
    collapsed = spread = thresholded = 0
    for i, (s, e) in enumerate(_slabs(p)):
        pc.check_tv(desc, Y[s:e], Z[s:e], rho[i])
        got = np.asarray(host.factor_matrix_update(Y[s:e].copy(), rho[i], None))
        assert np.abs(got - Z[s:e]).max() <= 1e-12 * max(1.0, np.abs(Y[s:e]).max())
        if e - s < 3:
            continue  # (a slab of one or two rows meets both conditions trivially)
        T = pc.orc.tv_columns(Y[s:e], 2.0 * desc["reg_strength"] / rho[i])
        for c in range(rank):
            distinct = len(np.unique(T[:, c]))
            collapsed += distinct == 1 and len(np.unique(Y[s:e, c])) > 1   # a column that was not constant to begin with
            spread += 2 * distinct >= e - s
            thresholded += bool(np.any(Z[s:e, c] != T[:, c]))
    assert collapsed >= 1 and spread >= 1, (collapsed, spread)
    assert (thresholded >= 1) == (desc["l1_strength"] > 0)


@pytest.mark.parametrize("rank", sorted({pc.rank_of(r) for r in pc.RANKS["simplex"]}))
def test_simplex_reference_is_optimal_and_leaves_the_easy_regime(rank):
    from matcouply_amd import penalties as pen

    p = pc.ragged_problem(rank)
    Y = p["Y"]
    desc = pc.PARAMS["simplex"][0]
    Z = pc.reference(desc, Y, p["row_ptr"], 1.0)
    vertex = full = tied = 0
    for s, e in _slabs(p):
        mu, count = pc.check_simplex(Y[s:e], Z[s:e])
        got = np.asarray(pen.UnitSimplex().factor_matrix_update(Y[s:e].copy(), 1.0, None))
        assert np.abs(got - Z[s:e]).max() <= 1e-12 * max(1.0, np.abs(Y[s:e]).max())
        if e - s >= 3:
            vertex += int(np.sum(count == 1))
            full += int(np.sum(count == e - s))
            tied += int(np.sum(np.any((np.abs(Y[s:e] - mu[None, :]) <= 1e-12) & (Z[s:e] == 0), axis=0)))  # entries AT the root
    assert vertex >= 1 and full >= 1, (vertex, full)
    assert tied >= 1


@pytest.mark.parametrize("rank", sorted({pc.rank_of(r) for r in pc.RANKS["l2ball"]}))
@pytest.mark.parametrize("desc", pc.PARAMS["l2ball"], ids=pc.desc_id)
def test_l2ball_reference_is_optimal_and_leaves_the_easy_regime(rank, desc):
    from matcouply_amd import penalties as pen

    p = pc.ragged_problem(rank)
    Y = p["Y"]
    Z = pc.reference(desc, Y, p["row_ptr"], 1.0)
    host = pen.L2Ball(desc["norm_bound"], non_negativity=desc["non_negativity"])
    inside_nonzero = outside = zero_inside = 0
    for i, (s, e) in enumerate(_slabs(p)):
        out = pc.check_l2ball(desc, Y[s:e], Z[s:e])
        got = np.asarray(host.factor_matrix_update(Y[s:e].copy(), 1.0, None))
        assert np.abs(got - Z[s:e]).max() <= 1e-12 * max(1.0, np.abs(Y[s:e]).max())
        outside += int(out.sum())
        for c in np.nonzero(~out)[0]:
            if pc.column_kind(i, c) == "zero":
                zero_inside += 1
            elif np.any(Z[s:e, c] != 0):
                inside_nonzero += 1  # strictly inside, and not the trivial zero
    assert outside >= 1 and zero_inside >= 1 and inside_nonzero >= 1, (outside, zero_inside, inside_nonzero)


@pytest.mark.parametrize("rank", sorted({pc.rank_of(r) for r in pc.RANKS["rowsep"]}))
@pytest.mark.parametrize("desc", pc.PARAMS["rowsep"], ids=pc.desc_id)
def test_rowsep_reference_is_optimal_and_leaves_the_easy_regime(rank, desc):
    from matcouply_amd import penalties as pen

    p = pc.ragged_problem(rank)
    Y, rho = p["Y"], p["rho"]
    Z = pc.reference(desc, Y, p["row_ptr"], rho)
    kind = desc["kind"]
    host = {"nn": lambda: pen.NonNegativity(), "box": lambda: pen.Box(desc["min_val"], desc["max_val"]),
            "l1": lambda: pen.L1Penalty(desc["reg_strength"], non_negativity=desc["non_negativity"])}[kind]()
    sides = {}  # threshold -> [entries below it, entries above it]

    def count(name, below, above):
        got = sides.setdefault(name, [0, 0])
        got[0], got[1] = got[0] + int(below), got[1] + int(above)

    for i, (s, e) in enumerate(_slabs(p)):
        y, z = Y[s:e], Z[s:e]
        got = np.asarray(host.factor_matrix_update(y.copy(), rho[i], None))
        assert np.abs(got - z).max() <= 1e-12 * max(1.0, np.abs(y).max())
        if kind == "nn":
            pc.check_box(y, z, 0.0, None)
            count("zero", np.sum(y < 0), np.sum(y > 0))
        elif kind == "box":
            pc.check_box(y, z, desc["min_val"], desc["max_val"])
            for name in ("min_val", "max_val"):
                if desc[name] is not None:
                    count(name, np.sum(y < desc[name]), np.sum(y > desc[name]))
        else:
            thr = desc["reg_strength"] / rho[i]
            pc.check_l1(y, z, thr, desc["non_negativity"])
            count("thr", np.sum((y < thr) & (y > 0)), np.sum(y > thr))
            if not desc["non_negativity"]:
                count("-thr", np.sum(y < -thr), np.sum((y > -thr) & (y < 0)))
    assert sides and all(min(v) >= 1 for v in sides.values()), sides


@pytest.mark.parametrize("n", pc.GL2_N)
@pytest.mark.parametrize("rank", pc.GL2_RANKS)
@pytest.mark.parametrize("which", ["laplacian", "random_psd"])
def test_gl2_reference_is_the_direct_solve(n, rank, which):
    from matcouply_amd import penalties as pen

    p = pc.gl2_problem(n, rank, which)
    M, Y, rho = p["M"], p["Y"], p["rho"]
    assert np.array_equal(M, M.T) and np.linalg.eigvalsh(M).min() > -1e-13
    if which == "laplacian":
        assert np.abs(M @ np.ones(n)).max() < 1e-15  # singular
    else:
        assert np.linalg.matrix_rank(M) <= max(n // 2, 1)
    desc = {"kind": "gl2", "norm_matrix": M}
    Z = pc.reference(desc, Y, p["row_ptr"], rho)
    host = pen.GeneralizedL2Penalty(M, validate=False)
    for i, (s, e) in enumerate(_slabs(p)):
        pc.check_gl2(M, Y[s:e], Z[s:e], rho[i])
        got = np.asarray(host.factor_matrix_update(Y[s:e].copy(), rho[i], None))
        assert np.abs(got - Z[s:e]).max() <= 1e-11 * max(1.0, np.abs(Y[s:e]).max())
    # [U | s | U^T] of the native kernel reproduces M, and the value through it is trace(F^T M F)
    mat, nm = pc.native_matrix(M)
    U, sv, UT = mat[:n * n].reshape(n, n), mat[n * n:n * n + n], mat[n * n + n:].reshape(n, n)
    assert nm == n and np.array_equal(UT, U.T) and np.abs((U * sv) @ U.T - M).max() < 1e-13
    B = p["B"].astype(np.float64)
    T = np.concatenate([U.T @ B[s:e] for s, e in _slabs(p)])
    val = pc.gl2_value(B, p["row_ptr"], M)
    assert abs(float(np.sum(np.tile(sv, pc.GL2_SLABS)[:, None] * T * T)) - val) <= 1e-12 * max(1.0, abs(val))
