"""Inputs and fp64 references of the prox-kernel tests (csrc/slabprox.hip: k_slab_tv, k_slab_simplex, k_gl2_pass, k_gl2_value,
k_slab_colsq + k_rows_l2ball; csrc/rows.hip: k_rows_prox_rowsep, k_rows_dual; csrc/wide.hip: their k_wide_* forms).  Shared by the GPU tests
(tests/test_gpu_prox_kernels.py) and the CPU checks that the references solve the problems they stand for and that the inputs
leave the easy regime (tests/test_prox_cases_host.py).  No GPU, no torch.

Every input value is a float32: Y = B + U is designed on a grid (multiples of 2^-10, the 1e-3 column of 2^-20), U on the grid
of 2^-6, so B = Y - U and the sum B + U are exact in float32 AND in float64 - the kernels that add in fp32 (TV, L2 ball, the
row-separable kinds) and those that add in fp64 (simplex, GeneralizedL2) see the same Y."""
import functools

import numpy as np

from oracle import aoadmm_oracle as orc

J_RAGGED = (1, 2, 3, 15, 16, 17, 63, 64, 65, 130, 257)  # every 16-row block edge, the 64-row tile edge, a slab over several tiles
K = 8
# ranks per kind: 1, a non-multiple of 4, 16, one of 33 / 48 (the bucket that rounds up to NB = 4) and 64 for every kind; "16u" =
# rank 16 with aux / dual one float into a larger buffer (4-byte aligned only: the non-VEC row kernels at a rank divisible by 4)
RANKS = {"tv": (1, 3, 16, "16u", 17, 33, 64), "simplex": (1, 3, 16, "16u", 17, 48, 64),
         "l2ball": (1, 3, 4, 16, "16u", 32, 48, 64), "rowsep": (1, 3, 16, "16u", 17, 32, 33, 64)}
COLUMN_KINDS = ("zero", "const", "ints", "alternating", "ramp", "step", "gauss_1e3", "gauss_1e-3", "spike_last", "spike_first",
                "gauss")

PARAMS = {
    "tv": [{"kind": "tv", "reg_strength": 0.05, "l1_strength": 0.0}, {"kind": "tv", "reg_strength": 0.05, "l1_strength": 0.02}],
    "simplex": [{"kind": "simplex"}],
    "l2ball": [{"kind": "l2ball", "norm_bound": 0.75, "non_negativity": False},
               {"kind": "l2ball", "norm_bound": 0.75, "non_negativity": True}],
    "rowsep": [{"kind": "l1", "reg_strength": 0.05, "non_negativity": False},
               {"kind": "l1", "reg_strength": 0.02, "non_negativity": True},
               {"kind": "box", "min_val": 0.25, "max_val": 0.8},  # a minimum above 0: a padding lane that stores would show
               {"kind": "box", "min_val": None, "max_val": 0.8}, {"kind": "box", "min_val": 0.25, "max_val": None},
               {"kind": "nn"}],
}


def rank_of(rank):
    return 16 if rank == "16u" else int(rank)


def desc_id(d):
    return "-".join([d["kind"]] + [f"{k}={v}" for k, v in sorted(d.items()) if k not in ("kind", "norm_matrix")])


# ---- inputs -------------------------------------------------------------------------------------------------------------------------
def _grid(v, q):
    return np.round(np.asarray(v, dtype=np.float64) / q) * q


def column(kind, n, rng):
    """one designed column of Y (float64 holding float32 values on the grid)"""
    j = np.arange(n)
    g = rng.standard_normal(n)
    if kind == "zero":
        return np.zeros(n)
    if kind == "const":
        return np.full(n, 0.75)
    if kind == "ints":
        y = np.round(2.0 * g)  # ties; the largest entry stands alone, exactly 1 above the next: the simplex multiplier IS that next value
        y[n // 2] = y.max() + 1.0
        return y
    if kind == "alternating":
        return np.where(j % 2 == 0, 1.0, -1.0)
    if kind == "ramp":
        return _grid(np.linspace(-1.0, 2.0, n) if n > 1 else [0.5], 2.0 ** -10)
    if kind == "step":
        return np.where(j < (n + 1) // 2, -0.5, 1.5)
    if kind == "gauss_1e3":
        return _grid(1e3 * g, 2.0 ** -10)
    if kind == "gauss_1e-3":
        return _grid(1e-3 * g, 2.0 ** -20)
    if kind == "spike_last":
        y = _grid(0.25 * g, 2.0 ** -10)
        y[-1] = 5.0
        return y
    if kind == "spike_first":
        y = _grid(0.25 * g, 2.0 ** -10)
        y[0] = -5.0
        return y
    return _grid(g, 2.0 ** -10)


def column_kind(slab, col):
    """the kinds cycle through the columns, shifted from slab to slab: a rank-1 problem still meets all eleven"""
    return COLUMN_KINDS[(col + 4 * slab) % len(COLUMN_KINDS)]


def designed_Y(J, r, rng):
    return np.concatenate([np.stack([column(column_kind(i, c), int(n), rng) for c in range(r)], axis=1) for i, n in enumerate(J)])


def split_Y(Y, rng):
    """-> (B, U) float32 with B + U == Y exactly, in float32 and in float64"""
    U = np.round(0.1 * rng.standard_normal(Y.shape) * 64.0) / 64.0
    B = Y - U
    B32, U32 = B.astype(np.float32), U.astype(np.float32)
    assert np.array_equal(B32.astype(np.float64), B) and np.array_equal((B32 + U32).astype(np.float64), Y)
    return B32, U32


# log10 of the scale of the rows of A per slab: rho_i ~ a_i^2 then spans eight decades over the eleven slabs
_A_EXPONENT = np.linspace(-2.0, 2.0, 11)[[5, 3, 7, 1, 0, 9, 6, 4, 10, 8, 2]]


def rho_B(A, C, scale=1.0):
    """the B-phase feasibility penalties (decomposition.py:243-249) in fp64 from the float32 factors"""
    A, C = np.asarray(A, dtype=np.float64), np.asarray(C, dtype=np.float64)
    return 0.5 * scale * (A * A) @ np.sum(C * C, axis=0)


def ragged_problem(rank):
    """the 633 x 8 problem of the ragged kinds at `rank` -> dict of float32 arrays X, A, B, U, C, float64 Y = B + U, row_ptr, and
    the fp64 feasibility penalties rho of the B-phase ("16u" is the problem of rank 16: only the buffers differ)"""
    return _ragged_problem(rank_of(rank))


@functools.lru_cache(maxsize=None)
def _ragged_problem(r):
    rng = np.random.RandomState(1000 + r)
    J = np.asarray(J_RAGGED)
    row_ptr = np.concatenate([[0], np.cumsum(J)]).astype(np.int64)
    Y = designed_Y(J, r, rng)
    B, U = split_Y(Y, rng)
    A = ((10.0 ** _A_EXPONENT)[:, None] * (rng.rand(len(J), r) + 0.5) / np.sqrt(r)).astype(np.float32)
    C = rng.rand(K, r).astype(np.float32)
    X = rng.rand(int(row_ptr[-1]), K).astype(np.float32)
    out = dict(X=X, A=A, B=B, U=U, C=C, Y=Y, row_ptr=row_ptr, rho=rho_B(A, C))
    for v in out.values():
        v.setflags(write=False)
    return out


# ---- GeneralizedL2 ---------------------------------------------------------------------------------------------------------------------
GL2_N = (1, 16, 17, 64, 65, 130)
GL2_RANKS = (1, 4, 5, 17, 64)
GL2_SLABS = 3


def norm_matrix(which, n):
    if which == "laplacian":  # the path Laplacian: singular (constants cost nothing)
        M = 2.0 * np.eye(n) - np.eye(n, k=1) - np.eye(n, k=-1)
        M[0, 0] = M[-1, -1] = 1.0
        if n == 1:
            M[0, 0] = 0.0
        return 0.3 * M
    W = np.random.RandomState(77 + n).standard_normal((n, max(n // 2, 1)))  # random PSD of rank n / 2
    M = W @ W.T / n
    return 0.5 * (M + M.T)


def native_matrix(M):
    """[U | s | U^T] as GeneralizedL2Penalty._native_matrix builds it, and n"""
    from matcouply_amd import penalties as pen

    return pen.GeneralizedL2Penalty(M, validate=False)._native_matrix()


@functools.lru_cache(maxsize=None)
def gl2_problem(n, rank, which):
    rng = np.random.RandomState(2000 + 100 * n + rank)
    J = np.full(GL2_SLABS, n)
    row_ptr = np.concatenate([[0], np.cumsum(J)]).astype(np.int64)
    Y = designed_Y(J, rank, rng)
    B, U = split_Y(Y, rng)
    A = ((10.0 ** np.array([-2.0, 0.0, 2.0]))[:, None] * (rng.rand(GL2_SLABS, rank) + 0.5) / np.sqrt(rank)).astype(np.float32)
    C = rng.rand(K, rank).astype(np.float32)
    X = rng.rand(int(row_ptr[-1]), K).astype(np.float32)
    out = dict(X=X, A=A, B=B, U=U, C=C, Y=Y, row_ptr=row_ptr, rho=rho_B(A, C), M=norm_matrix(which, n))
    for v in out.values():
        v.setflags(write=False)
    return out


# ---- one inner iteration of a whole phase ------------------------------------------------------------------------------------------
PHASE_SHAPES = ((1, 3), (17, 17), (64, 16), (65, 33), (130, 64))  # (rows of the factor = K or I, rank): modes 2 and 0
PHASE_B = ((None, 4), (None, 17), (65, 5), (130, 17))             # (n, rank) of mode 1: the ragged slabs, or three slabs of n rows


@functools.lru_cache(maxsize=None)
def phase_problem(mode, size, rank):
    """a problem whose mode-`mode` factor has `size` rows in one slab (mode 1: the slabs of J_RAGGED when size is None, else three
    slabs of `size` rows) -> float32 X, A, B, C, aux0, dual0 of that mode, row_ptr, and `slabs`: the row_ptr of the mode's slabs.
    aux0 carries the designed columns, dual0 is small (at most 1 / 16): the factor the solve returns then adds the designed
    patterns to the sum F + U at the slabs of large rho, and |F| <= |F + U| + 1 / 16."""
    rng = np.random.RandomState(3000 + 1000 * mode + 7 * (size or 0) + rank)
    if mode == 1:
        J = np.asarray(J_RAGGED) if size is None else np.full(GL2_SLABS, size)
        Kk = K
    elif mode == 2:
        J, Kk = np.array([5, 9, 7]), size
    else:
        J, Kk = 2 + np.arange(size) % 3, K
    row_ptr = np.concatenate([[0], np.cumsum(J)]).astype(np.int64)
    I, N = len(J), int(row_ptr[-1])
    slabs = row_ptr if mode == 1 else np.array([0, (Kk if mode == 2 else I)], dtype=np.int64)
    exponent = _A_EXPONENT if (mode == 1 and size is None) else (np.array([-2.0, 0.0, 2.0]) if mode == 1 else np.zeros(I))
    A = ((10.0 ** exponent)[:, None] * (rng.rand(I, rank) + 0.5) / np.sqrt(rank)).astype(np.float32)
    B = rng.standard_normal((N, rank)).astype(np.float32)
    C = rng.rand(Kk, rank).astype(np.float32)
    X = rng.rand(N, Kk).astype(np.float32)
    aux0 = designed_Y(np.diff(slabs), rank, rng).astype(np.float32)
    dual0 = (np.round(0.1 * rng.standard_normal(aux0.shape) * 64.0) / 512.0).astype(np.float32)
    out = dict(X=X, A=A, B=B, C=C, aux0=aux0, dual0=dual0, row_ptr=row_ptr, slabs=slabs)
    for v in out.values():
        v.setflags(write=False)
    return out


def gl2_value(F, row_ptr, M):
    """trace(F_i^T M F_i) summed over the slabs, fp64"""
    F = np.asarray(F, dtype=np.float64)
    return float(sum(np.sum(F[s:e] * (M @ F[s:e])) for s, e in zip(row_ptr[:-1], row_ptr[1:])))


# ---- references -----------------------------------------------------------------------------------------------------------------------
def reference(desc, Y, row_ptr, rho):
    """prox of `desc` on every slab of the packed fp64 Y at the slab's rho (oracle/aoadmm_oracle.py), fp64"""
    Y = np.asarray(Y, dtype=np.float64)
    rho = np.broadcast_to(np.asarray(rho, dtype=np.float64), (len(row_ptr) - 1,))
    return np.concatenate([orc.prox_matrix(desc, Y[s:e].copy(), float(rho[i])) for i, (s, e) in enumerate(zip(row_ptr[:-1], row_ptr[1:]))])


def threshold(desc, rho):
    """the largest constant the prox of `desc` adds to or compares with its input at feasibility penalty rho"""
    kind = desc["kind"]
    if kind == "tv":
        return max(2.0 * desc["reg_strength"], desc.get("l1_strength", 0.0)) / rho
    if kind == "l1":
        return desc["reg_strength"] / rho
    if kind == "l2ball":
        return desc["norm_bound"]
    if kind == "box":
        return max(abs(v) for v in (desc["min_val"], desc["max_val"]) if v is not None)
    return 0.0


def column_scale(desc, Y, row_ptr, rho):
    """max(1, max |Y| of the slab column, threshold) for every element of the packed Y: the unit of the error bars"""
    Y = np.asarray(Y, dtype=np.float64)
    rho = np.broadcast_to(np.asarray(rho, dtype=np.float64), (len(row_ptr) - 1,))
    out = np.empty_like(Y)
    for i, (s, e) in enumerate(zip(row_ptr[:-1], row_ptr[1:])):
        if e > s:
            out[s:e] = np.maximum(np.maximum(np.abs(Y[s:e]).max(axis=0), threshold(desc, float(rho[i]))), 1.0)[None, :]
    return out


# ---- optimality conditions of the problems (not of the algorithms) -------------------------------------------------------------------------
def _tv_kkt(x, y, lam, tol=1e-9):
    u = np.cumsum(x - y)           # -u[:-1] is the dual variable of the differences
    assert abs(u[-1]) < tol * max(1.0, np.abs(x).sum())
    s, d = -u[:-1], np.diff(y)
    assert np.all(np.abs(s) <= lam + tol)
    assert np.all(np.abs(s[d > 1e-12] - lam) < 1e-7) and np.all(np.abs(s[d < -1e-12] + lam) < 1e-7)


def check_tv(desc, Y, Z, rho):
    """Z = soft(tv(Y, 2 alpha / rho), l1 / rho) for one slab: the dual-variable system of the TV problem, then the threshold"""
    lam, l1 = 2.0 * desc["reg_strength"] / rho, desc.get("l1_strength", 0.0) / rho
    T = orc.tv_columns(Y, lam)
    for c in range(Y.shape[1]):
        if Y.shape[0] == 1:
            assert abs(T[0, c] - Y[0, c]) <= 1e-15 * max(abs(Y[0, c]), lam)  # (y - lam) + lam, rounded twice
        else:
            _tv_kkt(Y[:, c], T[:, c], lam)
    check_l1(T, Z, l1, False)


def check_l1(Y, Z, thr, nonneg):
    """Z = argmin 1/2 |z - y|^2 + thr |z| (over z >= 0 when nonneg): y - z is thr times a subgradient of |z|"""
    tol = 1e-12 * np.maximum(1.0, np.abs(Y))
    on = Z != 0
    if nonneg:
        assert np.all(Z >= 0) and np.all(np.abs((Y - Z)[on] - thr) <= tol[on]) and np.all((Y <= thr + tol)[~on])
    else:
        assert np.all(np.abs((Y - Z)[on] - thr * np.sign(Z[on])) <= tol[on]) and np.all((np.abs(Y) <= thr + tol)[~on])


def check_box(Y, Z, lo, hi):
    lo, hi = (-np.inf if lo is None else lo), (np.inf if hi is None else hi)
    assert np.all(Z >= lo) and np.all(Z <= hi)
    assert np.all(Z[(Y >= lo) & (Y <= hi)] == Y[(Y >= lo) & (Y <= hi)]) and np.all(Z[Y < lo] == lo) and np.all(Z[Y > hi] == hi)


def check_simplex(Y, Z):
    """non-negative, sums to 1, ONE multiplier on the active set, inactive entries at or below it -> (mu, active count) per column"""
    n, r = Y.shape
    tol = 1e-12 * max(1.0, float(np.abs(Y).max()))
    assert np.all(Z >= 0) and np.all(np.abs(Z.sum(axis=0) - 1.0) <= n * tol)
    mus, counts = [], []
    for c in range(r):
        on = Z[:, c] > 0
        assert on.any()
        mu = (Y[on, c] - Z[on, c])
        assert mu.max() - mu.min() <= 2 * tol and np.all(Y[~on, c] <= mu.min() + 2 * tol)
        mus.append(float(mu.mean())), counts.append(int(on.sum()))
    return np.array(mus), np.array(counts)


def check_l2ball(desc, Y, Z):
    """unchanged inside, norm equals the bound outside, direction preserved -> True per column that lies outside the ball"""
    bound = desc["norm_bound"]
    P = np.maximum(Y, 0.0) if desc.get("non_negativity", False) else Y
    nrm, nz = np.sqrt(np.sum(P * P, axis=0)), np.sqrt(np.sum(Z * Z, axis=0))
    outside = nrm > bound
    assert np.array_equal(Z[:, ~outside], P[:, ~outside])
    assert np.all(np.abs(nz[outside] - bound) <= 1e-13 * bound)
    assert np.all(np.abs(Z[:, outside] * nrm[outside] - P[:, outside] * bound) <= 1e-12 * np.maximum(1.0, np.abs(P[:, outside])) * nrm[outside])
    return outside


def check_gl2(M, Y, Z, rho):
    want = np.linalg.solve(M + 0.5 * rho * np.eye(len(M)), 0.5 * rho * Y)
    assert np.abs(Z - want).max() <= 1e-11 * max(1.0, float(np.abs(Y).max()))
