"""Inputs and fp64 references of the PARAFAC2 polar-factor tests (csrc/pf2polar.hip: k_pf2_gram, k_pf2_algebra_ns, k_pf2_algebra,
k_pf2_polar_qr, k_pf2_sum, k_pf2_delta; csrc/rows.hip: k_pf2_apply, k_rows_pf2_dual; csrc/wide.hip: their fp64-state forms).
Shared by the GPU tests (tests/test_gpu_pf2_polar.py) and the CPU checks that the fixtures are well-posed and reach the routes
they are designed for (tests/test_polar_cases_host.py).  numpy only: no GPU, no torch.

A slab is DESIGNED: A_i = Y_i Delta^T = Q_i diag(sigma) R_i^T with log-spaced singular values from 1 down to 1 / cond, and
Y_i = A_i Delta^-T is stored as the two floats the kernels add exactly in fp64, B = fp32(Y) and U = fp32(Y - B): the conditioning
survives the storage (the pair holds Y to 2^-48).  The prox (penalties.py:1224-1250, 1280-1281):
    P_i = polar(Y_i Delta^T),   Delta_new = sum rho_i P_i^T Y_i / sum rho_i,   dual = B - (P Delta_new - U)."""
import functools

import numpy as np

HALF_ULP = 2.0 ** -24
RANKS = (1, 3, 16, "16u", 17, 32, 33, 45, 46, 51, 52, 63, 64)
J_EDGES = (15, 16, 17, 63, 64, 65, 130, 257)   # the 16-row rounds of k_pf2_gram, its j < e guard, its four-wave merge
GRAM_CONDS = (1.0, 10.0, 1e3, 1e4)             # the Gram routes (Newton-Schulz, Jacobi)
QR_CONDS = (1e6, 1e7)                          # flagged 2 and redone by k_pf2_polar_qr (full rank, J >= r only)
SPECIAL_RANKS = (3, 17, 33)                    # the diagonal-Delta engine (deficient_tall) and the engine with an all-zero slab
JACOBI_RANKS = (3, 16, 17, 32)                 # MCL_PF2_JACOBI=1: Jacobi against Newton-Schulz on the same data
PLAIN_RANKS = (16, 32)                         # MCL_NS_PLAIN=1
SVD_KEEP = 1e-7                                # singular values kept: the device's 1e-14 on the eigenvalues of the Gram matrix
J_RAGGED = (1, 2, 3, 15, 16, 17, 63, 64, 65, 130, 257)


def rank_of(rank):
    return 16 if rank == "16u" else int(rank)


def slab_list(rank):
    """the (J, target cond, kind) of the main engine of `rank`: J from {1, r - 1, r, r + 1} and J_EDGES with the Gram conds in
    turn (the turn starts at another cond on each side of J = r, so both sides meet 1e4), then two full-rank QR slabs"""
    r = rank_of(rank)
    Js = sorted({j for j in (1, r - 1, r, r + 1) + J_EDGES if j >= 1})
    out, n_short, n_tall = [], 0, 0
    for J in Js:
        if J < r:
            cond = GRAM_CONDS[(3 + n_short) % 4]
            n_short += J > 1  # (a one-row slab has one singular value: cond 1 whatever the target)
        else:
            cond = GRAM_CONDS[(3 + n_tall) % 4]
            n_tall += 1
        out.append((J, cond if min(J, r) > 1 else 1.0, "full"))
    if r > 1:
        tall = [j for j in Js if j >= r]
        out.append((tall[1], QR_CONDS[0], "full"))
        out.append((tall[min(4, len(tall) - 1)], QR_CONDS[1], "full"))
    return out


def special_slabs(rank, which):
    """the short engines of SPECIAL_RANKS: `diag` (Delta a diagonal of powers of two, one deficient_tall slab) and `zero` (one
    all-zero slab).  The diag engine also holds the one slab on which the pseudo-inverse threshold of the Jacobi route (1e-14
    lambda_max) decides the kept rank: J = r - 1 rows at cond 1e6 - never flagged for the QR kernel (J < r), its smallest
    eigenvalue 1e-12 lambda_max, two decades above the device's threshold and one above the reference's 1e-7 sigma_max"""
    r = rank_of(rank)
    odd = (r + 3, 10.0, "deficient_tall") if which == "diag" else (r + 2, 1.0, "zero")
    out = [(r, 1e3, "full"), (17, 10.0 if r > 1 else 1.0, "full"), odd, (65, 1e4, "full"), (max(r - 1, 1), 10.0, "full")]
    return out + [(r - 1, 1e6, "full")] if which == "diag" else out


def _orth(n, k, rng):
    q, _ = np.linalg.qr(rng.standard_normal((n, k)))
    return q


def make_delta(r, rng, diagonal=False):
    """float32 [r, r] with singular values in [1, 2]; diagonal: powers of two (a product with it is exact)"""
    if diagonal:
        return np.diag(2.0 ** rng.randint(0, 2, size=r)).astype(np.float32)
    s = np.linspace(1.01, 1.99, r) if r > 1 else np.array([1.5])  # (the fp32 rounding must not leave [1, 2])
    return ((_orth(r, r, rng) * s) @ _orth(r, r, rng).T).astype(np.float32)


def design_slab(J, r, cond, kind, Dm, rng):
    """Y_i [J, r] in fp64 with Y_i Delta^T = Q diag(sigma) R^T"""
    if kind == "zero":
        return np.zeros((J, r))
    cols = np.arange(r)
    if kind == "deficient_tall":  # two exactly zero columns (a diagonal Delta keeps them zero)
        cols = np.array([c for c in range(r) if c not in (1 % r, r - 1)])
    k = min(J, len(cols))
    sigma = np.logspace(0.0, -np.log10(cond), k) if k > 1 else np.ones(1)
    A = np.zeros((J, r))
    A[:, cols] = (_orth(J, k, rng) * sigma) @ _orth(len(cols), k, rng).T
    return np.linalg.solve(Dm.astype(np.float64), A.T).T  # Y = A Delta^-T


def rho_B(A, C):
    """the B-phase feasibility penalties (decomposition.py:243-249) in fp64 from the float32 factors"""
    A, C = np.asarray(A, dtype=np.float64), np.asarray(C, dtype=np.float64)
    return 0.5 * (A * A) @ np.sum(C * C, axis=0)


def designed_problem(rank, slabs, delta="random", seed=0):
    """-> dict: float32 X, A, B, U, C, Delta, float64 rho, row_ptr and the slab list.  K = max(rank, 8), A and C positive (they
    only have to make B_begin and B_factor run; the rows of A are scaled so that rho spans two decades)"""
    r = rank_of(rank)
    rng = np.random.RandomState(7000 + 97 * r + seed)
    Dm = make_delta(r, rng, diagonal=(delta == "diagonal"))
    Y = np.concatenate([design_slab(J, r, cond, kind, Dm, rng) for J, cond, kind in slabs])
    B = Y.astype(np.float32)
    U = (Y - B.astype(np.float64)).astype(np.float32)
    row_ptr = np.concatenate([[0], np.cumsum([s[0] for s in slabs])]).astype(np.int64)
    I, K = len(slabs), max(r, 8)
    A = ((10.0 ** np.linspace(-1.0, 1.0, I)[rng.permutation(I)])[:, None] * (rng.rand(I, r) + 0.5) / np.sqrt(r)).astype(np.float32)
    C = (rng.rand(K, r) + 0.1).astype(np.float32)
    X = rng.rand(int(row_ptr[-1]), K).astype(np.float32)
    out = dict(X=X, A=A, B=B, U=U, C=C, Delta=Dm, row_ptr=row_ptr, rho=rho_B(A, C))
    for v in out.values():
        v.setflags(write=False)
    out["slabs"] = tuple(slabs)
    return out


@functools.lru_cache(maxsize=None)
def main_problem(rank):
    return designed_problem(rank, slab_list(rank))


@functools.lru_cache(maxsize=None)
def special_problem(rank, which):
    return designed_problem(rank, special_slabs(rank, which), delta="diagonal" if which == "diag" else "random", seed=1 + (which == "zero"))


# ---- the slab counts of the four-slabs-per-workgroup Newton-Schulz kernel (rank 8) ---------------------------------------------------
CLAMP_RANK, CLAMP_I = 8, (1, 4, 5, 7)


@functools.lru_cache(maxsize=None)
def clamp_problem(n_slabs, last):
    """n_slabs slabs at rank 8; the last one a Newton-Schulz slab (`ns`) or a J < r slab for the in-kernel Jacobi (`short`)"""
    pool = [(8, 10.0, "full"), (17, 1e3, "full"), (9, 1e4, "full"), (64, 1.0, "full"), (16, 1e3, "full"), (65, 10.0, "full")]
    slabs = pool[:n_slabs - 1] + [(13, 1e4, "full") if last == "ns" else (5, 1e3, "full")]
    return designed_problem(CLAMP_RANK, slabs, seed=10 * n_slabs + (last == "ns"))


# ---- a stale Newton-Schulz starting estimate ------------------------------------------------------------------------------------------
STALE_RANKS = (8, 24)


@functools.lru_cache(maxsize=None)
def stale_problems(rank):
    """(easy, hard): the same shape and Delta at cond 1 (leaves the carried estimate near its largest value) and at cond 1e4"""
    Js = (rank, rank + 1, 17, 64, 65, 33, 130)
    easy = designed_problem(rank, [(J, 1.0, "full") for J in Js], seed=5)
    hard = designed_problem(rank, [(J, 1e4, "full") for J in Js], seed=5)
    assert np.array_equal(easy["Delta"], hard["Delta"]) and np.array_equal(easy["A"], hard["A"])
    return easy, hard


# ---- rank 4, 65 slabs: the QR kernel is deliberately not launched by the fast kernels --------------------------
@functools.lru_cache(maxsize=None)
def many_slabs_problem():
    conds = (1.0, 10.0, 1e3, 1e4)
    slabs = [((4, 5, 7, 16, 17)[i % 5], conds[i % 4], "full") for i in range(64)] + [(9, 1e7, "full")]
    return designed_problem(4, slabs, seed=3)


# ---- routes ---------------------------------------------------------------------------------------------------------------------------------
def route(rank, slab, variant="default"):
    """the route the policy of mcl_launch_pf2_polar gives a designed slab: `ns` (Newton-Schulz converges), `jacobi` (every
    other Gram route: the in-kernel fallback, k_pf2_algebra behind the status, or Jacobi for every slab), `qr`, `zero`"""
    r = rank_of(rank)
    J, cond, kind = slab
    if kind == "zero":
        return "zero"
    if J >= r and (kind == "deficient_tall" or cond >= 1e5):
        return "qr"
    if r > 32 or variant == "jacobi" or J < r:
        return "jacobi"
    return "ns"


def compared(rank, slabs, variant="default", qr_launched=True):
    """the slabs whose P_i is held against the reference: all but an all-zero slab (numpy's polar factor of a zero matrix is
    arbitrary) and a QR slab where the QR kernel is deliberately not launched"""
    routes = [route(rank, s, variant) for s in slabs]
    return np.array([rt != "zero" and (rt != "qr" or qr_launched) for rt in routes])


# ---- references -----------------------------------------------------------------------------------------------------------------------------
def reference(B, U, Delta, row_ptr, rho):
    """fp64 from the stored values: per slab the thin SVD of A_i = Y_i Delta^T, P_i = U_k V_k^T over the singular values above
    SVD_KEEP sigma_max, W_i = V_k Sigma_k^-1 V_k^T, T_i = Delta^T W_i, S_i = Y_i^T Y_i; Delta_new = sum rho_i P_i^T Y_i / sum rho_i;
    the dual as k_rows_pf2_dual forms it: z = P Delta_new, u = f - (z - u), i.e. B - (P Delta_new - U).  An all-zero slab has
    P_i = 0 (and counts in sum rho_i)."""
    Y = np.asarray(B, dtype=np.float64) + np.asarray(U, dtype=np.float64)
    D = np.asarray(Delta, dtype=np.float64)
    rho = np.asarray(rho, dtype=np.float64)
    r = Y.shape[1]
    n = len(row_ptr) - 1
    P, T, W, S = np.zeros_like(Y), np.zeros((n, r, r)), np.zeros((n, r, r)), np.zeros((n, r, r))
    cond, sigma, kept = np.ones(n), [], np.zeros(n, dtype=np.int64)
    num = np.zeros((r, r))
    for i, (s, e) in enumerate(zip(row_ptr[:-1], row_ptr[1:])):
        Yi = Y[s:e]
        S[i] = Yi.T @ Yi
        u, sv, vt = np.linalg.svd(Yi @ D.T, full_matrices=False)
        sigma.append(sv)
        # (less a part in 1e6: the designed sigma_min = 1e-7 sigma_max of a cond-1e7 slab is kept whichever way its last bit
        # rounds - the QR route that takes such a slab keeps everything above 1e-14 sigma_max)
        k = int(np.sum(sv > SVD_KEEP * (1.0 - 1e-6) * sv[0])) if sv[0] > 0 else 0
        kept[i] = k
        if k == 0:
            continue
        cond[i] = sv[0] / sv[k - 1]
        P[s:e] = u[:, :k] @ vt[:k]
        W[i] = (vt[:k].T / sv[:k]) @ vt[:k]
        T[i] = D.T @ W[i]
        num += rho[i] * (P[s:e].T @ Yi)
    Delta_new = num / rho.sum()
    dual = np.asarray(B, dtype=np.float64) - (P @ Delta_new - np.asarray(U, dtype=np.float64))
    return dict(Y=Y, P=P, T=T, W=W, S=S, Delta_new=Delta_new, dual=dual, cond=cond, sigma=sigma, kept=kept)


def gram_route(Yi, Si, D):
    """the Gram route in fp64: eigh of Delta S_i Delta^T, pseudo-inverse square root at 1e-14 lambda_max -> (P_i, T_i^T S_i)"""
    lam, V = np.linalg.eigh(D @ Si @ D.T)
    inv = np.where((lam > 1e-14 * lam[-1]) & (lam > 0), 1.0 / np.sqrt(np.where(lam > 0, lam, 1.0)), 0.0)
    Tm = D.T @ ((V * inv) @ V.T)
    return Yi @ Tm, Tm.T @ Si


def emulated_error(ref, Delta, row_ptr):
    """per slab, from the reference alone: e32 = the relative Frobenius error of fp32(B + U) @ fp32(T_i) in numpy float32, eG =
    that of the Gram route in fp64, `rigorous` = the componentwise bound (r + 4) 2^-24 || |Y| |T| ||_F / ||P||_F (printed, never
    asserted), and M_gram = T_i^T S_i of the Gram route (the Delta bar)"""
    D = np.asarray(Delta, dtype=np.float64)
    Y, P = ref["Y"], ref["P"]
    n, r = len(row_ptr) - 1, Y.shape[1]
    e32, eG, rig, M = np.zeros(n), np.zeros(n), np.zeros(n), np.zeros((n, r, r))
    for i, (s, e) in enumerate(zip(row_ptr[:-1], row_ptr[1:])):
        nP = np.linalg.norm(P[s:e])
        if nP == 0:
            continue
        P32 = Y[s:e].astype(np.float32) @ ref["T"][i].astype(np.float32)
        e32[i] = np.linalg.norm(P32.astype(np.float64) - P[s:e]) / nP
        PG, M[i] = gram_route(Y[s:e], ref["S"][i], D)
        eG[i] = np.linalg.norm(PG - P[s:e]) / nP
        rig[i] = (r + 4) * HALF_ULP * np.linalg.norm(np.abs(Y[s:e]) @ np.abs(ref["T"][i])) / nP
    return dict(e32=e32, eG=eG, rigorous=rig, M_gram=M)


def p_bar(emu, gram_handled):
    """the bar on the relative Frobenius error of P_i: max(8 e32_i, 8 eG_i, 8 x 2^-24), eG only for the Gram routes"""
    return np.maximum(np.maximum(8.0 * emu["e32"], 8.0 * HALF_ULP), np.where(gram_handled, 8.0 * emu["eG"], 0.0))


def delta_bar(ref, emu, rho, row_ptr, gram_handled):
    """4 x 2^-24 max(1, max |want|) (three fp32 roundings: each sum, the division) + 8 x the elementwise maximum of the
    reference's own Gram-route Delta minus its SVD Delta (a slab of the QR route keeps its SVD term)"""
    rho = np.asarray(rho, dtype=np.float64)
    num = np.zeros_like(ref["Delta_new"])
    for i, (s, e) in enumerate(zip(row_ptr[:-1], row_ptr[1:])):
        num += rho[i] * (emu["M_gram"][i] if gram_handled[i] else ref["P"][s:e].T @ ref["Y"][s:e])
    gram_term = float(np.abs(num / rho.sum() - ref["Delta_new"]).max())
    return 4.0 * HALF_ULP * max(1.0, float(np.abs(ref["Delta_new"]).max())) + 8.0 * gram_term


# ---- (b) one inner iteration of a whole B-phase on the fp64 state ---------------------------------------------------------------------------
WIDE_CASES = ((None, 4), (None, 17), (65, 33), (130, 64))  # (rows of each of three slabs, or the ragged slabs; rank)


@functools.lru_cache(maxsize=None)
def wide_problem(size, rank):
    """random factors and data, a PARAFAC2 member with orthonormal-column P_i, a well-conditioned Delta and a small dual"""
    rng = np.random.RandomState(9000 + 7 * (size or 0) + rank)
    J = np.asarray(J_RAGGED) if size is None else np.full(3, size)
    row_ptr = np.concatenate([[0], np.cumsum(J)]).astype(np.int64)
    I, N, K = len(J), int(row_ptr[-1]), max(rank, 8)
    A = ((10.0 ** np.linspace(-1.0, 1.0, I)[rng.permutation(I)])[:, None] * (rng.rand(I, rank) + 0.5) / np.sqrt(rank)).astype(np.float32)
    B = rng.standard_normal((N, rank)).astype(np.float32)
    C = (rng.rand(K, rank) + 0.1).astype(np.float32)
    X = rng.rand(N, K).astype(np.float32)
    P0 = np.concatenate([np.linalg.qr(rng.standard_normal((max(j, rank), rank)))[0][:j] for j in J]).astype(np.float32)
    Delta0 = make_delta(rank, rng)
    dual0 = (np.round(0.1 * rng.standard_normal((N, rank)) * 64.0) / 512.0).astype(np.float32)
    out = dict(X=X, A=A, B=B, C=C, P0=P0, Delta0=Delta0, dual0=dual0, row_ptr=row_ptr)
    for v in out.values():
        v.setflags(write=False)
    return out
