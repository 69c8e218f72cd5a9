"""Fixtures of the device SVD initialiser's edge-case tests (csrc/svdinit.hip, jacobi_lds of csrc/symeig_lds.h) and a plain fp64
NumPy restatement of its subspace iteration.  Shared by the GPU tests (tests/test_gpu_svd_init.py) and the CPU checks that the
fixtures are well posed and that the restatement is the algorithm (tests/test_svd_init_host.py).

Every matrix is designed: (U * s) @ V.T with orthonormal U, V and a chosen spectrum s, rounded to float32.  The reference is
always LAPACK on those float32 values widened to float64."""
import functools
import zlib

import numpy as np

OVERSAMPLE, MAX_IT, BATCH = 8, 400, 256  # SVD_OVERSAMPLE, SVD_MAX_IT and the BS of svd_plan (csrc/svdinit.hip)


def svd_m(K, rank):
    return min(K, rank + OVERSAMPLE)


# ---- fixtures ---------------------------------------------------------------------------------------------------------------------
def _orth(rng, n, k):
    return np.linalg.qr(rng.standard_normal((n, k)))[0]


def designed(rng, J, K, s):
    """a J x K float32 matrix with the singular values s (before the rounding to float32)"""
    s = np.asarray(s, dtype=np.float64)
    assert len(s) <= min(J, K)
    return ((_orth(rng, J, len(s)) * s) @ _orth(rng, K, len(s)).T).astype(np.float32)


MANY_SPECTRUM = (4, 2, 1, .05, .04, .03, .02, .01)
# (rank, K): m = min(K, rank + 8) = K, the whole space is iterated
M_IS_K = [(1, 1), (2, 2), (3, 3), (1, 9), (57, 65), (64, 64), (63, 71), (64, 72)]
TILES = [(24, 33), (24, 97), (5, 65)]
CLUSTERS = {"cluster_inside": (3, 2, 2, 1) + (.05,) * 6, "cluster_boundary": (4, 3, 2, 1, 1, 1) + (.05,) * 4}

MANY_SLABS = ["many_slabs", "many_slabs_257", "many_slabs_late_max"]
ABC_CASES = MANY_SLABS + [f"m_is_K_{r}_{K}" for r, K in M_IS_K] + [f"tiles_{r}_{K}" for r, K in TILES]
X16_CASE = "tiles_24_33"  # also run stored as bfloat16 / float16


def _seed(name):
    return zlib.crc32(name.encode()) % (2 ** 31)


@functools.lru_cache(maxsize=None)
def problem(name):
    """-> (mats: tuple of float32 matrices, rank)"""
    rng = np.random.RandomState(_seed(name))
    if name.startswith("many_slabs"):
        # the second batch of 256: 44 matrices, or one; its matrices are the longer ones.  In many_slabs_late_max they are so
        # long that the second batch holds more rows than the first (44 x 18 > 256 x 3) and sizes the U scratch
        I, rank, K = (257 if name.endswith("257") else 300), 3, 12
        if name.endswith("late_max"):
            J = [3 if i < BATCH else rng.randint(18, 24) for i in range(I)]
        else:
            J = [rng.randint(3, 8) if i < BATCH else rng.randint(8, 13) for i in range(I)]
        mats = [designed(rng, j, K, MANY_SPECTRUM[:min(j, 8)]) for j in J]
    elif name.startswith("m_is_K"):
        rank, K = (int(v) for v in name.split("_")[-2:])
        mats = [designed(rng, j, K, np.geomspace(1, 0.125, min(j, K)) if K > 1 else [1.0]) for j in (max(rank, K), K + 16, K + 65)]
    elif name.startswith("tiles"):
        rank, K = (int(v) for v in name.split("_")[-2:])
        mats = []
        for j in (K + 3, rank, 2 * K + 1):
            floor = 0.02 * rng.uniform(0.5, 1, size=min(j, K) - rank)
            mats.append(designed(rng, j, K, np.concatenate([np.geomspace(2, 0.5, rank), floor])))
    elif name in CLUSTERS:
        rank, K = 4, 40
        mats = [designed(rng, j, K, CLUSTERS[name]) for j in (40, 57, 300)]
    elif name == "no_gap":
        rank, K = 3, 200
        mats = [designed(rng, j, K, np.linspace(1, 0.9, 200)) for j in (200, 260)]
    elif name in ("sign_ties", "sign_ties_swapped"):
        # noise-free rank one: rows 45 and 300 are exact negations of each other in float32, so their fp64 products with any
        # vector are exactly tied in magnitude; they fall in different passes of the 256-way strided scan of k_svd_left
        rank, K, J = 1, 8, 400
        u = rng.uniform(-0.5, 0.5, size=J).astype(np.float32)
        u[45], u[300] = (-1.0, 1.0) if name == "sign_ties" else (1.0, -1.0)
        v = rng.uniform(0.25, 0.75, size=K).astype(np.float32)
        v[5] = 1.0  # the unique largest entry of v
        mats = [np.outer(u, v).astype(np.float32)]  # (u_j = +-1: the row is +-v exactly)
    else:
        raise KeyError(name)
    for m in mats:
        m.setflags(write=False)
    return tuple(mats), rank


def stored_as(name, dtype):
    """the fixture's values after a round trip through a 16-bit storage type ("bfloat16" / "float16"), as float32 (exact)"""
    import torch

    mats, rank = problem(name)
    return [torch.as_tensor(np.array(m)).to(getattr(torch, dtype)).float().numpy() for m in mats], rank


def row_ptr_of(mats):
    return np.concatenate([[0], np.cumsum([m.shape[0] for m in mats])]).astype(np.int64)


# ---- the sign rule and the reference -------------------------------------------------------------------------------------------
def canon(V):
    """the sign rule of the device form: the entry of largest magnitude of every column is positive, the first one on ties"""
    V = np.array(V, dtype=np.float64)
    for c in range(V.shape[1]):
        if V[np.argmax(np.abs(V[:, c])), c] < 0:  # (np.argmax: the first one on ties)
            V[:, c] = -V[:, c]
    return V


def lapack(M):
    """thin SVD of the stored values widened to float64 -> (U, s, V) with V's COLUMNS the right vectors"""
    U, s, Vt = np.linalg.svd(np.asarray(M, dtype=np.float64), full_matrices=False)
    return U, s, Vt.T


@functools.lru_cache(maxsize=None)
def reference(name):
    """LAPACK's vectors under the sign rule -> (B_is: list of [J_i, rank], C [K, rank], sigma: list of [rank] per matrix)"""
    return reference_of(*problem(name))


def reference_of(mats, rank):
    dec = [lapack(m) for m in mats]
    C = lapack(np.concatenate(mats))[2]
    return [canon(U[:, :rank]) for U, _, _ in dec], canon(C[:, :rank]), [s[:rank] for _, s, _ in dec]


# ---- the restatement of k_svd_subspace ----------------------------------------------------------------------------------------
def hash_unit(a, b):
    """hash_unit of csrc/svdinit.hip on arrays of unsigned 32-bit values (wrap-around arithmetic) -> float64 in (-1, 1)"""
    M32 = np.uint64(0xFFFFFFFF)
    a, b = np.asarray(a, dtype=np.uint64) & M32, np.asarray(b, dtype=np.uint64) & M32
    mul = lambda x, c: (x * np.uint64(c)) & M32  # (operands below 2^32: the 64-bit product is exact)
    h = mul(a, 0x9E3779B1) ^ mul((b + np.uint64(0x7F4A7C15)) & M32, 0x85EBCA77)
    h ^= h >> np.uint64(15)
    h = mul(h, 0x2C1B3C6D)
    h ^= h >> np.uint64(12)
    h = mul(h, 0x297A2D39)
    h ^= h >> np.uint64(15)
    return (h >> np.uint64(8)).astype(np.float64) * (2.0 / 16777216.0) - 1.0


def start_vectors(K, m, b):
    """Y[i, c] = hash_unit(i, c + 977 (b + info0)); b + info0 is the matrix' index, I for the stack"""
    i, c = np.meshgrid(np.arange(K, dtype=np.uint64), np.arange(m, dtype=np.uint64), indexing="ij")
    return hash_unit(i, (c + np.uint64(977) * np.uint64(b)) & np.uint64(0xFFFFFFFF))


def restated_subspace(G, rank, b):
    """k_svd_subspace in NumPy, np.linalg.eigh in the place of the Jacobi sweeps.  G [K, K] float64, b the matrix' index (I for
    the stack) -> (Q [K, m]: the Ritz vectors, columns by descending Ritz value; iterations used, or -400)"""
    K = G.shape[0]
    m = svd_m(K, rank)
    Y = start_vectors(K, m, b)
    prev = np.zeros(m)
    stable, used = 0, -MAX_IT
    Q = None
    for it in range(MAX_IT):
        if it > 0:
            Y = G @ Q
        lam, W = np.linalg.eigh(Y.T @ Y)
        order = np.argsort(-lam, kind="stable")  # descending, ties by index
        lam, W = lam[order], W[:, order]
        lam_max = lam[0]
        keep = (lam > 1e-28 * lam_max) & (lam > 0.0)
        Q = np.zeros((K, m))
        Q[:, keep] = (Y @ W[:, keep]) / np.sqrt(lam[keep])
        th = np.sqrt(np.maximum(lam, 0.0))
        ok = it > 0 and bool(np.all(np.abs(th[:rank] - prev[:rank]) <= 1e-13 * max(np.sqrt(max(lam_max, 0.0)), 1e-300)))
        prev = th
        stable = stable + 1 if ok else 0
        if stable >= 2:
            used = it + 1
            break
    return Q, used


def restated_init_of(mats, rank):
    """mcl_svd_init in fp64 -> (B_is, C: under the sign rule, NOT rounded to float32; counts [I + 1], the stack last)"""
    grams = [m.astype(np.float64).T @ m.astype(np.float64) for m in mats]
    B_is, counts = [], []
    for i, (m_, G) in enumerate(zip(mats, grams)):
        Q, n = restated_subspace(G, rank, i)
        U = m_.astype(np.float64) @ Q[:, :rank]
        B_is.append(canon(U / np.linalg.norm(U, axis=0)))
        counts.append(n)
    Gs = np.zeros_like(grams[0])
    for G in grams:  # the slabs in ascending order
        Gs += G
    Q, n = restated_subspace(Gs, rank, len(mats))
    return B_is, canon(Q[:, :rank]), np.array(counts + [n])


@functools.lru_cache(maxsize=None)
def restated_init(name):
    return restated_init_of(*problem(name))


# ---- the quantities of the cluster and no-gap cases, the same for the device's and the restatement's vectors -----------------
def projector(V):
    return V @ V.T


def orthonormality_defect(B):
    B = np.asarray(B, dtype=np.float64)
    return float(np.max(np.abs(B.T @ B - np.eye(B.shape[1]))))


def captured_sigma(M, B):
    """||M^T b_k|| of every column: sigma_k where b_k is a singular vector"""
    return np.linalg.norm(np.asarray(M, dtype=np.float64).T @ np.asarray(B, dtype=np.float64), axis=0)


def cluster_figures(name, M, B):
    """what the cluster cases assert of one matrix' B, as a dict of figures that must all be <= their bound (2e-6 for the
    vectors and subspaces, 1e-6 for orthonormality and singular values on the device)"""
    from tests.helpers import rel_err

    U, s, _ = lapack(M)
    B = np.asarray(B, dtype=np.float64)
    ref = canon(U[:, :4])
    if name == "cluster_inside":  # (3, 2, 2, 1): columns 0 and 3 are determined, columns 1 and 2 only as a plane
        vec = max(rel_err(B[:, 0], ref[:, 0]), rel_err(B[:, 3], ref[:, 3]))
        sub = float(np.linalg.norm(projector(B[:, 1:3]) - projector(U[:, 1:3])))
    else:  # (4, 3, 2, 1, 1, 1): column 3 is some unit vector of the span of LAPACK's vectors 3 to 5
        vec = max(rel_err(B[:, k], ref[:, k]) for k in range(3))
        sub = float(np.linalg.norm(B[:, 3] - U[:, 3:6] @ (U[:, 3:6].T @ B[:, 3])))
    return dict(vec=vec, sub=sub, orth=orthonormality_defect(B), sigma=float(np.max(np.abs(captured_sigma(M, B) / s[:4] - 1))))
