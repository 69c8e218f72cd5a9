"""-m gpu: the device SVD initialiser (mcl_svd_init of csrc/svdinit.hip, jacobi_lds of csrc/symeig_lds.h) against LAPACK in fp64
at every rank, batch and tile edge it serves: second and later batches of 256 matrices, Rayleigh-Ritz blocks up to m = 72 (dynamic
LDS above 64 KiB), odd and tiny Jacobi sizes, partial Gram tiles, repeated singular values, a spectrum without a gap (the iteration
cap) and the tie-break of the sign rule.  The fixtures and the fp64 restatement of the iteration are in tests/svd_init_cases.py;
tests/test_svd_init_host.py shows on the CPU that every fixture meets these bounds with a quarter of the error allowed here.

Every test prints the figures it asserts (pytest -s shows them)."""
import ctypes
import functools
import warnings

import numpy as np
import pytest

from matcouply_amd import _engine
from matcouply_amd import decomposition as dec
from tests import svd_init_cases as S
from tests.helpers import rel_err

pytestmark = pytest.mark.gpu

BOUND = 2e-6  # the bound of test_device_svd_initialiser (tests/test_converters_inits.py)
# |device's iteration count - restatement's|, the largest over every matrix of a case.  The stop rule needs two stable iterations
# in a row, so a rounding-level difference (cyclic Jacobi here, LAPACK's eigh there) can move a count by one or two: the largest
# difference measured on the MI355X, + 2, is allowed.  Measured (device / restatement, lowest..highest of the matrices, the stack):
#   many_slabs 5..34, 34 / 5..34, 34 (difference <= 2)      many_slabs_257 5..45, 45 / 5..45, 45 (<= 2)
#   many_slabs_late_max 5..34, 34 / 5..34, 34 (<= 1)         m_is_K 1_1, 2_2, 3_3, 1_9: 4 everywhere (0)
#   m_is_K_57_65 4..5, 5 / 4..5, 5 (0)                       m_is_K_64_64 4..5, 4 / 4..5, 4 (0)
#   m_is_K_63_71 4..4, 4 / 4..5, 4 (1)                       m_is_K_64_72 4..4, 4 / 4..5, 5 (1)
#   tiles_24_33 5..19, 19 / 5..19, 19 (0)                    tiles_24_97 5..42, 42 / 7..42, 42 (2: the matrix of `rank` rows)
#   tiles_5_65 5..11, 11 / 5..11, 11 (0)                     tiles_24_33 as bfloat16 (0), as float16 5..19, 19 / 6..19, 19 (2)
#   cluster_inside 5..7, 7 / 5..7, 7 (0)                     cluster_boundary 5..10, 10 / 5..10, 10 (0)
MEASURED_COUNT_DIFF = 2
COUNT_SLACK = MEASURED_COUNT_DIFF + 2


def _np(t):
    return t.detach().cpu().numpy()


def _run(mats, rank, threshold, dtype="float32"):
    import torch

    X = torch.as_tensor(np.concatenate(mats), device="cuda").to(getattr(torch, dtype)).contiguous()
    B, C, info = _engine.svd_init(X, S.row_ptr_of(mats), rank, threshold=threshold)
    torch.cuda.synchronize()
    return _np(B), _np(C), _np(info)


@functools.lru_cache(maxsize=None)
def device_result(name, threshold):
    """(B packed, C, info) of _engine.svd_init on the float32 fixture, computed once"""
    out = _run(*S.problem(name), threshold)
    for a in out:
        a.setflags(write=False)
    return out


def _assert_info(info, I):
    assert info.shape == (I + 1,) and info.dtype == np.int32
    assert np.all(info >= 1) and np.all(info < S.MAX_IT), info


def _assert_counts(what, info, counts):
    d = int(np.max(np.abs(info.astype(np.int64) - counts)))
    print(f"SVDFIG {what}: iterations device {info.min()}..{info.max()} (stack {info[-1]}), restatement {counts.min()}..{counts.max()} "
          f"(stack {counts[-1]}), largest difference {d}")
    worst = int(np.argmax(np.abs(info - counts)))
    assert d <= COUNT_SLACK, (what, f"matrix {worst}", int(info[worst]), int(counts[worst]))  # measured: at most 2 (the table above)


def _assert_vectors(what, mats, rank, threshold, B, C, ref_B, ref_C):
    """every B_i and C against LAPACK's under the sign rule (threshold: clipped at 0) -> the worst figures"""
    rp = S.row_ptr_of(mats)
    assert B.shape == (rp[-1], rank) and C.shape == (mats[0].shape[1], rank) and B.dtype == C.dtype == np.float32
    clip = (lambda a: np.clip(a, 0, None)) if threshold else (lambda a: a)
    errs = [rel_err(B[rp[i]:rp[i + 1]], clip(ref_B[i])) for i in range(len(mats))]
    eC = rel_err(C, clip(ref_C))
    print(f"SVDFIG {what} threshold={int(threshold)}: worst B_i {max(errs):.2e} (matrix {int(np.argmax(errs))}), C {eC:.2e}")
    for i, e in enumerate(errs):
        assert e < BOUND, (what, threshold, f"B of matrix {i} ({mats[i].shape[0]} rows)", e)
    assert eC < BOUND, (what, threshold, "C", eC)


# ---- A, B, C: batches, Jacobi sizes and high rank, Gram tiles -------------------------------------------------------------------
@pytest.mark.parametrize("threshold", [False, True])
@pytest.mark.parametrize("name", S.ABC_CASES)
def test_vectors_match_lapack(name, threshold):
    """Measured on the MI355X, worst rel_err of a B_i / of C over both threshold values: many_slabs 3.7e-8 / 7.2e-8,
    many_slabs_257 3.8e-8 / 1.7e-7, many_slabs_late_max 3.7e-8 / 1.0e-7, m_is_K_1_1 4.8e-9 / 0, m_is_K_2_2 3.1e-8 / 8.4e-9,
    m_is_K_3_3 2.5e-8 / 1.7e-8, m_is_K_1_9 2.8e-8 / 2.0e-8, m_is_K_57_65, 64_64, 63_71 and 64_72 2.6e-8 / 2.6e-8,
    tiles_24_33 2.6e-8 / 2.7e-8, tiles_24_97 2.7e-8 / 7.9e-8, tiles_5_65 2.8e-8 / 2.5e-8: the rounding of the output to float32,
    and for C what the restatement gives too (tests/test_svd_init_host.py)"""
    mats, rank = S.problem(name)
    B, C, info = device_result(name, threshold)
    ref_B, ref_C, _ = S.reference(name)
    _assert_info(info, len(mats))
    _assert_vectors(name, mats, rank, threshold, B, C, ref_B, ref_C)
    _assert_counts(name, info, S.restated_init(name)[2])
    assert np.array_equal(info, device_result(name, not threshold)[2])  # the clip is applied after the iteration


@pytest.mark.parametrize("name", S.MANY_SLABS)
def test_every_batch_holds_its_own_matrices(name):
    """I > 256: the second batch's U scratch offset, info offset and start vectors, and the reuse of Q / Y / theta.  Every batch's
    rows against the references of its own matrices, so that a mixed-up batch fails by its name."""
    mats, rank = S.problem(name)
    B, _, info = device_result(name, False)
    ref_B, _, _ = S.reference(name)
    counts = S.restated_init(name)[2]
    rp = S.row_ptr_of(mats)
    for k, b0 in enumerate(range(0, len(mats), S.BATCH)):
        b1 = min(len(mats), b0 + S.BATCH)
        got, want = B[rp[b0]:rp[b1]], np.concatenate(ref_B[b0:b1])
        assert np.isfinite(got).all(), f"batch {k} (matrices {b0} to {b1 - 1}) of {name}: rows not written"
        e = rel_err(got, want)
        print(f"SVDFIG {name} batch {k}: matrices {b0}..{b1 - 1}, rows {rp[b0]}..{rp[b1] - 1}, rel_err {e:.2e}")
        assert e < BOUND, f"batch {k} (matrices {b0} to {b1 - 1}) of {name}: rel_err {e:.2e}"
        d = np.abs(info[b0:b1].astype(np.int64) - counts[b0:b1]).max()
        assert d <= COUNT_SLACK, f"batch {k} (matrices {b0} to {b1 - 1}) of {name}: iteration counts differ by {d}"


# ---- D: repeated singular values ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(S.CLUSTERS))
def test_repeated_singular_values(name):
    """a repeated value inside the leading `rank` (cluster_inside) and across the cut at `rank` (cluster_boundary): the vectors of
    the simple values are LAPACK's, those of the repeated value span LAPACK's subspace / lie in it; all are orthonormal and carry
    their singular values"""
    mats, rank = S.problem(name)
    B, C, info = device_result(name, False)
    assert info.shape == (len(mats) + 1,) and np.all(info > 0), info
    rp = S.row_ptr_of(mats)
    for i, M in enumerate(mats):
        f = S.cluster_figures(name, M, B[rp[i]:rp[i + 1]])
        print(f"SVDFIG {name} matrix {i} ({M.shape[0]} rows): " + ", ".join(f"{k} {v:.2e}" for k, v in f.items()) + f", iterations {info[i]}")
        # measured: vec <= 2.7e-8, sub <= 5.4e-8 (cluster_inside; 2.8e-8 cluster_boundary), orth <= 1.9e-8, sigma <= 9.6e-9,
        # 5 iterations for every matrix
        assert f["vec"] < BOUND and f["sub"] <= BOUND, (name, i, f)
        assert f["orth"] <= 1e-6 and f["sigma"] <= 1e-6, (name, i, f)
    eC = rel_err(C, S.reference(name)[1])  # the stack's spectrum is generic
    print(f"SVDFIG {name}: C {eC:.2e}, iterations {info[-1]}")
    assert eC < BOUND  # measured: 2.7e-8 in 7 (cluster_inside) and 10 (cluster_boundary) iterations
    _assert_counts(name, info, S.restated_init(name)[2])


# ---- E: no gap behind the leading values ----------------------------------------------------------------------------------------
def test_iteration_cap_is_reported_and_warned_of():
    import torch

    mats, rank = S.problem("no_gap")
    B, C, info = device_result("no_gap", False)
    print(f"SVDFIG no_gap: info {info.tolist()}")
    assert info.tolist() == [-S.MAX_IT] * 3

    def check(B_is):
        for M, Bi in zip(mats, B_is):
            sig, orth = S.captured_sigma(M, Bi), S.orthonormality_defect(Bi)
            print(f"SVDFIG no_gap ({M.shape[0]} rows): |B^T B - I| {orth:.2e}, ||X^T b_k|| {sig.tolist()}")
            # measured: 5.9e-8 (200 rows) and 7.9e-8 (260 rows), the restatement 6.0e-8: X q_k of Ritz vectors that have not
            # settled; ||X^T b_k|| 0.999999, 0.999497, 0.998988 and 0.999998, 0.999496, 0.998990
            assert np.isfinite(Bi).all() and orth <= 1e-6
            assert np.all(sig >= 0.9 * (1 - 1e-5)) and np.all(sig <= 1 + 1e-5), sig

    rp = S.row_ptr_of(mats)
    check([B[rp[i]:rp[i + 1]] for i in range(len(mats))])
    assert np.isfinite(C).all() and S.orthonormality_defect(C) <= 1e-6
    dev = [torch.as_tensor(np.array(M), device="cuda") for M in mats]
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        _, (A, B_is, C2) = dec.initialize_cmf(dev, rank, "svd", None)
    said = [str(w.message) for w in caught]
    assert not any("numerical rank" in s for s in said), said
    runtime = [str(w.message) for w in caught if issubclass(w.category, RuntimeWarning)]
    assert len(runtime) == 1 and "had not settled after 400 iterations" in runtime[0], said
    assert A.is_cuda and C2.is_cuda and all(b.is_cuda for b in B_is)  # the device's factors, not the host path's
    assert bool(torch.all(A == 1)) and bool(torch.isfinite(C2).all())
    check([_np(b) for b in B_is])
    assert np.array_equal(_np(torch.cat(B_is)), B) and np.array_equal(_np(C2), C)


# ---- F: the tie-break of the sign rule ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sign_ties", "sign_ties_swapped"])
def test_sign_rule_takes_the_first_entry_on_ties(name):
    """rows 45 and 300 are tied for the largest magnitude; thread 45 holds row 45, thread 44 row 300 (second pass of its scan):
    the tree reduction must keep the smaller index whichever of the two comes first in it"""
    mats, rank = S.problem(name)
    ref_B, ref_C, _ = S.reference(name)
    B, C, info = device_result(name, False)
    print(f"SVDFIG {name}: B[45] {B[45, 0]!r}, B[300] {B[300, 0]!r}, iterations {info.tolist()}")
    _assert_info(info, 1)
    assert B[45, 0] > 0 and B[300, 0] == -B[45, 0]  # measured: 0.1697884 (sign_ties), 0.17144878 (sign_ties_swapped)
    _assert_vectors(name, mats, rank, False, B, C, ref_B, ref_C)
    Bt, Ct, _ = device_result(name, True)
    assert Bt[45, 0] > 0 and Bt[45, 0] == B[45, 0] and Bt[300, 0] == 0
    _assert_vectors(name, mats, rank, True, Bt, Ct, ref_B, ref_C)


# ---- workspace bounds -----------------------------------------------------------------------------------------------------------
GUARD, FILL = 4096, 0xA5


class Guarded:
    """`nbytes` bytes, 256-byte aligned, inside one larger uint8 tensor with at least 4 KiB of 0xA5 on each side"""

    def __init__(self, nbytes):
        import torch

        self.nbytes = int(nbytes)
        self.buf = torch.full((self.nbytes + 2 * GUARD + 256,), FILL, dtype=torch.uint8, device="cuda")
        self.off = GUARD + (-(self.buf.data_ptr() + GUARD)) % 256
        self.ptr = self.buf.data_ptr() + self.off

    def inside(self, dtype, shape):
        return self.buf[self.off:self.off + self.nbytes].view(dtype).reshape(shape)

    def guards_intact(self):
        lo, hi = self.buf[:self.off], self.buf[self.off + self.nbytes:]
        assert lo.numel() >= GUARD and hi.numel() >= GUARD
        return bool((lo == FILL).all()), bool((hi == FILL).all())


@pytest.mark.parametrize("name", ["many_slabs", "many_slabs_late_max", "m_is_K_64_72"])
def test_workspace_and_outputs_stay_inside_their_bounds(name):
    """the C ABI directly, with exactly mcl_svd_init_workspace_bytes of workspace: nothing is written outside the workspace, B, C
    or info, and what the workspace held before does not matter (the results are those of _engine.svd_init bit for bit)"""
    import torch

    mats, rank = S.problem(name)
    rp = S.row_ptr_of(mats)
    I, K, N = len(mats), mats[0].shape[1], int(rp[-1])
    lib = _engine.load_library()
    rp_c = rp.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
    nbytes = lib.mcl_svd_init_workspace_bytes(rp_c, I, K, rank)
    assert nbytes > 0
    X = torch.as_tensor(np.concatenate(mats), device="cuda").contiguous()
    for threshold in (False, True):
        ws, gB, gC, gi = Guarded(nbytes), Guarded(N * rank * 4), Guarded(K * rank * 4), Guarded((I + 1) * 4)
        stream = torch.cuda.current_stream().cuda_stream
        rc = lib.mcl_svd_init(X.data_ptr(), rp_c, I, K, rank, int(threshold), gB.ptr, gC.ptr, ws.ptr, nbytes, gi.ptr,
                              ctypes.c_void_p(stream))
        torch.cuda.synchronize()
        assert rc == 0, lib.mcl_svd_init_last_error().decode()
        for what, g in (("workspace", ws), ("B", gB), ("C", gC), ("info", gi)):
            assert g.guards_intact() == (True, True), f"{name}: bytes (before, after) {what} intact: {g.guards_intact()}"
        B, C, info = device_result(name, threshold)
        assert np.array_equal(_np(gi.inside(torch.int32, (I + 1,))), info)
        assert np.array_equal(_np(gB.inside(torch.int32, (N, rank))), B.view(np.int32))
        assert np.array_equal(_np(gC.inside(torch.int32, (K, rank))), C.view(np.int32))
    # one byte less is refused, not overrun
    rc = lib.mcl_svd_init(X.data_ptr(), rp_c, I, K, rank, 0, gB.ptr, gC.ptr, ws.ptr, nbytes - 1, gi.ptr, ctypes.c_void_p(stream))
    assert rc != 0 and b"workspace too small" in lib.mcl_svd_init_last_error()


# ---- 16-bit storage -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["bfloat16", "float16"])
def test_16_bit_storage_matches_lapack_on_the_stored_values(dtype):
    """the Gram sums are exact products of the stored values in fp64 whatever the storage type: the bound is unchanged.
    Measured: B_i 2.6e-8 / C 2.7e-8 (bfloat16), 2.7e-8 / 2.7e-8 (float16)"""
    import torch

    stored, rank = S.stored_as(S.X16_CASE, dtype)
    assert not np.array_equal(stored[0], S.problem(S.X16_CASE)[0][0])  # another matrix than the float32 fixture
    ref_B, ref_C, _ = S.reference_of(stored, rank)
    counts = S.restated_init_of(stored, rank)[2]
    for threshold in (False, True):
        B, C, info = _run(stored, rank, threshold, dtype)
        _assert_info(info, len(stored))
        _assert_vectors(f"{S.X16_CASE} as {dtype}", stored, rank, threshold, B, C, ref_B, ref_C)
    _assert_counts(f"{S.X16_CASE} as {dtype}", info, counts)
