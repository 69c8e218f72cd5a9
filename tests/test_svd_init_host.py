"""CPU: the fixtures of the device SVD initialiser's edge-case tests (tests/svd_init_cases.py) are well posed and the NumPy
restatement of its subspace iteration is the algorithm - by the reference (LAPACK in fp64) and the restatement alone, so that a
failure of tests/test_gpu_svd_init.py on these inputs is the kernel's.

The bound on the restatement is 5e-7 (helpers.rel_err of its float32-rounded vectors under the sign rule against LAPACK's): a
quarter of the 2e-6 at which the kernel is held, which keeps that headroom over what the rounding of the output to float32 alone
costs.  The restatement gave at worst 1.7e-7 (C of many_slabs_257), 1.0e-7 (C of many_slabs_late_max) and 4.8e-9 to 7.9e-8
elsewhere, in 4 to 45 iterations.

many_slabs_late_max is a case of this file's own: with the shapes of many_slabs (3 to 7 rows in the first 256 matrices, 8 to 12 in
the other 44) the FIRST batch holds the most rows (1303 against 443), so it is kept as it is and joined by one whose second batch
does (768 against 899 rows)."""
import numpy as np
import pytest

from tests import svd_init_cases as S
from tests.helpers import rel_err

RESTATEMENT_BOUND = 5e-7


def _f32(a):
    return np.asarray(a, dtype=np.float32)


def _assert_matches_lapack(mats, rank, B_is, C, counts, ref_B, ref_C, what):
    assert len(counts) == len(mats) + 1 and np.all(counts > 0) and np.all(counts < S.MAX_IT), (what, counts)
    for i, (got, want) in enumerate(zip(B_is, ref_B)):
        assert got.shape == want.shape == (mats[i].shape[0], rank)
        assert rel_err(_f32(got), want) < RESTATEMENT_BOUND, (what, i, rel_err(_f32(got), want))
    assert rel_err(_f32(C), ref_C) < RESTATEMENT_BOUND, (what, "C", rel_err(_f32(C), ref_C))


@pytest.mark.parametrize("name", S.ABC_CASES)
def test_restatement_matches_lapack(name):
    mats, rank = S.problem(name)
    B_is, C, counts = S.restated_init(name)
    ref_B, ref_C, _ = S.reference(name)
    _assert_matches_lapack(mats, rank, B_is, C, counts, ref_B, ref_C, name)


@pytest.mark.parametrize("dtype", ["bfloat16", "float16"])
def test_restatement_matches_lapack_on_16_bit_values(dtype):
    """the 16-bit runs of the GPU file: the fixture rounded to the storage type is another matrix, and is well posed too"""
    mats, rank = S.stored_as(S.X16_CASE, dtype)
    B_is, C, counts = S.restated_init_of(mats, rank)
    ref_B, ref_C, _ = S.reference_of(mats, rank)
    _assert_matches_lapack(mats, rank, B_is, C, counts, ref_B, ref_C, dtype)


@pytest.mark.parametrize("name", sorted(S.CLUSTERS))
def test_cluster_cases_are_well_posed(name):
    """repeated singular values: the restatement converges, and what the GPU test asserts of the device's vectors holds for the
    restatement's (fp64, not rounded) at 1e-12.  Measured: <= 8.3e-15."""
    mats, rank = S.problem(name)
    B_is, C, counts = S.restated_init(name)
    assert np.all(counts > 0) and np.all(counts < S.MAX_IT), counts
    for M, B in zip(mats, B_is):
        s = S.lapack(M)[1]
        want = np.array(S.CLUSTERS[name])
        assert np.allclose(s[:len(want)], want, rtol=1e-6), s[:len(want)]  # the repeated values survive the rounding to float32
        figures = S.cluster_figures(name, M, B)
        assert max(figures.values()) <= 1e-12, figures
    assert rel_err(_f32(C), S.reference(name)[1]) < RESTATEMENT_BOUND  # the stack's spectrum is generic


def test_no_gap_hits_the_iteration_cap():
    mats, rank = S.problem("no_gap")
    B_is, C, counts = S.restated_init("no_gap")
    assert counts.tolist() == [-S.MAX_IT] * 3
    # ... and what the GPU test asserts of the unsettled vectors holds for the restatement's.  (X q_k of Ritz vectors q_k that
    # have not settled are orthogonal only as far as the iteration has come: 6.0e-8 here, against the 1e-6 asserted)
    for M, B in zip(mats, B_is):
        assert S.orthonormality_defect(B) <= 1e-6 / 4
        sig = S.captured_sigma(M, B)
        assert np.all(sig >= 0.9 * (1 - 1e-5)) and np.all(sig <= 1 + 1e-5), sig


@pytest.mark.parametrize("name", ["sign_ties", "sign_ties_swapped"])
def test_sign_ties_fixture(name):
    (M,), rank = S.problem(name)
    assert M.dtype == np.float32 and M.shape == (400, 8) and rank == 1
    assert np.array_equal(M[45], -M[300]) and np.any(M[45] != 0)  # exact negations: every product with them is exactly tied
    assert 45 // S.BATCH != 300 // S.BATCH  # different passes of the 256-way strided scan
    others = np.delete(np.abs(M).max(axis=1), [45, 300])
    assert others.max() <= 0.5 * np.abs(M[45]).max()
    v = np.abs(M[300])
    assert np.sum(v == v.max()) == 1
    (ref_B,), ref_C, _ = S.reference(name)
    (B,), C, counts = S.restated_init(name)
    for vec in (ref_B, B):
        assert vec[45, 0] > 0 and vec[300, 0] == -vec[45, 0]
    assert np.all(counts > 0)
    assert rel_err(_f32(B), ref_B) < RESTATEMENT_BOUND and rel_err(_f32(C), ref_C) < RESTATEMENT_BOUND


def test_canon_takes_the_first_entry_on_ties():
    V = np.array([[0.5, -1.0], [-2.0, 1.0], [2.0, 0.25]])
    assert np.array_equal(S.canon(V), [[-0.5, 1.0], [2.0, -1.0], [-2.0, -0.25]])


def test_hash_restatement():
    """deterministic, in (-1, 1), 32-bit wrap-around; the start vectors of different matrices differ"""
    a, b = np.meshgrid(np.arange(300), np.arange(80 + 977 * 301), indexing="ij", sparse=True)
    h = S.hash_unit(a, b[:, ::997])
    assert h.dtype == np.float64 and np.all(h > -1) and np.all(h < 1)
    assert np.array_equal(h, S.hash_unit(a, b[:, ::997]))
    assert np.array_equal(h * 8388608.0, np.round(h * 8388608.0))  # 24 bits
    assert abs(h.mean()) < 0.02 and abs(h.std() - 3 ** -0.5) < 0.02
    # operands that wrap: the same as with the carries dropped by hand (Python integers)
    def by_hand(a, b):
        M = 0xFFFFFFFF
        h = (a * 0x9E3779B1 & M) ^ (((b + 0x7F4A7C15) & M) * 0x85EBCA77 & M)
        h ^= h >> 15
        h = h * 0x2C1B3C6D & M
        h ^= h >> 12
        h = h * 0x297A2D39 & M
        h ^= h >> 15
        return (h >> 8) * (2.0 / 16777216.0) - 1.0

    for a, b in [(0, 0), (1, 0), (2047, 71 + 977 * 300), (5, 0xFFFFFFFF), (0xFFFFFFFF, 0x80B583EB), (123456789, 0x80B583EA)]:
        assert S.hash_unit(a, b) == by_hand(a, b), (a, b)
    Y0, Y1 = S.start_vectors(12, 11, 0), S.start_vectors(12, 11, 1)
    assert Y0.shape == (12, 11) and not np.array_equal(Y0, Y1)
    assert Y1[3, 4] == by_hand(3, 4 + 977)


def test_case_tables_hit_what_they_claim():
    """the paths the cases are there for are live at their shapes (svd_plan, k_svd_subspace, jacobi_lds, k_svd_gram, k_svd_left)"""
    for name, I in (("many_slabs", 300), ("many_slabs_257", 257), ("many_slabs_late_max", 300)):
        mats, rank = S.problem(name)
        rows = np.array([m.shape[0] for m in mats])
        assert len(mats) == I > S.BATCH and rows.min() >= rank
        batch_rows = [rows[b0:b0 + S.BATCH].sum() for b0 in range(0, I, S.BATCH)]
        assert len(batch_rows) == 2
        # a later batch holds the most rows and sizes the U scratch: only where its 44 matrices outweigh the first 256
        assert (batch_rows[1] > batch_rows[0]) == (name == "many_slabs_late_max")
        assert name != "many_slabs_257" or I - S.BATCH == 1  # a last batch of one matrix
        assert rows[:S.BATCH].max() < rows[S.BATCH:].min()  # the batches' references cannot be mistaken for each other
    ms = {S.svd_m(K, r): (r, K) for r, K in S.M_IS_K}
    assert all(m == K for m, (r, K) in ms.items())  # the whole space is iterated
    assert {1, 2, 72} <= set(ms) and any(m % 2 == 1 and m > 14 for m in ms) and max(r for r, _ in S.M_IS_K) == 64
    m = 72  # dynamic LDS of k_svd_subspace (svd_init of csrc/svdinit.hip): above the 64 KiB a kernel gets unasked
    assert 8 * (2 * m * m + m + 2 * ((m + 1) // 2 + 1) + m) + 4 * m + 64 > 64 * 1024
    for r, K in S.M_IS_K:
        rows = [M.shape[0] for M in S.problem(f"m_is_K_{r}_{K}")[0]]
        assert rows == [max(r, K), K + 16, K + 65] and min(rows) >= r
    assert sum(r == K for r, K in S.M_IS_K) == 4  # ... of which the first matrix has exactly `rank` rows
    assert any(K % 32 == 1 for _, K in S.TILES) and any(K % 2 == 1 and K > 32 for _, K in S.TILES)
    assert all(M.shape[0] > 256 for name in S.CLUSTERS for M in S.problem(name)[0][2:])  # rows past the 256-thread stride
    for r, K in S.TILES:
        rows = [M.shape[0] for M in S.problem(f"tiles_{r}_{K}")[0]]
        assert r in rows and S.svd_m(K, r) < K and max(rows) == 2 * K + 1
    assert S.svd_m(200, 3) == 11 and S.X16_CASE in S.ABC_CASES
