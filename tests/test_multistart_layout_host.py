"""CPU: the layout of one job's slice of the fused kernels' state matrix (matcouply_amd/multistart.py: _StateLayout) on the
smallest problems that hold every kind of segment - factors, aux and dual of every mode, the Delta of a PARAFAC2, a mode that
is not updated, an empty matrix."""
import functools

import numpy as np
import pytest
import torch

from matcouply_amd import _engine, decomposition as dec, multistart as ms
from matcouply_amd import penalties as pen

K, RANK = 4, 2
NN, L1, PF2 = _engine.PEN_NN, _engine.PEN_L1, _engine.PEN_PARAFAC2
PENALTIES = dict(non_negative={0: True, 1: True}, l1_penalty={2: 0.1})
CASES = {
    "every segment": ((3, 5, 2), dict(PENALTIES, parafac2=True), [[NN], [PF2, NN], [L1]]),
    "mode 2 not updated": ((3, 5, 2), dict(PENALTIES, parafac2=True, update_C=False), [[NN], [PF2, NN], []]),
    "an empty matrix": ((3, 0, 2), dict(PENALTIES, l2_penalty=0.1), [[NN], [NN], [L1]]),
}


@functools.lru_cache(maxsize=None)
def _case(name):
    """the problem, its keywords and one start of it, drawn once and shared (nothing below changes them)"""
    rows, kwargs, kinds = CASES[name]
    rng = np.random.RandomState(0)
    mats = [rng.standard_normal((j, K)) for j in rows]
    kw = dec._cmf_kwargs(kwargs)
    cmf, regs, auxes, duals = dec._start_penalties(kw, mats, RANK, np.random.RandomState(1))
    assert [[pen.native_descriptor_of(reg)[0] for reg in regs[mode]] for mode in range(3)] == kinds
    row_ptr = np.concatenate([[0], np.cumsum(rows)]).astype(np.int64)
    return mats, kw, row_ptr, kinds, (cmf, auxes, duals)


@pytest.fixture(params=list(CASES))
def case(request):
    return _case(request.param)


def _rounded(x):
    """x in its nesting (a tuple for a PARAFAC2's (P_i list, Delta), a list for the B_i) with every array through fp32"""
    if isinstance(x, (tuple, list)):
        return type(x)(_rounded(v) for v in x)
    return np.asarray(x, dtype=np.float32).astype(np.float64)


def _assert_same(got, expect):
    assert type(got) is type(expect)
    if isinstance(expect, (tuple, list)):
        assert len(got) == len(expect)
        for g, e in zip(got, expect):
            _assert_same(g, e)
    else:
        assert got.dtype == expect.dtype and got.shape == expect.shape
        np.testing.assert_array_equal(got, expect)


def test_length_is_the_engine_s(case):
    _, _, row_ptr, kinds, _ = case
    layout = ms._StateLayout(row_ptr, K, RANK, kinds)
    assert layout.length == _engine.multistart_state_len(len(row_ptr) - 1, int(row_ptr[-1]), K, RANK, kinds)
    assert layout.length == sum(seg.rows * seg.cols for seg in layout.segments)


def test_pack_then_unpack_returns_the_start_rounded_to_fp32(case):
    mats, _, row_ptr, kinds, (cmf, auxes, duals) = case
    layout = ms._StateLayout(row_ptr, K, RANK, kinds)
    vector = layout.pack(cmf, auxes, duals)
    assert vector.dtype == np.float64 and vector.shape == (layout.length,)
    A, B, C, admm = layout.unpack(torch.from_numpy(vector))  # a CPU tensor: no device in this test
    assert not A.is_cuda and [[entry[0] for entry in admm[mode]] for mode in range(3)] == kinds
    out = dec._Out(mats)
    A0, B0_is, C0 = cmf[1]
    _assert_same([out(A), out.split(B, row_ptr), out(C)], _rounded([np.asarray(A0), [np.asarray(b) for b in B0_is], np.asarray(C0)]))
    got = dec._admm_vars_out(out, row_ptr, admm)
    for mode in range(3):
        assert len(got.auxes[mode]) == len(got.duals[mode]) == len(kinds[mode])
        _assert_same(got.auxes[mode], _rounded(list(auxes[mode])))
        _assert_same(got.duals[mode], _rounded(list(duals[mode])))


def test_the_order_of_a_mode_s_penalties_is_part_of_the_layout():
    _, _, row_ptr, kinds, (cmf, auxes, duals) = _case("every segment")
    swapped = [kinds[0], kinds[1][::-1], kinds[2]]
    first, second = ms._StateLayout(row_ptr, K, RANK, kinds), ms._StateLayout(row_ptr, K, RANK, swapped)
    assert first.length == second.length  # a check of the length alone does not tell them apart
    turn = lambda v: [v[0], v[1][::-1], v[2]]
    a, b = first.pack(cmf, auxes, duals), second.pack(cmf, turn(auxes), turn(duals))
    assert a.shape == b.shape and not np.array_equal(a, b)
    n = (len(row_ptr) + int(row_ptr[-1]) + K - 1) * RANK
    np.testing.assert_array_equal(a[:n], b[:n])  # the factors lie where they lay
    admm = second.unpack(torch.from_numpy(b))[3]
    assert [entry[0] for entry in admm[1]] == swapped[1]
    np.testing.assert_array_equal(admm[1][1][2].numpy(), _rounded(np.asarray(auxes[1][0][1])))  # the Delta follows its penalty


def test_length_from_the_penalties_names_alone(case):
    mats, kw, row_ptr, kinds, _ = case
    modes, _ = ms._multistart_layout(mats, RANK, kw)
    layout = ms._StateLayout.from_names(row_ptr, K, RANK, [names for names, _ in modes])
    assert layout.kinds == kinds
    assert layout.length == _engine.multistart_state_len(len(row_ptr) - 1, int(row_ptr[-1]), K, RANK, kinds)
