"""CPU: the host side of 16-bit data matrices - which inputs stay 16-bit, which are packed in float32, and what a substituted
checker engine without 16-bit support is handed."""
import numpy as np
import pytest
import torch

from matcouply_amd import _engine
from matcouply_amd import decomposition as dec


def test_x_type_of_names_the_three_dtypes():
    assert _engine.x_type_of(torch.float32) == _engine.X_F32
    assert _engine.x_type_of(torch.bfloat16) == _engine.X_BF16
    assert _engine.x_type_of(torch.float16) == _engine.X_F16
    with pytest.raises(TypeError, match="float32, bfloat16 or float16"):
        _engine.x_type_of(torch.float64)


@pytest.mark.parametrize("dtype", [torch.float64, torch.int32, torch.int8])
def test_packed_matrices_rejects_other_dtypes(dtype):
    X = torch.zeros((10, 4), dtype=dtype)
    with pytest.raises(TypeError, match="float32, bfloat16 or float16"):
        dec._pack(dec.PackedMatrices(X, [0, 4, 10]), torch.device("cpu"))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_packed_matrices_accepts_the_three_dtypes_on_the_device_only(dtype):
    X = torch.zeros((10, 4), dtype=dtype)  # a CPU tensor: the dtype is fine, the place is not
    with pytest.raises(TypeError, match="CUDA"):
        dec._pack(dec.PackedMatrices(X, [0, 4, 10]), torch.device("cpu"))


def test_x16_dtype_of_lists():
    bf = [torch.ones(3, 4, dtype=torch.bfloat16), torch.ones(2, 4, dtype=torch.bfloat16)]
    hf = [torch.ones(3, 4, dtype=torch.float16)] * 2
    npf = [np.ones((3, 4), np.float16), np.ones((5, 4), np.float16)]
    assert dec._x16_dtype(bf) == torch.bfloat16
    assert dec._x16_dtype(hf) == torch.float16
    assert dec._x16_dtype(npf) == torch.float16
    # mixed lists and everything else: float32
    assert dec._x16_dtype(bf + hf) is None
    assert dec._x16_dtype([bf[0], torch.ones(2, 4)]) is None
    assert dec._x16_dtype([npf[0], np.ones((2, 4), np.float32)]) is None
    assert dec._x16_dtype([torch.ones(3, 4)]) is None
    assert dec._x16_dtype([np.ones((3, 4))]) is None


@pytest.mark.parametrize("kind", ["bf16", "f16", "np_f16"])
def test_pack_keeps_homogeneous_16bit_lists(kind):
    rng = np.random.RandomState(0)
    host = [rng.randn(j, 6).astype(np.float16) for j in (3, 5, 2)]
    if kind == "np_f16":
        mats, want = host, torch.float16
    else:
        want = torch.bfloat16 if kind == "bf16" else torch.float16
        mats = [torch.from_numpy(m.astype(np.float32)).to(want) for m in host]
    X, row_ptr = dec._pack(mats, torch.device("cpu"))
    assert X.dtype == want and X.shape == (10, 6) and X.is_contiguous()
    assert list(row_ptr) == [0, 3, 8, 10]
    ref = torch.cat([torch.as_tensor(np.asarray(m)) if not torch.is_tensor(m) else m for m in mats], 0)
    assert torch.equal(X, ref.to(want))


def test_pack_mixed_lists_go_to_float32():
    mats = [torch.ones(3, 4, dtype=torch.bfloat16), torch.ones(2, 4, dtype=torch.float16)]
    X, _ = dec._pack(mats, torch.device("cpu"))
    assert X.dtype == torch.float32
    X, _ = dec._pack([np.ones((3, 4), np.float16), np.ones((2, 4), np.float64)], torch.device("cpu"))
    assert X.dtype == torch.float32


def test_upcast_for_engines_without_x16():
    torch.manual_seed(0)
    X = torch.randn(10, 4).to(torch.bfloat16)
    pm = dec._upcast_x16(dec.PackedMatrices(X, [0, 4, 10]))
    assert pm.X.dtype == torch.float32 and torch.equal(pm.X, X.float())
    mats = dec._upcast_x16([X[:4], X[4:].to(torch.float16), np.ones((2, 4), np.float16)])
    assert [m.dtype for m in mats[:2]] == [torch.float32, torch.float32] and mats[2].dtype == np.float16
    assert _engine.HipEngine.supports_x16


def test_checker_engine_receives_fp32_x(monkeypatch):
    """a substituted checker engine (no `supports_x16`) is handed X.float() of a list of bf16 matrices; the results come
    back in the caller's dtype"""
    from tests.oracle_engine import OracleEngineFactory

    seen = []

    class Factory(OracleEngineFactory):
        def pack(self, matrices):
            seen.extend(m.dtype for m in matrices)
            return super().pack(matrices)

    monkeypatch.setenv("MATCOUPLY_AMD_TEST_ENGINE", "1")
    monkeypatch.setattr(dec, "_ENGINE_FACTORY", Factory())
    rng = np.random.RandomState(1)
    mats = [torch.from_numpy(rng.rand(j, 5).astype(np.float32)).to(torch.bfloat16) for j in (6, 8, 7)]
    cmf, diag = dec.cmf_aoadmm(mats, 2, n_iter_max=2, tol=None, absolute_tol=None, non_negative=True, return_errors=True,
                               random_state=0)
    assert seen and all(d == torch.float32 for d in seen)
    assert cmf[1][2].dtype == torch.bfloat16
    ref, diag32 = dec.cmf_aoadmm([m.float() for m in mats], 2, n_iter_max=2, tol=None, absolute_tol=None, non_negative=True,
                                 return_errors=True, random_state=0)
    assert list(diag.rec_errors) == list(diag32.rec_errors)
