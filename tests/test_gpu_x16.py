"""-m gpu: 16-bit data matrices (bfloat16 / float16 X, csrc/xload.h).  X stays 16-bit in device memory and every kernel that
reads it converts the elements exactly to fp32 on load, so a run on 16-bit X must reproduce, bit for bit, the run of the fp32
engine on X.float(): every factor, every ADMM variable, every error list - and with the 16-bit twin of the fp32 kernel
variant at every launch site that reads X."""
import ctypes
import re

import numpy as np
import pytest

from matcouply_amd import _engine
from matcouply_amd import decomposition as dec

pytestmark = pytest.mark.gpu

X16 = ["bfloat16", "float16"]
SITES = (_engine.PROF_XC, _engine.PROF_XT, _engine.PROF_SWEEP, _engine.PROF_ROWS_FUSED)


def _torch():
    import torch

    return torch


def _problem(J, K, r, dtype, seed=0):
    """X_i = B_i diag(a_i) C^T + noise, rounded to `dtype` on the device; -> (X16 [N, K] CUDA, row_ptr)"""
    torch = _torch()
    g = torch.Generator().manual_seed(seed)
    row_ptr = np.concatenate([[0], np.cumsum(J)]).astype(np.int64)
    C = torch.rand(K, r, generator=g)
    parts = []
    for j in J:
        parts.append((torch.rand(j, r, generator=g) * torch.rand(1, r, generator=g)) @ C.T + 0.05 * torch.randn(j, K, generator=g))
    X = torch.cat(parts, 0).to(device="cuda", dtype=getattr(torch, dtype)).contiguous()
    return X, row_ptr


class _Recorder:
    """engine factory that keeps every engine of a call and the kernel variants of the X launch sites"""

    def __init__(self):
        self.engines, self.variants = [], []

    def __call__(self, **kw):
        eng = _engine.HipEngine(**kw)
        self.engines.append(eng)
        close = eng.close

        def close_and_record():
            self.variants.append(self._variants(eng))
            close()

        eng.close = close_and_record
        return eng

    @staticmethod
    def _variants(eng):
        v = {s: eng.kernel_variant(s) for s in SITES}
        v["exact"] = eng.kernel_variant(_engine.VARIANT_EXACT_MODE)
        return v

    def finish(self):
        for eng in self.engines[len(self.variants):]:
            self.variants.append(self._variants(eng))


def _run(fn, X, row_ptr, rank, monkeypatch, **kw):
    rec = _Recorder()
    monkeypatch.setattr(dec, "_default_engine_factory", rec)
    out = fn(dec.PackedMatrices(X, row_ptr), rank, tol=None, absolute_tol=None, return_errors=True, return_admm_vars=True,
             random_state=3, **kw)
    rec.finish()
    return out, rec


def _twin_of(v16):
    """the fp32 variant string of a 16-bit variant: k_name_h<bf16,ARGS> -> k_name<ARGS>, k_name_h<f16> -> k_name"""
    v = re.sub(r"_h<(bf16|f16),", "<", v16)
    return re.sub(r"_h<(bf16|f16)>", "", v)


def _flat(x):
    torch = _torch()
    if isinstance(x, torch.Tensor):
        return [x]
    if isinstance(x, (list, tuple)):
        return [t for e in x for t in _flat(e)]
    if hasattr(x, "_asdict"):
        return _flat(list(x._asdict().values()))
    return []


def _engine_state(eng):
    ts = [eng.A, eng.B, eng.C]
    for mode in eng.regs:
        for reg in mode:
            ts += [reg.aux, reg.dual] + ([reg.aux2] if reg.aux2 is not None else [])
    return ts


def _assert_twins(out16, rec16, out32, rec32, dtype):
    torch = _torch()
    assert len(rec16.engines) == len(rec32.engines)
    for e16, e32 in zip(rec16.engines, rec32.engines):
        assert e16.x_type in (_engine.X_BF16, _engine.X_F16) and e32.x_type == _engine.X_F32
        for a, b in zip(_engine_state(e16), _engine_state(e32)):  # the fp32 / fp64 device state, bit for bit
            assert a.dtype == b.dtype and torch.equal(a, b)
    for v16, v32 in zip(rec16.variants, rec32.variants):
        for s in SITES:
            if v32[s] and re.match(r"k_(sweep|contract_x|exact_gr)", v32[s]):
                assert v16[s] != v32[s] and _twin_of(v16[s]) == v32[s], (s, v16[s], v32[s])
            else:
                assert v16[s] == v32[s], (s, v16[s], v32[s])
        assert v16["exact"] == v32["exact"]
    (cmf16, vars16, diag16), (cmf32, vars32, diag32) = out16, out32
    t16, t32 = _flat(cmf16) + _flat(vars16), _flat(cmf32) + _flat(vars32)
    assert len(t16) == len(t32) and len(t16) > 3
    for a, b in zip(t16, t32):  # results follow the input's dtype
        assert a.dtype == getattr(torch, dtype) and torch.equal(a, b.to(a.dtype))
    for name in ("rec_errors", "feasibility_gaps", "regularized_loss"):
        assert list(getattr(diag16, name)) == list(getattr(diag32, name)), name


NN = dict(non_negative=True)
# name: (function, J_i, K, rank, keyword arguments, fast kernels (MCL_EXACT=0), kernel that must have run)
CASES = {
    "exact_products": ("cmf", [60, 90, 75, 33], 64, 6, dict(NN, l1_penalty={2: 0.05}), False, "k_exact_gr"),
    "sweep": ("cmf", [300, 64, 1100, 257, 80], 256, 16, dict(NN, l1_penalty={2: 0.1}), True, "k_sweep"),
    "sweep_half_width": ("cmf", [150, 400, 260, 97], 100, 8, dict(NN), True, "k_sweep"),
    "xc256_xt_parafac2": ("pf2", [130, 400, 260, 1000, 96], 256, 16, dict(l2_norm_bound={1: 1.0}), True, "k_contract_xc_256"),
    "xc_row_k768": ("cmf", [150, 300, 97], 768, 12, dict(NN), True, "k_contract_xc_row"),
    "not_vectorised_k102": ("cmf", [150, 300, 97], 102, 8, dict(l2_norm_bound={1: 1.0}), True, "k_contract_xc<"),
    "xc_lds_k1024_r32": ("pf2", [140, 260, 97], 1024, 32, dict(non_negative={0: True}, unimodal={1: True},
                                                             l2_norm_bound={1: 1.0}), True, "k_contract_xc_lds"),
}


def _call(kind):
    return dec.cmf_aoadmm if kind == "cmf" else dec.parafac2_aoadmm


@pytest.mark.parametrize("dtype", X16)
@pytest.mark.parametrize("case", list(CASES))
def test_x16_run_is_bit_identical_to_fp32_on_the_upcast(case, dtype, monkeypatch):
    kind, J, K, r, kw, fast, must = CASES[case]
    if fast:
        monkeypatch.setenv("MCL_EXACT", "0")
    else:
        monkeypatch.delenv("MCL_EXACT", raising=False)
    X16_, row_ptr = _problem(J, K, r, dtype, seed=sum(map(ord, case)))
    X32 = X16_.float()
    fn = _call(kind)
    args = dict(n_iter_max=4, **kw)
    ref_a, rec_a = _run(fn, X32, row_ptr, r, monkeypatch, **args)
    ref_b, rec_b = _run(fn, X32.clone(), row_ptr, r, monkeypatch, **args)
    _assert_twins_fp32(ref_a, rec_a, ref_b, rec_b)  # the fp32 run is itself reproducible
    out, rec = _run(fn, X16_, row_ptr, r, monkeypatch, **args)
    assert any(must in _twin_of(v) for vs in rec.variants for v in vs.values()), (must, rec.variants)
    _assert_twins(out, rec, ref_a, rec_a, dtype)


def _assert_twins_fp32(out_a, rec_a, out_b, rec_b):
    torch = _torch()
    for e1, e2 in zip(rec_a.engines, rec_b.engines):
        for a, b in zip(_engine_state(e1), _engine_state(e2)):
            assert torch.equal(a, b)
    assert rec_a.variants == rec_b.variants
    assert list(out_a[2].rec_errors) == list(out_b[2].rec_errors)


@pytest.mark.parametrize("dtype", X16)
def test_x16_auto_arithmetic_mid_size(dtype, monkeypatch):
    """arithmetic="auto" between 2^20 and 2^24 elements: the trial, the condition monitor and the choice all see the same values"""
    monkeypatch.delenv("MCL_EXACT", raising=False)
    X16_, row_ptr = _problem([1500, 900, 2100, 700], 512, 8, dtype, seed=7)
    assert 2 ** 20 < X16_.numel() < 2 ** 24
    out32, rec32 = _run(dec.cmf_aoadmm, X16_.float(), row_ptr, 8, monkeypatch, n_iter_max=4, arithmetic="auto", non_negative=True)
    out16, rec16 = _run(dec.cmf_aoadmm, X16_, row_ptr, 8, monkeypatch, n_iter_max=4, arithmetic="auto", non_negative=True)
    _assert_twins(out16, rec16, out32, rec32, dtype)


@pytest.mark.parametrize("dtype", X16)
def test_x16_device_svd_init(dtype):
    torch = _torch()
    X16_, row_ptr = _problem([120, 300, 77], 96, 6, dtype, seed=11)
    B16, C16, i16 = _engine.svd_init(X16_, row_ptr, 6)
    B32, C32, i32 = _engine.svd_init(X16_.float(), row_ptr, 6)
    assert torch.equal(B16, B32) and torch.equal(C16, C32) and torch.equal(i16, i32)
    # and through the public call: init="svd" on a 16-bit PackedMatrices takes the device initialiser
    out16 = dec.cmf_aoadmm(dec.PackedMatrices(X16_, row_ptr), 6, init="svd", n_iter_max=2, tol=None, absolute_tol=None,
                           non_negative=True, return_errors=True, random_state=3)
    out32 = dec.cmf_aoadmm(dec.PackedMatrices(X16_.float(), row_ptr), 6, init="svd", n_iter_max=2, tol=None, absolute_tol=None,
                           non_negative=True, return_errors=True, random_state=3)
    assert list(out16[1].rec_errors) == list(out32[1].rec_errors)


def test_x16_host_svd_fallback_takes_bfloat16():
    """the host (LAPACK) path of init="svd" (K above the device initialiser's limit) upcasts before NumPy, which has no bfloat16"""
    torch = _torch()
    X16_, row_ptr = _problem([40, 30, 50], dec._DEVICE_SVD_MAX_K + 52, 4, "bfloat16", seed=5)
    mats = [X16_[row_ptr[i]: row_ptr[i + 1]] for i in range(3)]
    cmf, diag = dec.cmf_aoadmm(mats, 4, init="svd", n_iter_max=2, tol=None, absolute_tol=None, return_errors=True)
    assert cmf[1][2].dtype == torch.bfloat16 and np.isfinite(diag.rec_errors[-1])


@pytest.mark.parametrize("as_list", [False, True])
def test_x16_makes_no_fp32_copy(as_list):
    """2^27 elements of bfloat16 X at rank 4: the call's peak allocation above what the caller holds stays below 2 N K bytes
    for a PackedMatrices (an fp32 copy of X alone is 4 N K).  A list of bf16 CUDA tensors is packed once, in bfloat16 (2 N K):
    its bound is 3 N K, still below an fp32 copy."""
    torch = _torch()
    I, J, K = 256, 2048, 256
    N = I * J
    assert N * K >= 2 ** 27
    X = torch.rand(N, K, device="cuda").to(torch.bfloat16)
    row_ptr = np.arange(0, N + 1, J, dtype=np.int64)
    data = [X[row_ptr[i]: row_ptr[i + 1]] for i in range(I)] if as_list else dec.PackedMatrices(X, row_ptr)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    cmf, diag = dec.cmf_aoadmm(data, 4, n_iter_max=2, tol=None, absolute_tol=None, non_negative=True, return_errors=True)
    torch.cuda.synchronize()
    grew = torch.cuda.max_memory_allocated() - base
    bound = (3 if as_list else 2) * N * K
    print(f"as_list={as_list}: peak growth {grew / 2 ** 20:.0f} MiB, bound {bound / 2 ** 20:.0f} MiB")
    assert grew < bound, (grew, bound)
    assert cmf[1][2].dtype == torch.bfloat16


def test_x16_config3_against_the_oracle():
    """one full-size config-3 trajectory on bf16 X: within the flat 1e-5 of the fp64 oracle on the upcast data"""
    torch = _torch()
    import bench
    from oracle import aoadmm_oracle as orc

    cfg = dict(bench.CONFIGS["c3"])
    X, row_ptr, I_loc = bench.make_shard(cfg, 0, 1, torch.device("cuda", 0))
    X16_ = X.to(torch.bfloat16)
    Xd = X16_.double().cpu().numpy()
    st = orc.random_state_for(Xd, row_ptr, cfg["r"], cfg["regs"], seed=1)
    r32 = lambda a: np.asarray(a, np.float32).astype(np.float64)
    st.A, st.B, st.C = r32(st.A), r32(st.B), r32(st.C)
    from matcouply_amd import penalties as pen

    split = lambda P: [P[row_ptr[i]: row_ptr[i + 1]].copy() for i in range(len(row_ptr) - 1)]
    regs = [[pen.NonNegativity(aux_init=st.aux[0][0].copy(), dual_init=st.dual[0][0].copy())],
            [pen.NonNegativity(aux_init=split(st.aux[1][0]), dual_init=split(st.dual[1][0]))],
            [pen.L1Penalty(0.1, non_negativity=True, aux_init=st.aux[2][0].copy(), dual_init=st.dual[2][0].copy())]]
    cmf, diag = dec.cmf_aoadmm(dec.PackedMatrices(X16_, row_ptr), cfg["r"], init=(None, (st.A, split(st.B), st.C)), regs=regs,
                               n_iter_max=3, tol=None, absolute_tol=None, return_errors=True)
    del cmf
    res = orc.run(st, 3, tol=None, absolute_tol=None)
    eR = max(abs(a - b) / b for a, b in zip(diag.rec_errors, res["rec_errors"]))
    assert eR < 1e-5, eR


def test_x16_sweep_is_faster_at_config3():
    """speed guard: the 16-bit sweep site is no slower than the fp32 one at config 3 (fastest of 7 repetitions, same process).
    Measured 0.96x (125.5 against 130.4 us): the sweep is co-limited by the fp32 matrix core, which half the bytes of X do not
    relieve; a deeper prefetch of the 16-bit tiles is the open lever (profiles/x16_rate.txt)."""
    torch = _torch()
    import bench

    cfg = dict(bench.CONFIGS["c3"])
    dev = torch.device("cuda", 0)
    X, row_ptr, I_loc = bench.make_shard(cfg, 0, 1, dev)
    best = {}
    for name, Xt in (("f32", X.to(torch.bfloat16).float()), ("bf16", X.to(torch.bfloat16))):
        eng = bench.make_engine(cfg, Xt, row_ptr, I_loc, 0, dev)
        eng.iterate(20)
        eng.profile_enable(4096)
        b = float("inf")
        for _ in range(7):
            eng.iterate(50)
            torch.cuda.synchronize()
            ms, n = eng.profile_read(_engine.PROF_SWEEP)
            b = min(b, 1e3 * ms / n if n else float("inf"))
            eng.profile_enable(4096)
        best[name] = b
        assert eng.kernel_variant(_engine.PROF_SWEEP).startswith("k_sweep_h<bf16," if name == "bf16" else "k_sweep<")
        eng.close()
    print(f"config 3 sweep site: fp32 {best['f32']:.1f} us, bf16 {best['bf16']:.1f} us")
    assert best["bf16"] <= best["f32"], best


def test_set_problem_typed_rejects_bad_input():
    torch = _torch()
    lib = _engine.load_library()
    h = ctypes.c_void_p()
    stream = torch.cuda.current_stream().cuda_stream
    assert lib.mcl_create(ctypes.byref(h), 0, ctypes.c_void_p(stream)) == 0
    try:
        X = torch.zeros(64 * 16 + 4, dtype=torch.bfloat16, device="cuda")
        row_ptr = np.array([0, 64], dtype=np.int64)
        rp = row_ptr.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
        assert lib.mcl_set_problem_typed(h, X.data_ptr(), 7, rp, 1, 16, 4) != 0
        assert b"x_type" in lib.mcl_last_error(h)
        assert lib.mcl_set_problem_typed(h, X.data_ptr() + 2, _engine.X_BF16, rp, 1, 16, 4) != 0
        assert b"8-byte aligned" in lib.mcl_last_error(h)
        assert lib.mcl_set_problem_typed(h, X.data_ptr(), _engine.X_BF16, rp, 1, 16, 4) == 0
        X32 = torch.zeros(64 * 16, dtype=torch.float32, device="cuda")
        assert lib.mcl_set_problem(h, X32.data_ptr(), rp, 1, 16, 4) == 0  # still the fp32 wrapper
    finally:
        lib.mcl_destroy(h)
    B = torch.empty(1)
    assert lib.mcl_svd_init_typed(B.data_ptr(), 9, rp, 1, 16, 4, 0, None, None, None, 0, None, None) != 0
    assert b"x_type" in lib.mcl_svd_init_last_error()
