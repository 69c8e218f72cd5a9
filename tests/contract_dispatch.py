"""The dispatch of the two passes over X, restated in Python: which kernel the library launches for X C and for [G | R], on
which segment / wave tables.  tests/test_contract_cases.py proves on a CPU that CONTRACT_CASES (tests/kernel_edge_cases.py) reach
every edge and every built instantiation; tests/test_gpu_contract.py holds the device to the same predictions (kernel_variant
strings and the planner's tables), so the proofs are about the real dispatch.

Restated: mcl_set_problem (csrc/api.hip: NB, x_streams, segments and waves), plan() (exact mode, sweep_planned),
mcl_xc_chunks / mcl_cfrag_chunks (mcl_internal.h), mcl_sweep_shape_ok (sweep.hip), xt_KB / launch_xt / launch_xc / mcl_exact_mode
(contract.hip), try_xc_lds (xclds.hip), mcl_launch_exact_xc (admm.hip).  A `sw` argument is a dict of MCL_* environment switches."""

import functools

X_TYPES = ("f32", "bf16", "f16")
_KTYPE = {"bf16": "XBF16", "f16": "XF16"}
SEG_ROWS = 256  # MCL_SEG_ROWS (mcl_internal.h)
SWITCHES = ("MCL_XC_WAVES", "MCL_SEG_ROWS", "MCL_X_NT_MB", "MCL_XC_LDS_DEPTH", "MCL_NO_XC_LDS", "MCL_XC_DEPTH1", "MCL_XC_NOROW",
            "MCL_XT_DEPTH", "MCL_NO_SWEEP", "MCL_EXACT")


def _num(sw, name, dflt=0):
    return int(sw[name]) if name in sw else dflt


def _flag(sw, name):
    return name in sw


def nb_of(rank):
    nb = (rank + 15) // 16
    return 4 if nb == 3 else nb


def plan_segments(J, sw=None):
    """(seg_slab, seg_row0, seg_nrows, wave_seg_ptr) of mcl_set_problem"""
    sw = sw or {}
    return _plan_segments(tuple(J), _num(sw, "MCL_XC_WAVES"), _num(sw, "MCL_SEG_ROWS"))


@functools.lru_cache(maxsize=None)
def _plan_segments(J, xc_waves, sw_seg_rows):
    seg_rows = SEG_ROWS
    if sw_seg_rows > 0:
        seg_rows = max(16, (sw_seg_rows // 16) * 16)
    total_units = sum((j + 15) // 16 for j in J)
    target = xc_waves if xc_waves > 0 else 1024
    n_waves = max(1, min(target, max(min(512, total_units), total_units // 8)))
    quota = max(1, -(-total_units // n_waves))
    slab, row0, nrows, ptr = [], [], [], [0]
    used, base = 0, 0
    for i, Ji in enumerate(J):
        j = base
        while j < base + Ji:
            take = min(seg_rows, base + Ji - j, (quota - used) * 16)
            slab.append(i), row0.append(j), nrows.append(take)
            j += take
            used += (take + 15) // 16
            if used >= quota:
                ptr.append(len(slab))
                used = 0
        base += Ji
    if used > 0:
        ptr.append(len(slab))
    return slab, row0, nrows, ptr


def xc_chunks(K, NB):
    """mcl_xc_chunks: (chunks of the fragment image, KCT template argument)"""
    raw, budget = (K + 63) // 64, 4 // NB
    if raw <= 2 and budget >= 2:
        return 2, 2
    if raw <= 4 and budget >= 4:
        return 4, 4
    return (raw + 3) & ~3, 0


def xt_KB(K, NB):
    kb = max(1, 4 // NB)
    need = (K + 63) // 64
    return (1 if need <= 1 else 2 if need <= 2 else 4) if need < kb else kb


def exact_mode(N, K, sw):
    if "MCL_EXACT" in sw and int(sw["MCL_EXACT"]) >= 0:
        return int(sw["MCL_EXACT"]) != 0
    return N * K <= 1 << 20


def x_streams(N, K, sw):
    mb = _num(sw, "MCL_X_NT_MB")
    return N * K * 4.0 > (mb if mb > 0 else 256) * 1048576.0


def sweep_planned(J, K, NB, sw):
    N, I = sum(J), len(J)
    if exact_mode(N, K, sw) or _flag(sw, "MCL_NO_SWEEP"):
        return False
    if K < 4 or K > 512 or K % 4:
        return False
    if NB > 2 or ((K + 255) // 256) * NB > 2 or N == 0 or I == 0:
        return False
    return N // I >= 64


def cfrag_chunks(J, K, NB, sw):
    xc = xc_chunks(K, NB)[0]
    if not sweep_planned(J, K, NB, sw):
        return xc
    sweep_kc = 2 if (K <= 128 and NB == 1) else 4 * ((K + 255) // 256)
    return max(xc, sweep_kc)


def xc_lds_depth(J, K, NB, aligned, sw, n_segs):
    """try_xc_lds: 0 when the LDS-resident form does not serve the shape, else the ring depth the launcher asks for"""
    if _flag(sw, "MCL_NO_XC_LDS") or NB > 2 or K % 512 or not aligned:
        return 0
    if (K >> 6) * 4 * NB * 256 * 4 + 4 * 4 * 16 * 128 > 160 * 1024 or n_segs == 0:
        return 0
    if cfrag_chunks(J, K, NB, sw) != K >> 6:
        return 0
    want = _num(sw, "MCL_XC_LDS_DEPTH")
    return want if want in (4, 8) and K % (128 * want) == 0 else 4


def _name(kernel, xt, args):
    """the demangled name tools/kernel_resources.py gives an instantiation"""
    a = ", ".join(str(v).lower() if isinstance(v, bool) else str(v) for v in args)
    return f"{kernel}<{a}>" if xt == "f32" else f"{kernel}_h<{_KTYPE[xt]}, {a}>"


def _variant(kernel, xt, text):
    return f"{kernel}<{text}>" if xt == "f32" else f"{kernel}_h<{xt},{text}>"


def launch_xc(J, K, rank, xt, aligned, sw, gram_request):
    """mcl_launch_contract_xc / mcl_launch_exact_xc.  gram_request: 0 (B_begin), 1 / 2 (A_begin with / without a penalty on mode 0).
    Returns dict(variant, kernels, family, gram: the per-segment reductions came out of this launch, slab_gram: k_slab_gram follows)"""
    N, NB = sum(J), nb_of(rank)
    if exact_mode(N, K, sw):
        v = "k_contract_xc_f64" if xt == "f32" else f"k_contract_xc_f64_h<{xt}>"
        return dict(variant=v, kernels=[_name("k_contract_xc_f64", xt, [NB])], family="xc_f64", gram=0, slab_gram=gram_request != 0)
    vec = K % 4 == 0 and aligned
    kc, kct = xc_chunks(K, NB)
    n_segs = len(plan_segments(J, sw)[0])
    nt = x_streams(N, K, sw)
    kernels = ["k_build_cfrag"]
    if vec and K % 256 == 0 and not _flag(sw, "MCL_XC_NOROW"):
        creg = K == 256 and NB == 1
        gram = gram_request
        if NB == 4 and gram == 2:
            gram = 0
        depth = 0 if creg else xc_lds_depth(J, K, NB, aligned, sw, n_segs)
        if depth:
            if xt != "f32":
                depth = 4  # the depth-8 ring has no 16-bit twin
            return dict(variant=_variant("k_contract_xc_lds", xt, f"NB={NB},GRAM={gram}"), family="xc_lds", depth=depth,
                        kernels=kernels + [_name("k_contract_xc_lds", xt, [NB, gram, nt, depth])], gram=gram, slab_gram=gram_request != 0 and gram == 0)
        if creg and not _flag(sw, "MCL_XC_DEPTH1"):
            return dict(variant=_variant("k_contract_xc_256", xt, f"DEPTH=2,GRAM={gram}"), family="xc_256",
                        kernels=kernels + [_name("k_contract_xc_256", xt, [gram, 2, nt])], gram=gram, slab_gram=gram_request != 0 and gram == 0)
        return dict(variant=_variant("k_contract_xc_row", xt, f"NB={NB},CREG={int(creg)},GRAM={gram}"), family="xc_row",
                    kernels=kernels + [_name("k_contract_xc_row", xt, [NB, creg, gram, nt])], gram=gram, slab_gram=gram_request != 0 and gram == 0)
    V = 4 if vec else 1
    return dict(variant=_variant("k_contract_xc", xt, f"NB={NB},VEC={V},KCT={kct}"), family="xc",
                kernels=kernels + [_name("k_contract_xc", xt, [NB, V, kct])], gram=0, slab_gram=gram_request != 0)


def xc_block_partition(N, sw):
    """launch_xc for k_contract_xc: (16-row blocks, blocks per wave, waves)"""
    nblk = (N + 15) // 16
    target = _num(sw, "MCL_XC_WAVES") if _num(sw, "MCL_XC_WAVES") > 0 else 1024
    bpw = max(1, -(-nblk // target))
    return nblk, bpw, -(-nblk // bpw)


def launch_xt(J, K, rank, xt, aligned, sw):
    """mcl_update_C_local on a fresh context: dict(variant, kernels, KB, NB, vec, depth, n_slices, nb)"""
    N, NB = sum(J), nb_of(rank)
    if exact_mode(N, K, sw):
        v = ("k_exact_gr" if xt == "f32" else f"k_exact_gr_h<{xt}>") + " (+ k_exact_gr_reduce)"
        n_chunks = max(1, (N + 255) // 256)
        return dict(variant=v, family="exact_gr", n_chunks=n_chunks,
                    kernels=[_name("k_exact_gr", xt, [NB])] + (["k_exact_gr_reduce"] if n_chunks > 1 else []))
    KB = xt_KB(K, NB)
    n_seg_waves = len(plan_segments(J, sw)[3]) - 1
    nb = max(1, (n_seg_waves + 3) // 4)
    vec = K % 4 == 0 and aligned
    depth = _num(sw, "MCL_XT_DEPTH") if _num(sw, "MCL_XT_DEPTH") > 0 else 4
    nt = x_streams(N, K, sw)
    rmode = 1 if NB == 4 else 0
    if vec:
        kernels = [_name("k_contract_xt", xt, [KB, NB, 4, 2 if depth == 2 else 4, rmode, nt])]
    else:
        kernels = [_name("k_contract_xt", xt, [KB, NB, 1, 2, rmode, False])]
    if NB == 4:
        kernels.append(_name("k_contract_xt", xt, [KB, NB, 1, 2, 2, False]))
    return dict(variant=_variant("k_contract_xt", xt, f"KB={KB},NB={NB},VEC={4 if vec else 1}"), family="xt", KB=KB, NB=NB, vec=vec,
                depth=2 if (not vec or depth == 2) else 4, n_slices=-(-K // (64 * KB)), nb=nb, kernels=kernels + ["k_reduce_partials"])


def slab_gram_kernel(rank):
    return f"k_slab_gram<{nb_of(rank)}>"
