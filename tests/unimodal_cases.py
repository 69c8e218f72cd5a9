"""Designed columns for the unimodal prox kernel (csrc/unimodal.hip: k_slab_unimodal_v4<0>, <1> + <2>, <3> at 1, 2 and 4 waves per
workgroup, each with and without the cooperative ring refill) and the slab layouts that carry them.  Shared by the GPU test
(tests/test_gpu_unimodal_edges.py) and the CPU checks that the columns are what they claim (tests/test_unimodal_cases_host.py).
No GPU, no torch.

Every column Y is a multiple of 1/64 with |Y| < 2^10 and is handed to the kernel as B = Y - U, U a multiple of 1/64 in [-1, 1]:
the fp32 sum the kernel forms is exact and equals Y.  A wrong pop, refill, tie or batch edge then moves the fit by at least 1/64,
five orders above the bar of the GPU test.

The block stack of the kernel, in the terms used here: the DEPTH of a column after an element is the number of blocks of the
pool-adjacent-violators stack (the block being built, the cached top, the ring of RC entries per lane, the spill area below
it).  A strictly rising column of L elements has depth L; an element that pools d blocks beneath it pops d entries (the first
from the cached top, the others from the ring, which refills from the spill area when it runs dry) and leaves depth L - d + 1.
Every element pushes one entry, so the ring of a falling flank drains by one entry per element when every element pops TWO
blocks: the block the flank has built so far and one more of the rising flank beneath it."""
import functools

import numpy as np

from oracle import aoadmm_oracle as orc

# constants of csrc/unimodal.hip: ring entries per lane, entries per cooperative refill, elements per load batch of the sweeps,
# records per batch of the emit loops, errors per batch of the split search of <2>
RC, NRF, UB, EB, SB = 16, 8, 8, 16, 16
GRID = 1.0 / 64.0
K = 8
MAX_SLAB, MAX_ROWS = 400, 4200


# ---- the stack, in plain Python ---------------------------------------------------------------------------------------------------
def _push(blocks, v):
    """push v on the stack `blocks` ([sum, count] per block, bottom first) and pool while mean(top) <= mean(below) -> blocks popped"""
    blocks.append([float(v), 1])
    pops = 0
    while len(blocks) >= 2 and blocks[-1][0] * blocks[-2][1] <= blocks[-2][0] * blocks[-1][1]:
        s, c = blocks.pop()
        blocks[-1][0] += s
        blocks[-1][1] += c
        pops += 1
    return pops


def depth_profile(y, direction="left"):
    """-> (depth, popped): the depth of the block stack after each element and the number of blocks that element popped, for the
    left-to-right sweep over y or (direction "right") the right-to-left one, in the order the sweep visits the elements"""
    y = np.asarray(y, dtype=np.float64)
    if direction == "right":
        y = y[::-1]
    blocks, depth, popped = [], [], []
    for v in y:
        popped.append(_push(blocks, v))
        depth.append(len(blocks))
    return np.array(depth, dtype=np.int64), np.array(popped, dtype=np.int64)


def _mean(b):
    return b[0] / b[1]


def _pooling_value(blocks, d, gap):
    """the value that pools exactly the top d blocks of `blocks`: the pooled mean lands `gap` above the mean of the block beneath
    them (`gap` below the lowest of them when the stack empties)"""
    assert 1 <= d <= len(blocks)
    S, C = sum(b[0] for b in blocks[-d:]), sum(b[1] for b in blocks[-d:])
    target = _mean(blocks[-d - 1]) + gap if d < len(blocks) else _mean(blocks[0]) - gap
    v = target * (C + 1) - S
    trial = [list(b) for b in blocks]
    assert _push(trial, v) == d, (d, v)
    return v


def _checked(y):
    y = np.asarray(y, dtype=np.float64)
    assert np.array_equal(np.round(y / GRID) * GRID, y) and (np.abs(y).max() if len(y) else 0.0) < 2.0 ** 10
    y.setflags(write=False)
    return y


# ---- collapse family --------------------------------------------------------------------------------------------------------------
COLLAPSE_L = (15, 16, 17, 18, 24, 25, 26, 33, 48, 100)


def collapse_depths(L):
    """the collapse sizes tried at ramp length L"""
    return sorted({d for d in (1, RC // 2, RC - 1, RC, RC + 1, RC + NRF, L - 1, L) if 1 <= d <= L})


def collapse(L, d, up=3, down=2, step=1.0 / 16.0):
    """L strictly rising elements (depth L), ONE element that pools exactly d of them, `up` elements rising above everything so far
    to the peak, `down` falling ones: the left fit ends at the peak and contains the pooled block.  The dip is element L."""
    ramp = step * np.arange(1, L + 1)
    blocks = [[v, 1] for v in ramp]
    dip = _pooling_value(blocks, d, step / 2)
    top = np.floor(ramp[-1]) + 1.0
    # a deep dip below a short, low peak would rather be fitted by the falling side: that peak stands well above the dip's depth
    h = 8.0 if abs(dip) < 30.0 or up > 3 else 300.0
    rise = top + h * np.arange(1, up + 1)
    fall = rise[-1] - 1.5 * h * np.arange(1, down + 1)
    return _checked(np.concatenate([ramp, [dip], rise, fall]))


DIP_L = 40  # ramp of the columns whose dip sits at m - 1, m, m + 1 (m = n / 2, where the pruned schedule pauses): the stack of the
            # pause is DIP_L or DIP_L - 1 deep, so more than RC + NRF entries are in the spill area when phase C resumes


def collapse_at_pause(d, where):
    """collapse(DIP_L, d) with a tail that puts the dip at m + where, where = -1, 0, 1"""
    n = 2 * (DIP_L - where)  # m = n // 2 = DIP_L - where
    y = collapse(DIP_L, d, up=n - DIP_L - 1 - 2, down=2)
    assert len(y) == n and n // 2 + where == DIP_L
    return y


# ---- slow falling flank -----------------------------------------------------------------------------------------------------------
FLANK_RAMP, FLANK_FALL, FLANK_RISE2, FLANK_FALL2 = 80, 60, 24, 20


def flank(step=0.25):
    """a ramp of 80 (62 entries spilled), 60 elements that each pool the flank's own block and exactly ONE block of the ramp (the
    ring drains by one entry per element: the cooperative refill from prefetched registers), 24 rising elements (the ring
    spills again, which invalidates the prefetch), 20 falling ones as before (the first cooperative refill now has to load),
    then a peak above everything and a short fall: the left fit carries all of it."""
    ramp = step * np.arange(1, FLANK_RAMP + 1)
    blocks = [[v, 1] for v in ramp]
    out = list(ramp)

    def fall(count):
        for _ in range(count):
            v = _pooling_value(blocks, 2, step / 2)
            _push(blocks, v)
            out.append(v)

    fall(FLANK_FALL)
    for j in range(1, FLANK_RISE2 + 1):
        v = ramp[-1] + 1.0 + step * j
        assert _push(blocks, v) == 0
        out.append(v)
    fall(FLANK_FALL2)
    out += [100.0, 200.0, 300.0, 150.0, 50.0]
    return _checked(out)


FLANK_THEN_FALL, FLANK_THEN_D = 50, 20


def flank_collapse(step=0.25):
    """the ramp of 80 and 50 elements of the same falling flank (the ring is being topped up from prefetched entries), then ONE
    element that pools the flank's block and 19 more: more than the ring holds, so the lane runs dry inside one pooling loop
    with valid prefetched entries at hand; then the peak"""
    ramp = step * np.arange(1, FLANK_RAMP + 1)
    blocks = [[v, 1] for v in ramp]
    out = list(ramp)
    for _ in range(FLANK_THEN_FALL):
        v = _pooling_value(blocks, 2, step / 2)
        _push(blocks, v)
        out.append(v)
    out.append(_pooling_value(blocks, FLANK_THEN_D, step / 2))
    top = ramp[-1] + 1.0
    out += [top + 300.0, top + 600.0, top + 900.0, top + 450.0, top]
    return _checked(out)


def ring_events(y, direction="left", coop=True, pause=None):
    """The ring of ONE lane whose wave is in step with it (all 64 lanes carry the same column), as the kernel keeps it (ur4_push,
    ur4_refill_coop, the pooling loop, ur4_refill_dry): how often it spills, refills cooperatively from prefetched registers /
    with a load, and runs dry inside a pooling loop with / without valid prefetched entries.  pause: the element before which the
    pruned schedule has written the ring out (phase C resumes with an empty ring).  coop=False: MCL_NO_UNI_COOP."""
    depth, popped = depth_profile(y, direction)
    ev = dict(spill=0, coop_prefetched=0, coop_load=0, dry_prefetched=0, dry_load=0)
    cnt = mem = pf = before = 0
    for i, pops in enumerate(popped):
        if pause is not None and i == pause:
            mem, cnt, pf = mem + cnt, 0, 0
        if coop and cnt <= 1 and mem > 0:
            room = RC - 2 - cnt if cnt <= RC // 2 else 0
            if pf > 0:
                if room >= pf:
                    mem, cnt = mem - pf, cnt + pf
                    pf = min(mem, NRF)
                    ev["coop_prefetched"] += 1
            elif room > 0:
                nref = min(mem, room, NRF)
                mem, cnt = mem - nref, cnt + nref
                pf = min(mem, NRF)
                ev["coop_load"] += 1
        if before >= 2:  # the cached top goes to the ring
            if cnt == RC:
                mem, cnt, pf = mem + 1, RC - 1, 0
                ev["spill"] += 1
            cnt += 1
        for _ in range(pops):
            if cnt == 0 and mem > 0:
                if pf > 0:
                    mem, cnt, pf = mem - pf, pf, 0
                    ev["dry_prefetched"] += 1
                else:
                    nref = min(mem, RC // 2)
                    mem, cnt = mem - nref, nref
                    ev["dry_load"] += 1
            cnt = max(cnt, 1) - 1
        assert cnt + mem == max(depth[i] - 2, 0) and 0 <= cnt <= RC
        before = depth[i]
    return ev


# ---- ties -------------------------------------------------------------------------------------------------------------------------
def tie_odd(n, a, scale=1.0):
    """palindrome 0, 2, ..., P | P - 1 (k times) | P, ..., 2, 0 with a elements per flank and k = n - 2 a, k + 1 a power of two:
    the valley pools with ONE of the two peaks, to the left peak at splits a - 1 and a, to the right one at n - a and n - a + 1,
    with equal totals (every block count is a power of two: the errors are exact in any arithmetic)"""
    k = n - 2 * a
    assert a >= 2 and k >= 1 and (k + 1) & k == 0
    up = 2.0 * np.arange(a)
    return _checked(scale * np.concatenate([up, np.full(k, up[-1] - 1.0), up[::-1]]))


def tie_even(n, a):
    """the even-length form: the valley pools with a peak AND its outer neighbour P - 2 (k + 2 a power of two), k = 2, 6, 14"""
    k = n - 2 * a
    valley = {2: 4.0, 6: 3.0, 14: 4.0}[k]  # pooled mean P - 2.5, P - 2.5, P - 3.625: between P - 4 and P - 2
    assert a >= 3
    up = 2.0 * np.arange(a)
    return _checked(np.concatenate([up, np.full(k, up[-1] - valley), up[::-1]]))


TIES_ODD = ((5, 2), (9, 3), (9, 4), (17, 5), (33, 9), (33, 13), (65, 17), (65, 29),  # n = 4q + 1
            (7, 3), (15, 4), (31, 12), (63, 16))                                      # n = 4q - 1
TIES_EVEN = ((8, 3), (16, 5), (32, 13), (32, 9), (64, 25))                            # n = 4q
CONST_N = (7, 16, 33)


def plateau(reps):
    """rises with plateaus of equal values between them (the pooling test sees equality), a peak, a fall with plateaus"""
    left = np.repeat(np.arange(6.0), reps)
    return _checked(np.concatenate([left, [9.0], np.repeat([7.0, 3.0, 1.0], reps)]))


# ---- length edges -----------------------------------------------------------------------------------------------------------------
EDGE_N = (1, 2, 3, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65)


def edge(n, shape):
    """strictly monotone columns and columns with the peak second / second to last: optimal splits 0 | 1, n - 1 | n, 1 | 2 and
    n - 2 | n - 1.  A third of every column is negative, so non-negativity changes the fit."""
    inc = np.arange(n, dtype=np.float64) - n // 3
    if shape == "inc":
        y = inc
    elif shape == "dec":
        y = inc[::-1]
    elif shape == "peak_first":
        y = inc[::-1].copy()
        y[0] = y[1] - 1.5
    else:  # peak_last
        y = inc.copy()
        y[-1] = y[-2] - 1.5
    return _checked(y.copy())


# ---- the families: name -> column -------------------------------------------------------------------------------------------------
def _with_mirrors(cols):
    out = {}
    for name, y in cols.items():
        out[name] = y
        if not np.array_equal(y, y[::-1]):
            out[name + "/mirror"] = _checked(y[::-1].copy())
    return out


@functools.lru_cache(maxsize=None)
def family(name):
    """-> dict column name -> column (read-only fp64 array), in a fixed order"""
    cols = {}
    if name in ("collapse_short", "collapse_long"):
        for L in COLLAPSE_L:
            if (L <= 26) == (name == "collapse_short"):
                for d in collapse_depths(L):
                    cols[f"collapse-L{L}-d{d}"] = collapse(L, d)
        if name == "collapse_short":
            for d in (1, RC + 1, DIP_L):
                for where in (-1, 0, 1):
                    cols[f"pause-d{d}-at{where:+d}"] = collapse_at_pause(d, where)
        return _with_mirrors(cols)
    if name == "flank":
        return _with_mirrors({"flank": flank(), "flank-collapse": flank_collapse()})
    if name == "ties":
        for n, a in TIES_ODD:
            cols[f"tie-n{n}-a{a}"] = tie_odd(n, a)
        cols["tie-n5-a2-x4"] = tie_odd(5, 2, 4.0)
        cols["tie-n17-a5-x4"] = tie_odd(17, 5, 4.0)
        for n, a in TIES_EVEN:
            cols[f"tie-n{n}-a{a}"] = tie_even(n, a)
        for n in CONST_N:
            cols[f"const-n{n}"] = _checked(np.full(n, 0.75))
            cols[f"negconst-n{n}"] = _checked(np.full(n, -0.75))
            cols[f"zero-n{n}"] = _checked(np.zeros(n))
        cols["plateau-1"], cols["plateau-3"] = plateau(1), plateau(3)
        return _with_mirrors(cols)
    if name == "edges":
        for n in EDGE_N:
            shapes = ("inc", "dec", "peak_first", "peak_last") if n >= 3 else ("inc", "dec")
            for shape in shapes:
                cols[f"edge-n{n}-{shape}"] = edge(n, shape)
        cols["edge-n1-pos"], cols["edge-n2-pair"] = _checked([3.0]), _checked([-2.0, -1.0])
        return cols
    if name == "wave_span":
        # the columns of the layout whose wave spans slabs of 1 to 300 rows (and of the in-phase layout)
        long_a, long_b = collapse(294, RC + NRF, step=1.0 / 32.0), collapse(294, RC + 1, step=1.0 / 32.0)
        mid = collapse(124, 124)
        cols.update({"span-n1-a": _checked([3.0]), "span-n1-b": _checked([-3.0]), "span-n1-c": _checked([0.5]),
                     "span-n2-a": _checked([1.0, 2.0]), "span-n2-b": _checked([2.0, -1.0]), "span-n2-c": _checked([-1.0, -2.0]),
                     "span-n300-a": long_a, "span-n300-b": _checked(long_a[::-1].copy()), "span-n300-c": long_b,
                     "span-n65-a": tie_odd(65, 17), "span-n65-b": collapse(59, RC + 1), "span-n65-c": edge(65, "peak_last"),
                     "span-n130-a": mid, "span-n130-b": _checked(mid[::-1].copy()), "span-n130-c": tie_even(130, 62),
                     "inphase-collapse": collapse(100, RC + NRF), "inphase-flank": flank(), "inphase-flank-collapse": flank_collapse()})
        for k in INPHASE:
            cols[k + "/mirror"] = _checked(cols[k][::-1].copy())
        return cols
    raise KeyError(name)


FAMILIES = ("collapse_short", "collapse_long", "flank", "ties", "edges")
ALL_FAMILIES = FAMILIES + ("wave_span",)


def is_tie(name):
    """declared tie columns: two mirrored optimal splits with different fits (the constant columns: with equal fits)"""
    return name.startswith(("tie-", "span-n65-a", "span-n130-c", "const-", "negconst-", "zero-"))


def is_flat(name):
    return name.startswith(("const-", "negconst-", "zero-"))


def all_columns():
    """every designed column once, in the order of the fixture tests/golden/unimodal_edges.npz"""
    out = {}
    for fam in ALL_FAMILIES:
        for name, y in family(fam).items():
            assert name not in out
            out[name] = y
    return out


# ---- the split search in fp64 -----------------------------------------------------------------------------------------------------
def split_margin(y, nonneg):
    """-> [(total, split, fit)] over all splits t = 0 .. n, sorted by (total, split): the totals the oracle compares
    (oracle/aoadmm_oracle.py: unimodal_vector_py) with the fit each split yields"""
    y = np.asarray(y, dtype=np.float64)
    n = len(y)
    lvL, stL, eL = orc._prefix_isotonic_py(y, nonneg)
    lvR, stR, eR = orc._prefix_isotonic_py(y[::-1], nonneg)
    out = []
    for t in range(n + 1):
        fit = np.concatenate([orc._fit_from_prefix(t, lvL, stL), orc._fit_from_prefix(n - t, lvR, stR)[::-1]])
        out.append((float(eL[t] + eR[n - t]), t, fit))
    return sorted(out, key=lambda e: (e[0], e[1]))


# ---- packings ---------------------------------------------------------------------------------------------------------------------
# name: (rank, number of slabs or None, lanes mod 64 or None, aux / dual one float into their buffers)
PACKINGS = {
    "r1_64k+1": (1, None, 1, False),   # n_slabs r = 64 k + 1: one live lane in the last wave
    "r1_64k-1": (1, None, 63, True),   # 64 k - 1: one idle lane
    "r3": (3, None, None, False),
    "r17_5waves": (17, 16, None, False),  # nwav mod 4 = 1, 2, 3 under four waves per workgroup
    "r17_6waves": (17, 19, None, True),
    "r17_7waves": (17, 23, None, False),
    "r64": (64, None, None, True),
}
SPECIAL = ("span_r3", "inphase_r64")  # layouts with columns of their own (family "wave_span")
SPAN_J = (1, 300, 2, 65, 1, 130)
INPHASE = ("inphase-collapse", "inphase-flank", "inphase-flank-collapse")


def fillers():
    """the edge columns of 3 to 9 elements"""
    return {k: y for k, y in family("edges").items() if 3 <= len(y) <= 9}


def _layout(fam, packing):
    """-> (rank, [[column name per lane] per slab])"""
    if packing == "span_r3":
        by_n = {n: [k for k in family("wave_span") if k.startswith(f"span-n{n}-")] for n in set(SPAN_J)}
        seen = {n: 0 for n in by_n}
        slabs = []
        for n in SPAN_J:  # the second slab of one row carries the same three columns in another order
            slabs.append(by_n[n][seen[n]:] + by_n[n][:seen[n]])
            seen[n] += 1
        return 3, slabs
    if packing == "inphase_r64":
        return 64, [[k + m] * 64 for k in INPHASE for m in ("", "/mirror")]  # all 64 lanes of a wave in step
    r, n_slabs, lanes_mod, _ = PACKINGS[packing]
    by_len = {}
    for name, y in family(fam).items():
        by_len.setdefault(len(y), []).append(name)
    slabs = []
    for n in sorted(by_len):
        names = by_len[n]
        for s in range(-(-len(names) // r)):
            slabs.append([names[(s * r + c) % len(names)] for c in range(r)])
    # short and long slabs alternate, so that the lanes of a wave differ in length and in (L, d)
    order = [slabs[i // 2] if i % 2 == 0 else slabs[-1 - i // 2] for i in range(len(slabs))]
    slabs = list(order)
    # the slabs that bring the layout to its lane count carry short edge columns: few rows, and lanes of another length
    fill = fillers()
    fill_len = sorted({len(y) for y in fill.values()})
    i = 0
    while (n_slabs is not None and len(slabs) < n_slabs) or (lanes_mod is not None and (len(slabs) * r) % 64 != lanes_mod):
        names = [k for k, y in fill.items() if len(y) == fill_len[i % len(fill_len)]]
        slabs.append([names[(i + c) % len(names)] for c in range(r)])
        i += 1
    assert n_slabs is None or len(slabs) == n_slabs, (fam, packing, len(slabs))
    return r, slabs


@functools.lru_cache(maxsize=None)
def problem(fam, packing):
    """the columns of family `fam` tiled over layout `packing` -> dict: rank r, row_ptr, names (per slab, per lane), float64 Y,
    float32 B and U with B + U == Y exactly, float32 X, A, C for the engine, unaligned"""
    import zlib

    cols = dict(fillers())
    cols.update(family("wave_span" if packing in SPECIAL else fam))
    r, slabs = _layout(fam, packing)
    J = np.array([len(cols[s[0]]) for s in slabs], dtype=np.int64)
    row_ptr = np.concatenate([[0], np.cumsum(J)]).astype(np.int64)
    Y = np.concatenate([np.stack([cols[name] for name in s], axis=1) for s in slabs])
    rng = np.random.RandomState(zlib.crc32(f"{fam}/{packing}".encode()) & 0x7FFFFFFF)
    U = rng.randint(-64, 65, size=Y.shape) / 64.0
    B = Y - U
    B32, U32 = B.astype(np.float32), U.astype(np.float32)
    N, I = int(row_ptr[-1]), len(J)
    out = dict(Y=Y, B=B32, U=U32, row_ptr=row_ptr, X=rng.rand(N, K).astype(np.float32),
               A=(rng.rand(I, r) + 0.1).astype(np.float32), C=rng.rand(K, r).astype(np.float32))
    for v in out.values():
        v.setflags(write=False)
    out.update(r=r, names=slabs, unaligned=PACKINGS[packing][3] if packing in PACKINGS else packing == "span_r3")
    return out


def cases():
    """(family, packing) of every problem of the GPU test"""
    return [(f, p) for f in FAMILIES for p in PACKINGS] + [("wave_span", p) for p in SPECIAL]


def reference(p, nonneg):
    """the oracle's regression of every slab of problem p, fp64"""
    rp = p["row_ptr"]
    return np.concatenate([orc.unimodal_columns(p["Y"][s:e], nonneg) for s, e in zip(rp[:-1], rp[1:])])
