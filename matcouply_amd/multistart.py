"""Many fits of one problem in one launch: `cmf_aoadmm_multistart`, `cmf_aoadmm_grid`, their `parafac2_aoadmm_*` forms,
`best_start` and `parafac2_als_multistart` (not in the reference: its examples hand-roll these loops), all readable through
decomposition.py too.  resampling.py (a weight per matrix and job) and missing.py (a mask per job) build their fused calls from
the same parts: `_StateLayout`, a job's slice of the state matrix; `_multistart_fused` and `_pf2als_fused`, which build the jobs
on the host, launch them and read the results; `_fused_serves`, the ``method=`` decision."""
from collections import namedtuple
import inspect

import numpy as np

from . import _engine, decomposition as dec, penalties
from ._utils import check_random_state, shape, to_numpy, torch
from .coupled_matrices import CoupledMatrixFactorization
from .decomposition import DiagnosticMetrics, PackedMatrices

# ------------------------------------------------------------------------------------------------------------
# many random starts of one problem
# ------------------------------------------------------------------------------------------------------------
# fused starts are served up to this many elements of X (sum J_i * K): the largest shape of profiles/multistart_rate.txt, where
# 16 fused starts take 0.42 x the time of 16 sequential calls.  method="auto" takes the fused kernel from the first start up to
# _MULTISTART_AUTO_ANY_N elements (examples' size: 1 fused start 0.53 x one call) and from _MULTISTART_AUTO_MIN_N starts above
# (one fused start is a whole fit on one CU: 1.9 x one call at 2^16 elements, 6.3 x at 2^18; the crossovers lie at 2 and 7 starts)
_MULTISTART_MAX_ELEMENTS = 1 << 18
_MULTISTART_AUTO_ANY_N = 1 << 13
_MULTISTART_AUTO_MIN_N = 8
_MULTISTART_KINDS = (_engine.PEN_NN, _engine.PEN_BOX, _engine.PEN_L1, _engine.PEN_L2BALL, _engine.PEN_PARAFAC2)
_KIND_NAMES = {_engine.PEN_NN: "NonNegativity", _engine.PEN_BOX: "Box", _engine.PEN_L1: "L1Penalty", _engine.PEN_L2BALL: "L2Ball",
               _engine.PEN_PARAFAC2: "Parafac2"}


def _check_method(method):
    if method not in ("auto", "fused", "sequential"):
        raise ValueError(f'method must be "auto", "fused" or "sequential", not {method!r}')


def _check_start_keywords(name, kwargs, where="", check_init=True):
    """an entry point that draws one start per random state takes no random_state and, unless it reads a fitted model from
    `init` itself (check_init False), init="random" alone; `where`: " in param_grid[g]" for the keywords of a grid point"""
    if "random_state" in kwargs:
        raise TypeError(f"{name} takes random_states, not random_state{where}")
    init = kwargs.get("init", "random")
    if check_init and not (isinstance(init, str) and init == "random"):
        raise ValueError(f"{name} needs init=\"random\" (init={init!r}{where} gives the same start every time)")


def _parafac2_keywords(name, kwargs, points=()):
    """the cmf_aoadmm keywords of a parafac2_aoadmm_* entry point: parafac2=True, which the caller may not pass, and
    parafac2_aoadmm's default l2_penalty=0 unless one of the grid points `points` sets l2_penalty"""
    if "parafac2" in kwargs or any("parafac2" in p for p in points):
        raise TypeError(f"{name}() got an unexpected keyword argument 'parafac2'")
    kwargs = dict(kwargs, parafac2=True)
    if not any("l2_penalty" in p for p in points):
        kwargs.setdefault("l2_penalty", 0)
    return kwargs


def _rows_and_K(matrices):
    """([J_i], K) of a list of matrices or a PackedMatrices"""
    rows = [int(matrices.row_ptr[i + 1] - matrices.row_ptr[i]) for i in range(len(matrices))] \
        if isinstance(matrices, PackedMatrices) else [int(shape(m)[0]) for m in matrices]
    return rows, int(shape(matrices[0])[1])


def _fused_serves(name, method, reason, n_jobs, few):
    """The ``method=`` decision of every entry point: True to run the `n_jobs` jobs in the fused kernel, False for the sequential
    loop.  `reason()`, not called for "sequential", is the sentence why the kernel does not serve the call, or None; `few(n_jobs)`
    the sentence why so few jobs run faster one by one, or None: it counts for "auto" alone.  "fused" with a reason raises."""
    _check_method(method)
    if method == "sequential":
        return False
    why = reason()
    if why is None and method == "auto":
        why = few(n_jobs)
    if why is not None and method == "fused":
        raise NotImplementedError(f"{name}(method=\"fused\"): {why}")
    return why is None


def _few_aoadmm_jobs(matrices, n_jobs, noun):
    """the rule of the thresholds above, for `n_jobs` fits ("starts" or "jobs") of cmf_aoadmm"""
    if n_jobs < _MULTISTART_AUTO_MIN_N:
        rows, K = _rows_and_K(matrices)
        if sum(rows) * K > _MULTISTART_AUTO_ANY_N:
            return f"{n_jobs} {noun} of {sum(rows) * K} elements run faster one by one"
    return None


def _multistart_unfused_reason(matrices, rank, kw):
    """why the fused kernel cannot run these starts (a sentence), or None.  Looks at the arguments only: no device call."""
    if dec._test_engine_factory() is not None:
        return "a substitute compute engine is installed (the fused kernel runs on the HIP engine only)"
    if not 1 <= rank <= _engine.MS_MAX_RANK:
        return f"rank {rank} is above {_engine.MS_MAX_RANK}"
    if kw["verbose"]:
        return "verbose output is not produced by the fused kernel"
    if kw["group"] is not None or kw["gather_A"]:
        return "group= (sharded runs) is not served"
    if kw["arithmetic"] != "auto":
        return f"arithmetic={kw['arithmetic']!r} is not served (the fused kernel is fp64 throughout)"
    if kw["_byproducts"] is not None:
        return "_byproducts is not served"
    if kw["tol"] and kw["absolute_tol"] is None:
        return "tol with absolute_tol=None (the reference raises TypeError in its comparison)"
    if kw["inner_n_iter_max"] is None or int(kw["inner_n_iter_max"]) != kw["inner_n_iter_max"] or kw["n_iter_max"] is None \
            or int(kw["n_iter_max"]) != kw["n_iter_max"] or kw["n_iter_max"] > (1 << 30):
        return "n_iter_max and inner_n_iter_max must be integers"
    try:
        rows, K = _rows_and_K(matrices)
    except Exception:
        return "the matrices are not a list of 2-D arrays"
    if sum(rows) * K > _MULTISTART_MAX_ELEMENTS:
        return f"X has {sum(rows) * K} elements, above the fused bound of {_MULTISTART_MAX_ELEMENTS}"
    try:
        _, regs, _, _ = dec._start_penalties(kw, matrices, rank, np.random.RandomState(0))
    except Exception as e:  # let the sequential path raise the reference's error
        return f"the penalties could not be set up ({type(e).__name__})"
    constant_A, _ = dec._constant_flags(kw["constant_feasibility_penalty"])
    for mode in range(3):
        if len(regs[mode]) > _engine.MCL_MAX_REGS:
            return f"more than {_engine.MCL_MAX_REGS} penalties on mode {mode}"
        for reg in regs[mode]:
            desc = penalties.native_descriptor_of(reg)
            if desc is None or desc[0] not in _MULTISTART_KINDS:
                return f"{type(reg).__name__} on mode {mode} is not served (NonNegativity, Box, L1Penalty, L2Ball, Parafac2)"
            if desc[0] == _engine.PEN_PARAFAC2 and (mode != 1 or min(rows) < rank):
                return "Parafac2 is served on mode 1 with every J_i >= rank"
            if desc[0] == _engine.PEN_L2BALL and mode == 0 and not constant_A:
                return "an L2Ball on mode 0 needs constant_feasibility_penalty"
    if min(rows) == 0:
        # an empty X_i has B_i^T B_i = 0 and a_i = 0: its A row and B_i systems are l2 + rho n times the identity, where rho is
        # the slab's own (zero) feasibility penalty unless it is held constant over the slabs.  Singular systems raise in the
        # reference; the fused kernel would invert them
        l2 = dec._listify(kw["l2_penalty"], "l2_penalty")
        _, constant_B = dec._constant_flags(kw["constant_feasibility_penalty"])
        for mode, constant in ((0, constant_A), (1, constant_B)):
            if not ((l2[mode] or 0) > 0 or (constant and regs[mode])):
                return (f"an empty matrix leaves its mode-{mode} system singular (needs l2_penalty on mode {mode}, or a "
                        "penalty there with constant_feasibility_penalty)")
    return None


def _multistart_options(kw, descs):
    """the mcl_multistart_options of one fit: `kw` the complete cmf_aoadmm keywords, `descs` the native descriptors per mode"""
    o = _engine.MultistartOptions()
    for mode in range(3):
        o.n_regs[mode] = len(descs[mode])
        for k, (kind, nonneg, p0, p1) in enumerate(descs[mode]):
            o.regs[mode][k].kind, o.regs[mode][k].non_negativity = int(kind), int(bool(nonneg))
            o.regs[mode][k].p0, o.regs[mode][k].p1 = float(p0), float(p1)
    l2 = [0 if v is None else v for v in dec._listify(kw["l2_penalty"], "l2_penalty")]
    for mode in range(3):
        o.l2_penalty[mode] = float(l2[mode])
    o.feasibility_penalty_scale = float(kw["feasibility_penalty_scale"])
    o.inner_tol = float(kw["inner_tol"]) if kw["inner_tol"] and kw["inner_tol"] > 0 else 0.0
    o.inner_n_iter_max = int(kw["inner_n_iter_max"])
    o.tol, o.absolute_tol = float(kw["tol"] or 0), float(kw["absolute_tol"] or 0)
    o.feasibility_tol = float(kw["feasibility_tol"] or 0)
    o.constant_A, o.constant_B = dec._constant_flags(kw["constant_feasibility_penalty"])
    o.update_A, o.update_B, o.update_C = bool(kw["update_A"]), bool(kw["update_B_is"]), bool(kw["update_C"])
    o.evaluate_loss_always = bool(kw["return_errors"])
    o.n_iter_max = max(int(kw["n_iter_max"]), 0)
    return o


# a piece of a job's state slice; what: "factor", "aux", "delta" (the Delta of a PARAFAC2: the whole job's, not a matrix's) or
# "dual"; k: the penalty's place on its mode (None for a factor); rows x cols doubles, row-major
_Segment = namedtuple("_Segment", ["what", "mode", "k", "rows", "cols"])


class _StateLayout:
    """One job's slice of the state matrix of mcl_multistart_run and its variants (the layout of matcouply_hip.h): A, B (the B_i
    stacked), C, then mode by mode and penalty by penalty (`kinds`: their PEN_* kinds per mode) the aux, for a PARAFAC2 its
    Delta, and the dual.  `segments` is the one statement of that order on the host besides _engine.multistart_state_len, the
    engine's restatement of the length; packing, unpacking, the zero-weight mask and the length all walk the list."""

    def __init__(self, row_ptr, K, rank, kinds):
        self.row_ptr, self.rank, self.kinds = row_ptr, rank, [list(k) for k in kinds]
        n_rows = (len(row_ptr) - 1, int(row_ptr[-1]), int(K))
        self.segments = [_Segment("factor", mode, None, n_rows[mode], rank) for mode in range(3)]
        for mode in range(3):
            for k, kind in enumerate(self.kinds[mode]):
                self.segments.append(_Segment("aux", mode, k, n_rows[mode], rank))
                if kind == _engine.PEN_PARAFAC2:
                    self.segments.append(_Segment("delta", mode, k, rank, rank))
                self.segments.append(_Segment("dual", mode, k, n_rows[mode], rank))
        self.length = sum(seg.rows * seg.cols for seg in self.segments)
        assert self.length == _engine.multistart_state_len(*n_rows, rank, self.kinds), "multistart: state layout mismatch"

    @classmethod
    def from_names(cls, row_ptr, K, rank, names):
        """the layout from the penalties' names per mode as _multistart_layout gives them, before anything is drawn"""
        kinds = {name: kind for kind, name in _KIND_NAMES.items()}
        return cls(row_ptr, K, rank, [[kinds[name.split("(")[0]] for name in names[mode]] for mode in range(3)])

    def pack(self, cmf, auxes, duals):
        """a start as _start_penalties draws it -> its float64 slice, every value through fp32 (cmf_aoadmm's state is fp32)"""
        f32 = lambda a: np.asarray(to_numpy(a), dtype=np.float32).astype(np.float64).ravel()
        parts = []
        for seg in self.segments:
            v = cmf[1][seg.mode] if seg.what == "factor" else (duals if seg.what == "dual" else auxes)[seg.mode][seg.k]
            if isinstance(v, tuple):  # the aux of a PARAFAC2: (P_i list, Delta)
                v = v[seg.what == "delta"]
            parts.append(np.concatenate([f32(x) for x in v]) if seg.mode == 1 and seg.what != "delta" else f32(v))
            assert parts[-1].size == seg.rows * seg.cols, f"multistart: the start's {seg} has {parts[-1].size} values"
        return np.concatenate(parts)

    def unpack(self, row):
        """one row of the state matrix (a tensor on any device) -> A, B, C and per mode the (kind, aux, aux2, dual) of every
        penalty, as _admm_vars_out takes them (aux2: the Delta of a PARAFAC2, else None); all views of `row`"""
        pieces = torch.split(row, [seg.rows * seg.cols for seg in self.segments])
        at = {seg[:3]: t.view(seg.rows, seg.cols) for seg, t in zip(self.segments, pieces)}
        admm = [[(kind, at["aux", mode, k], at.get(("delta", mode, k)), at["dual", mode, k])
                 for k, kind in enumerate(self.kinds[mode])] for mode in range(3)]
        return at["factor", 0, None], at["factor", 1, None], at["factor", 2, None], admm

    def zero_weight_mask(self, w):
        """which doubles of the slice belong to a matrix of weight 0: its row of A, its B_i and its rows of every aux and dual
        of modes 0 and 1 (its P_i for PARAFAC2; Delta and mode 2 are the whole job's)"""
        dead = np.asarray(w) == 0
        dead_rows = {0: dead, 1: np.repeat(dead, np.diff(self.row_ptr))}
        return np.concatenate([np.repeat(dead_rows[seg.mode], seg.cols) if seg.mode in dead_rows and seg.what != "delta"
                               else np.zeros(seg.rows * seg.cols, dtype=bool) for seg in self.segments])


# the jobs of one launch: their _StateLayout; per job its start (_StateLayout.pack), complete cmf_aoadmm keywords, MultistartOptions
_Jobs = namedtuple("_Jobs", ["layout", "vectors", "kws", "options"])


def _build_jobs(matrices, rank, random_states, kws):
    """The jobs of one launch, on the host (no device call): every keyword set of `kws` (complete cmf_aoadmm keywords with one
    state layout) from every start; job g * len(random_states) + s is kws[g] from random_states[s], drawn in that order."""
    rows, K = _rows_and_K(matrices)
    row_ptr = np.concatenate([[0], np.cumsum(rows)]).astype(np.int64)
    layout, vectors, job_kws, options = None, [], [], []
    for kw in kws:
        for rs in random_states:
            cmf, regs, auxes, duals = dec._start_penalties(kw, matrices, rank, check_random_state(rs))
            descs = [[penalties.native_descriptor_of(r) for r in regs[m]] for m in range(3)]
            kinds = [[d[0] for d in descs[m]] for m in range(3)]
            layout = layout or _StateLayout(row_ptr, K, rank, kinds)
            assert kinds == layout.kinds, "multistart: the jobs differ in their state layout"
            vectors.append(layout.pack(cmf, auxes, duals))
            job_kws.append(kw)
        options += [_multistart_options(kw, descs)] * len(random_states)
    return _Jobs(layout, vectors, job_kws, options)


def _launch_jobs(matrices, jobs, run):
    """X and the jobs' starts on the device and the one engine call: ``run(X, row_ptr, rank, options, state)`` with `options`
    the list of every job's MultistartOptions -> the state matrix (on the device) and diag, n_iter, stop as host arrays"""
    X, row_ptr = dec._pack(matrices, dec._device())
    state = torch.from_numpy(np.stack(jobs.vectors)).to(X.device)
    diag, n_iter, stop = run(X, row_ptr, jobs.layout.rank, jobs.options, state)
    return state, diag.cpu().numpy(), n_iter.cpu().numpy(), stop.cpu().numpy()


def _job_results(matrices, jobs, state, diag, n_iter, stop):
    """per job what cmf_aoadmm returns for its keywords, from its state row and its rows of the tables of the launch"""
    out = dec._Out(matrices)
    row_ptr, kinds = jobs.layout.row_ptr, jobs.layout.kinds
    results = []
    for s, kw in enumerate(jobs.kws):
        A, B, C, admm = jobs.layout.unpack(state[s])
        result = [CoupledMatrixFactorization((None, (out(A), out.split(B, row_ptr), out(C))))]
        if kw["return_admm_vars"]:
            result.append(dec._admm_vars_out(out, row_ptr, admm))
        if kw["return_errors"]:
            n, code = int(n_iter[s]), int(stop[s])
            d = diag[s, : n + 1]
            flags = d[:, 2].astype(np.int64)
            kept = [0] + [t for t in range(1, n + 1) if flags[t] & 2]
            gaps = [tuple([np.float64(d[t, 4 + m * _engine.MCL_MAX_REGS + k]) for k in range(len(kinds[m]))] for m in range(3))
                    for t in range(n + 1)]
            result.append(DiagnosticMetrics(
                rec_errors=[float(d[t, 0]) for t in kept], feasibility_gaps=gaps, regularized_loss=[float(d[t, 1]) for t in kept],
                satisfied_stopping_condition=bool(code) if (kw["tol"] or kw["absolute_tol"]) else None,
                satisfied_feasibility_condition=dec._check_feasibility(gaps[-1], kw["feasibility_tol"]) if kw["feasibility_tol"] else None,
                message=dec._StopRule.message_of(code), n_iter=n))
        results.append(result[0] if len(result) == 1 else tuple(result))
    return results


def _multistart_fused(matrices, rank, random_states, kws, run, zero_weights=None):
    """every keyword set of `kws` from every start (both not empty: the jobs of _build_jobs) in one launch, through the engine
    call the caller names (`run`: see _launch_jobs).  `zero_weights` [n_jobs, I] (cmf_aoadmm_resample): the start is the full
    problem's draw with the part of every matrix of weight 0 in its row set to zero afterwards."""
    jobs = _build_jobs(matrices, rank, random_states, kws)
    if zero_weights is not None:
        for v, w in zip(jobs.vectors, zero_weights):
            v[jobs.layout.zero_weight_mask(w)] = 0.0
    return _job_results(matrices, jobs, *_launch_jobs(matrices, jobs, run))


def cmf_aoadmm_multistart(matrices, rank, random_states, *, method="auto", **cmf_aoadmm_kwargs):
    """Fit the same problem from several random starts: element ``s`` of the list returned is what
    ``cmf_aoadmm(matrices, rank, random_state=random_states[s], **cmf_aoadmm_kwargs)`` returns (same tuple structure, array
    types and dtypes).  Start ``s`` draws its initial factors, auxiliary and dual variables with the initialisers of
    ``cmf_aoadmm``, in its order.  The usual selection afterwards: the lowest ``regularized_loss[-1]`` among the starts with
    ``satisfied_stopping_condition``.

    ``method="sequential"`` calls ``cmf_aoadmm`` once per start (every option).  ``method="fused"`` fits all starts in one launch
    of a HIP kernel, one workgroup per start, in fp64 (csrc/multistart.hip); it serves rank <= 16, the penalties NonNegativity,
    Box, L1Penalty, L2Ball (mode 0: with ``constant_feasibility_penalty``) and Parafac2 on the B_i (every J_i >= rank), and X of
    at most ``_MULTISTART_MAX_ELEMENTS`` elements; anything else raises ``NotImplementedError`` before the device is touched
    (``verbose``, ``group=``, ``arithmetic`` other than ``"auto"``, Unimodality, TV, GeneralizedL2, UnitSimplex, user penalty
    classes).  ``method="auto"`` takes the fused kernel when it serves the call, else the sequential loop.  Only
    ``init="random"``: any other start would be the same N times (``ValueError``).
    """
    _check_method(method)
    _check_start_keywords("cmf_aoadmm_multistart", cmf_aoadmm_kwargs)
    random_states = list(random_states)
    kw = dec._cmf_kwargs(cmf_aoadmm_kwargs)
    if _fused_serves("cmf_aoadmm_multistart", method, lambda: _multistart_unfused_reason(matrices, rank, kw), len(random_states),
                     lambda n: _few_aoadmm_jobs(matrices, n, "starts")):
        run = lambda X, row_ptr, r, options, state: _engine.multistart_run(X, row_ptr, r, options[0], state)  # one keyword set
        return _multistart_fused(matrices, rank, random_states, [kw], run) if random_states else []
    return [dec.cmf_aoadmm(matrices, rank, random_state=rs, **cmf_aoadmm_kwargs) for rs in random_states]


def parafac2_aoadmm_multistart(matrices, rank, random_states, *, method="auto", **parafac2_aoadmm_kwargs):
    """:func:`cmf_aoadmm_multistart` with the PARAFAC2 constraint on mode 1: element ``s`` is what
    ``parafac2_aoadmm(matrices, rank, random_state=random_states[s], **parafac2_aoadmm_kwargs)`` returns."""
    kwargs = _parafac2_keywords("parafac2_aoadmm_multistart", parafac2_aoadmm_kwargs)
    return cmf_aoadmm_multistart(matrices, rank, random_states, method=method, **kwargs)


# ------------------------------------------------------------------------------------------------------------
# a grid of penalty strengths x random starts: the loop users write around the multi-start one
# ------------------------------------------------------------------------------------------------------------
# keywords that decide the shape of the result or are not options of one fit: common to the whole grid only
_GRID_COMMON_ONLY = ("return_errors", "return_admm_vars", "verbose", "group")
# device memory a fused grid may ask for (state, scratch, diagnostics and options of all jobs).  A Cartesian product grows
# quickly, and every job holds its slices for the whole launch although only a few hundred workgroups are resident at a time.
# 8 GiB is 1 / 36 of the MI355X's 288 GB and leaves the rest to the process's other tensors; it holds ~50 000 jobs of the
# examples' size with 1000 iterations of diagnostics (~165 kB each) and ~1300 of 64 x 64 x 64 at rank 16 with four penalties
# per mode (~6.5 MB each).  A larger grid runs as several calls
_GRID_MAX_BYTES = 1 << 33


def _grid_keywords(name, param_grid, common):
    """the grid's keyword sets: [(point, point merged into the common keywords as complete cmf_aoadmm keywords)], checked"""
    _check_start_keywords(name, common)
    points = []
    for g, point in enumerate(param_grid):
        if not isinstance(point, dict):
            raise TypeError(f"{name}: param_grid[{g}] is a {type(point).__name__}, not a dict of cmf_aoadmm keywords")
        _check_start_keywords(name, point, f" in param_grid[{g}]")
        for key in point:
            if key in _GRID_COMMON_ONLY:
                raise ValueError(f"{name}: {key!r} in param_grid[{g}] is not an option of one fit; pass it once for the whole grid")
            if key in common:
                raise TypeError(f"{name} got {key!r} both in param_grid[{g}] and as a common keyword")
        points.append((point, dec._cmf_kwargs({**common, **point})))
    return points


def _multistart_layout(matrices, rank, kw):
    """what the state layout and the phases of the fused kernel follow from, per mode: the (kind, non-negativity) of every
    penalty in order and whether the mode is updated; plus the constant-feasibility-penalty flags"""
    _, regs, _, _ = dec._start_penalties(kw, matrices, rank, np.random.RandomState(0))
    modes = []
    for mode, updated in enumerate((kw["update_A"], kw["update_B_is"], kw["update_C"])):
        descs = [penalties.native_descriptor_of(reg) for reg in regs[mode]]
        modes.append((tuple(_KIND_NAMES[d[0]] + ("(non_negativity)" if d[1] and d[0] != _engine.PEN_NN else "") for d in descs),
                      "updated" if updated else "not updated"))
    return modes, dec._constant_flags(kw["constant_feasibility_penalty"])


def _grid_unfused_reason(matrices, rank, kws, n_starts):
    """why the fused kernel cannot run this grid in one launch (a sentence), or None.  No device call."""
    for g, kw in enumerate(kws):
        reason = _multistart_unfused_reason(matrices, rank, kw)
        if reason is not None:
            return f"grid point {g}: {reason}"
    first = _multistart_layout(matrices, rank, kws[0])
    for g, kw in enumerate(kws[1:], 1):
        modes, constant = _multistart_layout(matrices, rank, kw)
        for mode in range(3):
            if modes[mode] != first[0][mode]:
                return (f"grid point {g} has the penalties {list(modes[mode][0])} ({modes[mode][1]}) on mode {mode}, grid point 0 "
                        f"{list(first[0][mode][0])} ({first[0][mode][1]}): one launch holds one state layout (a strength of 0 or "
                        "None drops its penalty)")
        if constant != first[1]:
            return f"grid point {g} differs from grid point 0 in constant_feasibility_penalty"
    rows, K = _rows_and_K(matrices)
    state_len = _StateLayout.from_names(np.concatenate([[0], np.cumsum(rows)]), K, rank, [names for names, _ in first[0]]).length
    diag_len = (max(max(int(kw["n_iter_max"]), 0) for kw in kws) + 1) * _engine.MS_DIAG
    per_job = 8 * (state_len + _engine.multistart_scratch_len(len(rows), sum(rows), K, rank) + diag_len) + _engine.MS_OPTIONS_BYTES
    n_jobs = len(kws) * n_starts
    if n_jobs * per_job > _GRID_MAX_BYTES or n_jobs >= 1 << 31:
        return (f"{n_jobs} jobs of {per_job} bytes each (state, scratch, diagnostics) need more than the {_GRID_MAX_BYTES} bytes "
                "a fused grid may take; split the grid")
    return None


def cmf_aoadmm_grid(matrices, rank, param_grid, random_states, *, method="auto", **cmf_aoadmm_kwargs):
    """Fit the same data over a grid of option values, every grid point from several random starts: ``result[g][s]`` is what
    ``cmf_aoadmm(matrices, rank, random_state=random_states[s], **cmf_aoadmm_kwargs, **param_grid[g])`` returns (same tuple
    structure, array types and dtypes, as for a start of :func:`cmf_aoadmm_multistart`).  ``param_grid`` is a sequence of dicts
    of ``cmf_aoadmm`` keywords, one per grid point (``itertools.product`` builds a Cartesian one); a keyword stands either in
    the grid points or among the common ones (``TypeError`` for both), and ``return_errors``, ``return_admm_vars``,
    ``verbose`` and ``group`` are common only (``ValueError``).  An empty grid gives ``[]``.  :func:`best_start` picks a grid
    point's start by the examples' rule.  Random-state objects among ``random_states`` (rather than seeds) are drawn from
    grid point by grid point, in the order of the sequential method.

    ``method="sequential"`` calls ``cmf_aoadmm`` once per grid point and start (every option).  ``method="fused"`` fits all
    ``len(param_grid) * len(random_states)`` jobs in one launch of the kernel of :func:`cmf_aoadmm_multistart`, one workgroup
    per job with options of its own (mcl_multistart_run_grid).  It serves what ``cmf_aoadmm_multistart(method="fused")`` serves
    for every grid point, and needs all grid points to parse to the same penalty classes, non-negativity flags and order on
    every mode, the same ``update_*`` and the same ``constant_feasibility_penalty``: the jobs share one state layout.  The
    strengths, bounds, ``l2_penalty``, ``feasibility_penalty_scale``, tolerances and iteration limits may differ.  A strength of
    0 or ``None`` drops its penalty when the keywords are parsed, so ``l1_penalty=0`` beside ``0.1`` is two layouts.  A grid
    whose jobs need more than ``_GRID_MAX_BYTES`` of device memory is not served either.  Each of these raises
    ``NotImplementedError`` naming the grid point, before the device is touched.  ``method="auto"`` takes the fused kernel when
    it serves the call and the jobs are many or small enough (the rule of ``cmf_aoadmm_multistart`` on the number of jobs),
    else the sequential loop.  A job's result does not depend on the grid it is part of.
    """
    return _aoadmm_grid("cmf_aoadmm_grid", matrices, rank, param_grid, random_states, method, cmf_aoadmm_kwargs)


def _aoadmm_grid(name, matrices, rank, param_grid, random_states, method, common):
    _check_method(method)
    points = _grid_keywords(name, list(param_grid), common)
    random_states = list(random_states)
    if not points:
        return []
    if not random_states:
        return [[] for _ in points]
    kws, n = [kw for _, kw in points], len(random_states)
    if _fused_serves(name, method, lambda: _grid_unfused_reason(matrices, rank, kws, n), len(kws) * n,
                     lambda n_jobs: _few_aoadmm_jobs(matrices, n_jobs, "jobs")):
        flat = _multistart_fused(matrices, rank, random_states, kws, _engine.multistart_run_grid)
        return [flat[g * n: (g + 1) * n] for g in range(len(kws))]
    return [[dec.cmf_aoadmm(matrices, rank, random_state=rs, **common, **point) for rs in random_states] for point, _ in points]


def parafac2_aoadmm_grid(matrices, rank, param_grid, random_states, *, method="auto", **parafac2_aoadmm_kwargs):
    """:func:`cmf_aoadmm_grid` with the PARAFAC2 constraint on mode 1: ``result[g][s]`` is what ``parafac2_aoadmm(matrices, rank,
    random_state=random_states[s], **parafac2_aoadmm_kwargs, **param_grid[g])`` returns."""
    param_grid = list(param_grid)
    common = _parafac2_keywords("parafac2_aoadmm_grid", parafac2_aoadmm_kwargs, [p for p in param_grid if isinstance(p, dict)])
    if "l2_penalty" not in common:  # a grid point sets it: the others get the default of parafac2_aoadmm
        param_grid = [dict(p, l2_penalty=0) if isinstance(p, dict) and "l2_penalty" not in p else p for p in param_grid]
    return _aoadmm_grid("parafac2_aoadmm_grid", matrices, rank, param_grid, random_states, method, common)


def best_start(results):
    """The examples' selection among the starts of one grid point (or of :func:`cmf_aoadmm_multistart`), fitted with
    ``return_errors=True``: the index of the lowest ``regularized_loss[-1]`` among the starts with
    ``satisfied_stopping_condition`` (the first of equal ones), or ``None`` when no start satisfied it."""
    best, best_loss = None, None
    for s, result in enumerate(results):
        diag = next((x for x in result if isinstance(x, DiagnosticMetrics)), None) if isinstance(result, tuple) else None
        if diag is None:
            raise ValueError("best_start needs results fitted with return_errors=True")
        if diag.satisfied_stopping_condition and (best is None or diag.regularized_loss[-1] < best_loss):
            best, best_loss = s, diag.regularized_loss[-1]
    return best


# ------------------------------------------------------------------------------------------------------------
# many random starts of parafac2_als (csrc/pf2als_multistart.hip)
# ------------------------------------------------------------------------------------------------------------
# method="auto" takes the fused kernel from the first start while elements of X x rank <= _PF2ALS_MS_AUTO_ANY_WORK, and from
# _PF2ALS_MS_AUTO_MIN_N starts above (profiles/pf2als_multistart_rate.txt: one fused start is 0.91 x one call at the
# semiconductor size, 2.5e5 elements x rank 2, and 5.1 x at 64 x 64 x 64 rank 8, where the crossover lies at about 5 starts)
_PF2ALS_MS_AUTO_ANY_WORK = 1 << 19
_PF2ALS_MS_AUTO_MIN_N = 8
_PF2ALS_SIGNATURE = inspect.signature(dec.parafac2_als)


def _pf2als_kwargs(kwargs):
    """the keyword arguments of a parafac2_als call as a complete dict of its parameters; TensorLy options stay in "kwargs"
    (checked by _parafac2_als_options)"""
    return dec._cmf_kwargs(kwargs, _PF2ALS_SIGNATURE)


def _pf2als_tolerances(kw):
    return (float(kw["tol"]) if kw["tol"] else 0.0), (float(kw["absolute_tol"]) if kw["absolute_tol"] else 0.0)


def _pf2als_unfused_reason(rank, rows, K):
    """why the fused kernel cannot run these starts (a sentence), or None.  Looks at the arguments only: no device call."""
    if dec._test_engine_factory() is not None:
        return "a substitute compute engine is installed (the fused kernel runs on the HIP engine only)"
    if rank > _engine.PF2ALS_MS_MAX_RANK:
        return f"rank {rank} is above {_engine.PF2ALS_MS_MAX_RANK}"
    if sum(rows) * K > _MULTISTART_MAX_ELEMENTS:
        return f"X has {sum(rows) * K} elements, above the fused bound of {_MULTISTART_MAX_ELEMENTS}"
    return None


def _pf2als_fused_serves(name, method, rank, rows, K, n_jobs, noun):
    """_fused_serves for the entry points of the PARAFAC2-ALS kernel, with the rule of the thresholds above"""
    few = lambda n: (f"{n} {noun} of {sum(rows) * K} elements at rank {rank} run faster one by one"
                     if n < _PF2ALS_MS_AUTO_MIN_N and sum(rows) * K * rank > _PF2ALS_MS_AUTO_ANY_WORK else None)
    return _fused_serves(name, method, lambda: _pf2als_unfused_reason(rank, rows, K), n_jobs, few)


def _pf2als_fused(matrices, rank, starts, modes, kw, scale=None):
    """every start (A0, B0, C0) of `starts` as one job of the fused PARAFAC2-ALS kernel -> per job what parafac2_als returns for
    the complete keywords `kw`.  `scale` [n_jobs, I], the square roots of a weight per job and matrix: job j fits the matrices
    scale[j, i] X_i from A0 with its rows scaled, and row i of its A is divided back (exact zeros where the scale is 0)."""
    device = dec._device()
    X, row_ptr = dec._pack(matrices, device)
    I, K = len(row_ptr) - 1, int(X.shape[1])
    if scale is not None:
        starts = [(A0 * scale[j][:, None], B0, C0) for j, (A0, B0, C0) in enumerate(starts)]
    factors = torch.from_numpy(np.stack([np.concatenate([np.ravel(F) for F in st]) for st in starts])).to(device)
    tol, absolute_tol = _pf2als_tolerances(kw)
    limits = (int(kw["n_iter_max"]), int(kw["n_iter_parafac"]), tol, absolute_tol, modes)
    if scale is None:
        P, errors, n_iter = _engine.pf2als_multistart_run(X, row_ptr, rank, factors, *limits)
    else:
        slab_scale = torch.from_numpy(np.ascontiguousarray(scale)).to(device)
        P, errors, n_iter = _engine.pf2als_multistart_run_weighted(X, row_ptr, rank, factors, slab_scale, *limits)
    errors, n_iter = errors.cpu().numpy(), n_iter.cpu().numpy()
    out = dec._Out(matrices)
    results = []
    for j in range(len(starts)):
        f = factors[j]
        A, B, C = f[: I * rank].view(I, rank), f[I * rank: (I + rank) * rank].view(rank, rank), f[(I + rank) * rank:].view(K, rank)
        if scale is not None:
            s = slab_scale[j][:, None]
            A = torch.where(s > 0, A / torch.where(s > 0, s, torch.ones_like(s)), torch.zeros_like(A))
        result = (None, (out(A), out(B), out(C)), out.split(P[j], row_ptr))
        if kw["return_errors"]:
            result = (result, [float(e) for e in errors[j, : int(n_iter[j]) if tol > 0 else 0]])
        results.append(result)
    return results


def parafac2_als_multistart(matrices, rank, random_states, *, method="auto", **parafac2_als_kwargs):
    """Fit one unconstrained PARAFAC2-ALS problem from several random starts: element ``s`` of the list returned is what
    ``parafac2_als(matrices, rank, random_state=random_states[s], **parafac2_als_kwargs)`` returns (same tuple structure, array
    types and dtypes).  The usual selection afterwards: the start with the lowest final error (``return_errors=True``).

    ``method="sequential"`` calls ``parafac2_als`` once per start.  ``method="fused"`` fits all starts in one launch of a HIP
    kernel, one workgroup per start, in fp64 (csrc/pf2als_multistart.hip); it serves rank <= 16 and X of at most
    ``_MULTISTART_MAX_ELEMENTS`` elements, anything else raises ``NotImplementedError`` before the device is touched.  Being fp64,
    it resolves the default ``tol=1e-8`` where the sequential fit's fp32 X passes do not, so the two
    methods can stop at different iterations.  ``method="auto"`` takes the fused kernel when it serves the call and is faster
    (DESIGN.md section 13), else the sequential loop.  Only ``init="random"``: any other start would be the same N times
    (``ValueError``).  ``parafac2_als``'s own refusals raise for every method.
    """
    _check_method(method)
    _check_start_keywords("parafac2_als_multistart", parafac2_als_kwargs)
    random_states = list(random_states)
    kw = _pf2als_kwargs(parafac2_als_kwargs)
    rank = int(rank)
    I, K, rows, modes = dec._parafac2_als_options(matrices, rank, kw["init"], kw["nn_modes"], kw["n_iter_max"], kw["n_iter_parafac"],
                                                  kw["kwargs"])
    if _pf2als_fused_serves("parafac2_als_multistart", method, rank, rows, K, len(random_states), "starts"):
        return _pf2als_fused(matrices, rank, [dec._pf2als_random_start(I, K, rank, rs) for rs in random_states], modes, kw) \
            if random_states else []
    return [dec.parafac2_als(matrices, rank, random_state=rs, **parafac2_als_kwargs) for rs in random_states]
