"""Factor match scores: how well do two fitted models, or the many starts of a multi-start fit, agree?

The examples that loop over random starts compare the fitted models with each other, or with a known truth, by the factor match
score (FMS).  A model is ``(weights, (A, B_is, C))`` of rank r; its three factor matrices are A (I x r), B (N x r, the B_i
stacked, N = sum J_i) and C (K x r); ``weights=None`` means ones.  For the models 1 and 2:

* every column of every mode is normalised to unit 2-norm, and ``w[p] = weights[p] * prod_modes ||column p||`` (over all three
  modes, a skipped one included); a zero column has congruence 0 with every column, never NaN;
* ``M[p, q] = prod_{modes m != skip_mode} <f1_m[:, p], f2_m[:, q]>`` on the normalised columns;
* ``consider_weights`` multiplies ``M[p, q]`` by ``1 - |w1[p] - w2[q]| / max(w1[p], w2[q])`` (1 when both weights are 0);
* ``absolute_value`` takes ``|M|``;
* the permutation is the ``col_ind`` of the assignment that maximises ``sum_p M[p, perm[p]]``, the score the mean of those r
  entries; ``factors2[:, perm]`` lines model 2 up with model 1 (:func:`permute_cmf`).

``method="host"`` is NumPy and SciPy (one ``linear_sum_assignment`` per pair); ``method="device"`` computes all pairs of a call in
one launch of a HIP kernel (csrc/similarity.hip): the r x r products on the fp64 matrix core and an exact
assignment solver in the same wave.
"""
import numpy as np

from . import _engine
from ._utils import is_tensor, is_torch, to_numpy
from .coupled_matrices import CoupledMatrixFactorization

try:
    import torch
except ImportError:  # pragma: no cover
    torch = None

__all__ = ["factor_match_score", "multistart_similarity", "permute_cmf"]

# the permutations of an all-pairs call are n x n x rank int32.  2 GiB of them is 5792 models at rank 16 (the all-pairs matrix
# of the 1024 starts a multi-start call fits is 64 MiB); like _GRID_MAX_BYTES of decomposition.py the bound keeps a quadratic
# request from taking the memory of the host and of the device without being asked twice.  A larger comparison passes `pairs`
_ALL_PAIRS_MAX_BYTES = 1 << 31

# method="auto" takes the device whenever it serves the call and a device is present: the crossover in the number of pairs
# below which the host loop is faster is NOT MEASURED yet (tools/similarity_rate.py writes profiles/similarity_rate.txt, from
# which it is to be taken)
_AUTO_MIN_PAIRS = 1


class _Model:
    """one model as the scores see it: the three factor matrices (B stacked) as they were given, and the weights"""

    def __init__(self, cmf):
        if isinstance(cmf, CoupledMatrixFactorization):
            weights, (A, B, C) = cmf.weights, cmf.factors
        else:
            try:
                weights, (A, B, C) = cmf[0], cmf[1]
            except (TypeError, ValueError, IndexError, KeyError):
                raise TypeError("a model is a CoupledMatrixFactorization or (weights, (A, B_is, C))") from None
            if len(cmf) == 3:  # a PARAFAC2 tensor (weights, (A, B, C), projections): B_i = P_i B
                B = [P_i @ B for P_i in cmf[2]]
        if not is_tensor(B):  # the B_is; a tensor is the stacked B the examples pass
            B = list(B)
            if not B:
                raise ValueError("a model needs at least one B_i")
            B = torch.cat(B, 0) if is_torch(B[0]) else np.concatenate([np.asarray(B_i) for B_i in B], 0)
        self.factors = tuple(f if is_tensor(f) else np.asarray(f) for f in (A, B, C))
        if any(f.ndim != 2 for f in self.factors):
            raise ValueError("the factor matrices of a model are second-order")
        self.rank = int(self.factors[0].shape[1])
        if any(int(f.shape[1]) != self.rank for f in self.factors):
            raise ValueError(f"rank mismatch inside a model: its factor matrices have {[int(f.shape[1]) for f in self.factors]} columns")
        self.weights = None if weights is None else (weights if is_tensor(weights) else np.asarray(weights))
        if self.weights is not None and tuple(self.weights.shape) != (self.rank,):
            raise ValueError(f"rank mismatch: weights of shape {tuple(self.weights.shape)} for a rank-{self.rank} model")
        self.rows = tuple(int(f.shape[0]) for f in self.factors)
        self._host = None

    def tensors(self):
        return self.factors + ((self.weights,) if self.weights is not None else ())

    def host(self):
        """(normalised fp64 factor matrices, w) on the host"""
        if self._host is None:
            F = [to_numpy(f).astype(np.float64) for f in self.factors]
            norms = [np.linalg.norm(f, axis=0) for f in F]
            w = np.ones(self.rank) if self.weights is None else to_numpy(self.weights).astype(np.float64)
            self._host = ([f / np.where(n > 0, n, 1.0) for f, n in zip(F, norms)], w * norms[0] * norms[1] * norms[2])
        return self._host


def _check_options(skip_mode, method):
    if skip_mode is not None and not (isinstance(skip_mode, (int, np.integer)) and not isinstance(skip_mode, bool)
                                      and 0 <= skip_mode <= 2):
        raise ValueError(f"skip_mode must be None, 0, 1 or 2, not {skip_mode!r}")
    if method not in ("auto", "host", "device"):
        raise ValueError(f'method must be "auto", "host" or "device", not {method!r}')


def _check_pair(m1, m2, skip_mode):
    if m1.rank != m2.rank:
        raise ValueError(f"rank mismatch: a rank-{m1.rank} model cannot be matched with a rank-{m2.rank} one")
    for mode in range(3):
        if mode != skip_mode and m1.rows[mode] != m2.rows[mode]:
            raise ValueError(f"shape mismatch: mode {mode} has {m1.rows[mode]} rows in one model and {m2.rows[mode]} in the other")


def _host_pair(m1, m2, consider_weights, skip_mode, absolute_value):
    from scipy.optimize import linear_sum_assignment

    (F1, w1), (F2, w2) = m1.host(), m2.host()
    M = np.ones((m1.rank, m1.rank))
    for mode in range(3):
        if mode != skip_mode:
            M = M * (F1[mode].T @ F2[mode])
    if consider_weights:
        a, b = w1[:, None], w2[None, :]
        with np.errstate(divide="ignore", invalid="ignore"):
            M = M * np.where((a == 0) & (b == 0), 1.0, 1.0 - np.abs(a - b) / np.maximum(a, b))
    if absolute_value:
        M = np.abs(M)
    rows, cols = linear_sum_assignment(M, maximize=True)
    return float(M[rows, cols].mean()), cols.astype(np.int32)


def _device_present():
    return torch is not None and torch.cuda.is_available()


def _device_unserved_reason(models):
    """why the kernel cannot score these models (a sentence), or None.  Looks at shapes, types and host data only: no device
    call (the finiteness of device-resident factors is checked on the device, after they are packed)."""
    first = models[0]
    if not 1 <= first.rank <= _engine.FMS_MAX_RANK:
        return f"rank {first.rank} is outside 1 ... {_engine.FMS_MAX_RANK}"
    for k, m in enumerate(models):
        if (m.rows, m.rank) != (first.rows, first.rank):
            return (f"model {k} has (I, N, K, rank) = {m.rows + (m.rank,)}, model 0 {first.rows + (first.rank,)}: one launch holds "
                    "models of one shape")
        if min(m.rows) < 1:
            return f"model {k} has a mode without rows"
        for t in m.tensors():
            name = str(t.dtype).replace("torch.", "")
            if name not in ("float64", "float32"):
                return f"model {k} holds {name} factors (float64 and float32 are widened exactly, nothing else)"
            if not is_torch(t) and not np.isfinite(t).all():
                return f"model {k} holds a non-finite entry"
    return None


def _pack(models, device):
    """All models of a call as one fp64 tensor [n, (I + N + K) * r], every model [A; B; C] row-major, and their weights [n, r] (or
    None when no model has any).  This is the layout of the first (I + N + K) * r doubles of a multi-start state slice
    (include/matcouply_hip.h), so a later change can score the starts from the state of the fused fit without this copy."""
    if all(not is_torch(t) for m in models for t in m.factors):
        packed = torch.from_numpy(np.stack([np.concatenate([np.ravel(f).astype(np.float64) for f in m.factors]) for m in models]))
    else:
        def flat(f):
            return (f.detach() if is_torch(f) else torch.from_numpy(np.ascontiguousarray(f))).to(device=device, dtype=torch.float64).reshape(-1)

        packed = torch.stack([torch.cat([flat(f) for f in m.factors]) for m in models])
    weights = None
    if any(m.weights is not None for m in models):
        ones = np.ones(models[0].rank)
        weights = torch.stack([torch.as_tensor(ones if m.weights is None else m.weights).detach().to(device=device, dtype=torch.float64)
                               for m in models]).contiguous()
    return packed.to(device).contiguous(), weights


def _device_scores(models, pairs, consider_weights, skip_mode, absolute_value, want_perm):
    from .decomposition import _device

    device = _device()
    packed, weights = _pack(models, device)
    if not bool(torch.isfinite(packed).all()) or (weights is not None and not bool(torch.isfinite(weights).all())):
        raise NotImplementedError("factor match scores on the device: a model holds a non-finite entry")
    I, N, K = models[0].rows
    flags = _engine.FMS_CONSIDER_WEIGHTS * bool(consider_weights) | _engine.FMS_ABSOLUTE_VALUE * bool(absolute_value)
    score, perm = _engine.fms_scores(packed, I, N, K, models[0].rank, weights, pairs, flags, -1 if skip_mode is None else int(skip_mode),
                                     want_perm)
    return score.cpu().numpy(), perm.cpu().numpy() if want_perm else None


def _scores(models, pairs, want_perm, method, consider_weights=True, skip_mode=None, absolute_value=True):
    """(scores float64 [n_pairs], permutations int32 [n_pairs, r] or None) of the pairs (s, t) of indices into `models`; all the
    validation of a call happens here, before any device call"""
    _check_options(skip_mode, method)
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    for s, t in {(int(s), int(t)) for s, t in pairs}:
        _check_pair(models[s], models[t], skip_mode)
    rank = models[0].rank
    if method != "host":
        reason = _device_unserved_reason(models)
        if reason is None and method == "auto" and (len(pairs) < _AUTO_MIN_PAIRS or not _device_present()):
            reason = f"no device is present, or fewer than {_AUTO_MIN_PAIRS} pairs"  # "auto" only: the host loop below serves it
        if reason is None:
            return _device_scores(models, pairs.astype(np.int32), consider_weights, skip_mode, absolute_value, want_perm)
        if method == "device":
            raise NotImplementedError(f'factor match scores with method="device": {reason}')
    scores, perms = np.empty(len(pairs)), np.empty((len(pairs), rank), dtype=np.int32)
    for k, (s, t) in enumerate(pairs):
        scores[k], perms[k] = _host_pair(models[s], models[t], consider_weights, skip_mode, absolute_value)
    return scores, perms if want_perm else None


def factor_match_score(cmf1, cmf2, consider_weights=True, skip_mode=None, return_permutation=False, absolute_value=True,
                       method="auto"):
    """The factor match score of two models (the definition at the top of this module), or ``(fms, permutation)`` with
    ``return_permutation``: ``permute_cmf(cmf2, permutation)`` lines ``cmf2`` up with ``cmf1``.  The models are
    ``CoupledMatrixFactorization`` objects or ``(weights, (A, B_is, C))`` tuples of NumPy arrays or torch tensors; ``B_is`` may
    also be one matrix, the B_i stacked.  ``ValueError`` for models of different rank or different rows on a mode that is not
    skipped.  ``method``: see :func:`multistart_similarity`."""
    scores, perms = _scores([_Model(cmf1), _Model(cmf2)], [(0, 1)], return_permutation, method, consider_weights, skip_mode,
                            absolute_value)
    return (float(scores[0]), perms[0]) if return_permutation else float(scores[0])


def _model_of_result(result):
    def is_model(x):
        return isinstance(x, CoupledMatrixFactorization) or (
            isinstance(x, (tuple, list)) and len(x) in (2, 3) and (x[0] is None or is_tensor(x[0]))
            and isinstance(x[1], (tuple, list)) and len(x[1]) == 3)

    if is_model(result):
        return result
    if isinstance(result, tuple) and result and is_model(result[0]):
        return result[0]
    raise TypeError("every result is a model, or a tuple whose first element is one (what the multi-start functions return)")


def multistart_similarity(results, reference="best", *, pairs=None, all_pairs=False, return_permutations=False, method="auto",
                          **score_options):
    """Factor match scores among the starts of a multi-start fit.  ``results`` is what ``cmf_aoadmm_multistart``,
    ``cmf_aoadmm_grid`` (one grid point) or ``parafac2_als_multistart`` return: models, or tuples whose first element is the model.

    By default: the float64 array of the n scores ``factor_match_score(reference, results[s])``.  ``reference`` is ``"best"``
    (the start :func:`~matcouply_amd.decomposition.best_start` picks; ``ValueError`` when the results carry no diagnostics or no
    start satisfied its stopping condition), an index into ``results``, or a model.  ``pairs``: a sequence of index pairs
    ``(s, t)`` instead, giving ``factor_match_score(results[s], results[t])`` for each.  ``all_pairs=True``: the n x n matrix of
    all of them; only s <= t is computed and mirrored, so it is exactly symmetric.  ``return_permutations=True`` returns
    ``(scores, permutations)``, the permutations int32 with a last axis of length rank; an all-pairs call whose permutations
    exceed ``_ALL_PAIRS_MAX_BYTES`` raises ``ValueError``.  ``score_options``: ``consider_weights``, ``skip_mode`` and
    ``absolute_value`` of :func:`factor_match_score`.

    ``method="host"`` loops over the pairs with NumPy and SciPy and serves every call.  ``method="device"`` scores all pairs in
    one kernel launch; it serves rank 1 ... 16, models that all have one shape (I, N, K, rank) and finite float64 or float32
    factors (widened exactly), and raises ``NotImplementedError`` with the reason otherwise, before the device is touched.
    ``method="auto"`` takes the device when it serves the call and one is present, else the host."""
    unknown = set(score_options) - {"consider_weights", "skip_mode", "absolute_value"}
    if unknown:
        raise TypeError(f"multistart_similarity() got an unexpected keyword argument {sorted(unknown)[0]!r}")
    _check_options(score_options.get("skip_mode"), method)
    results = list(results)
    if not results:
        raise ValueError("multistart_similarity needs at least one result")
    if all_pairs and pairs is not None:
        raise ValueError("pass either pairs or all_pairs=True")
    models = [_Model(_model_of_result(result)) for result in results]
    n, rank = len(models), models[0].rank
    if all_pairs:
        if return_permutations and n * n * rank * 4 > _ALL_PAIRS_MAX_BYTES:
            raise ValueError(f"the permutations of all pairs of {n} rank-{rank} models take {n * n * rank * 4} bytes, more than the "
                             f"{_ALL_PAIRS_MAX_BYTES} of _ALL_PAIRS_MAX_BYTES; pass the pairs wanted as pairs=")
        s, t = np.triu_indices(n)
        scores, perms = _scores(models, np.stack([s, t], 1), return_permutations, method, **score_options)
        out = np.empty((n, n))
        out[s, t] = out[t, s] = scores
        if not return_permutations:
            return out
        out_perms = np.empty((n, n, rank), dtype=np.int32)
        out_perms[t, s] = np.argsort(perms, axis=1).astype(np.int32)  # the swapped pair: the inverse permutation
        out_perms[s, t] = perms
        return out, out_perms
    if pairs is not None:
        pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
        if len(pairs) and (pairs.min() < 0 or pairs.max() >= n):
            raise ValueError(f"pairs holds an index outside 0 ... {n - 1}")
    else:
        if isinstance(reference, str):
            if reference != "best":
                raise ValueError(f'reference must be "best", an index or a model, not {reference!r}')
            from .decomposition import best_start

            ref = best_start(results)
            if ref is None:
                raise ValueError('reference="best": no start satisfied its stopping condition; pass an index or a model')
        elif isinstance(reference, (int, np.integer)) and not isinstance(reference, bool):
            if not -n <= reference < n:
                raise ValueError(f"reference {reference} is outside the {n} results")
            ref = int(reference) % n
        else:
            models.append(_Model(reference))
            ref = n
        pairs = np.stack([np.full(n, ref), np.arange(n)], 1)
    scores, perms = _scores(models, pairs, return_permutations, method, **score_options)
    return (scores, perms) if return_permutations else scores


def permute_cmf(cmf, permutation):
    """The model with the columns of A, every B_i and C (and the weights, if it has any) in the order ``permutation``: with the
    permutation ``factor_match_score(cmf1, cmf2, return_permutation=True)`` returns, ``cmf2`` lined up with ``cmf1``.  A
    ``CoupledMatrixFactorization`` gives one, a tuple a tuple (a stacked B stays stacked)."""
    weights, (A, B, C) = (cmf.weights, cmf.factors) if isinstance(cmf, CoupledMatrixFactorization) else (cmf[0], cmf[1])
    rank = int(A.shape[1])
    idx = [int(p) for p in permutation]
    if sorted(idx) != list(range(rank)):
        raise ValueError(f"{list(permutation)} is not a permutation of 0 ... {rank - 1}")
    B = B[:, idx] if is_tensor(B) else [B_i[:, idx] for B_i in B]
    out = (None if weights is None else weights[idx], (A[:, idx], B, C[:, idx]))
    return CoupledMatrixFactorization(out) if isinstance(cmf, CoupledMatrixFactorization) else out
