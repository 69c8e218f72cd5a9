"""fp64 NumPy restatement of the missing-entry AO-ADMM fit of cmf_aoadmm_missing, built on the oracle's
public pieces (oracle/aoadmm_oracle.py: OracleState's update_B / update_C / update_A, feasibility_gaps and regularisation, and
the stopping rule of its run).  Its own code is the filled copy and the pass behind every outer iteration:

    X~ = X on the observed entries; elsewhere the fill (a constant per column, or the start's model)
    per outer iteration: the oracle's B, C and A phases on X~; M = B_i D_i C^T; rec_error = |X - M|_observed / |X|_observed;
    X~ = M on the missing entries; loss = 0.5 rec_error^2 + regularisation; the oracle's stopping rule on this loss

Row 0 of the diagnostics is the same pass on the start; it stores M only for the model fill (a constant fill would be gone
before any phase had read it).  tests/test_missing_host.py pins this file to the oracle itself."""
import numpy as np

from oracle import aoadmm_oracle as orc
from tests.weighted_aoadmm_restatement import start_of


class MissingOracleState(orc.OracleState):
    """`observed`: boolean [N, K]; `fill_values`: [K] or None (the start's model); `impute` False: the missing entries keep
    their fill for the whole fit (the comparison without imputation updates).  X may hold anything at a missing entry."""

    def __init__(self, X, row_ptr, observed, fill_values=None, impute=True, **start):
        X = np.array(X, dtype=np.float64)
        self.observed = np.asarray(observed, dtype=bool)
        assert self.observed.shape == X.shape
        fill = np.zeros(X.shape[1]) if fill_values is None else np.asarray(fill_values, dtype=np.float64)
        super().__init__(np.where(self.observed, X, fill[None, :]), row_ptr, **start)
        self.X_observed = np.where(self.observed, X, 0.0)  # the data, zeros where nothing was observed (never a NaN)
        self.fill_model = fill_values is None
        self.impute = bool(impute)
        self.norm_observed_sq = float(np.sum(self.X_observed ** 2))
        self.norm_X_sq = float("nan")  # the complete-data error formulas are not this fit's

    def model(self):
        return (self.B * self.A[self.slab_of_row]) @ self.C.T

    def impute_pass(self, store):
        """the relative error over the observed entries; with `store` the model goes into the missing entries of X~"""
        M = self.model()
        resid = float(np.sum(np.where(self.observed, self.X_observed - M, 0.0) ** 2))
        if store:
            self.X = np.where(self.observed, self.X, M)
        return np.sqrt(resid) / np.sqrt(self.norm_observed_sq)


def run(state, n_iter_max, tol=1e-8, absolute_tol=1e-10, feasibility_tol=1e-4, return_errors=True):
    """oracle.run with the pass over the entries in place of the reconstruction error: the same lists, verdict and message.
    The pass runs in every outer iteration, recorded or not: it is part of the iteration."""
    def feasible(gaps):
        worst = max([g for mode in gaps for g in mode], default=-np.inf)
        return worst < feasibility_tol

    rec = state.impute_pass(state.fill_model and state.impute)
    rec_errors, losses, gaps_hist = [rec], [state.loss(rec)], [state.feasibility_gaps()]
    satisfied, message, feas = False, "MAXIMUM NUMBER OF ITERATIONS REACHED", None
    it = -1
    for it in range(n_iter_max):
        state.update_B()
        state.update_C()
        state.update_A()
        rec = state.impute_pass(state.impute)
        gaps = state.feasibility_gaps()
        gaps_hist.append(gaps)
        if tol or absolute_tol:
            feas = feasibility_tol and feasible(gaps)
            if not feas and not return_errors:
                continue
        rec_errors.append(rec)
        losses.append(state.loss(rec))
        if tol:
            rel = abs(losses[-2] - losses[-1]) < tol * losses[-2]
            ab = losses[-1] < absolute_tol
            if feas and rel:
                satisfied, message = True, "FEASIBILITY GAP CRITERION AND RELATIVE LOSS CRITERION SATISFIED"
                break
            if feas and ab:
                satisfied, message = True, "FEASIBILITY GAP CRITERION AND ABSOLUTE LOSS CRITERION SATISFIED"
                break
    if feasibility_tol and return_errors:
        feas = feasible(state.feasibility_gaps())
    elif not feasibility_tol:
        feas = None
    if not satisfied and not (tol or absolute_tol):
        satisfied = None
    return dict(rec_errors=rec_errors, losses=losses, gaps=gaps_hist, n_iter=it + 1, message=message,
                satisfied_stopping_condition=satisfied, satisfied_feasibility_condition=feas)


def missing_state(mats, X, row_ptr, rank, seed, kw, observed, fill_values=None, impute=True):
    """the restatement started from the exact start of cmf_aoadmm(random_state=seed, **kw), stored in fp32 as the fused
    kernel receives it (tests/test_gpu_multistart.py: _oracle_state)"""
    return MissingOracleState(X, row_ptr, observed, fill_values, impute, **start_of(mats, rank, seed, kw))


def column_means(X, observed):
    """[K]: the mean of the observed entries per column, 0 for a column without one - a direct loop"""
    out = np.zeros(X.shape[1])
    for k in range(X.shape[1]):
        vals = [X[j, k] for j in range(X.shape[0]) if observed[j, k]]
        out[k] = sum(vals) / len(vals) if vals else 0.0
    return out
