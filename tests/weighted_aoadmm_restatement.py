"""fp64 NumPy restatement of the weighted AO-ADMM fit of cmf_aoadmm_resample, built on the oracle's
public pieces (oracle/aoadmm_oracle.py: OracleState, run, the prox functions).  Its own code is the weighted normal equations
and the zero-weight masks:

    0.5 sum_i w_i |X_i - B_i D_i C^T|^2 / sum_i w_i |X_i|^2 + penalties + l2 terms

is minimised by the oracle's AO-ADMM run with every per-matrix Gram and right-hand side multiplied by w_i.  A matrix of weight
0 is not in the job: its part of the start is set to zero, its systems get a zero inverse, its prox and dual steps are skipped,
and its rows stay exact zeros.  tests/test_cmf_resampling_host.py pins this file to the oracle itself."""
import numpy as np

from matcouply_amd import decomposition as dec
from matcouply_amd import penalties as pen
from matcouply_amd._utils import check_random_state
from oracle import aoadmm_oracle as orc


class WeightedOracleState(orc.OracleState):
    def __init__(self, X, row_ptr, A, B, C, regs, aux, dual, weights, **kw):
        super().__init__(X, row_ptr, A, B, C, regs, aux, dual, **kw)
        self.w = np.asarray(weights, dtype=np.float64)
        assert self.w.shape == (self.I,) and (self.w >= 0).all() and (self.w > 0).any()
        self.live = self.w > 0
        self.w_row = self.w[self.slab_of_row]
        self.live_row = self.live[self.slab_of_row]
        self.norm_X_sq = float(np.sum(self.w_row[:, None] * self.X ** 2))
        # the zero-weight rule on the start: the row of A, B_i and the rows of every aux and dual of modes 0 and 1 (P_i for PARAFAC2)
        self.A[~self.live] = 0
        self.B[~self.live_row] = 0
        for mode, dead in ((0, ~self.live), (1, ~self.live_row)):
            for z, u in zip(self.aux[mode], self.dual[mode]):
                (z[0] if isinstance(z, tuple) else z)[dead] = 0
                u[dead] = 0

    def _masked_inverse(self, L):
        Linv = np.zeros_like(L)
        Linv[self.live] = self._inv(L[self.live])
        return Linv

    def _constant(self, rho):
        return np.where(self.live, rho[self.live].max(), 0.0)

    def _prox_parafac2(self, Y, rho, aux):
        P_old, Delta = aux
        P, acc = np.zeros_like(Y), np.zeros_like(Delta)
        for i in np.flatnonzero(self.live):
            s, e = self.row_ptr[i], self.row_ptr[i + 1]
            P[s:e] = orc.polar_factor(Y[s:e] @ Delta.T)
            acc = acc + rho[i] * (P[s:e].T @ Y[s:e])
        return P, acc / np.sum(rho[self.live])

    def update_B(self):
        X, A, C, rp = self.X, self.A, self.C, self.row_ptr
        regs, aux, dual = self.regs[1], self.aux[1], self.dual[1]
        n, r = len(regs), A.shape[1]
        CtC = C.T @ C
        rhs = np.zeros((X.shape[0], r))
        for i in np.flatnonzero(self.live):
            rhs[rp[i]: rp[i + 1]] = self.w[i] * (X[rp[i]: rp[i + 1]] @ (C * A[i]))
        L = self.w[:, None, None] * (CtC[None] * A[:, :, None] * A[:, None, :])
        rho = 0.5 * np.trace(L, axis1=1, axis2=2) * self.scale
        if self.constant_B:
            rho = self._constant(rho)
        Linv = self._masked_inverse(L + (rho * n + self.l2[1])[:, None, None] * np.eye(r))
        rho_row = rho[self.slab_of_row][:, None]
        live = self.live_row
        B = self.B
        self.inner_iters[1] = 0
        for _ in range(self.inner):
            B_old = B
            self.inner_iters[1] += 1
            T = rhs
            if n:
                S = 0
                for d, z, u in zip(regs, aux, dual):
                    S = S + (orc.aux_as_packed(d, z) - u)
                T = rho_row * S + rhs
            B = self._solve_rows(T, Linv)
            for k, d in enumerate(regs):
                Y = B + dual[k]
                if d["kind"] in orc.ROW_SEPARABLE:
                    Z = aux[k].copy()
                    Z[live] = orc.prox_elementwise(d, Y[live], rho_row[live])
                    aux[k] = Z
                elif d["kind"] == "parafac2":
                    aux[k] = self._prox_parafac2(Y, rho, aux[k])
                else:
                    Z = aux[k].copy()
                    for i in np.flatnonzero(self.live):
                        Z[rp[i]: rp[i + 1]] = orc.prox_matrix(d, Y[rp[i]: rp[i + 1]], rho[i])
                    aux[k] = Z
                U = dual[k].copy()
                U[live] = (B - (orc.aux_as_packed(d, aux[k]) - dual[k]))[live]
                dual[k] = U
            if self._inner_converged(B, B_old, 1):
                break
        self.B = B
        self.rho_B = rho
        return rho

    def local_C_normal_equations(self):
        Ba = self.B * self.A[self.slab_of_row]
        wBa = self.w_row[:, None] * Ba
        return wBa.T @ Ba, self.X.T @ wBa

    def update_A(self, rho_max_reduce=None):
        X, B, C, rp = self.X, self.B, self.C, self.row_ptr
        regs, aux, dual = self.regs[0], self.aux[0], self.dual[0]
        n, r = len(regs), C.shape[1]
        CtC = C.T @ C
        XC = X @ C
        rhs = self.w[:, None] * orc.segment_sums(B * XC, rp)
        Q = np.empty((self.I, r, r))
        for i in range(self.I):
            Bi = B[rp[i]: rp[i + 1]]
            Q[i] = self.w[i] * ((Bi.T @ Bi) * CtC)
        rho = 0.5 * np.trace(Q, axis1=1, axis2=2) * self.scale
        if self.constant_A:
            rho = self._constant(rho)
        Linv = self._masked_inverse(Q + (rho * n + self.l2[0])[:, None, None] * np.eye(r))
        live = self.live
        A = self.A
        self.inner_iters[0] = 0
        for _ in range(self.inner):
            A_old = A
            self.inner_iters[0] += 1
            T = rhs
            if n:
                S = 0
                for z, u in zip(aux, dual):
                    S = S + (z - u)
                T = rho[:, None] * S + rhs
            A = np.einsum("ik,ikj->ij", T, Linv)
            for k, d in enumerate(regs):
                Y = A + dual[k]
                Z = aux[k].copy()
                if self.constant_A:
                    Z[live] = orc.prox_matrix(d, Y[live], rho[live][0])
                else:
                    if d["kind"] not in orc.ROW_SEPARABLE:
                        raise AttributeError(f"{d['kind']} on mode 0 needs constant_feasibility_penalty")
                    Z[live] = orc.prox_elementwise(d, Y[live], rho[live][:, None])
                aux[k] = Z
                U = dual[k].copy()
                U[live] = (A - (aux[k] - dual[k]))[live]
                dual[k] = U
            if self._inner_converged(A, A_old, 0):
                break
        self.A = A
        self.rho_A = rho
        self.last_A_byproducts = (rhs, Q)
        return rhs, Q

    def rec_error_full(self):
        A, B, C, rp, X = self.A, self.B, self.C, self.row_ptr, self.X
        Ba = B * A[self.slab_of_row]
        inner = float(np.sum(self.w_row[:, None] * ((X @ C) * Ba)))
        CtC = C.T @ C
        norm_sq = 0.0
        for i in range(self.I):
            Bi = Ba[rp[i]: rp[i + 1]]
            norm_sq += self.w[i] * float(np.sum((Bi.T @ Bi) * CtC))
        return np.sqrt(max(0.0, self.norm_X_sq - 2 * inner + norm_sq)) / np.sqrt(self.norm_X_sq)


# ---- a job's exact start, as cmf_aoadmm_resample draws it ---------------------------------------------------------------------
def describe(reg):
    if isinstance(reg, pen.Parafac2):
        return {"kind": "parafac2"}
    if isinstance(reg, pen.L1Penalty):
        return {"kind": "l1", "reg_strength": reg.reg_strength, "non_negativity": reg.non_negativity}
    if isinstance(reg, pen.L2Ball):
        return {"kind": "l2ball", "norm_bound": reg.norm_bound, "non_negativity": reg.non_negativity}
    if isinstance(reg, pen.Box):
        return {"kind": "box", "min_val": reg.min_val, "max_val": reg.max_val}
    if isinstance(reg, pen.NonNegativity):
        return {"kind": "nn"}
    raise AssertionError(type(reg))


def start_of(mats, rank, seed, kw, perturb=False):
    """the draw of cmf_aoadmm(random_state=seed, **kw), stored in fp32 as the fused kernel receives it -> the arguments of
    OracleState behind X and row_ptr, as a dict.  perturb: every entry moved by one unit in its last fp64 place, up or down at
    random - a relative 1e-16 (the seed-sensitivity rule of DESIGN.md section 18)"""
    full = dec._cmf_kwargs(kw)
    cmf, regs, auxes, duals = dec._start_penalties(full, mats, rank, check_random_state(seed))
    rng = np.random.RandomState(12345)

    def f(a):
        a = np.asarray(a, dtype=np.float32).astype(np.float64)
        return np.nextafter(a, rng.choice([-np.inf, np.inf], size=a.shape)) if perturb else a

    _, (A, B_is, C) = cmf
    descs = [[describe(r) for r in regs[m]] for m in range(3)]
    aux, dual = [[], [], []], [[], [], []]
    for m in range(3):
        for a_, d_ in zip(auxes[m], duals[m]):
            if isinstance(a_, tuple):
                aux[m].append((f(np.concatenate(a_[0])), f(a_[1])))
            else:
                aux[m].append(f(np.concatenate(a_)) if m == 1 else f(a_))
            dual[m].append(f(np.concatenate(d_)) if m == 1 else f(d_))
    l2 = dec._listify(full["l2_penalty"], "l2_penalty")
    cA, cB = dec._constant_flags(full["constant_feasibility_penalty"])
    return dict(A=f(A), B=f(np.concatenate(B_is)), C=f(C), regs=descs, aux=aux, dual=dual, l2=[v or 0.0 for v in l2],
                inner_n_iter_max=full["inner_n_iter_max"], feasibility_penalty_scale=full["feasibility_penalty_scale"],
                constant_A=cA, constant_B=cB)


def weighted_state(mats, X, row_ptr, rank, seed, kw, weights, perturb=False):
    return WeightedOracleState(np.asarray(X, dtype=np.float64), row_ptr, weights=weights, **start_of(mats, rank, seed, kw, perturb))


def oracle_state(mats, X, row_ptr, rank, seed, kw):
    return orc.OracleState(np.asarray(X, dtype=np.float64), row_ptr, **start_of(mats, rank, seed, kw))


def shortened(state_args, X, row_ptr, keep, scale=None):
    """the oracle's state for the list of matrices `keep` cut out of a full start (`state_args`: start_of's dict), matrix i
    multiplied by scale[i] with row i of A, aux_A and dual_A multiplied alike (the identity of the scaled fit)"""
    row_ptr = np.asarray(row_ptr)
    rows = np.concatenate([np.arange(row_ptr[i], row_ptr[i + 1]) for i in keep])
    s = np.ones(len(row_ptr) - 1) if scale is None else np.asarray(scale, dtype=np.float64)
    per_row = np.repeat(s[keep], np.diff(row_ptr)[keep])[:, None]
    cut = {0: lambda a: a[keep] * s[keep][:, None], 1: lambda a: a[rows], 2: lambda a: a}
    a = dict(state_args)
    a["A"], a["B"] = cut[0](a["A"]), cut[1](a["B"])
    a["aux"] = [[(cut[m](z[0]), z[1]) if isinstance(z, tuple) else cut[m](z) for z in a["aux"][m]] for m in range(3)]
    a["dual"] = [[cut[m](u) for u in a["dual"][m]] for m in range(3)]
    rp = np.concatenate([[0], np.cumsum(np.diff(row_ptr)[keep])])
    return orc.OracleState(np.asarray(X, dtype=np.float64)[rows] * per_row, rp, **a)


def compare(got, diag, st, res, floor=1e-3):
    """the worst relative differences of a fitted job (cmf, DiagnosticMetrics) against the restatement's state and run():
    (factors, rec_errors and losses), (gaps over a floor) - the comparison of tests/test_gpu_multistart.py"""
    _, (A, B_is, C) = got
    rel = lambda a, b: np.linalg.norm(np.asarray(a, dtype=np.float64) - b) / max(np.linalg.norm(b), 1e-300)
    errs = [rel(A, st.A), rel(np.concatenate([np.asarray(b) for b in B_is]), st.B), rel(C, st.C),
            np.max(np.abs(np.array(diag.rec_errors) - res["rec_errors"]) / np.array(res["rec_errors"])),
            np.max(np.abs(np.array(diag.regularized_loss) - res["losses"]) / np.array(res["losses"]))]
    gaps, worst = [0.0], None
    for g_got, g_ref in zip(diag.feasibility_gaps, res["gaps"]):
        for m in range(3):
            if len(g_ref[m]):
                d = np.abs(np.array(g_got[m]) - g_ref[m]) / np.maximum(np.abs(g_ref[m]), floor)
                if d.max() > max(gaps):
                    worst = (m, float(np.array(g_got[m])[d.argmax()]), float(np.asarray(g_ref[m])[d.argmax()]))
                gaps.append(float(d.max()))
    return errs, max(gaps), worst
