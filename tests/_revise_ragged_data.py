"""Inputs, references and call helpers of the ragged condition / forget tests (tests/test_revise_ragged_gpu.py).  A plain
module, not a conftest.  Every state starts as the posterior of 3 D base observations, so every downdate of a slice the state
contains stays positive definite.  References come from the CPU oracle, once per (D, counts, dtype, noise), and are shared."""
import functools

import numpy as np

from oracle import blr_oracle as O

COUNTS = (0, 1, 2, 16, 17, 3, 0, 1, 40)
SWEEP_MAX_K = 16  # kSweepMaxK (csrc/blr_update.hpp)


def routes(counts, D, direction, mode):
    """(sweep, refit, idle) index lists by the rule of csrc/blr_revise_ragged_plan.hpp: longest first, ties by index"""
    sweep, refit, idle = [], [], []
    for b, k in enumerate(counts):
        if k == 0:
            idle.append(b)
        elif direction == "downdate":
            sweep.append(b)
        elif D > 128 or mode == "never":
            refit.append(b)
        elif mode == "always":
            (sweep if k <= SWEEP_MAX_K else refit).append(b)
        else:
            (sweep if k == 1 else refit).append(b)
    key = lambda b: (-counts[b], b)
    return sorted(sweep, key=key), sorted(refit, key=key), idle


class Batch:
    """B regressors at dimension D with the given counts: packed data and, per noise kind, the states before and after."""

    def __init__(self, D, counts, dtype, seed=0):
        rng = np.random.Generator(np.random.PCG64(9100 + 17 * D + seed))
        r = lambda a: np.asarray(a, dtype=dtype).astype(np.float64)  # what the library is given, in double
        self.D, self.counts, self.dtype, self.nb = D, tuple(int(c) for c in counts), dtype, len(counts)
        self.offsets = np.concatenate([[0], np.cumsum(self.counts)]).astype(np.int64)
        total = self.total = int(self.offsets[-1])
        self.X = r(rng.standard_normal((D, total)) / np.sqrt(D))
        self.y = r(rng.standard_normal(total))
        self.s_diag = r(np.exp(0.3 * rng.standard_normal(total)))
        self.s_reg = r(np.exp(0.3 * rng.standard_normal(self.nb)))
        self.base = []  # (m, T upper) of every regressor: the posterior of 3 D observations, rounded to dtype
        for _ in range(self.nb):
            X0 = rng.standard_normal((D, 3 * D)) / np.sqrt(D)
            s0 = np.exp(0.3 * rng.standard_normal(3 * D))
            m, _, A = O.posterior_literal(rng.standard_normal(D), np.ones(D), X0, s0, rng.standard_normal(3 * D))
            self.base.append((r(m), r(np.linalg.cholesky(A).T)))

    def sl(self, b):
        return slice(int(self.offsets[b]), int(self.offsets[b + 1]))

    def noise(self, kind, b):
        """the variances of regressor b's slice under noise case `kind`: "diag", "iso0" (one shared), "iso1" (one per regressor)"""
        k = self.counts[b]
        return self.s_diag[self.sl(b)] if kind == "diag" else np.full(k, self.s_reg[0] if kind == "iso0" else self.s_reg[b])

    @functools.lru_cache(maxsize=None)
    def full(self, kind):
        """[(m, T upper)] after conditioning every base state on its slice (rounded to dtype): where a downdate starts"""
        out = []
        for b in range(self.nb):
            m, T = self.base[b]
            if self.counts[b]:
                m, _, A = O.posterior_literal(m, T.T @ T, self.X[:, self.sl(b)], self.noise(kind, b), self.y[self.sl(b)])
                T = np.linalg.cholesky(A).T
            out.append((np.asarray(m, dtype=self.dtype).astype(np.float64), np.asarray(T, dtype=self.dtype).astype(np.float64)))
        return out

    def start(self, direction, kind):
        return self.base if direction == "update" else self.full(kind)

    # ---- the library's operands ------------------------------------------------------------------------------------------------
    def x_operand(self, layout):
        """-> (array, layout flag name, ldx); padding rows hold NaN: "colvecs", "colvecs_odd" (ldx = D + 3), "rowvecs" (ldx = total + 5)"""
        D, total, dt = self.D, self.total, self.dtype
        if layout == "rowvecs":
            buf = np.full((total + 5, D), np.nan, dtype=dt, order="F")
            buf[:total, :] = self.X.T
            return buf, "LAYOUT_ROWVECS", total + 5
        ldx = D + 3 if layout == "colvecs_odd" else D
        buf = np.full((ldx, max(total, 1)), np.nan, dtype=dt, order="F")
        buf[:D, :total] = self.X
        return buf, "LAYOUT_COLVECS", ldx

    def s_operand(self, kind):
        """-> (array, noise kind name, strides)"""
        if kind == "diag":
            return self.s_diag.astype(self.dtype), "NOISE_DIAGONAL", 0
        return self.s_reg.astype(self.dtype), "NOISE_ISOTROPIC", 0 if kind == "iso0" else 1

    def state_operands(self, states):
        """dense state arrays: mw [nb, D], T [nb, D, D] with T[b] the column-major factor (strictly-lower part NaN)"""
        D = self.D
        mw = np.stack([m for m, _ in states]).astype(self.dtype)
        T = np.stack([np.where(np.tri(D, k=-1, dtype=bool).T, np.nan, U.T) for _, U in states]).astype(self.dtype)
        return mw, T


def call(a, h, direction, P, layout, kind, mw, T, memspace="host", counts=None):
    """One ragged call on dense state arrays (in place) through the host memspace -> (logpdf, info)"""
    Xa, lay, ldx = P.x_operand(layout)
    s, nk, strides = P.s_operand(kind)
    lp, info = np.full(P.nb, -7.0), np.full(P.nb, 7, dtype=np.int32)
    fn = h.update_factor_ragged if direction == "update" else h.downdate_factor_ragged
    fn(P.dtype, a.MEM_HOST, getattr(a, lay), P.nb, P.D, P.offsets, Xa, ldx, P.y.astype(P.dtype), getattr(a, nk), s, strides, mw, P.D, T, P.D,
       P.D * P.D, lp, info)
    return lp, info


def yardstick(a, h, route, P, kind, b, m0, T0, layout="colvecs"):
    """The B = 1 entry point the bit promise names, on regressor b's slice and a copy of its state -> (mw, T, logpdf, info).
    route "sweep": blr_update_factor_* (the caller has set SWEEP=always); "downdate": blr_downdate_factor_*; "refit":
    blr_posterior_ragged_* in place with BLR_PRIOR_UPPER_FACTOR."""
    D, k, dt = P.D, P.counts[b], P.dtype
    sl = P.sl(b)
    if layout == "rowvecs":
        Xb, lay, ldx = np.asfortranarray(P.X[:, sl].T.astype(dt)), a.LAYOUT_ROWVECS, k
    else:
        ldx = D + 3 if layout == "colvecs_odd" else D
        Xb = np.zeros((ldx, k), dtype=dt, order="F")
        Xb[:D] = P.X[:, sl]
        lay = a.LAYOUT_COLVECS
    yb = P.y[sl].astype(dt)
    if kind == "diag":
        sb, nk = P.s_diag[sl].astype(dt), a.NOISE_DIAGONAL
    else:
        sb, nk = np.array([P.s_reg[0] if kind == "iso0" else P.s_reg[b]], dtype=dt), a.NOISE_ISOTROPIC
    m, T = m0.copy(), T0.copy()
    lp, info = np.zeros(1), np.full(1, 7, dtype=np.int32)
    if route == "refit":
        h.posterior_ragged(dt, a.MEM_HOST, lay, 1, D, np.array([0, k], dtype=np.int64), Xb, ldx, yb, nk, sb, 0, a.PRIOR_UPPER_FACTOR, m, D, T, D,
                           D * D, m, D, T, D, D * D, None, D, D * D, lp, info)
    else:
        fn = h.update_factor if route == "sweep" else h.downdate_factor
        fn(dt, a.MEM_HOST, lay, 1, D, k, Xb, ldx, 0, yb, 0, nk, sb, 0, m, 0, T, D, 0, lp, info)
    return m, T, lp[0], int(info[0])


def same_bits(x, y):
    return np.asarray(x).tobytes() == np.asarray(y).tobytes()
