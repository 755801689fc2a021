"""Shared by tests/test_kfold_ragged_cpu.py and tests/test_kfold_ragged_gpu.py: packed batches of regressors with unequal observation
counts whose slices are drawn as tests/_kfold_ref.py `state` draws a problem (scale 0.7), and their posterior states.  The CPU test
asserts that no fold of any batch the GPU tests use is near-degenerate; the GPU tests share one cached batch per (D, counts, seed)."""
import numpy as np

from _kfold_ref import closed_form, rng_of, state

COUNTS = [0, 1, 7, 8, 9, 63, 64, 65, 200, 0, 333]
LEAD = 5  # offsets[0]: leading observations of the packed arrays that belong to nobody
DS = [5, 64, 128]
FS = [1, 3, 8, 21, 64]
NOISES = ["one", "per_regressor", "diagonal"]
# The draw of each D.  At D = 5 a fold of 64 that holds ALL 63 .. 65 observations of a regressor removes nearly everything the state
# knows: at scale 0.7 the largest eigenvalue of its H~ is typically 0.92 .. 0.94 (seeds 0 .. 11), over the 0.9 the tests allow; seed 7
# is the first draw that stays under it (tests/test_kfold_ragged_cpu.py asserts the bound for every batch the GPU tests use).
SEEDS = {5: 7, 64: 0, 128: 0}
LARGE_D, LARGE_COUNTS, LARGE_F = 129, [0, 5, 70], 8  # the D > 128 route


class Batch:
    """Packed data of len(counts) regressors (float64 masters, cast on use); slice b is `state(rng_of(..), D, counts[b], 0.7)`."""

    def __init__(self, D, counts, seed=0, lead=LEAD):
        self.D, self.counts = D, list(counts)
        self.off = np.concatenate([[lead], lead + np.cumsum(counts)]).astype(np.int64)
        nb, tot = len(counts), int(self.off[-1])
        self.nb, self.tot = nb, tot
        self.X, self.y, self.s_diag = np.zeros((D, tot)), np.zeros(tot), np.ones(tot)
        self.mw, self.U = np.zeros((nb, D)), np.zeros((nb, D, D))
        for b, n in enumerate(counts):
            mw, U, X, s, y = state(rng_of(1000 * seed + 37 * b + D), D, n, scale=0.7)
            self.mw[b], self.U[b] = mw, U
            self.X[:, self.sl(b)], self.y[self.sl(b)], self.s_diag[self.sl(b)] = X, y, s
        self.s_reg = np.exp(0.3 * rng_of(1000 * seed + 999 + D).standard_normal(nb))
        self._states = {}

    def sl(self, b):
        return slice(int(self.off[b]), int(self.off[b + 1]))

    def fold_offsets(self, F):
        return np.concatenate([[0], np.cumsum([-(-n // F) for n in self.counts])]).astype(np.int64)

    def noise(self, kind, b):
        """per-observation noise variances of regressor b under noise `kind`"""
        n = self.counts[b]
        if kind == "one":
            return np.full(n, self.s_reg[0])
        if kind == "per_regressor":
            return np.full(n, self.s_reg[b])
        return self.s_diag[self.sl(b)]

    def states(self, noise, dtype):
        """posterior states (mw' [nb, D], T [nb, D, D] COLUMN-major: entry [b, j, i] = T_b[i, j]) of every regressor in float64
        from the data as cast to dtype, then cast.  Cached: the GPU tests share them."""
        key = (noise, np.dtype(dtype).name)
        if key not in self._states:
            D = self.D
            mws, Ts = np.empty((self.nb, D)), np.empty((self.nb, D, D))
            for b in range(self.nb):
                X = self.X[:, self.sl(b)].astype(dtype).astype(np.float64)
                y = self.y[self.sl(b)].astype(dtype).astype(np.float64)
                s = self.noise(noise, b).astype(dtype).astype(np.float64)
                U = self.U[b].astype(dtype).astype(np.float64)
                mw = self.mw[b].astype(dtype).astype(np.float64)
                A = U.T @ U + (X / s) @ X.T
                Ts[b] = np.linalg.cholesky((A + A.T) / 2).T
                mws[b] = np.linalg.solve(A, U.T @ (U @ mw) + X @ (y / s))
            self._states[key] = (np.ascontiguousarray(mws, dtype=dtype), np.ascontiguousarray(Ts.transpose(0, 2, 1), dtype=dtype))
        return self._states[key]

    def reference(self, noise, dtype, F, b, state=None):
        """closed_form of slice b at float64 on the inputs as cast to dtype -> (mean, var, logpdf, largest eigenvalue of any H~)"""
        mwp, Tc = state or self.states(noise, dtype)
        return closed_form(mwp[b].astype(np.float64), Tc[b].astype(np.float64).T, self.X[:, self.sl(b)].astype(dtype).astype(np.float64),
                           self.noise(noise, b).astype(dtype).astype(np.float64), self.y[self.sl(b)].astype(dtype).astype(np.float64), F)


_BATCHES = {}


def batch(D, seed=None, counts=None):
    seed = SEEDS.get(D, 0) if seed is None else seed
    key = (D, seed, tuple(counts or COUNTS))
    if key not in _BATCHES:
        _BATCHES[key] = Batch(D, counts or COUNTS, seed)
    return _BATCHES[key]
