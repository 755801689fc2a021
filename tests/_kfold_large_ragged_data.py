"""Shared by tests/test_kfold_large_ragged_cpu.py and tests/test_kfold_large_ragged_gpu.py: packed batches of regressors with unequal
observation counts AND their own fold sizes (blr_kfold_large_ragged_*).  The slices are drawn as
tests/_kfold_ragged_data.py draws them (tests/_kfold_ref.py `state`: a unit-scale factor prior, noise O(1)), the states come from the
float64 oracle on the data as cast.  Each regressor of COUNTS / FOLDS sits on one seam of the route:
  (0, 3) no observations        (1, 1) the smallest regressor       (7, 1) folds of one       (7, 100) F_b > N_b: one fold of everything
  (130, 65) a fold that crosses a 64-row tile and ends on a partial one          (200, 64) a short last fold of 8
  (1100, 550) one column block, many stages        (2148, 2048) a two-block full fold, then a 100-row last fold with one block
  (4200, 2100) two full two-block folds whose second block ends off a 64-row boundary
The CPU test asserts that no fold of these inputs is near-degenerate; the GPU tests share one cached batch per (D, counts)."""
import numpy as np

import _kfold_ragged_data as K27
from _kfold_large_ref import closed_form_large, fp32_bounds_large

LEAD = K27.LEAD
COUNTS = [0, 1, 7, 7, 130, 200, 1100, 2148, 4200]
FOLDS = [3, 1, 1, 100, 65, 64, 550, 2048, 2100]
DS = [5, 17]
BIG_D, BIG_COUNTS, BIG_FOLDS = 128, [300, 70], [150, 35]  # the LDS-heavy instantiations
NOISES = K27.NOISES
# largest max diag(A) / min diag(A_f) any fold may have (closed_form_large's fourth output).  By construction the worst fold is the
# first of (2148, 2048): it removes 2048 of 2148 observations, so A_f keeps 100 / 2148 of the data's information plus the prior --
# a factor of at most 21.5 -- and the quotient takes the LARGEST diagonal entry of A over the SMALLEST of A_f, whose sampling scatter
# over 100 rows of scale 0.7 / sqrt(D) under noise exp(0.3 N(0, 1)) is within 1.5.  Every other regressor halves its data (factor 2)
# or, where one fold holds ALL of it (N_b <= 7), leaves the unit-scale prior under at most 7 such observations.  32 = 21.5 x 1.5.
CANCEL_CAP = 32.0


def nfolds(n, F):
    return 0 if n == 0 else (1 if F >= n else -(-n // F))


class Batch(K27.Batch):
    def __init__(self, D, counts, folds, seed=0):
        super().__init__(D, counts, seed)
        self.folds = list(folds)

    def fold_offsets(self, regs=None):
        regs = range(self.nb) if regs is None else regs
        return np.concatenate([[0], np.cumsum([nfolds(self.counts[b], self.folds[b]) for b in regs])]).astype(np.int64)

    def slice64(self, noise, dtype, b):
        """(mw', T upper, X, s, y) of regressor b in float64 as the library sees them at dtype"""
        c = lambda a: np.asarray(a).astype(dtype).astype(np.float64)  # noqa: E731
        mw, Tc = self.states(noise, dtype)
        return c(mw[b]), c(Tc[b]).T, c(self.X[:, self.sl(b)]), c(self.noise(noise, b)), c(self.y[self.sl(b)])

    def reference(self, noise, dtype, b):
        """closed_form_large of slice b in float64 on the inputs as cast -> (mean, var, logpdf, cancellation)"""
        key = ("ref", noise, np.dtype(dtype).name, b)
        if key not in self._states:
            self._states[key] = closed_form_large(*self.slice64(noise, dtype, b), self.folds[b])
        return self._states[key]

    def bounds32(self, noise, b):
        key = ("b32", noise, b)
        if key not in self._states:
            self._states[key] = fp32_bounds_large(*self.slice64(noise, np.float32, b), self.folds[b])
        return self._states[key]


_BATCHES = {}


def batch(D, counts=None, folds=None):
    counts, folds = counts or COUNTS, folds or FOLDS
    key = (D, tuple(counts), tuple(folds))
    if key not in _BATCHES:
        _BATCHES[key] = Batch(D, counts, folds, seed=3)
    return _BATCHES[key]
