"""Shared by tests/test_kfold_multi_cpu.py and tests/test_kfold_multi_gpu.py: multi-output states for the generator of
tests/_kfold_ref.py and the yardsticks of that file applied column by column (include/blr_mi355x.h blr_kfold_multi_batched_*).  The
factor T of a posterior does not depend on y, so one `posterior_state` per column gives the shared T and the columns of M.  A column's
data depend on its index alone, never on S: column c of an S = 19 problem IS the S = 1 problem of that column."""
import functools

import numpy as np

from _kfold_ref import brute_force, closed_form, fp32_bounds, posterior_state, rng_of, state


@functools.lru_cache(maxsize=None)
def _base(seed, D, N):
    mw, U, X, s, y = state(rng_of(seed), D, N)
    mwp, T = posterior_state(mw, U, X, s, y)
    return mw, U, X, s, y, mwp, T


@functools.lru_cache(maxsize=None)
def _column(seed, D, N, c):
    """(targets, posterior mean) of column c; column 0 is the generator's own y"""
    mw, U, X, s, y, mwp, _ = _base(seed, D, N)
    if c == 0:
        return y, mwp
    yc = np.random.Generator(np.random.PCG64([seed, D, N, c])).standard_normal(N)
    return yc, posterior_state(mw, U, X, s, yc)[0]


def columns_state(seed, D, N, S):
    """-> (mw, U, X, s, Y [N, S], M [D, S], T): the prior, the data and the multi-output state that contains them"""
    mw, U, X, s, _, _, T = _base(seed, D, N)
    cols = [_column(seed, D, N, c) for c in range(S)]
    Y = np.stack([c[0] for c in cols], axis=1) if S else np.zeros((N, 0))
    M = np.stack([c[1] for c in cols], axis=1) if S else np.zeros((D, 0))
    return mw, U, X, s, Y, M, T


def closed_form_columns(M, T, X, s, Y, F, dtype=np.float64):
    """closed_form of tests/_kfold_ref.py per column -> (mean [N, S], var [N] (column 0's: it does not depend on the column),
    logpdf [nfolds, S], largest eigenvalue of any H~)"""
    cols = [closed_form(M[:, c], T, X, s, Y[:, c], F, dtype) for c in range(Y.shape[1])]
    return (np.stack([c[0] for c in cols], axis=1), cols[0][1], np.stack([c[2] for c in cols], axis=1), max(c[3] for c in cols))


def brute_force_columns(mw, Lw, X, s, Y, F):
    """brute_force of tests/_kfold_ref.py (refits with the oracle) per column -> (mean [N, S], var [N, S], logpdf [nfolds, S])"""
    cols = [brute_force(mw, Lw, X, s, Y[:, c], F) for c in range(Y.shape[1])]
    return tuple(np.stack([c[i] for c in cols], axis=1) for i in range(3))


def fp32_bounds_columns(M, T, X, s, Y, F):
    """fp32_bounds of tests/_kfold_ref.py per column -> [(truth, bounds)] with truth = (mean [N], var [N], logpdf [nfolds])"""
    return [fp32_bounds(M[:, c], T, X, s, Y[:, c], F) for c in range(Y.shape[1])]
