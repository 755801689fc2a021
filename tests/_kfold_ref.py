"""Shared by tests/test_kfold_cpu.py and tests/test_kfold_gpu.py: the data generator of tests/test_loo_gpu.py (`_state`, copied), the
closed form of the leave-fold-out predictives in plain NumPy (include/blr_mi355x.h blr_kfold_batched_*), the brute force by refits with
the CPU oracle, and the fp32 yardstick (the principle of tests/_yardsticks.py: the float64 closed form on the fp32-rounded inputs is the
truth, the same closed form run in NumPy float32 on them sets the error a careful fp32 computation makes)."""
import math

import numpy as np

from oracle import blr_oracle as O

LOG2PI = math.log(2.0 * math.pi)


def rng_of(i=0):
    return np.random.Generator(np.random.PCG64(777 + i))


def state(rng, D, N, scale=0.7):
    """A prior (mw, U upper, Lw = U'U) and N observations of dimension D (tests/test_loo_gpu.py `_state`)."""
    U = np.triu(rng.standard_normal((D, D))) * (0.3 / np.sqrt(D))
    U[np.diag_indices(D)] = 1.0 + np.abs(U[np.diag_indices(D)])
    mw = rng.standard_normal(D)
    X = np.asfortranarray(rng.standard_normal((D, N)) * (scale / np.sqrt(D)))
    s = np.exp(0.3 * rng.standard_normal(N))
    y = rng.standard_normal(N)
    return mw, U, X, s, y


def posterior_state(mw, U, X, s, y):
    """(mw', T upper) of the posterior that contains the observations, by the oracle."""
    mwp, T, _ = O.posterior_literal(mw, U.T @ U, X, np.diag(np.broadcast_to(s, (X.shape[1],))), y)
    return mwp, np.triu(T)


def closed_form(mwp, T, X, s, y, F, dtype=np.float64):
    """The identities of the header in NumPy at `dtype`: (mean [N], var [N], logpdf [nfolds], largest eigenvalue of any H~)."""
    mwp, T, X, y = (np.asarray(a, dtype=dtype) for a in (mwp, T, X, y))
    N = X.shape[1]
    s = np.broadcast_to(np.asarray(s, dtype=dtype), (N,))
    Z = np.linalg.solve(T.T, X).astype(dtype) if X.shape[0] else X
    r = y - X.T @ mwp
    mean, var, lps, lam = np.empty(N, dtype=dtype), np.empty(N, dtype=dtype), [], 0.0
    for a in range(0, N, F):
        b = min(a + F, N)
        q = (1 / np.sqrt(s[a:b])).astype(dtype)
        Zf = Z[:, a:b]
        Ht = (Zf.T @ Zf) * q[:, None] * q[None, :]
        lam = max(lam, float(np.linalg.eigvalsh(Ht.astype(np.float64)).max()))
        L = np.linalg.cholesky(np.eye(b - a, dtype=dtype) - Ht)
        Li = np.linalg.inv(L).astype(dtype)
        u = Li @ (r[a:b] * q)
        mean[a:b] = y[a:b] - np.sqrt(s[a:b]) * (Li.T @ u)
        var[a:b] = s[a:b] * np.sum(Li * Li, axis=0)
        lps.append(-0.5 * ((b - a) * dtype(LOG2PI) + np.sum(np.log(s[a:b])) - 2 * np.sum(np.log(np.diag(L))) + u @ u))
    return mean, var, np.array(lps, dtype=dtype), lam


def brute_force(mw, Lw, X, s, y, F):
    """The chain rule with the oracle: log p(y_F | rest) = logpdf_literal(all) - logpdf_literal(rest); mean and var from
    posterior_literal(rest).  Lw dense D x D, s a vector."""
    N = X.shape[1]
    full = O.logpdf_literal(mw, Lw, X, np.diag(s), y)
    mean, var, lps = np.empty(N), np.empty(N), []
    for a in range(0, N, F):
        b = min(a + F, N)
        rest = [j for j in range(N) if not a <= j < b]
        if rest:
            lps.append(full - O.logpdf_literal(mw, Lw, X[:, rest], np.diag(s[rest]), y[rest]))
            mr, _, Ar = O.posterior_literal(mw, Lw, X[:, rest], np.diag(s[rest]), y[rest])
        else:  # F >= N: the predictive under the prior
            lps.append(full)
            mr, Ar = mw, Lw
        mean[a:b] = X[:, a:b].T @ mr
        var[a:b] = np.einsum("dn,dn->n", X[:, a:b], np.linalg.solve(Ar, X[:, a:b])) + s[a:b]
    return mean, var, np.array(lps)


def fp32_bounds(mwp, T, X, s, y, F):
    """-> (truth, bounds): truth = the float64 closed form on the fp32-rounded inputs; bounds[k] = 4 x the largest error the closed
    form makes in NumPy float32 on them + a floor of 8 eps32 of the output's scale, per output (mean, var, logpdf)."""
    r = [np.asarray(a, dtype=np.float32) for a in (mwp, T, X, s, y)]
    truth = closed_form(*[a.astype(np.float64) for a in r], F)[:3]
    low = closed_form(*r, F, dtype=np.float32)[:3]
    eps = float(np.finfo(np.float32).eps)
    bounds = [4.0 * float(np.max(np.abs(l.astype(np.float64) - t))) + 8 * eps * max(1.0, float(np.max(np.abs(t)))) for l, t in zip(low, truth)]
    return truth, bounds
