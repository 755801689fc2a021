"""Shared by tests/test_kfold_large_cpu.py and tests/test_kfold_large_gpu.py: the weight-space closed form of the leave-fold-out
predictives in plain NumPy (include/blr_mi355x.h blr_kfold_large_batched_*) at a given dtype, and the fp32 yardstick by the principle
of `fp32_bounds` in tests/_kfold_ref.py (the float64 closed form on the fp32-rounded inputs is the truth; the same closed form run in
NumPy float32 on them sets the error a careful fp32 computation makes).  Data generator, posterior state and brute force: _kfold_ref."""
import numpy as np

from _kfold_ref import LOG2PI

# the shapes (D, N, F) of the issue's CPU check: tiny, D = 1 with one fold of everything, a last fold of fewer than 64 rows, a partial
# last tile, F > N, several column blocks (32, 2200, 2100) and the two shapes shared with blr_kfold_batched_*
SHAPES = [(7, 13, 5), (1, 65, 65), (16, 130, 65), (17, 200, 100), (100, 200, 128), (128, 200, 200), (128, 130, 300), (64, 1100, 220),
          (32, 2200, 2100), (128, 640, 128), (128, 200, 64), (100, 130, 16)]


def closed_form_large(mwp, T, X, s, y, F, dtype=np.float64):
    """The identities of the header in NumPy at `dtype`: (mean [N], var [N], logpdf [nfolds], cancellation), the last one the largest
    diagonal entry of A over the smallest of any A_f.  logdet, q_f, l_f and |u|^2 are formed in float64, as the library forms them."""
    mwp, T, X, y = (np.asarray(a, dtype=dtype) for a in (mwp, T, X, y))
    D, N = X.shape
    s = np.broadcast_to(np.asarray(s, dtype=dtype), (N,))
    A = (T.T @ T).astype(dtype)
    logdet_A = 2.0 * np.sum(np.log(np.diag(T).astype(np.float64)))
    mean, var, lps, cancel = np.empty(N, dtype=dtype), np.empty(N, dtype=dtype), [], 0.0
    for a in range(0, N, F):
        b = min(a + F, N)
        Xf, sf = X[:, a:b], s[a:b]
        W = (Xf / sf).astype(dtype)
        G = (W @ Xf.T).astype(dtype)
        r0 = (y[a:b] - Xf.T @ mwp).astype(dtype)
        d = (W @ r0).astype(dtype)
        q = float(np.sum(r0.astype(np.float64) ** 2 / sf.astype(np.float64)))
        l = float(np.sum(np.log(sf.astype(np.float64))))
        Af = (A - G).astype(dtype)
        cancel = max(cancel, float(np.max(np.diag(A)) / np.min(np.diag(Af))))
        L = np.linalg.cholesky(Af).astype(dtype)  # A_f = L L', U_f = L'
        u = np.linalg.solve(L, d).astype(dtype)
        mwf = (mwp - np.linalg.solve(L.T, u)).astype(dtype)
        Z = np.linalg.solve(L, Xf).astype(dtype)
        mean[a:b] = Xf.T @ mwf
        var[a:b] = sf + np.sum(Z * Z, axis=0)
        logdet_Af = 2.0 * np.sum(np.log(np.diag(L).astype(np.float64)))
        uu = float(np.sum(u.astype(np.float64) ** 2))
        lps.append(-0.5 * ((b - a) * LOG2PI + l + logdet_A - logdet_Af + q + uu))
    return mean, var, np.array(lps, dtype=np.float64), cancel


def fp32_bounds_large(mwp, T, X, s, y, F):
    """-> (truth, bounds): truth = the float64 closed form on the fp32-rounded inputs; bounds[k] = 4 x the largest error the closed
    form makes in NumPy float32 on them + a floor of 8 eps32 of the output's scale, per output (mean, var, logpdf)."""
    r = [np.asarray(a, dtype=np.float32) for a in (mwp, T, X, s, y)]
    truth = closed_form_large(*[a.astype(np.float64) for a in r], F)[:3]
    low = closed_form_large(*r, F, dtype=np.float32)[:3]
    eps = float(np.finfo(np.float32).eps)
    bounds = [4.0 * float(np.max(np.abs(np.asarray(l, dtype=np.float64) - t))) + 8 * eps * max(1.0, float(np.max(np.abs(t))))
              for l, t in zip(low, truth)]
    return truth, bounds
