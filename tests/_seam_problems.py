"""Problems and fp64 references for tests/test_chunk_seams_gpu.py: batches in which every regressor has its own X, targets,
noise, prior mean and factor (a swapped regressor index cannot cancel), sentinel-filled padded outputs, and a VECTORISED numpy
restatement of the marginals, the leave-one-out predictives and the evidence gradient for batches too large to loop the Python
oracle over (tests/test_seam_problems_cpu.py pins it against oracle/ on the first regressors)."""
import numpy as np

LOG2PI = float(np.log(2.0 * np.pi))
SENTINEL = 0xA5


class Out:
    """A flat output array: nb items of rows x cols (column-major, leading dimension ld) at `stride`, the sentinel byte everywhere;
    `init` (nb x cols x rows) seeds the payload of an array the call updates in place."""

    def __init__(self, dtype, rows, cols=1, nb=1, pad=3, init=None):
        self.rows, self.cols, self.nb = rows, cols, nb
        self.ld = rows + pad if cols > 1 else rows
        one = (cols - 1) * self.ld + rows
        self.stride = one + pad if nb > 1 else one
        n = (nb - 1) * self.stride + one
        self.idx = (np.arange(nb)[:, None, None] * self.stride + np.arange(cols)[None, :, None] * self.ld + np.arange(rows)[None, None, :])
        self.a = np.frombuffer(bytes([SENTINEL]) * (n * np.dtype(dtype).itemsize), dtype=dtype).copy()
        if init is not None:
            self.a[self.idx.ravel()] = np.asarray(init, dtype=dtype).ravel()

    def payload(self, a):
        """nb x cols x rows (cols == 1: nb x rows)"""
        p = a[self.idx]
        return p[:, 0, :] if self.cols == 1 else p

    def gaps_kept(self, a):
        gap = np.ones(a.size, dtype=bool)
        gap[self.idx.ravel()] = False
        return bool((a.view(np.uint8).reshape(a.size, -1)[gap] == SENTINEL).all())

    def per_regressor(self, a):
        """the payload with the regressor first: an array of nb items, or ONE item whose rows are the regressors (info, loo_total)"""
        p = self.payload(a)
        return p[0][:, None] if self.nb == 1 else p


def batch(B, D, N, S, seed, shared_x=False):
    """fp64 batch: X [B | 1, N, D] (ColVecs, column-major per regressor), y [B, N], Y [B, S, N], s [B, N], mw [B, D], M [B, S, D],
    U [B, D, D] upper factors stored COLUMN-major (U[b].T is the upper triangle), built as triu(U0) * c_b + diag(d_b) in one
    broadcast.  Every regressor differs in every operand."""
    rng = np.random.Generator(np.random.PCG64(seed))
    p = {"B": B, "D": D, "N": N, "S": S}
    p["X"] = rng.standard_normal((1 if shared_x else B, N, D)) * (0.7 / np.sqrt(D))
    p["y"] = rng.standard_normal((B, N))
    p["Y"] = rng.standard_normal((B, S, N))
    p["s"] = np.exp(0.3 * rng.standard_normal((B, N)))
    p["mw"] = rng.standard_normal((B, D))
    p["M"] = rng.standard_normal((B, S, D))
    U0 = np.triu(rng.standard_normal((D, D)), 1) * (0.3 / np.sqrt(D))
    c = 0.5 + rng.random(B)
    d = 1.0 + rng.random((B, D))
    Uu = U0[None] * c[:, None, None]            # [b, i, j], i < j
    Uu[:, np.arange(D), np.arange(D)] = d
    p["U"] = np.ascontiguousarray(np.swapaxes(Uu, 1, 2))  # column-major storage
    return p


def upper(p):
    """[B, D, D] upper triangular matrices (row i, column j) of a batch"""
    return np.swapaxes(p["U"], 1, 2)


def condition(p, Y=None):
    """The states that CONTAIN the batch's observations: T [B, D, D] (column-major storage of the upper factor of A = U'U + X S^-1 X')
    and the means of the targets `Y` [B, S, N] (default: p["y"] as one column) -> (Mpost [B, S, D], T)."""
    X = np.broadcast_to(p["X"], (p["B"],) + p["X"].shape[1:])  # [B, N, D]
    Uu = upper(p)
    Lw = np.swapaxes(Uu, 1, 2) @ Uu
    A = Lw + np.swapaxes(X / p["s"][:, :, None], 1, 2) @ X
    L = np.linalg.cholesky(A)  # lower: A = L L', T = L'
    prior = p["mw"][:, None, :] if Y is None else p["M"]
    Y = p["y"][:, None, :] if Y is None else Y
    rhs = prior @ Lw + (Y / p["s"][:, None, :]) @ X  # (Lw symmetric)
    Mpost = np.swapaxes(np.linalg.solve(A, np.swapaxes(rhs, 1, 2)), 1, 2)
    return Mpost, np.ascontiguousarray(L)  # (L row-major == T = L' column-major)


# ---- the vectorised references (fp64, stacked) ---------------------------------------------------------------------------------
def marginals_ref(X, Mw, Ucm, s):
    """X [B | 1, N, D], Mw [B, S, D], Ucm [B, D, D] (column-major upper factor), s [B, N] -> mean [B, S, N], var [B, N]
    (mean_n = x_n'm, var_n = |U^-T x_n|^2 + s_n: oracle marginals_direct, stacked)"""
    mean = Mw @ np.swapaxes(X, 1, 2)
    # U' alpha = x: Ucm[b] as a row-major matrix IS U' (lower triangular)
    Ut = np.tril(Ucm)
    alpha = np.linalg.solve(Ut, np.swapaxes(np.broadcast_to(X, (Ucm.shape[0],) + X.shape[1:]), 1, 2))  # [B, D, N]
    return mean, np.sum(alpha * alpha, axis=1) + s


def diag_marginals_ref(X, Mw, dprec, s):
    """a diagonal prior PRECISION dprec [B, D]"""
    Xb = np.broadcast_to(X, (Mw.shape[0],) + X.shape[1:])
    return np.einsum("bnd,bsd->bsn", Xb, Mw), np.einsum("bnd,bd->bn", Xb * Xb, 1.0 / dprec) + s


def loo_ref(X, Mpost, Tcm, s, Y):
    """Leave-one-out predictives of observations the states contain: X [B | 1, N, D], Mpost [B, S, D], Tcm [B, D, D], s [B, N],
    Y [B, S, N] -> mean [B, S, N], var [B, N], logpdf [B, S, N], total [B, S] (h_n = x_n'A^-1 x_n / s_n; mean = y - r / (1 - h),
    var = s / (1 - h))"""
    m, lat = marginals_ref(X, Mpost, Tcm, np.zeros_like(s))
    omh = 1.0 - lat / s
    r = Y - m
    mean = Y - r / omh[:, None, :]
    var = s / omh
    lp = -0.5 * (LOG2PI + np.log(var)[:, None, :] + (Y - mean) ** 2 / var[:, None, :])
    return mean, var, lp, lp.sum(axis=2)


def grad_ref(X, y, s, mw, Ucm):
    """Evidence and its gradient (oracle logpdf_grad, stacked): -> logpdf [B], dX [B, N, D], dy, ds [B, N], dmw, mw_post [B, D]"""
    B = y.shape[0]
    Xb = np.broadcast_to(X, (B,) + X.shape[1:])
    Uu = np.swapaxes(np.tril(Ucm), 1, 2)
    Lw = np.swapaxes(Uu, 1, 2) @ Uu
    w = 1.0 / s
    A = Lw + np.swapaxes(Xb * w[:, :, None], 1, 2) @ Xb
    delta = y - np.einsum("bnd,bd->bn", Xb, mw)
    b = np.einsum("bnd,bn->bd", Xb, w * delta)
    L = np.linalg.cholesky(A)
    u = np.linalg.solve(L, b[:, :, None])[:, :, 0]
    m = np.linalg.solve(np.swapaxes(L, 1, 2), u[:, :, None])[:, :, 0]
    logdet_A = 2.0 * np.log(np.diagonal(L, axis1=1, axis2=2)).sum(axis=1)
    logdet_Lw = 2.0 * np.log(np.diagonal(Uu, axis1=1, axis2=2)).sum(axis=1)
    lp = -0.5 * (y.shape[1] * LOG2PI + np.log(s).sum(axis=1) + (delta * delta * w).sum(axis=1) + logdet_A - logdet_Lw - (u * u).sum(axis=1))
    mwp = mw + m
    r = y - np.einsum("bnd,bd->bn", Xb, mwp)
    Z = np.linalg.solve(L, np.swapaxes(Xb, 1, 2))                # [B, D, N]
    G = np.linalg.solve(np.swapaxes(L, 1, 2), Z)                 # A^-1 X
    v = (Z * Z).sum(axis=1)
    dX = (mwp[:, None, :] * r[:, :, None] - np.swapaxes(G, 1, 2)) * w[:, :, None]
    return lp, dX, -w * r, -(s - r * r - v) / (2.0 * s * s), np.einsum("bnd,bn->bd", Xb, w * r), mwp
