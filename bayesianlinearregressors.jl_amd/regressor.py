"""Host-side mirror of BayesianLinearRegressors.jl's AbstractGPs surface, backed by the MI355X library.

Julia is not available in the build image, so this is the reference's operator interface restated
in Python over the same C ABI a Julia ``ccall`` shim binds: same names, same
argument meaning, same error behaviour.  Every number is computed by the HIP kernels; there is no
CPU fallback.

    f   = BayesianLinearRegressor(mw, Lw)            # reference src/bayesian_linear_regression.jl:11-14
    fx  = f(ColVecs(X), Sigma)                       # FiniteGP (AbstractGPs)
    logpdf(fx, y); posterior(fx, y)                  # :55-58, :60-69
    mean(fx); var(fx); mean_and_var(fx); marginals(fx)   # :33, :40-43, :47
    rand(rng, fx, S)                                 # :49-53
    rand(rng, f) / rand(rng, f, dims)                # src/sampling_functions.jl:27-38
    BasisFunctionRegressor(f, phi)                   # src/basis_function_regression.jl:34-65
"""
from __future__ import annotations

import math
from collections import namedtuple

import numpy as np

from . import _abi

__all__ = [
    "ColVecs", "RowVecs", "Diagonal", "Symmetric", "PDMat", "Normal", "RandomFourierFeatures",
    "BayesianLinearRegressor", "BasisFunctionRegressor", "BLRFunctionSample", "FiniteGP",
    "mean", "var", "cov", "std", "mean_and_var", "mean_and_cov", "marginals", "rand", "rand_b", "logpdf", "posterior",
    "LOO", "loo", "loo_map", "loo_columns", "loo_columns_map",
    "KFold", "kfold", "kfold_map", "kfold_large", "kfold_large_map", "cross_validate", "kfold_columns", "kfold_columns_map",
    "EvidenceGrid", "logpdf_grid", "posterior_best", "logpdf_grid_map", "logpdf_grid_ragged", "posterior_best_ragged",
    "posterior_ragged", "logpdf_ragged", "mean_ragged", "var_ragged", "mean_and_var_ragged", "loo_ragged", "kfold_ragged",
    "kfold_large_ragged", "cross_validate_ragged",
    "posterior_columns", "logpdf_columns_map", "posterior_columns_map",
    "mean_and_var_columns", "mean_columns", "mean_and_var_columns_map",
    "cov_map", "mean_and_cov_map",
    "rand_columns", "rand_columns_map",
]


# ---------------------------------------------------------------------------------------------------
# containers (KernelFunctions.ColVecs / RowVecs, LinearAlgebra.Diagonal / Symmetric, PDMats.PDMat)
# ---------------------------------------------------------------------------------------------------
class ColVecs:
    """D x N matrix whose columns are the inputs."""

    def __init__(self, X):
        X = np.asarray(X)
        if X.ndim != 2:
            raise ValueError("ColVecs expects a matrix")
        self.X = X

    def __len__(self):
        return self.X.shape[1]

    def __getitem__(self, idx):
        return ColVecs(self.X[:, idx])


class RowVecs:
    """N x D matrix whose rows are the inputs."""

    def __init__(self, X):
        X = np.asarray(X)
        if X.ndim != 2:
            raise ValueError("RowVecs expects a matrix")
        self.X = X

    def __len__(self):
        return self.X.shape[0]

    def __getitem__(self, idx):
        return RowVecs(self.X[idx, :])


class Diagonal:
    def __init__(self, diag):
        self.diag = np.asarray(diag)
        if self.diag.ndim != 1:
            raise ValueError("Diagonal expects a vector")

    @property
    def shape(self):
        n = self.diag.shape[0]
        return (n, n)

    def toarray(self):
        return np.diag(self.diag)


class Symmetric:
    def __init__(self, data):
        self.data = np.asarray(data)

    @property
    def shape(self):
        return self.data.shape

    def toarray(self):
        u = np.triu(self.data)
        return u + np.triu(self.data, 1).T


class PDMat:
    """Positive-definite matrix carried by its upper Cholesky factor (PDMats.PDMat(Cholesky(U)))."""

    def __init__(self, U):
        self.U = np.asarray(U)

    @property
    def shape(self):
        return self.U.shape

    def toarray(self):
        u = np.triu(self.U)
        return u.T @ u


class Normal:
    """Distributions.Normal(mu, sigma) -- what `marginals` returns per input."""

    __slots__ = ("mu", "sigma")

    def __init__(self, mu, sigma):
        self.mu, self.sigma = float(mu), float(sigma)

    def __repr__(self):
        return f"Normal(mu={self.mu}, sigma={self.sigma})"


def std(n):
    return n.sigma if isinstance(n, Normal) else np.array([k.sigma for k in n])


# ---------------------------------------------------------------------------------------------------
# x_as_colvecs: reference :20-31.  Index/shape work only -- resolved to (pointer, layout flag, ld)
# ---------------------------------------------------------------------------------------------------
def _x_layout(x, dtype):
    """-> (array kept alive, layout flag, ldx, D, N) with zero copies for C- or F-contiguous input."""
    if isinstance(x, ColVecs):
        M, colvecs = x.X, True
    elif isinstance(x, RowVecs):
        M, colvecs = x.X, False
    elif isinstance(x, np.ndarray) and x.ndim == 2:
        M, colvecs = x, True  # AbstractGPs turns a raw D x N matrix into ColVecs
    else:
        raise TypeError(
            f"{type(x).__name__} is not a subtype of AbstractVector that is known. "
            "Please provide either a ColVecs or RowVecs."
        )
    M = np.asarray(M, dtype=dtype)
    if not (M.flags.c_contiguous or M.flags.f_contiguous):
        M = np.ascontiguousarray(M)
    if colvecs:
        D, N = M.shape
        # (D, N) Fortran order  == D x N column-major == COLVECS;  C order == N x D column-major == ROWVECS
        if M.flags.f_contiguous:
            return M, _abi.LAYOUT_COLVECS, max(D, 1), D, N
        return M, _abi.LAYOUT_ROWVECS, max(N, 1), D, N
    N, D = M.shape
    if M.flags.f_contiguous:
        return M, _abi.LAYOUT_ROWVECS, max(N, 1), D, N
    return M, _abi.LAYOUT_COLVECS, max(D, 1), D, N


def _first_nonpositive(v):
    """1-based index of the first entry that is not > 0 (NaN included), 0 if all are: LAPACK `info` of a diagonal Cholesky."""
    bad = np.flatnonzero(~(np.asarray(v) > 0))
    return int(bad[0]) + 1 if bad.size else 0


def _noise(Sy, N, dtype, need_cholesky=False):
    """-> (array, noise_kind).  Scalar = f(x, sigma^2); vector / Diagonal = Diagonal(v).
    ``need_cholesky``: the caller's reference method runs _cholesky(Sigma_y) (rand, :52) and the kernel behind it does not
    report a non-positive variance itself -- raise PosDefException here, as the reference would (logpdf / posterior get it
    from the kernel's info)."""
    if isinstance(Sy, Diagonal):
        Sy = Sy.diag
    Sy = np.asarray(Sy, dtype=dtype)
    if Sy.ndim <= 1 and need_cholesky:
        k = _first_nonpositive(Sy.reshape(-1))
        if k:
            raise _abi.PosDefException(k)
    if Sy.ndim == 0:
        return Sy.reshape(1).copy(), _abi.NOISE_ISOTROPIC
    if Sy.ndim == 1:
        if Sy.shape[0] != N:
            raise ValueError("length of the noise diagonal != number of inputs")
        return np.ascontiguousarray(Sy), _abi.NOISE_DIAGONAL
    if Sy.ndim == 2:  # dense N x N covariance (the reference's own toy problems, test/test_utils.jl:7-8)
        if Sy.shape != (N, N):
            raise ValueError("size of the noise covariance != number of inputs")
        return np.asfortranarray(Sy), _abi.NOISE_DENSE
    raise ValueError("noise covariance must be a scalar, a vector / Diagonal, or an N x N matrix")


def _mean_vector(mw, D, dtype):
    """The prior mean as a contiguous vector of the working dtype; its length must be the input dimension (the library copies
    D elements from this buffer: a shorter one would be read past its end instead of raising the reference's DimensionMismatch)."""
    mw = np.ascontiguousarray(mw, dtype=dtype)
    if mw.ndim != 1 or mw.shape[0] != D:
        raise ValueError(f"length(mw) = {mw.shape[0] if mw.ndim == 1 else mw.shape} != dimension of the inputs ({D})")
    return mw


def _prior(Lw, D, dtype, need_cholesky=False):
    """-> (array, prior_kind, ldl).  ``need_cholesky``: see _noise (var / rand / weight draws with a Diagonal precision are
    elementwise kernels that do not report a non-positive entry; the reference's _cholesky(Lw) at :41 / :51 throws)."""
    if isinstance(Lw, Diagonal):
        d = np.ascontiguousarray(Lw.diag, dtype=dtype)
        if d.shape[0] != D:
            raise ValueError("size of the prior precision != length(mw)")
        if need_cholesky:
            k = _first_nonpositive(d)
            if k:
                raise _abi.PosDefException(k)
        return d, _abi.PRIOR_DIAGONAL, 1
    if isinstance(Lw, PDMat):
        U = np.asfortranarray(Lw.U, dtype=dtype)
        kind = _abi.PRIOR_UPPER_FACTOR
    else:
        A = Lw.data if isinstance(Lw, Symmetric) else Lw
        U = np.asfortranarray(A, dtype=dtype)  # upper triangle is read (LAPACK 'U')
        kind = _abi.PRIOR_DENSE
    if U.shape != (D, D):
        raise ValueError("size of the prior precision != length(mw)")
    return U, kind, max(D, 1)


def _dtype_of(*arrays):
    dts = [np.asarray(a).dtype for a in arrays if a is not None]
    if dts and all(dt == np.float32 for dt in dts):
        return np.float32
    return np.float64


# ---------------------------------------------------------------------------------------------------
# the regressors
# ---------------------------------------------------------------------------------------------------
class BayesianLinearRegressor:
    """w ~ Normal(mw, inv(Lw));  f(x) = dot(x, w).   reference :11-14"""

    def __init__(self, mw, Lw):
        self.mw = np.asarray(mw)
        if self.mw.ndim != 1:
            raise ValueError("mw must be a vector")
        self.Lw = Lw

    # field name used by the reference
    @property
    def Λw(self):  # noqa: PLC2401
        return self.Lw

    def __call__(self, x, Sy=1e-18):
        return FiniteGP(self, x, Sy)


class BasisFunctionRegressor:
    """bfr(X) = blr(phi(X)).   reference src/basis_function_regression.jl:34-37"""

    def __init__(self, blr, phi):
        if not isinstance(blr, BayesianLinearRegressor):
            raise TypeError("BasisFunctionRegressor wraps a BayesianLinearRegressor")
        self.blr = blr
        self.phi = phi

    @property
    def ϕ(self):  # noqa: PLC2401
        return self.phi

    def __call__(self, x, Sy=1e-18):
        return FiniteGP(self, x, Sy)


class RandomFourierFeatures:
    """phi(x) = scale * cos(Omega' x + phase): the random-Fourier basis of BASELINE config 5, usable as the `phi`
    of a BasisFunctionRegressor (the reference accepts any callable, src/basis_function_regression.jl:7-9).
    Omega is D_in x D.  Calling it materialises the features through the device kernel; `logpdf` / `posterior`
    on a BasisFunctionRegressor with this phi take the fused path (features never leave the GPU)."""

    def __init__(self, Omega, phase, scale=None):
        self.Omega = np.asarray(Omega)
        self.phase = np.asarray(phase)
        if self.Omega.ndim != 2 or self.phase.shape != (self.Omega.shape[1],):
            raise ValueError("Omega must be D_in x D and phase of length D")
        self.scale = float(np.sqrt(2.0 / self.Omega.shape[1])) if scale is None else float(scale)

    def _operands(self, x, dtype):
        X, layout, ldx, Din, N = _x_layout(x, dtype)
        if layout != _abi.LAYOUT_COLVECS:  # the feature kernel reads ColVecs inputs (D_in is tiny: one small copy)
            # ROWVECS layout = N x D_in column-major.  Which axis of the numpy array is N follows from the CONTAINER and the
            # memory order that _x_layout resolved -- never from comparing shapes (a square N == D_in input is ambiguous).
            M = X if isinstance(x, RowVecs) else X.T  # -> (N, D_in) view of the same memory
            X = np.asfortranarray(M.T, dtype=dtype)     # (D_in, N) column-major: ColVecs
            ldx = max(Din, 1)
        if Din != self.Omega.shape[0]:
            raise ValueError("input dimension != rows of Omega")
        Om = np.asfortranarray(self.Omega, dtype=dtype)
        ph = np.ascontiguousarray(self.phase, dtype=dtype)
        return X, ldx, Din, N, Om, ph

    def __call__(self, x):
        dtype = _dtype_of(self.Omega, x.X if hasattr(x, "X") else x)
        X, ldx, Din, N, Om, ph = self._operands(x, dtype)
        D = Om.shape[1]
        Phi = np.empty((D, N), dtype=dtype, order="F")
        _handle().rff_features(dtype, _abi.MEM_HOST, Din, D, N, X, ldx, Om, max(Din, 1), ph, self.scale, Phi, max(D, 1))
        if isinstance(x, RowVecs):
            return RowVecs(Phi.T)
        if isinstance(x, ColVecs):
            return ColVecs(Phi)
        return Phi


class FiniteGP:
    """AbstractGPs.FiniteGP: a regressor evaluated at inputs x with observation-noise covariance Sy."""

    def __init__(self, f, x, Sy):
        self.f, self.x, self.Sy = f, x, Sy

    @property
    def Σy(self):  # noqa: PLC2401
        return self.Sy


def _to_finite_blr(fx):
    """reference src/basis_function_regression.jl:41"""
    if isinstance(fx.f, BasisFunctionRegressor):
        return FiniteGP(fx.f.blr, fx.f.phi(fx.x), fx.Sy)
    if isinstance(fx.f, BayesianLinearRegressor):
        return fx
    raise TypeError("expected a FiniteGP over a BayesianLinearRegressor or BasisFunctionRegressor")


def _handle():
    return _abi.default_handle()


def _wrap_like(prior_Lw, T, A):
    """__build_Lambda, reference :92-93: PDMat prior -> PDMat posterior carrying T; else Symmetric(T'T)."""
    if isinstance(prior_Lw, PDMat):
        return PDMat(T)
    return Symmetric(A)


# ---------------------------------------------------------------------------------------------------
# AbstractGPs API
# ---------------------------------------------------------------------------------------------------
def _fused_rff(fx, y, want_posterior):
    """BasisFunctionRegressor with a RandomFourierFeatures phi: features + inference in one library call."""
    bfr, rff, blr = fx.f, fx.f.phi, fx.f.blr
    dtype = _dtype_of(blr.mw, y, rff.Omega)
    X, ldx, Din, N, Om, ph = rff._operands(fx.x, dtype)
    D = Om.shape[1]
    y = np.ascontiguousarray(y, dtype=dtype)
    if y.ndim != 1 or y.shape[0] != N:
        raise ValueError("length(y) != size(fx.x.X, 2)")  # reference :74
    mw = _mean_vector(blr.mw, D, dtype)
    s, noise_kind = _noise(fx.Sy, N, dtype)
    Lw, prior_kind, ldl = _prior(blr.Lw, D, dtype)
    lp = np.zeros(1, dtype=np.float64)
    info = np.zeros(1, dtype=np.int32)
    mw_post = T = A = None
    if want_posterior:
        mw_post = np.empty(D, dtype=dtype)
        T = np.empty((D, D), dtype=dtype, order="F")
        A = np.empty((D, D), dtype=dtype, order="F") if not isinstance(blr.Lw, PDMat) else None
    _handle().posterior_rff(dtype, _abi.MEM_HOST, Din, D, N, X, ldx, Om, max(Din, 1), ph, rff.scale, y, noise_kind, s,
                            prior_kind, mw, Lw, ldl, mw_post, T, max(D, 1), A, max(D, 1), lp, info)
    if info[0] > 0:
        raise _abi.PosDefException(int(info[0]))
    return float(lp[0]), mw_post, T, A


def _fused(fx, y, want_posterior):
    if isinstance(fx.f, BasisFunctionRegressor) and isinstance(fx.f.phi, RandomFourierFeatures):
        return _fused_rff(fx, y, want_posterior)
    fx = _to_finite_blr(fx)
    blr = fx.f
    dtype = _dtype_of(blr.mw, y)
    X, layout, ldx, D, N = _x_layout(fx.x, dtype)
    y = np.ascontiguousarray(y, dtype=dtype)
    if y.ndim != 1:
        raise ValueError("y must be a vector")
    if y.shape[0] != N:
        raise ValueError("length(y) != size(fx.x.X, 2)")  # reference :74
    mw = _mean_vector(blr.mw, D, dtype)
    s, noise_kind = _noise(fx.Sy, N, dtype)
    Lw, prior_kind, ldl = _prior(blr.Lw, D, dtype)
    lp = np.zeros(1, dtype=np.float64)
    if want_posterior:
        mw_post = np.empty(D, dtype=dtype)
        T = np.empty((D, D), dtype=dtype, order="F")
        A = np.empty((D, D), dtype=dtype, order="F") if not isinstance(blr.Lw, PDMat) else None
    else:
        mw_post = T = A = None
    if noise_kind == _abi.NOISE_DENSE:  # reference :79-82 general branch: whitened on the device (blr_posterior_dense_noise_*)
        info = np.zeros(1, dtype=np.int32)
        _handle().posterior_dense_noise(dtype, _abi.MEM_HOST, layout, D, N, X, ldx, y, s, max(N, 1), prior_kind, mw, Lw, ldl, mw_post, T,
                                        max(D, 1), A, max(D, 1), lp, info)
        if info[0] > 0:
            raise _abi.PosDefException(int(info[0]))
        return float(lp[0]), mw_post, T, A
    _handle().posterior(dtype, layout, D, N, X, ldx, y, noise_kind, s, prior_kind, mw, Lw, ldl, mw_post, T, max(D, 1),
                        A, max(D, 1), lp)
    return float(lp[0]), mw_post, T, A


def logpdf(fx, y):
    """reference :55-58.  A matrix Y (N x S) gives the column-wise log densities (AbstractGPs fallback)."""
    y = np.asarray(y)
    if y.ndim == 2:
        return logpdf_columns(fx, y)
    return _fused(fx, y, want_posterior=False)[0]


def logpdf_columns(fx, Y, return_means=False):
    """Shared-X multi-output evidence (AbstractGPs' logpdf(fx, Y::AbstractMatrix)): the Gram matrix and its factor are
    formed once, per column only one GEMM column and two triangular solves remain (blr_logpdf_multi_*).
    ``return_means=True`` also returns the D x S matrix of per-column posterior means."""
    fx = _to_finite_blr(fx)
    blr = fx.f
    dtype = _dtype_of(blr.mw, Y)
    X, layout, ldx, D, N = _x_layout(fx.x, dtype)
    Yf = np.asfortranarray(Y, dtype=dtype)
    if Yf.shape[0] != N:
        raise ValueError("length(y) != size(fx.x.X, 2)")
    S = Yf.shape[1]
    mw = _mean_vector(blr.mw, D, dtype)
    s, noise_kind = _noise(fx.Sy, N, dtype)
    if noise_kind == _abi.NOISE_DENSE:  # AbstractGPs' column-wise fallback (each column re-whitens; test sizes only)
        lps, means = [], []
        for j in range(S):
            lp_j, m_j, _, _ = _fused(fx, Yf[:, j], want_posterior=return_means)
            lps.append(lp_j)
            means.append(m_j)
        return (np.array(lps), np.stack(means, axis=1)) if return_means else np.array(lps)
    Lw, prior_kind, ldl = _prior(blr.Lw, D, dtype)
    lp = np.zeros(S, dtype=np.float64)
    if D <= 128 and S <= 256 and not return_means:
        # few columns of a small problem: S independent fused updates in one launch (X shared through strideX = 0) beat the
        # fixed cost of the shared-X pipeline (measured: 0.57 ms vs 1.13 ms at D=128, N=4096, S=64)
        infos = np.zeros(S, dtype=np.int32)
        _handle().posterior_batched(dtype, _abi.MEM_HOST, layout, S, D, N, X, ldx, 0, Yf, N, noise_kind, s, 0, prior_kind,
                                    mw, 0, Lw, ldl, 0, None, D, None, max(D, 1), D * D, None, max(D, 1), D * D, lp, infos)
        bad = np.flatnonzero(infos)
        if bad.size:
            raise _abi.PosDefException(int(infos[bad[0]]))
        return lp
    info = np.zeros(1, dtype=np.int32)
    M = np.empty((D, S), dtype=dtype, order="F") if return_means else None
    _handle().logpdf_multi(dtype, _abi.MEM_HOST, layout, D, N, S, X, ldx, Yf, max(N, 1), noise_kind, s, prior_kind, mw, Lw, ldl,
                           lp, M, max(D, 1), info)
    if info[0] != 0:
        raise _abi.PosDefException(int(info[0]))
    return (lp, M) if return_means else lp


def _upper_inverse_on_device(h, dtype, prior_kind, Lw, D):
    """Uw^-1 (D x D, float64) for Uw = chol(Lw).U or the given upper factor: blr_sample_weights_* on the identity (w = 0 + Uw^-1 z
    per column, reference sampling_functions.jl:29) -- the library factorises a dense prior itself; no host LAPACK."""
    eye = np.asfortranarray(np.eye(D, dtype=dtype))
    W = np.zeros((D, D), dtype=dtype, order="F")
    Lw_arr = np.asfortranarray(np.asarray(Lw, dtype=dtype))
    h.sample_weights(dtype, _abi.MEM_HOST, D, D, prior_kind, np.zeros(D, dtype=dtype), Lw_arr, max(D, 1), eye, D, W, D)
    return W.astype(np.float64)


def _prior_inverse_on_device(h, dtype, prior_kind, Lw, D):
    """Lw^-1 = Uw^-1 Uw^-T for a dense precision or an upper factor, by two triangular-solve calls on the device (the second one
    solves against the rows of the first result); used by the prior tangent of the evidence gradient."""
    Ui = _upper_inverse_on_device(h, dtype, prior_kind, Lw, D)
    Z = np.asfortranarray(Ui.T.astype(dtype))
    W = np.zeros((D, D), dtype=dtype, order="F")
    Lw_arr = np.asfortranarray(np.asarray(Lw, dtype=dtype))
    h.sample_weights(dtype, _abi.MEM_HOST, D, D, prior_kind, np.zeros(D, dtype=dtype), Lw_arr, max(D, 1), Z, D, W, D)
    Wd = W.astype(np.float64)
    return 0.5 * (Wd + Wd.T)


def logpdf_and_gradient(fx, y):
    """The value of logpdf(fx, y) (reference :55-58) and its gradient with respect to every input of the path -- the
    reverse-mode rule the reference gets from Zygote through its Julia code (README.md:56-71) and a ccall-backed logpdf
    must provide itself.

    Returns ``(lp, grads)`` with ``grads`` a dict: ``X`` (same container layout as the inputs: D x N for ColVecs / a
    matrix, N x D for RowVecs), ``y`` (N), ``noise`` (N for Diagonal noise, a scalar for isotropic noise), ``mw`` (D)
    and ``Lw`` -- the gradient with respect to the precision: symmetric D x D for a dense / Symmetric / PDMat prior
    (for PDMat(U) chain with dU = U (G + G')), the diagonal (D) for a Diagonal prior."""
    fx = _to_finite_blr(fx)
    blr = fx.f
    dtype = _dtype_of(blr.mw, y)
    X, layout, ldx, D, N = _x_layout(fx.x, dtype)
    y = np.ascontiguousarray(y, dtype=dtype)
    if y.ndim != 1 or y.shape[0] != N:
        raise ValueError("length(y) != size(fx.x.X, 2)")  # reference :74
    mw = _mean_vector(blr.mw, D, dtype)
    s, noise_kind = _noise(fx.Sy, N, dtype)
    if noise_kind == _abi.NOISE_DENSE:
        raise NotImplementedError("logpdf_and_gradient: closed-form rule implemented for isotropic / Diagonal noise only")
    Lw, prior_kind, ldl = _prior(blr.Lw, D, dtype)
    lp = np.zeros(1, dtype=np.float64)
    info = np.zeros(1, dtype=np.int32)
    dX = np.empty_like(X)  # same memory order and leading dimension as the staged inputs
    dy = np.empty(N, dtype=dtype)
    ds = np.empty(N, dtype=dtype)
    dmw = np.empty(D, dtype=dtype)
    mw_post = np.empty(D, dtype=dtype)
    Ainv = np.empty((D, D), dtype=dtype, order="F")
    _handle().logpdf_grad_batched(dtype, _abi.MEM_HOST, layout, 1, D, N, X, ldx, 0, y, 0, noise_kind, s, 0, prior_kind, mw, 0,
                                  Lw, ldl, 0, lp, dX, ldx, 0, dy, 0, ds, 0, dmw, 0, mw_post, 0, Ainv, D, 0, info)
    if info[0] != 0:
        raise _abi.PosDefException(int(info[0]))
    # dL/dLw = -(m m' + A^-1 - Lw^-1) / 2: D x D host work on the device's A^-1 and posterior mean
    m = (mw_post - mw).astype(np.float64)
    Ai = np.asarray(Ainv, dtype=np.float64)
    Ai = np.tril(Ai) + np.tril(Ai, -1).T  # symmetric by construction; use one triangle
    if prior_kind == _abi.PRIOR_DIAGONAL:
        gL = -0.5 * (m * m + np.diag(Ai) - 1.0 / np.asarray(Lw, dtype=np.float64))
    else:
        # (the prior's inverse in float64 whatever the element type of the call: D x D work, and the three terms cancel)
        gL = -0.5 * (np.outer(m, m) + Ai - _prior_inverse_on_device(_handle(), np.float64, prior_kind, Lw, D))
    # hand dX back in the caller's container orientation
    x = fx.x
    if isinstance(x, RowVecs):
        gX = dX if dX.shape == (N, D) else dX.T
    else:
        gX = dX if dX.shape == (D, N) else dX.T
    grads = {"X": np.asarray(gX), "y": dy, "noise": ds if noise_kind == _abi.NOISE_DIAGONAL else dtype(ds.sum(dtype=np.float64)),
             "mw": dmw, "Lw": gL.astype(dtype)}
    return float(lp[0]), grads


def posterior(fx, y):
    """reference :60-69 (and basis_function_regression.jl:62-65): same wrapper type as the prior."""
    _, mw_post, T, A = _fused(fx, y, want_posterior=True)
    base = fx.f.blr if isinstance(fx.f, BasisFunctionRegressor) else fx.f
    post = BayesianLinearRegressor(mw_post, _wrap_like(base.Lw, T, A))
    if isinstance(fx.f, BasisFunctionRegressor):
        return BasisFunctionRegressor(post, fx.f.phi)
    return post


# ---------------------------------------------------------------------------------------------------
# many independent regressors in ONE library call: what `map(posterior, fxs, ys)` / `logpdf.(fxs, ys)` are in the reference
# (config 4 of BASELINE.json is this with 8192 regressors; at D > 128 the regressors share every launch of the update)
# ---------------------------------------------------------------------------------------------------
def _fused_many(fxs, ys, want_posterior):
    """[(logpdf, mw', T, A)] in ONE library call: equally shaped problems through blr_posterior_batched_*, problems that agree
    on everything but the number of observations (same D, layout, isotropic or diagonal noise, prior kind, dtype) packed side
    by side through blr_posterior_ragged_*.  Layouts, noise or prior kinds that differ (or a dense noise covariance, or a
    fused random-Fourier basis) fall back to one call per problem.
    The first problem (in order) whose prior, noise or posterior precision is not positive definite raises
    PosDefException, as the map over the reference's methods would; its position is the exception's ``index``."""
    fxs, ys = list(fxs), list(ys)
    if len(fxs) != len(ys):
        raise ValueError("as many observation vectors as finite regressors are needed")
    if not fxs:
        return []
    one_by_one = lambda: [_fused(fx, y, want_posterior) for fx, y in zip(fxs, ys)]  # noqa: E731
    if any(isinstance(fx.f, BasisFunctionRegressor) and isinstance(fx.f.phi, RandomFourierFeatures) for fx in fxs):
        return one_by_one()
    fbs = [_to_finite_blr(fx) for fx in fxs]
    dtype = np.float32 if all(_dtype_of(fb.f.mw, y) == np.float32 for fb, y in zip(fbs, ys)) else np.float64
    probs = []
    for fb, y in zip(fbs, ys):
        X, layout, ldx, D, N = _x_layout(fb.x, dtype)
        y = np.ascontiguousarray(y, dtype=dtype)
        if y.ndim != 1:
            raise ValueError("y must be a vector")
        if y.shape[0] != N:
            raise ValueError("length(y) != size(fx.x.X, 2)")  # reference :74
        s, noise_kind = _noise(fb.Sy, N, dtype)
        Lw, prior_kind, ldl = _prior(fb.f.Lw, D, dtype)
        probs.append((X, layout, ldx, D, N, y, s, noise_kind, _mean_vector(fb.f.mw, D, dtype), Lw, prior_kind, ldl,
                      isinstance(fb.f.Lw, PDMat)))
    X0, layout, ldx, D, N, _, s0, noise_kind, _, _, prior_kind, ldl, pdmat = probs[0]
    if noise_kind == _abi.NOISE_DENSE or D == 0:
        return one_by_one()
    sig = {(q[0].shape, q[0].flags.f_contiguous, q[1], q[3], q[4], q[7], q[10], q[12]) for q in probs}
    ragged = len(sig) != 1
    if ragged and len({(q[1], q[3], q[7], q[10], q[12]) for q in probs}) != 1:
        return one_by_one()
    if not ragged and N == 0:
        return one_by_one()
    nb = len(probs)
    mwb = np.stack([q[8] for q in probs])
    Lb = np.stack([q[9].reshape(-1, order="A") for q in probs])  # D, or D x D column-major
    lp = np.zeros(nb, dtype=np.float64)
    info = np.zeros(nb, dtype=np.int32)
    if want_posterior:
        mw_post = np.empty((nb, D), dtype=dtype)
        Tb = np.empty((nb, D * D), dtype=dtype)
        Ab = np.empty((nb, D * D), dtype=dtype) if not pdmat else None
    else:
        mw_post = Tb = Ab = None
    if ragged:
        # the observations side by side: ColVecs problems are D x N_b column-major each (their columns simply follow one
        # another), RowVecs problems N_b x D column-major (stacked by rows into one offsets[-1] x D column-major matrix)
        offsets = np.concatenate(([0], np.cumsum([q[4] for q in probs]))).astype(np.int64)
        if layout == _abi.LAYOUT_COLVECS:
            Xp, ldxp = np.concatenate([q[0].reshape(-1, order="A") for q in probs]), D
        else:
            Xp = np.asfortranarray(np.concatenate([q[0].reshape(-1, order="A").reshape((q[4], D), order="F") for q in probs]))
            ldxp = max(int(offsets[-1]), 1)
        yp = np.concatenate([q[5] for q in probs])
        sp = np.concatenate([q[6] for q in probs])  # isotropic: one variance per problem (strides = 1); diagonal: packed like y
        _handle().posterior_ragged(dtype, _abi.MEM_HOST, layout, nb, D, offsets, Xp, ldxp, yp, noise_kind, sp, 1, prior_kind, mwb, D,
                                   Lb, ldl, Lb.shape[1], mw_post, D, Tb, D, D * D, Ab, D, D * D, lp, info)
    else:
        # one contiguous block per operand: problem b at b * stride (each X already is ldx x cols column-major in memory)
        Xb = np.stack([q[0].reshape(-1, order="A") for q in probs])
        yb = np.stack([q[5] for q in probs])
        sb = np.stack([q[6] for q in probs])
        _handle().posterior_batched(dtype, _abi.MEM_HOST, layout, nb, D, N, Xb, ldx, Xb.shape[1], yb, yb.shape[1], noise_kind, sb,
                                    sb.shape[1], prior_kind, mwb, D, Lb, ldl, Lb.shape[1], mw_post, D, Tb, D, D * D, Ab, D, D * D, lp, info)
    return _unpack_many(lp, info, mw_post, Tb, Ab, D)


def _unpack_many(lp, info, mw_post, Tb, Ab, D):
    """Per-problem results of a batched / ragged call; the first failed problem raises PosDefException with its ``index``."""
    bad = np.flatnonzero(info > 0)
    if bad.size:
        e = _abi.PosDefException(int(info[bad[0]]))
        e.index = int(bad[0])
        raise e
    out = []
    for b in range(lp.shape[0]):
        if mw_post is not None:
            out.append((float(lp[b]), mw_post[b], Tb[b].reshape((D, D), order="F"), Ab[b].reshape((D, D), order="F") if Ab is not None else None))
        else:
            out.append((float(lp[b]), None, None, None))
    return out


def _ragged_operands(f, x, offsets, Sy, y):
    """The packed arguments every ragged entry point shares, as the library wants them (``y`` None: a call without targets; ``Sy``
    None: a call that does not read the noise) -> None for an empty batch."""
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    if offsets.ndim != 1 or offsets.shape[0] < 1:
        raise ValueError("offsets must be a vector of B + 1 entries")
    nb, total = offsets.shape[0] - 1, int(offsets[-1])
    fs = [f] * nb if isinstance(f, BayesianLinearRegressor) else list(f)
    if len(fs) != nb or not all(isinstance(g, BayesianLinearRegressor) for g in fs):
        raise ValueError("f must be one BayesianLinearRegressor or B = len(offsets) - 1 of them")
    if nb == 0:
        return None, fs
    dtype = np.float32 if all(_dtype_of(g.mw, y if y is not None else g.mw) == np.float32 for g in fs) else np.float64
    X, layout, ldx, D, N = _x_layout(x, dtype)
    if N != total:
        raise ValueError("offsets[-1] != number of inputs")
    if y is not None:
        y = np.ascontiguousarray(y, dtype=dtype)
        if y.ndim != 1 or y.shape[0] != N:
            raise ValueError("length(y) != size(fx.x.X, 2)")  # reference :74
    if Sy is None:
        s, noise_kind = None, _abi.NOISE_ISOTROPIC
    elif isinstance(Sy, Diagonal):
        s, noise_kind = _noise(Sy, N, dtype)
    else:
        Sy = np.asarray(Sy, dtype=dtype)
        if Sy.ndim == 1 and Sy.shape[0] != N and Sy.shape[0] == nb:  # one variance per regressor
            s, noise_kind = np.ascontiguousarray(Sy), _abi.NOISE_ISOTROPIC
        else:
            s, noise_kind = _noise(Sy, N, dtype)
    if noise_kind == _abi.NOISE_DENSE:
        raise ValueError("a dense noise covariance is not supported for packed regressors")
    shared = isinstance(f, BayesianLinearRegressor)
    priors = [_prior(g.Lw, D, dtype) for g in ([f] if shared else fs)]
    if len({(k, isinstance(g.Lw, PDMat)) for (_, k, _), g in zip(priors, fs)}) != 1:
        raise ValueError("the regressors must share one kind of prior precision")
    _, prior_kind, ldl = priors[0]
    pdmat = isinstance(fs[0].Lw, PDMat)
    mwb = np.stack([_mean_vector(g.mw, D, dtype) for g in ([f] if shared else fs)])
    Lb = np.stack([q[0].reshape(-1, order="A") for q in priors])
    strides = 1 if s is not None and s.shape[0] == nb and noise_kind == _abi.NOISE_ISOTROPIC else 0
    return (dtype, offsets, nb, X, layout, ldx, D, y, s, noise_kind, strides, prior_kind, ldl, pdmat, mwb, 0 if shared else D, Lb,
            0 if shared else Lb.shape[1]), fs


def _ragged_packed(f, x, offsets, Sy, y, want_posterior):
    """The packed form behind posterior_ragged / logpdf_ragged -> ([(logpdf, mw', T, A)], the B prior regressors)."""
    ops, fs = _ragged_operands(f, x, offsets, Sy, y)
    if ops is None:
        return [], fs
    dtype, offsets, nb, X, layout, ldx, D, y, s, noise_kind, strides, prior_kind, ldl, pdmat, mwb, stridemw, Lb, strideLw = ops
    lp = np.zeros(nb, dtype=np.float64)
    info = np.zeros(nb, dtype=np.int32)
    if want_posterior:
        mw_post = np.empty((nb, D), dtype=dtype)
        Tb = np.empty((nb, D * D), dtype=dtype)
        Ab = np.empty((nb, D * D), dtype=dtype) if not pdmat else None
    else:
        mw_post = Tb = Ab = None
    _handle().posterior_ragged(dtype, _abi.MEM_HOST, layout, nb, D, offsets, X, ldx, y, noise_kind, s, strides,
                               prior_kind, mwb, stridemw, Lb, ldl, strideLw, mw_post, D, Tb, D, D * D, Ab, D,
                               D * D, lp, info)
    return _unpack_many(lp, info, mw_post, Tb, Ab, D), fs


def logpdf_ragged(f, x, offsets, Sy, y):
    """Log evidence of B regressors whose observations are already packed side by side: regressor b owns the inputs / entries
    of y ``offsets[b]:offsets[b+1]`` (reference :55-58 under a map over fxs of different lengths), one library call.
    ``f``: one BayesianLinearRegressor shared by all, or B of them with one kind of prior precision.  ``Sy``: a scalar (one
    variance for all), a vector of B variances (one per regressor), or a vector / Diagonal of ``offsets[-1]``
    per-observation variances (a plain vector whose length equals both is read per observation)."""
    return np.array([r[0] for r in _ragged_packed(f, x, offsets, Sy, y, want_posterior=False)[0]])


def posterior_ragged(f, x, offsets, Sy, y):
    """[posterior(f_b(x[offsets[b]:offsets[b+1]], Sy_b), y[...])] (reference :60-69 under a map) from packed arrays in one
    library call; arguments as logpdf_ragged."""
    res, fs = _ragged_packed(f, x, offsets, Sy, y, want_posterior=True)
    return [BayesianLinearRegressor(mw_post, _wrap_like(g.Lw, T, A)) for g, (_, mw_post, T, A) in zip(fs, res)]


def _raise_first_failed(info):
    """The first non-zero ``info[b]`` raises PosDefException(info[b]) with ``index`` = b."""
    bad = np.flatnonzero(info)
    if bad.size:
        e = _abi.PosDefException(int(info[bad[0]]))
        e.index = int(bad[0])
        raise e


def _marginals_ragged(f, x, offsets, Sy, want_mean, want_var):
    """The packed form behind mean_ragged / var_ragged / mean_and_var_ragged -> (mean or None, var or None), offsets[-1] long."""
    ops, _ = _ragged_operands(f, x, offsets, Sy if want_var else None, None)
    if ops is None:
        return (np.empty(0) if want_mean else None), (np.empty(0) if want_var else None)
    dtype, offsets, nb, X, layout, ldx, D, _, s, noise_kind, strides, prior_kind, ldl, _, mwb, stridemw, Lb, strideLw = ops
    total = int(offsets[-1])
    mean = np.zeros(total, dtype=dtype) if want_mean else None
    var = np.zeros(total, dtype=dtype) if want_var else None
    info = np.zeros(nb, dtype=np.int32)
    _handle().marginals_ragged(dtype, _abi.MEM_HOST, layout, nb, D, offsets, X, ldx, noise_kind, s, strides, prior_kind, mwb, stridemw,
                               Lb if want_var else None, ldl, strideLw, mean, var, info)
    _raise_first_failed(info)
    return mean, var


def mean_ragged(f, x, offsets):
    """mean(f_b(x[offsets[b]:offsets[b+1]])) for every b (reference :33 under a map over fxs of different lengths) from packed
    inputs in one library call (blr_marginals_ragged_*); the result is packed as the inputs are, ``offsets[-1]`` long.  ``f``: one
    BayesianLinearRegressor shared by all, or B of them with one kind of prior precision."""
    return _marginals_ragged(f, x, offsets, None, True, False)[0]


def var_ragged(f, x, offsets, Sy):
    """var(f_b(x[offsets[b]:offsets[b+1]], Sy_b)) for every b (reference :40-43 under a map), packed; ``f`` and ``Sy`` as
    `posterior_ragged` takes them.  A dense prior that is not positive definite raises PosDefException with ``index``."""
    return _marginals_ragged(f, x, offsets, Sy, False, True)[1]


def mean_and_var_ragged(f, x, offsets, Sy):
    """(mean, var) of every packed regressor at its own inputs (reference :47 under a map) in one library call; arguments as
    `var_ragged`."""
    return _marginals_ragged(f, x, offsets, Sy, True, True)


def _heldout_ragged(ops, second, ll_offsets, result):
    """What `loo_ragged` and `kfold_ragged` do with their operands: the data staged once, blr_posterior_ragged_* into device buffers
    (mw', T), then ``second(h, head, tail)`` -- the held-out entry point on the same device inputs, ``head`` its arguments up to
    offsets, ``tail`` those from X on -- and the results copied back.  Regressor b owns ``ll_offsets[b]:ll_offsets[b + 1]`` of the
    log densities, ``ll_offsets[-1]`` in all; ``result``: LOO or KFold."""
    dtype, offsets, nb, X, layout, ldx, D, y, s, noise_kind, strides, prior_kind, ldl, _, mwb, stridemw, Lb, strideLw = ops
    h, item, total, n_ll = _handle(), np.dtype(dtype).itemsize, int(offsets[-1]), int(ll_offsets[-1])
    m, v = np.zeros(total, dtype=dtype), np.zeros(total, dtype=dtype)
    lp, tot, info = np.zeros(n_ll, dtype=np.float64), np.zeros(nb, dtype=np.float64), np.zeros(nb, dtype=np.int32)
    with _DeviceScope(h) as scope:
        dev, alloc = scope.dev, scope.alloc
        dX, dy, ds = dev(X.reshape(-1, order="A")), dev(y), dev(s)
        d_mwp, d_T = alloc(nb * D * item), alloc(nb * D * D * item)
        d_info = dev(info)
        head = (dtype, _abi.MEM_DEVICE, layout, nb, D, offsets)
        h.posterior_ragged(*head, dX, ldx, dy, noise_kind, ds, strides, prior_kind, dev(mwb), stridemw, dev(Lb), ldl, strideLw, d_mwp, D, d_T,
                           max(D, 1), D * D, None, max(D, 1), D * D, None, d_info)
        h.memcpy_d2h(info, d_info)
        if not np.any(info):
            d_m, d_v, d_ll, d_tot = alloc(max(total, 1) * item), alloc(max(total, 1) * item), alloc(max(n_ll, 1) * 8), alloc(nb * 8)
            second(h, head, (dX, ldx, dy, noise_kind, ds, strides, d_mwp, D, d_T, max(D, 1), D * D, d_m, d_v, d_ll, d_tot, d_info))
            for host, dptr in ((m, d_m), (v, d_v), (lp, d_ll), (tot, d_tot), (info, d_info)):
                h.memcpy_d2h(host, dptr)
    _raise_first_failed(info)
    return [result(m[offsets[b]:offsets[b + 1]], v[offsets[b]:offsets[b + 1]], lp[ll_offsets[b]:ll_offsets[b + 1]], float(tot[b]))
            for b in range(nb)]


def loo_ragged(f, x, offsets, Sy, y):
    """[loo(f_b(x[offsets[b]:offsets[b+1]], Sy_b), y[...])] from packed arrays: the data staged once, blr_posterior_ragged_* into
    device buffers (mw', T), then blr_loo_ragged_* on the same device inputs -- `_heldout_batch`'s pipeline for unequal counts.
    Nothing D x D comes back to the host.  Arguments as `posterior_ragged`.  The first regressor whose prior, noise or posterior is
    not positive definite raises PosDefException with its position as ``index``."""
    ops, _ = _ragged_operands(f, x, offsets, Sy, y)
    if ops is None:
        return []
    return _heldout_ragged(ops, lambda h, head, tail: h.loo_ragged(*head, *tail), ops[1], LOO)


def kfold_ragged(f, x, offsets, Sy, y, fold_size):
    """[kfold(f_b(x[offsets[b]:offsets[b+1]], Sy_b), y[...], fold_size)] from packed arrays: `loo_ragged`'s pipeline with
    blr_kfold_ragged_* as its second half -- the data staged once, blr_posterior_ragged_* into device buffers (mw', T), then the
    leave-fold-out predictives on the same device inputs.  Nothing D x D comes back to the host.  Regressor b has the folds
    [f fold_size, (f + 1) fold_size) of its own slice, 1 <= fold_size <= 64.  Arguments as `posterior_ragged`; returns a list of
    KFold(mean, var, logpdf, total).  The first regressor whose prior, noise or posterior is not positive definite raises
    PosDefException with its position as ``index``.  Given the same state, regressor b's result has the bits of `kfold` on that
    slice; the states themselves are bit-equal only where blr_posterior_ragged_* and the route `posterior` takes agree to the bit,
    which the handle options NO_I8_GRAM = 1 and NO_WAVE_KERNEL = 1 ensure (include/blr_mi355x.h, blr_posterior_ragged_*)."""
    F = _fold_size(fold_size)
    ops, _ = _ragged_operands(f, x, offsets, Sy, y)
    if ops is None:
        return []
    offsets, nb = ops[1], ops[2]
    fo = np.zeros(nb + 1, dtype=np.int64)
    rc = _abi.load_library().blr_kfold_ragged_fold_offsets(nb, _abi._ptr(offsets), F, _abi._ptr(fo))
    if rc != 0:
        raise ValueError(f"blr_kfold_ragged_fold_offsets: argument error {rc}")
    return _heldout_ragged(ops, lambda h, head, tail: h.kfold_ragged(*head, F, *tail), fo, KFold)


def _kfold_large_ragged(ops, fold_sizes):
    """`_heldout_ragged` with blr_kfold_large_ragged_* as its second half; ``fold_sizes``: int64 [nb]"""
    offsets, nb, D = ops[1], ops[2], ops[6]
    if D > _KFOLD_LARGE_MAX_D:
        raise NotImplementedError(f"kfold_large_ragged: D = {D} is beyond the limit of blr_kfold_large_ragged_* (D <= {_KFOLD_LARGE_MAX_D})")
    fo = np.zeros(nb + 1, dtype=np.int64)
    rc = _abi.load_library().blr_kfold_large_ragged_fold_offsets(nb, _abi._ptr(offsets), _abi._ptr(fold_sizes), _abi._ptr(fo))
    if rc != 0:
        raise ValueError(f"blr_kfold_large_ragged_fold_offsets: argument error {rc} (fold sizes >= 1, at most 1024 folds per regressor)")
    return _heldout_ragged(ops, lambda h, head, tail: h.kfold_large_ragged(*head, fold_sizes, *tail), fo, KFold)


def kfold_large_ragged(f, x, offsets, Sy, y, fold_sizes):
    """[kfold_large(f_b(x[offsets[b]:offsets[b+1]], Sy_b), y[...], fold_sizes[b])] from packed arrays: `kfold_ragged`'s pipeline with
    blr_kfold_large_ragged_* as its second half.  ``fold_sizes``: an int (one size for all) or a vector of B of them, each >= 1
    with at most 1024 folds of its regressor; D <= 128.  Arguments otherwise as `posterior_ragged`; returns a list of
    KFold(mean, var, logpdf, total).  The first regressor whose prior, noise or posterior is not positive definite raises
    PosDefException with its position as ``index``.  Given the same state, regressor b's result has the bits of `kfold_large` on
    that slice; for the states see `kfold_ragged` (handle options NO_I8_GRAM = 1 and NO_WAVE_KERNEL = 1)."""
    ops, _ = _ragged_operands(f, x, offsets, Sy, y)
    if ops is None:
        return []
    nb = ops[2]
    fs = np.asarray(fold_sizes)
    if fs.ndim > 1 or (fs.ndim == 1 and fs.shape[0] != nb) or np.any(fs != np.floor(fs)) or np.any(fs < 1):
        raise ValueError("fold_sizes must be an integer >= 1 or a vector of B such integers")
    return _kfold_large_ragged(ops, np.ascontiguousarray(np.broadcast_to(fs.astype(np.int64), (nb,))))


def cross_validate_ragged(f, x, offsets, Sy, y, n_folds):
    """K-fold cross-validation of every packed regressor with ``n_folds`` contiguous folds of its own F_b = ceil(N_b / n_folds)
    observations (blr_kfold_large_ragged_fold_sizes), in one blr_kfold_large_ragged_* call whatever the F_b are.  Arguments as
    `kfold_large_ragged`; returns a list of KFold(mean, var, logpdf, total), total the regressor's CV score."""
    K = int(n_folds)
    if K != n_folds or K < 1:
        raise ValueError("n_folds must be an integer >= 1")
    ops, _ = _ragged_operands(f, x, offsets, Sy, y)
    if ops is None:
        return []
    offsets, nb = ops[1], ops[2]
    fs = np.zeros(nb, dtype=np.int64)
    rc = _abi.load_library().blr_kfold_large_ragged_fold_sizes(nb, _abi._ptr(offsets), K, _abi._ptr(fs))
    if rc != 0:
        raise ValueError(f"blr_kfold_large_ragged_fold_sizes: argument error {rc} (1 <= n_folds <= 1024)")
    return _kfold_large_ragged(ops, fs)


def logpdf_map(fxs, ys):
    """[logpdf(fx, y) for fx, y in zip(fxs, ys)] (reference :55-58 under a map) in one library call."""
    return [r[0] for r in _fused_many(fxs, ys, want_posterior=False)]


def posterior_map(fxs, ys):
    """[posterior(fx, y) for fx, y in zip(fxs, ys)] (reference :60-69 under a map) in one library call."""
    fxs = list(fxs)
    posts = []
    for fx, (_, mw_post, T, A) in zip(fxs, _fused_many(fxs, ys, want_posterior=True)):
        base = fx.f.blr if isinstance(fx.f, BasisFunctionRegressor) else fx.f
        post = BayesianLinearRegressor(mw_post, _wrap_like(base.Lw, T, A))
        posts.append(BasisFunctionRegressor(post, fx.f.phi) if isinstance(fx.f, BasisFunctionRegressor) else post)
    return posts


# ---------------------------------------------------------------------------------------------------
# matrix targets: S columns per regressor share the design matrix, the noise and the prior (blr_posterior_multi_batched_*)
# ---------------------------------------------------------------------------------------------------
def _columns_many(fxs, Ys, want_posterior):
    """[(logpdf[S], means D x S, T, A)] per data set.  Equally shaped problems (same D, N, S, layout, noise and prior kind) with
    isotropic or diagonal noise go through blr_posterior_multi_batched_* in ONE call: one factor per data set, shared by its
    columns.  Mixed shapes or a dense noise covariance fall back to a loop over logpdf_columns / posterior.  The first data set
    (in order) that is not positive definite raises PosDefException with its position as ``index``."""
    fxs, Ys = list(fxs), list(Ys)
    if len(fxs) != len(Ys):
        raise ValueError("as many target matrices as finite regressors are needed")
    if not fxs:
        return []
    Ys = [np.asarray(Y) for Y in Ys]
    if any(Y.ndim != 2 for Y in Ys):
        raise ValueError("every Y must be an N x S matrix")

    def loop():
        out = []
        for fx, Y in zip(fxs, Ys):
            if not want_posterior:
                out.append((np.asarray(logpdf_columns(fx, Y)), None, None, None))
                continue
            cols = [_fused(fx, Y[:, j], want_posterior=True) for j in range(Y.shape[1])]
            out.append((np.array([c[0] for c in cols]), np.stack([c[1] for c in cols], axis=1) if cols else None,
                        cols[0][2] if cols else None, cols[0][3] if cols else None))
        return out

    if any(isinstance(fx.f, BasisFunctionRegressor) and isinstance(fx.f.phi, RandomFourierFeatures) for fx in fxs):
        return loop()
    fbs = [_to_finite_blr(fx) for fx in fxs]
    dtype = np.float32 if all(_dtype_of(fb.f.mw, Y) == np.float32 for fb, Y in zip(fbs, Ys)) else np.float64
    probs = []
    for fb, Y in zip(fbs, Ys):
        X, layout, ldx, D, N = _x_layout(fb.x, dtype)
        if Y.shape[0] != N:
            raise ValueError("length(y) != size(fx.x.X, 2)")  # reference :74
        s, noise_kind = _noise(fb.Sy, N, dtype)
        Lw, prior_kind, ldl = _prior(fb.f.Lw, D, dtype)
        probs.append((X, layout, ldx, D, N, np.asfortranarray(Y, dtype=dtype), s, noise_kind, _mean_vector(fb.f.mw, D, dtype), Lw,
                      prior_kind, ldl, isinstance(fb.f.Lw, PDMat)))
    X0, layout, ldx, D, N, Y0, _, noise_kind, _, _, prior_kind, ldl, pdmat = probs[0]
    S = Y0.shape[1]
    sig = {(q[0].shape, q[0].flags.f_contiguous, q[1], q[3], q[4], q[5].shape[1], q[7], q[10], q[12]) for q in probs}
    if noise_kind == _abi.NOISE_DENSE or D == 0 or S == 0 or len(sig) != 1:
        return loop()
    nb = len(probs)
    Xb = np.stack([q[0].reshape(-1, order="A") for q in probs])
    Yb = np.stack([q[5].reshape(-1, order="F") for q in probs])  # N x S column-major per data set, ldY = N
    sb = np.stack([q[6] for q in probs])
    mwb = np.stack([q[8] for q in probs])
    Lb = np.stack([q[9].reshape(-1, order="A") for q in probs])
    lp = np.zeros((nb, S), dtype=np.float64)
    info = np.zeros(nb, dtype=np.int32)
    if want_posterior:
        means = np.empty((nb, D * S), dtype=dtype)
        Tb = np.empty((nb, D * D), dtype=dtype)
        Ab = np.empty((nb, D * D), dtype=dtype) if not pdmat else None
    else:
        means = Tb = Ab = None
    _handle().posterior_multi_batched(dtype, _abi.MEM_HOST, layout, nb, D, N, S, Xb, ldx, Xb.shape[1], Yb, max(N, 1), Yb.shape[1],
                                      noise_kind, sb, sb.shape[1], prior_kind, mwb, D, Lb, ldl, Lb.shape[1], means, D, D * S, Tb, D,
                                      D * D, Ab, D, D * D, lp, S, info)
    bad = np.flatnonzero(info > 0)
    if bad.size:
        e = _abi.PosDefException(int(info[bad[0]]))
        e.index = int(bad[0])
        raise e
    out = []
    for b in range(nb):
        if want_posterior:
            out.append((lp[b], means[b].reshape((D, S), order="F"), Tb[b].reshape((D, D), order="F"),
                        Ab[b].reshape((D, D), order="F") if Ab is not None else None))
        else:
            out.append((lp[b], None, None, None))
    return out


def _column_posteriors(fx, means, T, A):
    base = fx.f.blr if isinstance(fx.f, BasisFunctionRegressor) else fx.f
    Lw_post = _wrap_like(base.Lw, T, A)  # ONE precision object: the S posteriors of a data set share the factor
    posts = [BayesianLinearRegressor(means[:, j], Lw_post) for j in range(means.shape[1])]
    if isinstance(fx.f, BasisFunctionRegressor):
        return [BasisFunctionRegressor(p, fx.f.phi) for p in posts]
    return posts


def posterior_columns(fx, Y):
    """[posterior(fx, Y[:, s]) for s in range(S)] (reference :60-69 per column of a matrix target) in one library call: the S
    posterior regressors differ in their mean only and share one precision object."""
    return posterior_columns_map([fx], [Y])[0]


def logpdf_columns_map(fxs, Ys):
    """logpdf(fx, Y::AbstractMatrix) under a map over data sets (reference :55-58): a (B, S) array, from one library call when the
    problems have one shape (blr_posterior_multi_batched_*)."""
    res = _columns_many(fxs, Ys, want_posterior=False)
    if not res:
        return np.zeros((0, 0))
    if len({r[0].shape for r in res}) != 1:
        raise ValueError("the target matrices must have one number of columns for a (B, S) result")
    return np.stack([r[0] for r in res])


def posterior_columns_map(fxs, Ys):
    """Per data set the S posterior regressors of its target columns, sharing one factor (reference :60-69 under a map over fxs with
    matrix targets), from one library call when the problems have one shape."""
    fxs = list(fxs)
    out = []
    for fx, (_, means, T, A) in zip(fxs, _columns_many(fxs, Ys, want_posterior=True)):
        out.append([] if means is None else _column_posteriors(fx, means, T, A))
    return out


# ---------------------------------------------------------------------------------------------------
# predictions from the S column posteriors of a matrix target: one variance per input, S means (blr_marginals_multi_batched_*)
# ---------------------------------------------------------------------------------------------------
def _columns_problem(fs, x, Sy, want_var):
    """The S regressors of posterior_columns at the inputs x -> (dtype of the weights, operands); they must share one precision."""
    fs = list(fs)
    if not fs:
        raise ValueError("at least one column regressor is needed")
    blrs = [f.blr if isinstance(f, BasisFunctionRegressor) else f for f in fs]
    if any(not isinstance(b, BayesianLinearRegressor) for b in blrs):
        raise TypeError("expected BayesianLinearRegressor or BasisFunctionRegressor columns")
    if any(b.Lw is not blrs[0].Lw for b in blrs):
        raise ValueError("the columns must share one precision object")
    fb = _to_finite_blr(FiniteGP(fs[0], x, Sy))  # (the columns of posterior_columns share phi as they share the factor)
    return blrs, fb, _dtype_of(*[b.mw for b in blrs])


def _columns_operands(blrs, fb, dtype, want_var):
    X, layout, ldx, D, N = _x_layout(fb.x, dtype)
    M = np.asfortranarray(np.stack([_mean_vector(b.mw, D, dtype) for b in blrs], axis=1))  # D x S
    s, noise_kind = _noise(fb.Sy, N, dtype)  # var adds diag(Sigma_y) (:43)
    if noise_kind == _abi.NOISE_DENSE:
        s, noise_kind = np.ascontiguousarray(np.diag(s)), _abi.NOISE_DIAGONAL
    Lw, prior_kind, ldl = _prior(blrs[0].Lw, D, dtype, need_cholesky=want_var)  # :41 _cholesky(Lw)
    return X, layout, ldx, D, N, M, s, noise_kind, Lw, prior_kind, ldl


def _marginals_columns(fs, x, Sy, want_var):
    blrs, fb, dtype = _columns_problem(fs, x, Sy, want_var)
    X, layout, ldx, D, N, M, s, noise_kind, Lw, prior_kind, ldl = _columns_operands(blrs, fb, dtype, want_var)
    S = M.shape[1]
    m = np.empty((N, S), dtype=dtype, order="F")
    v = np.empty(N, dtype=dtype) if want_var else None
    info = np.zeros(1, dtype=np.int32)
    _handle().marginals_multi_batched(dtype, _abi.MEM_HOST, layout, 1, D, N, S, X, ldx, 0, noise_kind, s if want_var else None, 0,
                                      prior_kind, M, max(D, 1), 0, Lw if want_var else None, ldl, 0, m, max(N, 1), 0, v, N, info)
    if info[0] > 0:
        raise _abi.PosDefException(int(info[0]))
    return m, v


def mean_and_var_columns(fs, x, Sy=1e-18):
    """mean_and_var(f(x, Sy)) (reference :47) for the S regressors f of posterior_columns -- one precision object, S means -- in one
    library call: (mean N x S, var N).  The variance does not depend on the column."""
    return _marginals_columns(fs, x, Sy, True)


def mean_columns(fs, x):
    """mean(f(x)) (reference :33) for the S regressors of posterior_columns in one library call: N x S."""
    return _marginals_columns(fs, x, 1e-18, False)[0]


def mean_and_var_columns_map(fss, xs, Sy=1e-18):
    """[mean_and_var_columns(fs, x, Sy)] over data sets: one library call when all have the same (D, N, S, layout, noise kind, prior
    kind, dtype), else a loop.  Sy: one value for all, or a list with one per data set.  The first regressor (in order) whose prior
    is not positive definite raises PosDefException with its position as ``index``."""
    fss, xs = [list(fs) for fs in fss], list(xs)
    if len(fss) != len(xs):
        raise ValueError("as many input sets as lists of column regressors are needed")
    if not fss:
        return []
    Sys = list(Sy) if isinstance(Sy, (list, tuple)) else [Sy] * len(fss)
    if len(Sys) != len(fss):
        raise ValueError("as many noise covariances as lists of column regressors are needed")
    heads = [_columns_problem(fs, x, sy, True) for fs, x, sy in zip(fss, xs, Sys)]
    dtype = np.float32 if all(h[2] == np.float32 for h in heads) else np.float64
    probs = [_columns_operands(h[0], h[1], dtype, True) for h in heads]
    X0, layout, ldx, D, N, M0, _, noise_kind, _, prior_kind, ldl = probs[0]
    S = M0.shape[1]
    sig = {(q[0].shape, q[0].flags.f_contiguous, q[1], q[3], q[4], q[5].shape[1], q[7], q[9]) for q in probs}
    if len(sig) != 1 or D == 0 or N == 0:
        return [mean_and_var_columns(fs, x, sy) for fs, x, sy in zip(fss, xs, Sys)]
    nb = len(probs)
    Xb = np.stack([q[0].reshape(-1, order="A") for q in probs])
    Mb = np.stack([q[5].reshape(-1, order="F") for q in probs])  # D x S column-major per data set, ldm = D
    sb = np.stack([q[6] for q in probs])
    Lb = np.stack([q[8].reshape(-1, order="A") for q in probs])
    m = np.empty((nb, N * S), dtype=dtype)
    v = np.empty((nb, N), dtype=dtype)
    info = np.zeros(nb, dtype=np.int32)
    _handle().marginals_multi_batched(dtype, _abi.MEM_HOST, layout, nb, D, N, S, Xb, ldx, Xb.shape[1], noise_kind, sb, sb.shape[1],
                                      prior_kind, Mb, D, D * S, Lb, ldl, Lb.shape[1], m, N, N * S, v, N, info)
    bad = np.flatnonzero(info > 0)
    if bad.size:
        e = _abi.PosDefException(int(info[bad[0]]))
        e.index = int(bad[0])
        raise e
    return [(m[b].reshape((N, S), order="F"), v[b]) for b in range(nb)]


# ---------------------------------------------------------------------------------------------------
# exact held-out predictives for equal observation counts: one problem record, one fit-then-score pipeline, a row of
# _HELDOUT per variant (leave-one-out and K-fold; a vector target, or the S columns of a matrix target sharing their factor)
# ---------------------------------------------------------------------------------------------------
LOO = namedtuple("LOO", ["mean", "var", "logpdf", "total"])
LOO.__doc__ = """Exact leave-one-out predictives: per observation n the predictive of y_n given all the other data (mean and var,
var including the noise as var(fx) does, in the element type; logpdf in float64) and total = sum_n logpdf_n (the LOO-CV
score).  An observation whose leverage is within rounding of 1 has NaN entries (blr_get_stat "loo_degenerate")."""

KFold = namedtuple("KFold", ["mean", "var", "logpdf", "total"])
KFold.__doc__ = """Exact leave-fold-out (K-fold) predictives for contiguous folds of ``fold_size`` observations: per observation n the
predictive of y_n given all the other FOLDS (mean and var, var including the noise, in the element type), per fold the JOINT log
density of its observations given the rest (logpdf, float64, ceil(N / fold_size) entries) and total = sum_f logpdf_f (the K-fold CV
score).  A fold the state does not contain (a pivot of I - H~ <= 0) has NaN entries (blr_get_stat "kfold_degenerate")."""


class _HeldoutProblem(namedtuple("_HeldoutProblem", "X layout ldx D N target s noise_kind mw Lw prior_kind ldl pdmat")):
    """One finite regressor with its targets, validated as `_fused` does; ``target``: y [N], or Y [N x S] column-major; ``pdmat``:
    the prior precision is carried by its factor."""
    __slots__ = ()

    @property
    def S(self):
        return self.target.shape[1] if self.target.ndim == 2 else None

    @property
    def signature(self):
        """what problems must share to go through the library in one batch"""
        return (self.X.shape, self.X.flags.f_contiguous, self.layout, self.D, self.N, self.S, self.noise_kind, self.prior_kind, self.pdmat)


def _heldout_problem(fx, target, dtype, what, rank, perm=None):
    """The record of fx with a vector (``rank`` 1) or N x S matrix (2) of targets.  ``perm`` (K-fold): observation n of the problem
    is observation perm[n] of the caller's -- X, the targets and a noise diagonal gathered here."""
    fb = _to_finite_blr(fx)
    X, layout, ldx, D, N = _x_layout(fb.x, dtype)
    packed = np.ascontiguousarray if rank == 1 else np.asfortranarray
    target = packed(target, dtype=dtype)
    if target.ndim != rank:
        raise ValueError("y must be a vector" if rank == 1 else "Y must be an N x S matrix")
    if target.shape[0] != N:
        raise ValueError("length(y) != size(fx.x.X, 2)")  # reference :74
    s, noise_kind = _noise(fb.Sy, N, dtype)
    if noise_kind == _abi.NOISE_DENSE:
        raise NotImplementedError(f"{what}: with a dense noise covariance one observation is not independent of the rest (that is a "
                                  "block leave-out); isotropic or diagonal noise only")
    if perm is not None:
        obs_axis = 0 if isinstance(fb.x, RowVecs) else 1
        X = np.asarray(np.take(X, perm, axis=obs_axis), order="F" if X.flags.f_contiguous else "C")
        target = packed(target[perm])
        if noise_kind == _abi.NOISE_DIAGONAL:
            s = np.ascontiguousarray(s[perm])
    Lw, prior_kind, ldl = _prior(fb.f.Lw, D, dtype)
    return _HeldoutProblem(X, layout, ldx, D, N, target, s, noise_kind, _mean_vector(fb.f.mw, D, dtype), Lw, prior_kind, ldl,
                           isinstance(fb.f.Lw, PDMat))


# A variant: the entry point that fits the device state and the arguments that follow the prior in its list, the entry point that
# scores it (``folds``: it takes a fold size) and the arguments that follow the data in its list, the rank of the targets and the
# record.  st: the means of the state (mw', or M with S columns), nl: log densities per column (N, or the number of folds).
_Heldout = namedtuple("_Heldout", ["fit", "fit_tail", "score", "score_tail", "folds", "rank", "record"])
_VECTOR = dict(
    rank=1, fit="posterior_batched",
    fit_tail=lambda D, S, st, T, info: (st, D, T, max(D, 1), D * D, None, max(D, 1), D * D, None, info),
    score_tail=lambda D, N, S, nl, st, stride_st, T, strideT, m, v, ll, tot, info: (
        st, stride_st, T, max(D, 1), strideT, m, N, v, N, ll, nl, tot, info))
_COLUMNS = dict(
    rank=2, fit="posterior_multi_batched",
    fit_tail=lambda D, S, st, T, info: (st, D, D * S, T, D, D * D, None, D, D * D, None, S, info),
    score_tail=lambda D, N, S, nl, st, stride_st, T, strideT, m, v, ll, tot, info: (
        st, max(D, 1), stride_st, T, max(D, 1), strideT, m, max(N, 1), N * S, v, N, ll, max(nl, 1), nl * S, tot, S, info))
_HELDOUT = {
    "loo": _Heldout(score="loo", folds=False, record=LOO, **_VECTOR),
    "kfold": _Heldout(score="kfold", folds=True, record=KFold, **_VECTOR),
    "kfold_large": _Heldout(score="kfold_large", folds=True, record=KFold, **_VECTOR),
    "loo_columns": _Heldout(score="loo_multi_batched", folds=False, record=LOO, **_COLUMNS),
    "kfold_columns": _Heldout(score="kfold_multi_batched", folds=True, record=KFold, **_COLUMNS),
}


def _heldout_operands(row, dtype, layout, B, D, N, S, dX, ldx, strideX, d_target, stride_target, noise_kind, ds, strides):
    """-> (head, data): the arguments every entry point of ``row`` starts with, and those that describe the staged data"""
    columns = row.rank == 2
    return ((dtype, _abi.MEM_DEVICE, layout, B, D, N) + ((S,) if columns else ()),
            (dX, ldx, strideX, d_target) + ((max(N, 1),) if columns else ()) + (stride_target, noise_kind, ds, strides))


def _heldout_call(scope, row, head, F, data, st, stride_st, T, strideT):
    """The scoring entry point of ``row`` on device operands -> (mean [B, N] or [B, N, S], var [B, N], logpdf [B, nl] or [B, nl, S],
    total [B] or [B, S], info [B]) on the host; the state (st, T) may be resident (B = 1, strides 0)."""
    h, dtype, B, D, N = scope.h, head[0], head[3], head[4], head[5]
    S = head[6] if row.rank == 2 else 1
    nl = -(-N // F) if row.folds else N
    m, v = np.empty((B, N * S), dtype=dtype), np.empty((B, N), dtype=dtype)
    lp, tot = np.empty((B, nl * S), dtype=np.float64), np.empty((B, S) if row.rank == 2 else B, dtype=np.float64)
    info = np.zeros(B, dtype=np.int32)
    d_m, d_v, d_ll, d_tot = (scope.alloc(a.nbytes) for a in (m, v, lp, tot))
    d_info = scope.dev(info)
    getattr(h, row.score)(*head, *((F,) if row.folds else ()), *data,
                          *row.score_tail(D, N, S, nl, st, stride_st, T, strideT, d_m, d_v, d_ll, d_tot, d_info))
    for host, dptr in ((m, d_m), (v, d_v), (lp, d_ll), (tot, d_tot), (info, d_info)):
        h.memcpy_d2h(host, dptr)
    if row.rank == 2:  # (column-major per regressor)
        m, lp = m.reshape((B, S, N)).transpose(0, 2, 1), lp.reshape((B, S, nl)).transpose(0, 2, 1)
    return m, v, lp, tot, info


def _heldout_records(row, m, v, lp, tot):
    return [row.record(m[b], v[b], lp[b], float(tot[b]) if row.rank == 1 else tot[b]) for b in range(len(v))]


def _heldout_empty(row, dtype, N, S, F):
    """what a matrix target with no weights, no observations or no columns gets without a call"""
    return row.record(np.empty((N, S), dtype=dtype), np.empty(N, dtype=dtype), np.empty((-(-N // F) if row.folds else N, S)), np.zeros(S))


def _heldout_batch(probs, dtype, row, F=None):
    """Held-out predictives of equally shaped problems: their data staged once, the fit of ``row`` into device buffers (mw', T) or
    (M, T) -- any prior kind, the usual routes -- then its scoring entry point on the same device inputs.  Nothing D x D comes back
    to the host.  The first problem that fails either call raises PosDefException with its position as ``index``."""
    q = probs[0]
    D, N, S, nb, item = q.D, q.N, q.S, len(probs), np.dtype(dtype).itemsize
    if row.rank == 2 and (D == 0 or N == 0 or S == 0):
        return [_heldout_empty(row, dtype, N, S, F) for _ in probs]
    h = _handle()
    Xb = np.stack([p.X.reshape(-1, order="A") for p in probs])
    tb = np.stack([p.target.reshape(-1, order="F") for p in probs])  # (N x S column-major per data set, ldY = N)
    sb = np.stack([p.s for p in probs])
    mwb = np.stack([p.mw for p in probs])
    Lb = np.stack([p.Lw.reshape(-1, order="A") for p in probs])
    with _DeviceScope(h) as scope:
        head, data = _heldout_operands(row, dtype, q.layout, nb, D, N, S, scope.dev(Xb), q.ldx, Xb.shape[1], scope.dev(tb), tb.shape[1],
                                       q.noise_kind, scope.dev(sb), sb.shape[1])
        d_st, d_T = scope.alloc(nb * D * (S or 1) * item), scope.alloc(nb * D * D * item)
        info = np.zeros(nb, dtype=np.int32)
        d_info = scope.dev(info)
        getattr(h, row.fit)(*head, *data, q.prior_kind, scope.dev(mwb), D, scope.dev(Lb), q.ldl, Lb.shape[1],
                            *row.fit_tail(D, S, d_st, d_T, d_info))
        h.memcpy_d2h(info, d_info)
        if not np.any(info):
            m, v, lp, tot, info = _heldout_call(scope, row, head, F, data, d_st, D * (S or 1), d_T, D * D)
    _raise_first_failed(info)
    return _heldout_records(row, m, v, lp, tot)


def _heldout_dtype(fx, target):
    return _dtype_of(fx.f.blr.mw if isinstance(fx.f, BasisFunctionRegressor) else fx.f.mw, target)


def _perm_of(perm, target, rank=1):
    if perm is None:
        return None
    perm = np.asarray(perm, dtype=np.int64)
    n = np.asarray(target).shape[0] if np.ndim(target) == rank else -1
    if perm.shape != (n,) or not np.array_equal(np.sort(perm), np.arange(n)):
        raise ValueError("perm must be a permutation of range(N)")
    return perm


def _heldout_one(fx, target, row, what, F=None, perm=None, check=None):
    """One problem through `_heldout_batch`; ``check(problem)`` runs before anything is staged.  With ``perm``, mean and var are
    scattered back to the caller's order; logpdf stays in fold order."""
    dtype = _heldout_dtype(fx, target)
    perm = _perm_of(perm, target, row.rank)
    q = _heldout_problem(fx, target, dtype, what, row.rank, perm)
    if check is not None:
        check(q)
    r = _heldout_batch([q], dtype, row, F)[0]
    if perm is None:
        return r
    m, v = np.empty_like(r.mean), np.empty_like(r.var)
    m[perm], v[perm] = r.mean, r.var
    return r._replace(mean=m, var=v)


def _heldout_map(fxs, targets, row, what, F=None, check=None):
    """The problems in one fit and one scoring call when they are equally shaped, else one pair of calls per problem (a
    RandomFourierFeatures basis, an empty dimension: always).  ``check(problem)`` runs for every problem before anything is staged."""
    fxs, targets = list(fxs), list(targets)
    if len(fxs) != len(targets):
        raise ValueError(f"as many {'observation vectors' if row.rank == 1 else 'target matrices'} as finite regressors are needed")
    if not fxs:
        return []
    dtype = np.float32 if all(_heldout_dtype(fx, t) == np.float32 for fx, t in zip(fxs, targets)) else np.float64
    probs = [_heldout_problem(fx, t, dtype, what, row.rank) for fx, t in zip(fxs, targets)]
    for q in probs if check is not None else ():
        check(q)
    rff = any(isinstance(fx.f, BasisFunctionRegressor) and isinstance(fx.f.phi, RandomFourierFeatures) for fx in fxs)
    if not rff and len({q.signature for q in probs}) == 1 and 0 not in (probs[0].D, probs[0].N, probs[0].S):
        return _heldout_batch(probs, dtype, row, F)
    out = []
    for i, q in enumerate(probs):
        try:
            out.append(_heldout_batch([q], dtype, row, F)[0])
        except _abi.PosDefException as e:
            e.index = i
            raise
    return out


def _fold_size(fold_size):
    F = int(fold_size)
    if F != fold_size or not 1 <= F <= 64:
        raise ValueError("fold_size must be an integer in 1..64")
    return F


_KFOLD_LARGE_MAX_D = 128      # blr_kfold_large_batched_*: the fold's D x D factorisation lives in LDS
_KFOLD_LARGE_MAX_FOLDS = 1024  # ... and the route is for few, large folds
_KFOLD_COLUMNS_MAX_D = 128    # blr_kfold_multi_batched_*: the fold's rows of Z live in LDS, there is no slow route


def _fold_size_large(fold_size):
    F = int(fold_size)
    if F != fold_size or F < 1:
        raise ValueError("fold_size must be an integer >= 1")
    return F


def _kfold_large_check(D, N, F, what):
    """The limits of blr_kfold_large_batched_* that depend on the problem, with Python's exceptions instead of argument errors."""
    if D > _KFOLD_LARGE_MAX_D:
        raise NotImplementedError(f"{what}: D = {D} is beyond the limit of blr_kfold_large_batched_* (D <= {_KFOLD_LARGE_MAX_D})")
    if -(-N // F) > _KFOLD_LARGE_MAX_FOLDS:
        raise ValueError(f"{what}: ceil(N / fold_size) = {-(-N // F)} folds; at most {_KFOLD_LARGE_MAX_FOLDS} (many small folds: kfold)")


def _kfold_columns_check(D, what):
    if D > _KFOLD_COLUMNS_MAX_D:
        raise ValueError(f"{what}: D = {D} is beyond the limit of blr_kfold_multi_batched_* (D <= {_KFOLD_COLUMNS_MAX_D})")


def loo(fx, y):
    """Exact leave-one-out predictives of the observations y at fx.x (include/blr_mi355x.h blr_loo_batched_*): for every n the
    predictive of y_n under posterior(fx without observation n) -- what a loop of forget / condition gives, from one marginal
    pass over the inputs.  Returns LOO(mean, var, logpdf, total).  Dense noise raises NotImplementedError (a block LOO)."""
    return _heldout_one(fx, y, _HELDOUT["loo"], "loo")


def loo_map(fxs, ys):
    """[loo(fx, y) for fx, y in zip(fxs, ys)] in one posterior call and one LOO call for equally shaped problems (else one call
    per problem, as `posterior_map`).  The first problem whose prior, noise or posterior is not positive definite raises
    PosDefException with its position as ``index``.  Problems with UNEQUAL observation counts whose data is already packed side
    by side go through `loo_ragged` in two library calls."""
    return _heldout_map(fxs, ys, _HELDOUT["loo"], "loo")


def kfold(fx, y, fold_size, perm=None):
    """Exact leave-fold-out (K-fold) predictives of the observations y at fx.x (include/blr_mi355x.h blr_kfold_batched_*): fold f
    holds the observations [f fold_size, (f + 1) fold_size), and every observation gets its predictive under posterior(fx without
    its fold) -- what a loop of forget / predict / condition per fold gives, from one call.  1 <= fold_size <= 64; at 1 this is
    `loo`.  ``perm``, a permutation of range(N), makes the folds random: fold f then holds the observations perm[f fold_size :
    (f + 1) fold_size]; mean and var come back in the caller's order, logpdf stays in fold order.  Returns KFold(mean, var, logpdf,
    total).  Dense noise raises NotImplementedError (it couples the folds)."""
    return _heldout_one(fx, y, _HELDOUT["kfold"], "kfold", _fold_size(fold_size), perm)


def kfold_map(fxs, ys, fold_size):
    """[kfold(fx, y, fold_size) for fx, y in zip(fxs, ys)] in one posterior call and one K-fold call for equally shaped problems
    (else one call per problem, as `loo_map`).  The first problem whose prior, noise or posterior is not positive definite raises
    PosDefException with its position as ``index``."""
    return _heldout_map(fxs, ys, _HELDOUT["kfold"], "kfold", _fold_size(fold_size))


def kfold_large(fx, y, fold_size, perm=None):
    """`kfold` for LARGE folds (include/blr_mi355x.h blr_kfold_large_batched_*): any integer fold_size >= 1 with
    ceil(N / fold_size) <= 1024 -- the K = 5 or 10 folds of N / K observations of ordinary cross-validation.  The fold is removed in
    weight space (one D x D factorisation per fold), so D <= 128 (NotImplementedError beyond) and a fold that carries nearly all of the
    state's information loses digits (float32 first).  ``perm`` and the KFold record as for `kfold`; fold_size > N is one fold, the
    predictive under the prior."""
    F = _fold_size_large(fold_size)
    return _heldout_one(fx, y, _HELDOUT["kfold_large"], "kfold_large", F, perm, lambda q: _kfold_large_check(q.D, q.N, F, "kfold_large"))


def kfold_large_map(fxs, ys, fold_size):
    """[kfold_large(fx, y, fold_size) for fx, y in zip(fxs, ys)] in one posterior call and one blr_kfold_large_batched_* call for
    equally shaped problems (else one call per problem, as `kfold_map`).  The first problem whose prior, noise or posterior is not
    positive definite raises PosDefException with its position as ``index``."""
    F = _fold_size_large(fold_size)
    return _heldout_map(fxs, ys, _HELDOUT["kfold_large"], "kfold_large", F, lambda q: _kfold_large_check(q.D, q.N, F, "kfold_large_map"))


def cross_validate(fx, y, n_folds, perm=None):
    """K-fold cross-validation with ``n_folds`` contiguous folds of F = ceil(N / n_folds) observations (random folds with ``perm``):
    `kfold` when F <= 64, else `kfold_large`.  Returns KFold(mean, var, logpdf, total); total is the CV score."""
    K = int(n_folds)
    if K != n_folds or K < 1:
        raise ValueError("n_folds must be an integer >= 1")
    N = np.asarray(y).shape[0] if np.ndim(y) == 1 else 0
    F = max(1, -(-N // K))
    return kfold(fx, y, F, perm) if F <= 64 else kfold_large(fx, y, F, perm)


def loo_columns(fx, Y):
    """Exact leave-one-out predictives of a matrix target (include/blr_mi355x.h blr_loo_multi_batched_*): for every observation n and
    column c the predictive of Y[n, c] under posterior(fx without observation n, Y[:, c]) -- `loo(fx, Y[:, c])` for every c, with the
    leverage of an input computed once.  Returns LOO(mean N x S, var N -- it does not depend on the column --, logpdf N x S, total S).
    Dense noise raises NotImplementedError (a block LOO)."""
    return loo_columns_map([fx], [Y])[0]


def loo_columns_map(fxs, Ys):
    """[loo_columns(fx, Y) for fx, Y in zip(fxs, Ys)] in one posterior call and one LOO call for equally shaped problems (else one
    pair of calls per problem).  The first problem whose prior, noise or posterior is not positive definite raises PosDefException
    with its position as ``index``."""
    return _heldout_map(fxs, [np.asarray(Y) for Y in Ys], _HELDOUT["loo_columns"], "loo_columns")


def kfold_columns(fx, Y, fold_size, perm=None):
    """Exact leave-fold-out (K-fold) predictives of a matrix target (include/blr_mi355x.h blr_kfold_multi_batched_*): for every
    column c what `kfold(fx, Y[:, c], fold_size)` gives, with X read once and every fold's hat block factored once for its S columns.
    1 <= fold_size <= 64 and D <= 128 (ValueError beyond).  ``perm`` as for `kfold`: fold f holds the observations
    perm[f fold_size : (f + 1) fold_size]; mean and var come back in the caller's order, logpdf stays in fold order.  Returns
    KFold(mean N x S, var N -- it does not depend on the column --, logpdf nfolds x S, total S).  Dense noise raises
    NotImplementedError (it couples the folds)."""
    F = _fold_size(fold_size)
    return _heldout_one(fx, np.asarray(Y), _HELDOUT["kfold_columns"], "kfold_columns", F, perm, lambda q: _kfold_columns_check(q.D, "kfold_columns"))


def kfold_columns_map(fxs, Ys, fold_size):
    """[kfold_columns(fx, Y, fold_size) for fx, Y in zip(fxs, Ys)] in one posterior call and one K-fold call for equally shaped
    problems (else one pair of calls per problem).  The first problem whose prior, noise or posterior is not positive definite raises
    PosDefException with its position as ``index``."""
    F = _fold_size(fold_size)
    return _heldout_map(fxs, [np.asarray(Y) for Y in Ys], _HELDOUT["kfold_columns"], "kfold_columns_map", F,
                        lambda q: _kfold_columns_check(q.D, "kfold_columns_map"))


EvidenceGrid = namedtuple("EvidenceGrid", ["logpdf", "best", "alpha", "tau"])
EvidenceGrid.__doc__ = """Evidence of one data set under every (prior scale alpha_i, noise scale tau_j): logpdf[i, j] is
logpdf(BayesianLinearRegressor(mw, alpha_i Lw)(x, tau_j Sy), y) (NaN where that setting is not positive definite), best the
(i, j) of the largest finite one (None when no setting succeeded), alpha and tau the two scale vectors."""


def _grid_problem(fx, y, dtype):
    """Operands of one finite regressor for blr_logpdf_grid_*, validated as `_fused` does.  A PDMat prior is passed as U'U formed
    on the host (a small D x D product): the entry scales a precision, not a carried-forward factor."""
    fb = _to_finite_blr(fx)
    X, layout, ldx, D, N = _x_layout(fb.x, dtype)
    y = np.ascontiguousarray(y, dtype=dtype)
    if y.ndim != 1:
        raise ValueError("y must be a vector")
    if y.shape[0] != N:
        raise ValueError("length(y) != size(fx.x.X, 2)")  # reference :74
    s, noise_kind = _noise(fb.Sy, N, dtype)
    if noise_kind == _abi.NOISE_DENSE:
        raise ValueError("logpdf_grid: isotropic or diagonal noise only (a dense noise covariance is not supported by "
                         "blr_logpdf_grid_*)")
    Lw = fb.f.Lw
    if isinstance(Lw, PDMat):
        U = np.triu(np.asarray(Lw.U, dtype=np.float64))
        Lw = U.T @ U
    Lw, prior_kind, ldl = _prior(Lw, D, dtype)
    return X, layout, ldx, D, N, y, s, noise_kind, _mean_vector(fb.f.mw, D, dtype), Lw, prior_kind, ldl


def _grid_scales(prior_scales, noise_scales, dtype):
    a = np.atleast_1d(np.asarray([1.0] if prior_scales is None else prior_scales, dtype=dtype))
    t = np.atleast_1d(np.asarray([1.0] if noise_scales is None else noise_scales, dtype=dtype))
    if a.ndim != 1 or t.ndim != 1 or a.size == 0 or t.size == 0:
        raise ValueError("prior_scales and noise_scales must be non-empty vectors")
    return a, t


def _grid_batch(probs, a, t, dtype, want_posterior):
    """blr_logpdf_grid_* over equally shaped problems: the outer product of the scales flattened to G settings, prior scale
    slowest.  -> [(EvidenceGrid, mw_best, T_best)]"""
    X0, layout, ldx, D, N, _, _, noise_kind, _, _, prior_kind, ldl = probs[0]
    nb, G = len(probs), a.size * t.size
    Xb = np.stack([q[0].reshape(-1, order="A") for q in probs])
    yb = np.stack([q[5] for q in probs])
    sb = np.stack([q[6] for q in probs])
    mwb = np.stack([q[8] for q in probs])
    Lb = np.stack([q[9].reshape(-1, order="A") for q in probs])
    alpha = np.ascontiguousarray(np.repeat(a, t.size))
    tau = np.ascontiguousarray(np.tile(t, a.size))
    lp = np.full((nb, G), np.nan, dtype=np.float64)
    info = np.zeros((nb, G), dtype=np.int32)
    best = np.full(nb, -1, dtype=np.int64)
    mw_best = np.empty((nb, D), dtype=dtype) if want_posterior else None
    T_best = np.empty((nb, D * D), dtype=dtype) if want_posterior else None
    _handle().logpdf_grid(dtype, _abi.MEM_HOST, layout, nb, D, N, Xb, ldx, Xb.shape[1], yb, yb.shape[1], noise_kind, sb,
                          sb.shape[1], prior_kind, mwb, D, Lb, ldl, Lb.shape[1], G, alpha, 0, tau, 0, lp, G, best, mw_best, D,
                          T_best, max(D, 1), D * D, info, G)
    out = []
    for b in range(nb):
        k = int(best[b])
        grid = EvidenceGrid(lp[b].reshape(a.size, t.size), divmod(k, t.size) if k >= 0 else None, a, t)
        if want_posterior and k < 0:
            e = _abi.PosDefException(int(info[b][0]))  # no setting is positive definite: the first setting's status, as a loop would raise
            e.index = b
            raise e
        out.append((grid, mw_best[b] if want_posterior else None,
                    T_best[b].reshape((D, D), order="F") if want_posterior else None))
    return out


def _grid_dtype(fx, y):
    return _dtype_of(fx.f.blr.mw if isinstance(fx.f, BasisFunctionRegressor) else fx.f.mw, y)


def logpdf_grid(fx, y, prior_scales=None, noise_scales=None):
    """Evidence of (fx, y) under every setting Lw -> alpha Lw, Sy -> tau Sy of the two scale vectors, from ONE pass over the
    inputs (include/blr_mi355x.h blr_logpdf_grid_*): the inner loop of type-II maximum likelihood.  ``None`` means [1.0].
    Returns EvidenceGrid(logpdf [len(prior_scales), len(noise_scales)], best (i, j), alpha, tau)."""
    dtype = _grid_dtype(fx, y)
    a, t = _grid_scales(prior_scales, noise_scales, dtype)
    return _grid_batch([_grid_problem(fx, y, dtype)], a, t, dtype, False)[0][0]


def posterior_best(fx, y, prior_scales=None, noise_scales=None):
    """(posterior at the evidence-maximising setting, EvidenceGrid) in the same library call; the posterior is wrapped like
    `posterior` wraps it (PDMat prior -> PDMat, else Symmetric).  Raises PosDefException when no setting succeeded."""
    dtype = _grid_dtype(fx, y)
    a, t = _grid_scales(prior_scales, noise_scales, dtype)
    grid, mw_best, T = _grid_batch([_grid_problem(fx, y, dtype)], a, t, dtype, True)[0]
    base = fx.f.blr if isinstance(fx.f, BasisFunctionRegressor) else fx.f
    Tu = np.triu(T)
    post = BayesianLinearRegressor(mw_best, _wrap_like(base.Lw, Tu, None if isinstance(base.Lw, PDMat) else Tu.T @ Tu))
    if isinstance(fx.f, BasisFunctionRegressor):
        post = BasisFunctionRegressor(post, fx.f.phi)
    return post, grid


def _grid_ragged_call(dtype, layout, nb, D, offsets, X, ldx, y, noise_kind, s, strides, prior_kind, mwb, stridemw, Lb, ldl, strideLw,
                      a, t, want_posterior):
    """blr_logpdf_grid_ragged_* on packed operands: the outer product of the scales flattened to G settings, prior scale slowest,
    one grid shared by all regressors.  -> [(EvidenceGrid, mw_best, T_best)]; ``want_posterior``: the first regressor without a
    winner raises PosDefException with its position as ``index``, as _grid_batch does."""
    G = a.size * t.size
    alpha = np.ascontiguousarray(np.repeat(a, t.size))
    tau = np.ascontiguousarray(np.tile(t, a.size))
    lp = np.full((nb, G), np.nan, dtype=np.float64)
    info = np.zeros((nb, G), dtype=np.int32)
    best = np.full(nb, -1, dtype=np.int64)
    mw_best = np.empty((nb, D), dtype=dtype) if want_posterior else None
    T_best = np.empty((nb, D * D), dtype=dtype) if want_posterior else None
    _handle().logpdf_grid_ragged(dtype, _abi.MEM_HOST, layout, nb, D, offsets, X, ldx, y, noise_kind, s, strides, prior_kind, mwb,
                                 stridemw, Lb, ldl, strideLw, G, alpha, 0, tau, 0, lp, G, best, mw_best, D, T_best, max(D, 1), D * D,
                                 info, G)
    out = []
    for b in range(nb):
        k = int(best[b])
        grid = EvidenceGrid(lp[b].reshape(a.size, t.size), divmod(k, t.size) if k >= 0 else None, a, t)
        if want_posterior and k < 0:
            e = _abi.PosDefException(int(info[b][0]))  # no setting is positive definite: the first setting's status, as a loop would raise
            e.index = b
            raise e
        out.append((grid, mw_best[b] if want_posterior else None,
                    T_best[b].reshape((D, D), order="F") if want_posterior else None))
    return out


def _grid_ragged(f, x, offsets, Sy, y, prior_scales, noise_scales, want_posterior):
    """The packed form behind logpdf_grid_ragged / posterior_best_ragged -> ([(EvidenceGrid, mw_best, T_best)], the B priors).  A
    PDMat prior goes in as U'U formed on the host, as _grid_problem passes it: the entry scales a precision, not a factor."""
    def as_precision(g):
        if isinstance(g, BayesianLinearRegressor) and isinstance(g.Lw, PDMat):
            U = np.triu(np.asarray(g.Lw.U, dtype=np.float64))
            return BayesianLinearRegressor(g.mw, U.T @ U)
        return g

    if y is None:
        raise ValueError("y must be a vector")
    shared = isinstance(f, BayesianLinearRegressor)
    fs_in = f if shared else list(f)
    ops, fs = _ragged_operands(as_precision(fs_in) if shared else [as_precision(g) for g in fs_in], x, offsets, Sy, y)
    fs = [fs_in] * len(fs) if shared else fs_in
    if ops is None:
        return [], fs
    dtype, offsets, nb, X, layout, ldx, D, y, s, noise_kind, strides, prior_kind, ldl, _, mwb, stridemw, Lb, strideLw = ops
    a, t = _grid_scales(prior_scales, noise_scales, dtype)
    return _grid_ragged_call(dtype, layout, nb, D, offsets, X, ldx, y, noise_kind, s, strides, prior_kind, mwb, stridemw, Lb, ldl,
                             strideLw, a, t, want_posterior), fs


def logpdf_grid_ragged(f, x, offsets, Sy, y, prior_scales=None, noise_scales=None):
    """[logpdf_grid(f_b(x[offsets[b]:offsets[b+1]], Sy_b), y[...], prior_scales, noise_scales)] from packed arrays in ONE library
    call (include/blr_mi355x.h blr_logpdf_grid_ragged_*; reference :55-58 per setting under a map over fxs of different lengths):
    a list of EvidenceGrid.  ``f``, ``x``, ``offsets``, ``Sy``, ``y`` as logpdf_ragged takes them (no dense noise)."""
    return [r[0] for r in _grid_ragged(f, x, offsets, Sy, y, prior_scales, noise_scales, False)[0]]


def posterior_best_ragged(f, x, offsets, Sy, y, prior_scales=None, noise_scales=None):
    """([posterior at the evidence-maximising setting], [EvidenceGrid]) per packed regressor, in the same library call; the
    posteriors are wrapped as `posterior_best` wraps them.  The first regressor none of whose settings succeeded raises
    PosDefException with its position as ``index``."""
    res, fs = _grid_ragged(f, x, offsets, Sy, y, prior_scales, noise_scales, True)
    posts = []
    for g, (_, mw_best, T) in zip(fs, res):
        Tu = np.triu(T)
        posts.append(BayesianLinearRegressor(mw_best, _wrap_like(g.Lw, Tu, None if isinstance(g.Lw, PDMat) else Tu.T @ Tu)))
    return posts, [r[0] for r in res]


def logpdf_grid_map(fxs, ys, prior_scales=None, noise_scales=None):
    """[logpdf_grid(fx, y, prior_scales, noise_scales) for fx, y in zip(fxs, ys)] in one library call for equally shaped
    problems (the B axis of blr_logpdf_grid_*), and in one call of blr_logpdf_grid_ragged_* for problems that differ only in
    their observation counts (a problem without observations goes with any layout); one call per problem when layouts, D or
    kinds differ."""
    fxs, ys = list(fxs), list(ys)
    if len(fxs) != len(ys):
        raise ValueError("as many observation vectors as finite regressors are needed")
    if not fxs:
        return []
    dtype = np.float32 if all(_grid_dtype(fx, y) == np.float32 for fx, y in zip(fxs, ys)) else np.float64
    a, t = _grid_scales(prior_scales, noise_scales, dtype)
    probs = [_grid_problem(fx, y, dtype) for fx, y in zip(fxs, ys)]
    sig = {(q[0].shape, q[0].flags.f_contiguous, q[1], q[3], q[4], q[7], q[10]) for q in probs}
    if len(sig) != 1:
        # Problems that differ only in N go side by side into ONE call of blr_logpdf_grid_ragged_*.  An empty problem has no element
        # whose order could matter -- its (0, D) or (D, 0) array is C- and F-contiguous at once, so _x_layout's answer for it is
        # arbitrary -- and takes the layout of the others.  (The contiguity flag of `sig` is not part of this key: with the layout
        # flag it only says which way the container was written, and the flat reshape(order="A") below reads either way.)
        full = [q for q in probs if q[4] > 0] or probs
        _, layout, _, D, _, _, _, noise_kind, _, _, prior_kind, ldl = full[0]
        if len({(q[1], q[3], q[7], q[10]) for q in full}) != 1 or len({(q[3], q[7], q[10]) for q in probs}) != 1:
            return [_grid_batch([q], a, t, dtype, False)[0][0] for q in probs]
        # the observations side by side, as _fused_many packs them for blr_posterior_ragged_*
        offsets = np.concatenate(([0], np.cumsum([q[4] for q in probs]))).astype(np.int64)
        if layout == _abi.LAYOUT_COLVECS:
            Xp, ldxp = np.concatenate([q[0].reshape(-1, order="A") for q in probs]), D
        else:
            Xp = np.asfortranarray(np.concatenate([q[0].reshape(-1, order="A").reshape((q[4], D), order="F") for q in probs]))
            ldxp = max(int(offsets[-1]), 1)
        yp = np.concatenate([q[5] for q in probs])
        sp = np.concatenate([q[6] for q in probs])  # isotropic: one variance per problem (strides = 1); diagonal: packed like y
        mwb = np.stack([q[8] for q in probs])
        Lb = np.stack([q[9].reshape(-1, order="A") for q in probs])
        return [r[0] for r in _grid_ragged_call(dtype, layout, len(probs), D, offsets, Xp, ldxp, yp, noise_kind, sp, 1, prior_kind, mwb, D,
                                                Lb, ldl, Lb.shape[1], a, t, False)]
    return [r[0] for r in _grid_batch(probs, a, t, dtype, False)]


class _DeviceBuffer:
    """device memory owned through the C ABI (blr_device_alloc): no GPU array library involved"""

    def __init__(self, handle, nbytes):
        self.handle, self.nbytes = handle, int(nbytes)
        self.ptr = handle.device_alloc(self.nbytes)

    @classmethod
    def of(cls, handle, host_array):
        buf = cls(handle, host_array.nbytes)
        handle.memcpy_h2d(buf.ptr, host_array)
        return buf

    def free(self):
        if self.ptr:
            try:
                self.handle.device_free(self.ptr)
            finally:
                self.ptr = 0

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class _DeviceScope:
    """The device temporaries of one call: ``dev(host_array)`` uploads and ``alloc(nbytes)`` reserves, both -> device pointer;
    leaving the ``with`` block frees them all, whichever way it is left."""

    def __init__(self, handle):
        self.h, self._temps = handle, []

    def alloc(self, nbytes):
        self._temps.append(_DeviceBuffer(self.h, nbytes))
        return self._temps[-1].ptr

    def dev(self, host_array):
        self._temps.append(_DeviceBuffer.of(self.h, host_array))
        return self._temps[-1].ptr

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for b in self._temps:
            b.free()


class ResidentPosterior:
    """A posterior kept ON THE DEVICE as its state (mw, T) -- T the upper factor of the precision -- and conditioned IN PLACE
    on further batches: the "repeated conditioning" pattern of reference test/bayesian_linear_regression.jl:49-70
    (``posterior(f'1(X2, S2), y2)``) without re-deriving reference :72-89 from a D x D precision every time
    (blr_update_factor_*: O(k D^2) Givens sweeps for single observations, in-place re-factorisation otherwise).

        st = ResidentPosterior(posterior(f(X1, S1), y1))      # or a prior: ResidentPosterior(f)
        lp2 = st.condition(X2, S2, y2)                         # log p(y2 | y1); state now = posterior given y1 and y2
        f12 = st.regressor()                                   # BayesianLinearRegressor(mw, PDMat(T))

    `forget` is the inverse of `condition` (blr_downdate_factor_*): it removes observations the state contains and returns
    their log density given the data that remains -- a sliding window over a stream, retraction of bad records, and the
    leave-k-out predictive density:

        st = ResidentPosterior(posterior(f(X[:, :W], S), y[:W]))   # window of the first W observations
        for t in range(W, N):
            st.condition(X[:, t:t+1], S, y[t:t+1])                 # the newest observation in
            lp_old = st.forget(X[:, t-W:t-W+1], S, y[t-W:t-W+1])   # the oldest out: log p(y_old | the window without it)

    The state is created by the library (a Diagonal or dense prior precision is factorised on the device -- reference :78, the
    failing leading minor comes back as PosDefException(info) exactly as from `posterior`), lives in device buffers owned
    through blr_device_alloc and is only copied back by `regressor()`.  A BasisFunctionRegressor keeps its basis: `condition`
    maps the inputs through phi (RandomFourierFeatures: on the device, the features never visit the host) and `regressor()`
    returns BasisFunctionRegressor(posterior, phi) like reference basis_function_regression.jl:62-65."""

    def __init__(self, f):
        self.phi = f.phi if isinstance(f, BasisFunctionRegressor) else None
        base = f.blr if isinstance(f, BasisFunctionRegressor) else f
        if not isinstance(base, BayesianLinearRegressor):
            raise TypeError("ResidentPosterior wraps a BayesianLinearRegressor or a BasisFunctionRegressor")
        dtype = _dtype_of(base.mw)
        D = base.mw.shape[0]
        self.dtype, self.D = dtype, D
        h = self._h = _handle()
        item = np.dtype(dtype).itemsize
        mw = np.array(_mean_vector(base.mw, D, dtype))
        self._mw = _DeviceBuffer.of(h, mw)
        self._T = _DeviceBuffer(h, D * D * item)
        Lw = base.Lw
        if isinstance(Lw, PDMat):
            U = np.asfortranarray(np.triu(np.asarray(Lw.U, dtype=dtype)))
            if U.shape != (D, D):
                raise ValueError("size of the prior precision != length(mw)")
            k = _first_nonpositive(np.diag(U))  # a factor with a non-positive diagonal is not a Cholesky factor
            if k:
                raise _abi.PosDefException(k)
            h.memcpy_h2d(self._T.ptr, U)
            return
        # Diagonal / dense precision: T = chol(Lw).U by the library's own factorisation -- the posterior update on ZERO
        # observations (A = Lw), written straight into the resident buffers
        Lw_h, prior_kind, ldl = _prior(Lw, D, dtype)
        d_Lw = _DeviceBuffer.of(h, Lw_h)
        d_one = _DeviceBuffer.of(h, np.ones(1, dtype=dtype))
        d_info = _DeviceBuffer.of(h, np.zeros(1, dtype=np.int32))
        try:
            h.posterior_batched(dtype, _abi.MEM_DEVICE, _abi.LAYOUT_COLVECS, 1, D, 0, None, max(D, 1), 0, None, 0,
                                _abi.NOISE_ISOTROPIC, d_one.ptr, 0, prior_kind, self._mw.ptr, 0, d_Lw.ptr, ldl, 0,
                                None, D, self._T.ptr, max(D, 1), D * D, None, max(D, 1), D * D, None, d_info.ptr)
            info = np.zeros(1, dtype=np.int32)
            h.memcpy_d2h(info, d_info.ptr)
        finally:
            for b in (d_Lw, d_one, d_info):
                b.free()
        if info[0] != 0:
            raise _abi.PosDefException(int(info[0]))

    def _inputs(self, x, scope):
        """-> (device pointer, layout, ldx, number of inputs) of phi(x) (RandomFourierFeatures: evaluated on the device)."""
        dtype, h, D = self.dtype, self._h, self.D
        if isinstance(self.phi, RandomFourierFeatures):
            Xin, ldxin, Din, k, Om, ph = self.phi._operands(x, dtype)
            if Om.shape[1] != D:
                raise ValueError(f"number of features ({Om.shape[1]}) != length(mw) = {D}")
            dX, ldx = scope.alloc(D * max(k, 1) * np.dtype(dtype).itemsize), max(D, 1)
            h.rff_features(dtype, _abi.MEM_DEVICE, Din, D, k, scope.dev(Xin), ldxin, scope.dev(Om), max(Din, 1), scope.dev(ph), self.phi.scale,
                           dX, ldx)
            return dX, _abi.LAYOUT_COLVECS, ldx, k
        X, layout, ldx, Dx, k = _x_layout(self.phi(x) if self.phi is not None else x, dtype)
        if Dx != D:
            raise ValueError(f"dimension of the inputs ({Dx}) != length(mw) = {D}")
        return scope.dev(X), layout, ldx, k

    def condition(self, x, Sy, y):
        """In-place update with the observations (x, Sy, y); returns log p(y | everything conditioned on so far)."""
        dtype, h, D = self.dtype, self._h, self.D
        with _DeviceScope(h) as scope:
            dX, layout, ldx, k = self._inputs(x, scope)
            y = np.ascontiguousarray(y, dtype=dtype)
            if y.shape != (k,):
                raise ValueError("length(y) != number of inputs")  # reference :74
            s, noise_kind = _noise(Sy, k, dtype)
            if noise_kind == _abi.NOISE_DENSE:
                raise NotImplementedError("ResidentPosterior.condition takes scalar or diagonal noise (whiten a dense block first)")
            d_lp = scope.dev(np.zeros(1, dtype=np.float64))
            d_info = scope.dev(np.zeros(1, dtype=np.int32))
            h.update_factor(dtype, _abi.MEM_DEVICE, layout, 1, D, k, dX, ldx, 0, scope.dev(y), 0, noise_kind, scope.dev(s), 0, self._mw.ptr, 0,
                            self._T.ptr, max(D, 1), 0, d_lp, d_info)
            lp = np.zeros(1, dtype=np.float64)
            info = np.zeros(1, dtype=np.int32)
            h.memcpy_d2h(lp, d_lp)
            h.memcpy_d2h(info, d_info)
        if info[0] != 0:
            raise _abi.PosDefException(int(info[0]))
        return float(lp[0])

    def forget(self, x, Sy, y):
        """In-place DOWNDATE: removes the observations (x, Sy, y), which the state must contain; returns log p(y | the data that
        remains) -- at one observation its leave-one-out predictive density.  A removal that would leave a precision that is not
        positive definite raises PosDefException(info) (include/blr_mi355x.h blr_downdate_factor_*) and leaves the state as it
        was."""
        dtype, h, D = self.dtype, self._h, self.D
        with _DeviceScope(h) as scope:
            dX, layout, ldx, k = self._inputs(x, scope)
            y = np.ascontiguousarray(y, dtype=dtype)
            if y.shape != (k,):
                raise ValueError("length(y) != number of inputs")  # reference :74
            s, noise_kind = _noise(Sy, k, dtype)
            if noise_kind == _abi.NOISE_DENSE:
                raise NotImplementedError("ResidentPosterior.forget takes scalar or diagonal noise (whiten a dense block first)")
            d_lp = scope.dev(np.zeros(1, dtype=np.float64))
            d_info = scope.dev(np.zeros(1, dtype=np.int32))
            h.downdate_factor(dtype, _abi.MEM_DEVICE, layout, 1, D, k, dX, ldx, 0, scope.dev(y), 0, noise_kind, scope.dev(s), 0, self._mw.ptr, 0,
                              self._T.ptr, max(D, 1), 0, d_lp, d_info)
            lp = np.zeros(1, dtype=np.float64)
            info = np.zeros(1, dtype=np.int32)
            h.memcpy_d2h(lp, d_lp)
            h.memcpy_d2h(info, d_info)
        if info[0] != 0:
            raise _abi.PosDefException(int(info[0]))
        return float(lp[0])

    def _heldout(self, row, what, why, x, Sy, target, F=None, means=None, S=None, check=None):
        """The scoring entry point of ``row`` on the resident pointers (B = 1, no strides) for the observations (x, Sy, target); the
        state is not touched.  ``means``, ``S``: the D x S block of a ResidentColumnsPosterior, whose factor this state is, and then
        ``target`` is N x S; ``check(N)`` runs before the targets and the noise are staged."""
        dtype, h, D = self.dtype, self._h, self.D
        with _DeviceScope(h) as scope:
            dX, layout, ldx, N = self._inputs(x, scope)
            if S is None:
                target = np.ascontiguousarray(target, dtype=dtype)
                if target.shape != (N,):
                    raise ValueError("length(y) != number of inputs")  # reference :74
            else:
                target = np.asfortranarray(target, dtype=dtype)
                if target.shape != (N, S):
                    raise ValueError("Y must be (number of inputs) x S")  # reference :74 per column
            s, noise_kind = _noise(Sy, N, dtype)
            if noise_kind == _abi.NOISE_DENSE:
                raise NotImplementedError(f"{what} takes scalar or diagonal noise ({why})")
            if check is not None:
                check(N)
            if S is not None and row.folds and N == 0:
                return _heldout_empty(row, dtype, 0, S, F)
            d_target = None if S is not None and N == 0 else scope.dev(target)
            head, data = _heldout_operands(row, dtype, layout, 1, D, N, S, dX, ldx, 0, d_target, 0, noise_kind, scope.dev(s), 0)
            m, v, lp, tot, info = _heldout_call(scope, row, head, F, data, self._mw.ptr if means is None else means, 0, self._T.ptr, 0)
        if info[0] != 0:
            raise _abi.PosDefException(int(info[0]))
        return _heldout_records(row, m, v, lp, tot)[0]

    def loo(self, x, Sy, y):
        """Exact leave-one-out predictives of the observations (x, Sy, y), which the caller vouches the state contains: for each
        n what ``forget`` of observation n alone would report, without touching the state (blr_loo_batched_*, B = 1).  Returns
        LOO(mean, var, logpdf, total); a state with a non-positive diagonal entry or a non-positive variance raises
        PosDefException(info)."""
        return self._heldout(_HELDOUT["loo"], "ResidentPosterior.loo", "dense noise: a block leave-out", x, Sy, y)

    def kfold(self, x, Sy, y, fold_size):
        """Exact leave-fold-out predictives of the observations (x, Sy, y), which the caller vouches the state contains, for
        contiguous folds of ``fold_size`` (1..64): per fold what ``forget`` of the fold, a prediction at its inputs and
        ``condition`` would give, without touching the state (blr_kfold_batched_*, B = 1, on the resident pointers).  Returns
        KFold(mean, var, logpdf, total); a state with a non-positive diagonal entry or a non-positive variance raises
        PosDefException(info)."""
        return self._heldout(_HELDOUT["kfold"], "ResidentPosterior.kfold", "dense noise couples the folds", x, Sy, y, _fold_size(fold_size))

    def kfold_large(self, x, Sy, y, fold_size):
        """`kfold` for LARGE folds: any integer ``fold_size`` >= 1 with ceil(N / fold_size) <= 1024, D <= 128
        (blr_kfold_large_batched_*, B = 1, on the resident pointers; the state is not touched).  Returns KFold(mean, var, logpdf,
        total); a state with a non-positive diagonal entry or a non-positive variance raises PosDefException(info)."""
        F = _fold_size_large(fold_size)
        return self._heldout(_HELDOUT["kfold_large"], "ResidentPosterior.kfold_large", "dense noise couples the folds", x, Sy, y, F,
                             check=lambda N: _kfold_large_check(self.D, N, F, "ResidentPosterior.kfold_large"))

    def rand(self, rng, x, S, Sy=None):
        """S draws at the inputs x from the resident state (N x S), without copying T to the host (blr_rand_batched_*, B = 1):
        with Sy, ``rand(rng, st.regressor()(x, Sy), S)`` (reference :49-53: Z1 drawn first, then Z2); without it the noise-free
        function values ``evaluate(rand(rng, st.regressor(), S), x)`` (sampling_functions.jl:16-18, 27-38: Z1 only)."""
        dtype, h, D, S = self.dtype, self._h, self.D, int(S)
        with _DeviceScope(h) as scope:
            dX, layout, ldx, N = self._inputs(x, scope)
            s, noise_kind = (np.ones(1, dtype=dtype), _abi.NOISE_ISOTROPIC) if Sy is None else _noise(Sy, N, dtype, need_cholesky=True)
            if noise_kind == _abi.NOISE_DENSE:
                raise NotImplementedError("ResidentPosterior.rand takes scalar or diagonal noise")
            Z1 = _randn(rng, D, S, dtype)
            Z2 = _randn(rng, N, S, dtype) if Sy is not None else None
            Y = np.empty((N, S), dtype=dtype, order="F")
            if N == 0 or S == 0:
                return Y
            dY = scope.alloc(Y.nbytes)
            d_info = scope.dev(np.zeros(1, dtype=np.int32))
            h.rand_batched(dtype, _abi.MEM_DEVICE, layout, 1, D, N, S, dX, ldx, 0, noise_kind, scope.dev(s), 0, _abi.PRIOR_UPPER_FACTOR,
                           self._mw.ptr, 0, self._T.ptr, max(D, 1), 0, scope.dev(Z1), D, 0, scope.dev(Z2) if Z2 is not None else None, N, 0,
                           None, D, 0, dY, N, 0, d_info)
            info = np.zeros(1, dtype=np.int32)
            h.memcpy_d2h(info, d_info)
            if info[0] != 0:
                raise _abi.PosDefException(int(info[0]))
            h.memcpy_d2h(Y, dY)
            return Y

    def _cov(self, x, Sy, want_mean):
        dtype, h, D = self.dtype, self._h, self.D
        with _DeviceScope(h) as scope:
            dX, layout, ldx, N = self._inputs(x, scope)
            s, noise_kind = _noise(Sy, N, dtype)
            m = np.empty(N, dtype=dtype) if want_mean else None
            Cv = np.empty((N, N), dtype=dtype, order="F")
            if N == 0:
                return m, Cv
            d_C = scope.alloc(Cv.nbytes)
            d_m = None
            if want_mean:
                d_m = scope.alloc(m.nbytes)
            info = np.zeros(1, dtype=np.int32)
            d_info = scope.dev(info)
            h.mean_and_cov_batched(dtype, _abi.MEM_DEVICE, layout, 1, D, N, dX, ldx, 0, noise_kind, scope.dev(s), N, 0, _abi.PRIOR_UPPER_FACTOR,
                                   self._mw.ptr if want_mean else None, 0, self._T.ptr, max(D, 1), 0, d_m, N, d_C, N, 0, d_info)
            h.memcpy_d2h(info, d_info)
            if info[0] > 0:
                raise _abi.PosDefException(int(info[0]))
            h.memcpy_d2h(Cv, d_C)
            if want_mean:
                h.memcpy_d2h(m, d_m)
            return m, Cv

    def cov(self, x, Sy=1e-18):
        """cov(f(x, Sy)) (reference :35-38) from the resident state: the full N x N predictive covariance, without copying T to the
        host (blr_mean_and_cov_batched_* on device pointers, B = 1).  Sy: scalar, vector / Diagonal, or a dense N x N matrix."""
        return self._cov(x, Sy, False)[1]

    def mean_and_cov(self, x, Sy=1e-18):
        """mean_and_cov(f(x, Sy)) (reference :45) from the resident state."""
        return self._cov(x, Sy, True)

    def state(self):
        """host copies (mw, T) of the resident state; T column-major upper"""
        mw = np.empty(self.D, dtype=self.dtype)
        T = np.empty((self.D, self.D), dtype=self.dtype, order="F")
        self._h.memcpy_d2h(mw, self._mw.ptr)
        self._h.memcpy_d2h(T, self._T.ptr)
        return mw, np.triu(T)

    def regressor(self):
        """The current state as a regressor of the type it was built from (precision carried by its factor, reference :93)."""
        mw, T = self.state()
        post = BayesianLinearRegressor(mw, PDMat(T))
        return BasisFunctionRegressor(post, self.phi) if self.phi is not None else post


class ResidentPosteriorBatch:
    """B posteriors kept ON THE DEVICE as one pair of buffers (mw [B x D], T [B x D x D]) and conditioned IN PLACE, each on its own
    number of new observations -- none included -- in one library call: the step an online or bandit loop takes after a round of
    draws, where most regressors saw nothing, some one observation and a few several (blr_update_factor_ragged_* /
    blr_downdate_factor_ragged_*).

        st = ResidentPosteriorBatch([f] * B)                        # or B posteriors
        lp = st.condition(ColVecs(X), offsets, 0.1, y)              # regressor b receives X[:, offsets[b]:offsets[b + 1]]
        lp = st.forget(ColVecs(X), offsets, 0.1, y)                 # ... and gives them back

    ``fs``: B BayesianLinearRegressors of one dimension with one kind of prior precision; the states are created the way
    `ResidentPosterior` creates one (a PDMat's factor is copied, a Diagonal or dense precision is factorised by the library on
    zero observations).  ``x``, ``offsets``, ``Sy``, ``y``: packed as `posterior_ragged` takes them."""

    def __init__(self, fs):
        fs = list(fs)
        if not fs or not all(isinstance(g, BayesianLinearRegressor) for g in fs):
            raise TypeError("ResidentPosteriorBatch wraps a non-empty list of BayesianLinearRegressors")
        dtype = np.float32 if all(_dtype_of(g.mw) == np.float32 for g in fs) else np.float64
        B, D = len(fs), fs[0].mw.shape[0]
        self.dtype, self.D, self.B = dtype, D, B
        h = self._h = _handle()
        item = np.dtype(dtype).itemsize
        self._mw = _DeviceBuffer.of(h, np.stack([_mean_vector(g.mw, D, dtype) for g in fs]))
        self._T = _DeviceBuffer(h, B * D * D * item)
        # the packed operands of condition / forget come from _ragged_operands with one stand-in prior: the state is on the device
        self._proto = BayesianLinearRegressor(np.zeros(D, dtype=dtype), Diagonal(np.ones(D, dtype=dtype)))
        priors = [_prior(g.Lw, D, dtype) for g in fs]
        if len({(k, isinstance(g.Lw, PDMat)) for (_, k, _), g in zip(priors, fs)}) != 1:
            raise ValueError("the regressors must share one kind of prior precision")
        _, prior_kind, ldl = priors[0]
        if isinstance(fs[0].Lw, PDMat):
            for b, (U, _, _) in enumerate(priors):
                k = _first_nonpositive(np.diag(U))  # a factor with a non-positive diagonal is not a Cholesky factor
                if k:
                    e = _abi.PosDefException(k)
                    e.index = b
                    raise e
            h.memcpy_h2d(self._T.ptr, np.stack([np.triu(q[0]).reshape(-1, order="F") for q in priors]))
            return
        # Diagonal / dense precisions: T_b = chol(Lw_b).U by the library's own factorisation, the posterior update on ZERO observations
        Lb = np.stack([q[0].reshape(-1, order="A") for q in priors])
        d_Lw = _DeviceBuffer.of(h, Lb)
        d_one = _DeviceBuffer.of(h, np.ones(1, dtype=dtype))
        d_info = _DeviceBuffer.of(h, np.zeros(B, dtype=np.int32))
        info = np.zeros(B, dtype=np.int32)
        try:
            h.posterior_batched(dtype, _abi.MEM_DEVICE, _abi.LAYOUT_COLVECS, B, D, 0, None, max(D, 1), 0, None, 0,
                                _abi.NOISE_ISOTROPIC, d_one.ptr, 0, prior_kind, self._mw.ptr, D, d_Lw.ptr, ldl, Lb.shape[1],
                                None, D, self._T.ptr, max(D, 1), D * D, None, max(D, 1), D * D, None, d_info.ptr)
            h.memcpy_d2h(info, d_info.ptr)
        finally:
            for b in (d_Lw, d_one, d_info):
                b.free()
        _raise_first_failed(info)

    def _revise(self, call, x, offsets, Sy, y):
        dtype, h, D, B = self.dtype, self._h, self.D, self.B
        if y is None or Sy is None:
            raise ValueError("condition / forget need the targets y and the noise Sy")
        ops, _ = _ragged_operands(self._proto, x, offsets, Sy, np.ascontiguousarray(y, dtype=dtype))
        if ops is None or ops[2] != B:
            raise ValueError(f"offsets must have B + 1 = {B + 1} entries")
        _, offsets, _, X, layout, ldx, Dx, y, s, noise_kind, strides = ops[:11]
        if Dx != D:
            raise ValueError(f"dimension of the inputs ({Dx}) != length(mw) = {D}")
        lp, info = np.zeros(B, dtype=np.float64), np.zeros(B, dtype=np.int32)
        with _DeviceScope(h) as scope:
            d_lp, d_info = scope.dev(lp), scope.dev(info)
            call(dtype, _abi.MEM_DEVICE, layout, B, D, offsets, scope.dev(X.reshape(-1, order="A")), ldx, scope.dev(y), noise_kind, scope.dev(s),
                 strides, self._mw.ptr, D, self._T.ptr, max(D, 1), D * D, d_lp, d_info)
            h.memcpy_d2h(lp, d_lp)
            h.memcpy_d2h(info, d_info)
        _raise_first_failed(info)
        return lp

    def condition(self, x, offsets, Sy, y):
        """In-place update of every state with its own slice of the packed observations; returns the B log densities
        log p(y_b | everything state b was conditioned on so far), 0 for a regressor without observations.  The first regressor whose
        state or noise is not positive definite raises PosDefException with its position as ``index``: its state is untouched, the
        other regressors have been updated."""
        return self._revise(self._h.update_factor_ragged, x, offsets, Sy, y)

    def forget(self, x, offsets, Sy, y):
        """In-place DOWNDATE of every state by its own slice of the packed observations, which the state must contain; returns the B
        log densities log p(y_b | the data that remains).  The first regressor whose removal would leave a precision that is not
        positive definite raises PosDefException with its position as ``index``: its state is untouched, the others are downdated."""
        return self._revise(self._h.downdate_factor_ragged, x, offsets, Sy, y)

    def state(self):
        """host copies (mw [B, D], T [B, D, D]) of the resident states; T[b] the upper factor of regressor b"""
        mw = np.empty((self.B, self.D), dtype=self.dtype)
        T = np.empty((self.B, self.D, self.D), dtype=self.dtype)
        self._h.memcpy_d2h(mw, self._mw.ptr)
        self._h.memcpy_d2h(T, self._T.ptr)
        return mw, np.triu(T.transpose(0, 2, 1))  # (the device keeps each factor column-major)

    def regressors(self):
        """The current states as B BayesianLinearRegressors (precision carried by its factor, reference :93)."""
        mw, T = self.state()
        return [BayesianLinearRegressor(mw[b], PDMat(np.asfortranarray(T[b]))) for b in range(self.B)]


class ResidentColumnsPosterior:
    """The S column posteriors of a matrix target kept ON THE DEVICE as one state (M, T): M the D x S block of means, T the ONE upper
    factor of the precision they share -- what `posterior_columns` returns -- conditioned IN PLACE on further observations with S
    targets each (blr_update_multi_factor_*), and `forget` as its inverse (blr_downdate_multi_factor_*).  One library call per
    step does the factor work once and costs two triangular solves per further column; fit -> stream -> predict never copies T
    to the host:

        st = ResidentColumnsPosterior(posterior_columns(f(X1, S1), Y1))   # or a prior: ResidentColumnsPosterior(f, S=3)
        lp = st.condition(X2, S2, Y2)                                      # (S,) log p(Y2[:, c] | Y1[:, c])
        lp_old = st.forget(X1[:, :1], S1, Y1[:1])                          # (S,) log density of the removed row given the rest
        m, v = st.mean_and_var(Xt, 0.1)                                    # (N x S, N) from the resident state

    The S regressors must share one precision object (as those of `posterior_columns` do); a BasisFunctionRegressor keeps its
    basis, exactly as in ResidentPosterior."""

    def __init__(self, fs, S=None):
        if isinstance(fs, (BayesianLinearRegressor, BasisFunctionRegressor)):
            if S is None or int(S) < 1:
                raise ValueError("a single prior regressor needs the number of columns S >= 1")
            fs = [fs] * int(S)
        else:
            fs = list(fs)
            if S is not None and int(S) != len(fs):
                raise ValueError("S != number of column regressors")
        if not fs:
            raise ValueError("at least one column regressor is needed")
        blrs = [f.blr if isinstance(f, BasisFunctionRegressor) else f for f in fs]
        if any(not isinstance(b, BayesianLinearRegressor) for b in blrs):
            raise TypeError("expected BayesianLinearRegressor or BasisFunctionRegressor columns")
        if any(b.Lw is not blrs[0].Lw for b in blrs):
            raise ValueError("the columns must share one precision object")
        self._col0 = ResidentPosterior(fs[0])  # the factor (a Diagonal / dense prior precision is factorised by the library), phi, the handle
        self.phi, self.dtype, self.D, self._h = self._col0.phi, self._col0.dtype, self._col0.D, self._col0._h
        self.S = len(fs)
        self._T = self._col0._T
        M = np.asfortranarray(np.stack([_mean_vector(b.mw, self.D, self.dtype) for b in blrs], axis=1))  # D x S
        self._M = _DeviceBuffer.of(self._h, M)

    def _step(self, call, what, x, Sy, Y):
        dtype, h, D, S = self.dtype, self._h, self.D, self.S
        with _DeviceScope(h) as scope:
            dX, layout, ldx, k = self._col0._inputs(x, scope)
            Y = np.asfortranarray(Y, dtype=dtype)
            if Y.shape != (k, S):
                raise ValueError("Y must be (number of inputs) x S")  # reference :74 per column
            s, noise_kind = _noise(Sy, k, dtype)
            if noise_kind == _abi.NOISE_DENSE:
                raise NotImplementedError(f"ResidentColumnsPosterior.{what} takes scalar or diagonal noise (whiten a dense block first)")
            lp = np.zeros(S, dtype=np.float64)
            info = np.zeros(1, dtype=np.int32)
            d_lp, d_info = scope.dev(lp), scope.dev(info)
            call(dtype, _abi.MEM_DEVICE, layout, 1, D, k, S, dX, ldx, 0, scope.dev(Y) if k else None, max(k, 1), 0, noise_kind, scope.dev(s), 0,
                 self._M.ptr, max(D, 1), 0, self._T.ptr, max(D, 1), 0, d_lp, S, d_info)
            h.memcpy_d2h(lp, d_lp)
            h.memcpy_d2h(info, d_info)
        if info[0] != 0:
            raise _abi.PosDefException(int(info[0]))
        return lp

    def condition(self, x, Sy, Y):
        """In-place update with the observations (x, Sy, Y), Y one row of S targets per input; returns the (S,) array of
        log p(Y[:, c] | everything column c was conditioned on so far).  PosDefException(info) leaves the state as it was."""
        return self._step(self._h.update_multi_factor, "condition", x, Sy, Y)

    def forget(self, x, Sy, Y):
        """In-place DOWNDATE: removes the observations (x, Sy, Y), which the state must contain; returns the (S,) array of
        log p(Y[:, c] | the data that remains).  A removal that would leave a precision that is not positive definite raises
        PosDefException(info) and leaves the state as it was."""
        return self._step(self._h.downdate_multi_factor, "forget", x, Sy, Y)

    def loo(self, x, Sy, Y):
        """Exact leave-one-out predictives of the observations (x, Sy, Y), Y one row of S targets per input, which the caller vouches
        the state contains: per input and column what ``forget`` of that observation alone would report, without touching the state
        (blr_loo_multi_batched_* on device pointers to the resident state, B = 1).  Returns LOO(mean N x S, var N, logpdf N x S,
        total S); a state with a non-positive diagonal entry or a non-positive variance raises PosDefException(info)."""
        return self._col0._heldout(_HELDOUT["loo_columns"], "ResidentColumnsPosterior.loo", "dense noise: a block leave-out", x, Sy, Y,
                                   means=self._M.ptr, S=self.S)

    def kfold(self, x, Sy, Y, fold_size):
        """Exact leave-fold-out (K-fold) predictives of the observations (x, Sy, Y), Y one row of S targets per input, which the
        caller vouches the state contains, for contiguous folds of ``fold_size`` <= 64 observations (D <= 128): per fold and column
        what ``forget`` of that fold, a prediction at its inputs and ``condition`` would give, without touching the state
        (blr_kfold_multi_batched_* on device pointers to the resident state, B = 1).  Returns KFold(mean N x S, var N, logpdf
        nfolds x S, total S); a state with a non-positive diagonal entry or a non-positive variance raises PosDefException(info)."""
        F = _fold_size(fold_size)
        _kfold_columns_check(self.D, "ResidentColumnsPosterior.kfold")
        return self._col0._heldout(_HELDOUT["kfold_columns"], "ResidentColumnsPosterior.kfold", "dense noise couples the folds", x, Sy, Y, F,
                                   means=self._M.ptr, S=self.S)

    def _marginals(self, x, Sy, want_var):
        dtype, h, D, S = self.dtype, self._h, self.D, self.S
        with _DeviceScope(h) as scope:
            dX, layout, ldx, N = self._col0._inputs(x, scope)
            s, noise_kind = _noise(Sy, N, dtype)
            if noise_kind == _abi.NOISE_DENSE:  # var adds diag(Sigma_y) (:43)
                s, noise_kind = np.ascontiguousarray(np.diag(s)), _abi.NOISE_DIAGONAL
            m = np.empty((N, S), dtype=dtype, order="F")
            v = np.empty(N, dtype=dtype) if want_var else None
            if N == 0:
                return m, v
            d_m = scope.alloc(m.nbytes)
            d_v = None
            if want_var:
                d_v = scope.alloc(v.nbytes)
            info = np.zeros(1, dtype=np.int32)
            d_info = scope.dev(info)
            h.marginals_multi_batched(dtype, _abi.MEM_DEVICE, layout, 1, D, N, S, dX, ldx, 0, noise_kind, scope.dev(s) if want_var else None, 0,
                                      _abi.PRIOR_UPPER_FACTOR, self._M.ptr, max(D, 1), 0, self._T.ptr if want_var else None, max(D, 1), 0,
                                      d_m, max(N, 1), 0, d_v, N, d_info)
            h.memcpy_d2h(info, d_info)
            if info[0] > 0:
                raise _abi.PosDefException(int(info[0]))
            h.memcpy_d2h(m, d_m)
            if want_var:
                h.memcpy_d2h(v, d_v)
            return m, v

    def mean_and_var(self, x, Sy=1e-18):
        """mean_and_var(f_c(x, Sy)) (reference :47) of the S resident columns: (mean N x S, var N), blr_marginals_multi_batched_* on
        device pointers to the resident state."""
        return self._marginals(x, Sy, True)

    def mean(self, x):
        """mean(f_c(x)) (reference :33) of the S resident columns: N x S."""
        return self._marginals(x, 1e-18, False)[0]

    def cov(self, x, Sy=1e-18):
        """cov(f_c(x, Sy)) (reference :35-38) of the resident columns: ONE N x N matrix -- the covariance does not depend on the column
        (blr_mean_and_cov_batched_* with mean = NULL on device pointers to the shared factor)."""
        return self._col0._cov(x, Sy, False)[1]

    def rand(self, rng, x, R, Sy=None):
        """R draws at the inputs x from each of the S resident columns: an (N, S, R) Fortran-ordered array, without copying T to
        the host (blr_rand_multi_batched_* on device pointers to the resident state, B = 1).  With Sy, ``[:, c, :]`` is
        ``rand(rng, st.regressors()[c](x, Sy), R)`` with the normals drawn column by column in the reference's order (:49-53: Z1_c,
        then Z2_c, for c = 0 .. S-1); without it the noise-free function values of sampling_functions.jl:16-18, 27-38 (Z1_c only)."""
        dtype, h, D, S, R = self.dtype, self._h, self.D, self.S, int(R)
        with _DeviceScope(h) as scope:
            dX, layout, ldx, N = self._col0._inputs(x, scope)
            s, noise_kind = (np.ones(1, dtype=dtype), _abi.NOISE_ISOTROPIC) if Sy is None else _noise(Sy, N, dtype, need_cholesky=True)
            if noise_kind == _abi.NOISE_DENSE:
                raise NotImplementedError("ResidentColumnsPosterior.rand takes scalar or diagonal noise")
            Z1 = np.empty((D, S * R), dtype=dtype, order="F")
            Z2 = np.empty((N, S * R), dtype=dtype, order="F") if Sy is not None else None
            for c in range(S):
                Z1[:, c * R:(c + 1) * R] = _randn(rng, D, R, dtype)
                if Z2 is not None:
                    Z2[:, c * R:(c + 1) * R] = _randn(rng, N, R, dtype)
            Y = np.empty((N, S * R), dtype=dtype, order="F")  # draw j = c R + r
            if N and R:
                dY = scope.alloc(Y.nbytes)
                d_info = scope.dev(np.zeros(1, dtype=np.int32))
                h.rand_multi_batched(dtype, _abi.MEM_DEVICE, layout, 1, D, N, S, R, dX, ldx, 0, noise_kind, scope.dev(s), 0,
                                     _abi.PRIOR_UPPER_FACTOR, self._M.ptr, max(D, 1), 0, self._T.ptr, max(D, 1), 0, scope.dev(Z1), D, 0,
                                     scope.dev(Z2) if Z2 is not None else None, N, 0, None, D, 0, dY, N, 0, d_info)
                info = np.zeros(1, dtype=np.int32)
                h.memcpy_d2h(info, d_info)
                if info[0] != 0:
                    raise _abi.PosDefException(int(info[0]))
                h.memcpy_d2h(Y, dY)
            return np.asfortranarray(Y.reshape((N, R, S), order="F").transpose(0, 2, 1))

    def state(self):
        """host copies (M, T) of the resident state: M D x S, T column-major upper"""
        M = np.empty((self.D, self.S), dtype=self.dtype, order="F")
        T = np.empty((self.D, self.D), dtype=self.dtype, order="F")
        self._h.memcpy_d2h(M, self._M.ptr)
        self._h.memcpy_d2h(T, self._T.ptr)
        return M, np.triu(T)

    def regressors(self):
        """The current state as S regressors of the type it was built from, sharing ONE PDMat (reference :93 per column)."""
        M, T = self.state()
        Lw = PDMat(T)
        posts = [BayesianLinearRegressor(M[:, c].copy(), Lw) for c in range(self.S)]
        return [BasisFunctionRegressor(p, self.phi) for p in posts] if self.phi is not None else posts


def _marginals(fx, want_mean, want_var):
    fx = _to_finite_blr(fx)
    blr = fx.f
    dtype = _dtype_of(blr.mw)
    X, layout, ldx, D, N = _x_layout(fx.x, dtype)
    mw = _mean_vector(blr.mw, D, dtype)
    s, noise_kind = _noise(fx.Sy, N, dtype)  # var adds diag(Sigma_y) (:43): no factorisation of the noise, no positivity check
    if noise_kind == _abi.NOISE_DENSE:
        s, noise_kind = np.ascontiguousarray(np.diag(s)), _abi.NOISE_DIAGONAL
    Lw, prior_kind, ldl = _prior(blr.Lw, D, dtype, need_cholesky=want_var)  # :41 _cholesky(Lw)
    m = np.empty(N, dtype=dtype) if want_mean else None
    v = np.empty(N, dtype=dtype) if want_var else None
    info = np.zeros(1, dtype=np.int32)
    _handle().marginals_batched(dtype, _abi.MEM_HOST, layout, 1, D, N, X, ldx, 0, noise_kind, s, 0, prior_kind, mw, 0,
                                Lw, ldl, 0, m, N, v, N, info)
    if info[0] > 0:
        raise _abi.PosDefException(int(info[0]))
    return m, v


def mean(fx):
    """reference :33"""
    return _marginals(fx, True, False)[0]


def var(fx):
    """reference :40-43"""
    return _marginals(fx, False, True)[1]


def mean_and_var(fx):
    """reference :47"""
    return _marginals(fx, True, True)


def marginals(fx):
    """AbstractGPs.marginals: Normal.(mean, sqrt.(var))"""
    m, v = mean_and_var(fx)
    return [Normal(mi, math.sqrt(vi)) for mi, vi in zip(m, v)]


def _mean_and_cov(fx, want_mean):
    fx = _to_finite_blr(fx)
    blr = fx.f
    dtype = _dtype_of(blr.mw)
    X, layout, ldx, D, N = _x_layout(fx.x, dtype)
    mw = _mean_vector(blr.mw, D, dtype)
    s, noise_kind = _noise(fx.Sy, N, dtype)
    Lw, prior_kind, ldl = _prior(blr.Lw, D, dtype, need_cholesky=True)  # :36 _cholesky(Lw)
    m = np.empty(N, dtype=dtype) if want_mean else None
    Cv = np.empty((N, N), dtype=dtype, order="F")
    info = np.zeros(1, dtype=np.int32)
    _handle().mean_and_cov(dtype, _abi.MEM_HOST, layout, D, N, X, ldx, noise_kind, s, max(N, 1), prior_kind, mw, Lw, ldl, m, Cv,
                           max(N, 1), info)
    if info[0] > 0:
        raise _abi.PosDefException(int(info[0]))
    return m, Cv


def cov(fx):
    """reference :35-38: Symmetric(alpha' alpha + Sigma_y), alpha = Uw' \\ X -- the full N x N predictive covariance
    (blr_mean_and_cov_*; moderate N, <= 16384)."""
    return _mean_and_cov(fx, False)[1]


def mean_and_cov(fx):
    """reference :45"""
    return _mean_and_cov(fx, True)


# ---------------------------------------------------------------------------------------------------
# joint predictive covariances of many problems in ONE library call: `[mean_and_cov(fx) for fx in fxs]` (reference :35-38 / :45 under
# a map) through blr_mean_and_cov_batched_*
# ---------------------------------------------------------------------------------------------------
def _cov_problem(fx):
    fx = _to_finite_blr(fx)
    blr = fx.f
    dtype = _dtype_of(blr.mw)
    X, layout, ldx, D, N = _x_layout(fx.x, dtype)
    mw = _mean_vector(blr.mw, D, dtype)
    s, noise_kind = _noise(fx.Sy, N, dtype)
    Lw, prior_kind, ldl = _prior(blr.Lw, D, dtype, need_cholesky=True)  # :36 _cholesky(Lw)
    return dict(dtype=dtype, X=X, layout=layout, ldx=ldx, D=D, N=N, mw=mw, Lw=Lw, prior_kind=prior_kind, ldl=ldl, s=s,
                noise_kind=noise_kind, x_obj=fx.x)


def _cov_many(fxs, want_mean):
    """[(mean_b, C_b)]: problems that agree in D, N, dtype, layout, noise kind and prior kind through ONE blr_mean_and_cov_batched_*
    call (the grouping of _draw_many); anything else falls back to one blr_mean_and_cov_* call per problem.  An input x that is the
    same object for every problem is passed once (strideX = 0)."""
    fxs = list(fxs)
    if not fxs:
        return []
    qs = []
    for b, fx in enumerate(fxs):
        try:
            qs.append(_cov_problem(fx))
        except _abi.PosDefException as e:
            e.index = b
            raise
    sig = {(q["dtype"], q["X"].shape, q["X"].flags.f_contiguous, q["layout"], q["D"], q["N"], q["noise_kind"], q["prior_kind"]) for q in qs}
    q0 = qs[0]
    if len(sig) != 1 or q0["N"] == 0:
        out = []
        for b, fx in enumerate(fxs):
            try:
                out.append(_mean_and_cov(fx, want_mean))
            except _abi.PosDefException as e:
                e.index = b
                raise
        return out
    dt, D, N, nb = q0["dtype"], q0["D"], q0["N"], len(qs)
    if all(q["x_obj"] is q0["x_obj"] for q in qs):
        Xb, strideX = q0["X"], 0
    else:
        Xb = np.stack([q["X"].reshape(-1, order="A") for q in qs])
        strideX = Xb.shape[1]
    sb = np.stack([q["s"].reshape(-1, order="A") for q in qs])
    mwb = np.stack([q["mw"] for q in qs]) if want_mean else None
    Lb = np.stack([q["Lw"].reshape(-1, order="A") for q in qs])
    mb = np.empty((nb, N), dtype=dt) if want_mean else None
    Cb = np.empty((nb, N * N), dtype=dt)
    info = np.zeros(nb, dtype=np.int32)
    _handle().mean_and_cov_batched(dt, _abi.MEM_HOST, q0["layout"], nb, D, N, Xb, q0["ldx"], strideX, q0["noise_kind"], sb, N, sb.shape[1],
                                   q0["prior_kind"], mwb, D, Lb, q0["ldl"], Lb.shape[1], mb, N, Cb, N, N * N, info)
    bad = np.flatnonzero(info > 0)
    if bad.size:
        e = _abi.PosDefException(int(info[bad[0]]))
        e.index = int(bad[0])
        raise e
    return [(mb[b] if want_mean else None, Cb[b].reshape((N, N), order="F")) for b in range(nb)]


def cov_map(fxs):
    """``[cov(fx) for fx in fxs]`` in one library call (blr_mean_and_cov_batched_*) when the problems agree in D, N, dtype, layout,
    noise kind and prior kind; a shared input object is read once.  The first problem whose prior is not positive definite raises
    PosDefException; its position is the exception's ``index``."""
    return [c for _, c in _cov_many(fxs, False)]


def mean_and_cov_map(fxs):
    """``[mean_and_cov(fx) for fx in fxs]`` in one library call (reference :45 under a map); see cov_map."""
    return _cov_many(fxs, True)


def _randn(rng, rows, cols, dtype):
    """randn(rng, rows, cols) filled in column-major order like Julia (memory order == draw order)."""
    return np.asarray(rng.standard_normal((cols, rows)), dtype=dtype).T  # F-contiguous (rows, cols)


class BLRFunctionSample:
    """A function sampled from a regressor by fixing w ~ p(w).  reference src/sampling_functions.jl:12-19"""

    def __init__(self, w, phi):
        self.w = w
        self.phi = phi

    def __call__(self, X):
        x = self.phi(X) if self.phi is not None else X
        f = BayesianLinearRegressor(self.w, Diagonal(np.ones_like(self.w)))
        return _marginals(FiniteGP(f, x, 0.0), True, False)[0]  # phi(X)' w through the mean-only stream


def evaluate(samples, X):
    """Every function sample of `samples` (BLRFunctionSamples of ONE regressor, e.g. ``rand(rng, f, S)``) at the inputs X in one
    pass over phi(X): an N x S matrix whose column j is ``samples[j](X)`` -- reference sampling_functions.jl:16-18 for a batch
    (blr_apply_weights_*)."""
    flat = list(np.asarray(samples, dtype=object).reshape(-1, order="F"))
    if not flat:
        raise ValueError("no samples")
    phi = flat[0].phi
    x = phi(X) if phi is not None else X
    dtype = _dtype_of(*[f.w for f in flat])
    Xa, layout, ldx, D, N = _x_layout(x, dtype)
    W = np.asfortranarray(np.stack([np.asarray(f.w, dtype=dtype) for f in flat], axis=1))
    if W.shape[0] != D:
        raise ValueError("dimension of the inputs != length of the sampled weights")
    Y = np.empty((N, len(flat)), dtype=dtype, order="F")
    _handle().apply_weights(dtype, _abi.MEM_HOST, layout, D, N, len(flat), Xa, ldx, W, max(D, 1), Y, max(N, 1))
    return Y


def _blr_and_mapping(b):
    """reference src/sampling_functions.jl:51-52"""
    if isinstance(b, BasisFunctionRegressor):
        return b.blr, b.phi
    if isinstance(b, BayesianLinearRegressor):
        return b, None
    raise TypeError("expected a BayesianLinearRegressor or BasisFunctionRegressor")


def _sample_weights(rng, blr, S):
    dtype = _dtype_of(blr.mw)
    D = blr.mw.shape[0]
    mw = _mean_vector(blr.mw, D, dtype)
    Lw, prior_kind, ldl = _prior(blr.Lw, D, dtype, need_cholesky=True)  # sampling_functions.jl:29,35,44 _cholesky(Lw)
    Z = _randn(rng, D, S, dtype)
    W = np.empty((D, S), dtype=dtype, order="F")
    _handle().sample_weights(dtype, _abi.MEM_HOST, D, S, prior_kind, mw, Lw, ldl, Z, D, W, D)
    return W


def rand(rng, f, *dims):
    """rand(rng, fx[, S]) -- reference :49-53;  rand(rng, f[, dims...]) -- sampling_functions.jl:27-38."""
    if isinstance(f, FiniteGP):
        if len(dims) == 0:
            return rand(rng, f, 1)[:, 0]
        if len(dims) != 1:
            raise TypeError("rand(rng, fx, samples::Int)")
        return _rand_finite(rng, f, int(dims[0]))
    blr, phi = _blr_and_mapping(f)
    if len(dims) == 0:
        return BLRFunctionSample(_sample_weights(rng, blr, 1)[:, 0].copy(), phi)
    if len(dims) == 1 and isinstance(dims[0], (tuple, list)):
        dims = tuple(dims[0])
    S = int(np.prod(dims))
    W = _sample_weights(rng, blr, S)
    out = np.empty(S, dtype=object)
    for i in range(S):
        out[i] = BLRFunctionSample(W[:, i].copy(), phi)
    return out.reshape(dims, order="F")


def rand_b(rng, A, f):
    """rand!(rng, A, f): fill an existing array of samples.  sampling_functions.jl:40-49"""
    blr, phi = _blr_and_mapping(f)
    W = _sample_weights(rng, blr, A.size)
    flat = A.reshape(-1, order="F")
    for i in range(A.size):
        flat[i] = BLRFunctionSample(W[:, i].copy(), phi)
    A[...] = flat.reshape(A.shape, order="F")
    return A


def rand_and_pullback(rng, fx, S):
    """(Y, pullback): the draws of `rand(rng, fx, S)` and their reverse-mode rule -- what Zygote derives through reference
    :49-53 in README.md:56-60 (``Zygote.pullback((X, Σ, mw, Λw) -> rand(rng, BLR(mw, Λw)(X, Σ), S), ...)``); a ccall is opaque
    to it, so the rule is spelled out here (julia/BLRMI355X.jl: the rrule of rand).  ``pullback(Ybar)`` with Ybar N x S returns
    dict(X, noise, mw, Lw): X in the layout of the primal container, noise a vector (Diagonal) or a scalar (isotropic), Lw a
    vector (Diagonal), the upper-factor tangent (PDMat: what flows into ``chol.factors``) or a symmetric matrix (dense).

    The two O(D N S) products run on the device as `blr_apply_weights_*` calls on re-interpreted layouts
    (Wbar = X Ybar, Xbar = W Ybar'); what is left is O(D^2 S) bookkeeping of the rule."""
    fxb = _to_finite_blr(fx)
    blr = fxb.f
    dtype = _dtype_of(blr.mw)
    X, layout, ldx, D, N = _x_layout(fxb.x, dtype)
    mw = _mean_vector(blr.mw, D, dtype)
    Lw, prior_kind, ldl = _prior(blr.Lw, D, dtype, need_cholesky=True)
    s, noise_kind = _noise(fxb.Sy, N, dtype, need_cholesky=True)
    if noise_kind == _abi.NOISE_DENSE:
        raise NotImplementedError("rand_and_pullback takes scalar or diagonal noise")
    Z1 = _randn(rng, D, S, dtype)  # FIRST draw  (reference :51)
    Z2 = _randn(rng, N, S, dtype)  # SECOND draw (reference :52)
    h = _handle()
    W = np.empty((D, S), dtype=dtype, order="F")
    h.sample_weights(dtype, _abi.MEM_HOST, D, S, prior_kind, mw, Lw, ldl, Z1, D, W, D)
    Y = np.empty((N, S), dtype=dtype, order="F")
    h.rand(dtype, _abi.MEM_HOST, layout, D, N, S, X, ldx, noise_kind, s, prior_kind, mw, Lw, ldl, Z1, D, Z2, N, Y, N)
    flip = _abi.LAYOUT_ROWVECS if layout == _abi.LAYOUT_COLVECS else _abi.LAYOUT_COLVECS

    def pullback(Ybar):
        Ybar = np.asarray(Ybar, dtype=dtype)
        if Ybar.shape != (N, S):
            raise ValueError("the cotangent must have the shape of the draws (N x S)")
        # Wbar (D x S) = X Ybar: the same memory read as the design matrix of N "features" at D "inputs" (layout flipped)
        Yb_f = np.asfortranarray(Ybar)
        Wbar = np.empty((D, S), dtype=dtype, order="F")
        h.apply_weights(dtype, _abi.MEM_HOST, flip, N, D, S, X, ldx, Yb_f, max(N, 1), Wbar, max(D, 1))
        # Xbar = W Ybar' in the layout of X: contraction over the S draws
        if layout == _abi.LAYOUT_COLVECS:   # out[d + n D]: "inputs" d, "draws" n, design matrix W read as S x D RowVecs
            Xbar = np.empty((D, N), dtype=dtype, order="F")
            Yb_t = np.ascontiguousarray(Ybar)  # (N, S) C order == S x N column-major
            h.apply_weights(dtype, _abi.MEM_HOST, _abi.LAYOUT_ROWVECS, S, D, N, W, max(D, 1), Yb_t, max(S, 1), Xbar, max(D, 1))
        else:                               # out[n + d N]: "inputs" n, "draws" d, design matrix Ybar read as S x N RowVecs
            Xbar = np.empty((N, D), dtype=dtype, order="F")
            W_t = np.ascontiguousarray(W)      # (D, S) C order == S x D column-major
            h.apply_weights(dtype, _abi.MEM_HOST, _abi.LAYOUT_ROWVECS, S, N, D, Yb_f, max(N, 1), W_t, max(S, 1), Xbar, max(N, 1))
        gX = Xbar if Xbar.shape == np.shape(X) else Xbar.T
        dmw = Wbar.sum(axis=1, dtype=np.float64).astype(dtype)
        V = W - mw[:, None]  # Uw \ Z1
        if prior_kind == _abi.PRIOR_DIAGONAL:
            gL = (-0.5 * np.sum(Wbar.astype(np.float64) * V, axis=1) / Lw).astype(dtype)  # Uw = diag(sqrt(d))
        else:
            if prior_kind == _abi.PRIOR_UPPER_FACTOR:
                U = np.triu(Lw).astype(np.float64)
            else:  # Uw = chol(Lw).U from the library: the posterior update on zero observations (as ResidentPosterior does)
                Tf = np.zeros((D, D), dtype=dtype, order="F")
                lp0 = np.zeros(1)
                rc = h.posterior(dtype, _abi.LAYOUT_COLVECS, D, 0, None, max(D, 1), None, _abi.NOISE_ISOTROPIC, np.ones(1, dtype=dtype),
                                 prior_kind, mw, Lw, ldl, None, Tf, max(D, 1), None, max(D, 1), lp0)
                if rc > 0:
                    raise _abi.PosDefException(rc)
                U = np.triu(Tf).astype(np.float64)
            # D x D bookkeeping of the rule on the host (like the prior tangent of logpdf_and_gradient): Ubar = -triu(Uw^-T Wbar V')
            Ui = _upper_inverse_on_device(h, dtype, _abi.PRIOR_UPPER_FACTOR, U.astype(dtype), D)  # Uw^-1 from the device; the rest is D x D products
            Ubar = -np.triu(Ui.T @ Wbar.astype(np.float64) @ V.T)
            if prior_kind == _abi.PRIOR_UPPER_FACTOR:
                gL = Ubar.astype(dtype)
            else:  # through the Cholesky A = L L', L = Uw': Abar = sym(L^-T Phi(L' Lbar) L^-1), Phi = lower triangle, halved diagonal
                M = np.tril(U @ Ubar.T)
                M[np.diag_indices(D)] *= 0.5
                Ab = Ui @ (Ui @ M.T).T
                gL = (0.5 * (Ab + Ab.T)).astype(dtype)
        sd = np.sum(Ybar.astype(np.float64) * Z2, axis=1) / (2.0 * np.sqrt(np.broadcast_to(s, (N,)).astype(np.float64)))
        gs = sd.astype(dtype) if noise_kind == _abi.NOISE_DIAGONAL else dtype(sd.sum())
        return {"X": np.asarray(gX), "noise": gs, "mw": dmw, "Lw": gL}

    return Y, pullback


def _rand_finite(rng, fx, S):
    fx = _to_finite_blr(fx)
    blr = fx.f
    dtype = _dtype_of(blr.mw)
    X, layout, ldx, D, N = _x_layout(fx.x, dtype)
    mw = _mean_vector(blr.mw, D, dtype)
    Lw, prior_kind, ldl = _prior(blr.Lw, D, dtype, need_cholesky=True)  # :51 _cholesky(Lw) ...
    s, noise_kind = _noise(fx.Sy, N, dtype, need_cholesky=True)          # ... then :52 _cholesky(Sigma_y)
    Z1 = _randn(rng, D, S, dtype)  # FIRST draw  (reference :51)
    Z2 = _randn(rng, N, S, dtype)  # SECOND draw (reference :52)
    Y = np.empty((N, S), dtype=dtype, order="F")
    if noise_kind == _abi.NOISE_DENSE:
        _handle().rand_dense_noise(dtype, _abi.MEM_HOST, layout, D, N, S, X, ldx, s, max(N, 1), prior_kind, mw, Lw, ldl, Z1, D, Z2, N, Y, N)
        return Y
    _handle().rand(dtype, _abi.MEM_HOST, layout, D, N, S, X, ldx, noise_kind, s, prior_kind, mw, Lw, ldl, Z1, D, Z2, N,
                   Y, N)
    return Y


# ---------------------------------------------------------------------------------------------------
# draws from many regressors in ONE library call: `[rand(rng, f, S) for f in fs]` (reference :49-53 / sampling_functions.jl:27-38
# under a map) through blr_rand_batched_*
# ---------------------------------------------------------------------------------------------------
def _draw_problem(rng, f, S, finite):
    """The operands of one draw, with its normals taken from rng in the reference's order (Z1 first, then Z2 for a FiniteGP)."""
    if finite:
        fx = _to_finite_blr(f)
        blr = fx.f
        dtype = _dtype_of(blr.mw)
        X, layout, ldx, D, N = _x_layout(fx.x, dtype)
        x_obj = fx.x
    else:
        blr, _ = _blr_and_mapping(f)
        dtype = _dtype_of(blr.mw)
        X, layout, ldx, D, N, x_obj = None, _abi.LAYOUT_COLVECS, 1, blr.mw.shape[0], 0, None
    mw = _mean_vector(blr.mw, D, dtype)
    Lw, prior_kind, ldl = _prior(blr.Lw, D, dtype, need_cholesky=True)
    s, noise_kind = _noise(fx.Sy, N, dtype, need_cholesky=True) if finite else (None, _abi.NOISE_ISOTROPIC)
    Z1 = _randn(rng, D, S, dtype)
    Z2 = _randn(rng, N, S, dtype) if finite else None
    return dict(dtype=dtype, X=X, layout=layout, ldx=ldx, D=D, N=N, mw=mw, Lw=Lw, prior_kind=prior_kind, ldl=ldl, s=s,
                noise_kind=noise_kind, Z1=Z1, Z2=Z2, x_obj=x_obj)


def _draw_one(q, S):
    """One problem through the single-regressor entry points, exactly as `rand` runs it."""
    h = _handle()
    dt, D, N = q["dtype"], q["D"], q["N"]
    if q["Z2"] is None:
        W = np.empty((D, S), dtype=dt, order="F")
        h.sample_weights(dt, _abi.MEM_HOST, D, S, q["prior_kind"], q["mw"], q["Lw"], q["ldl"], q["Z1"], D, W, D)
        return W
    Y = np.empty((N, S), dtype=dt, order="F")
    if q["noise_kind"] == _abi.NOISE_DENSE:
        h.rand_dense_noise(dt, _abi.MEM_HOST, q["layout"], D, N, S, q["X"], q["ldx"], q["s"], max(N, 1), q["prior_kind"], q["mw"],
                           q["Lw"], q["ldl"], q["Z1"], D, q["Z2"], N, Y, N)
    else:
        h.rand(dt, _abi.MEM_HOST, q["layout"], D, N, S, q["X"], q["ldx"], q["noise_kind"], q["s"], q["prior_kind"], q["mw"], q["Lw"],
               q["ldl"], q["Z1"], D, q["Z2"], N, Y, N)
    return Y


def _draw_many(qs, S):
    """[Y_b] (FiniteGPs) or [W_b] (regressors): equally shaped problems through ONE blr_rand_batched_* call (the grouping of
    _fused_many); differing dtypes, shapes, layouts, noise or prior kinds, or a dense noise covariance, fall back to one call per
    problem.  An input X that is the same object for every problem is passed once (strideX = 0)."""
    sig = {(q["dtype"], None if q["X"] is None else (q["X"].shape, q["X"].flags.f_contiguous), q["layout"], q["D"], q["N"],
            q["noise_kind"], q["prior_kind"], None if q["s"] is None else q["s"].shape) for q in qs}
    finite = qs[0]["Z2"] is not None
    q0 = qs[0]
    if len(sig) != 1 or q0["noise_kind"] == _abi.NOISE_DENSE or (finite and q0["N"] == 0):
        out = []
        for b, q in enumerate(qs):
            try:
                out.append(_draw_one(q, S))
            except _abi.PosDefException as e:
                e.index = b
                raise
        return out
    dt, D, N, nb = q0["dtype"], q0["D"], q0["N"], len(qs)
    mwb = np.stack([q["mw"] for q in qs])
    Lb = np.stack([q["Lw"].reshape(-1, order="A") for q in qs])
    Z1b = np.stack([q["Z1"].reshape(-1, order="F") for q in qs])
    info = np.zeros(nb, dtype=np.int32)
    if finite:
        if all(q["x_obj"] is q0["x_obj"] for q in qs):
            Xb, strideX = q0["X"], 0
        else:
            Xb = np.stack([q["X"].reshape(-1, order="A") for q in qs])
            strideX = Xb.shape[1]
        sb = np.stack([q["s"] for q in qs])
        Z2b = np.stack([q["Z2"].reshape(-1, order="F") for q in qs])
        Yb = np.empty((nb, N * S), dtype=dt)
        _handle().rand_batched(dt, _abi.MEM_HOST, q0["layout"], nb, D, N, S, Xb, q0["ldx"], strideX, q0["noise_kind"], sb, sb.shape[1],
                               q0["prior_kind"], mwb, D, Lb, q0["ldl"], Lb.shape[1], Z1b, D, D * S, Z2b, N, N * S, None, D, D * S,
                               Yb, N, N * S, info)
        out = [Yb[b].reshape((N, S), order="F") for b in range(nb)]
    else:
        Wb = np.empty((nb, D * S), dtype=dt)
        _handle().rand_batched(dt, _abi.MEM_HOST, _abi.LAYOUT_COLVECS, nb, D, 0, S, None, D, 0, _abi.NOISE_ISOTROPIC, None, 0,
                               q0["prior_kind"], mwb, D, Lb, q0["ldl"], Lb.shape[1], Z1b, D, D * S, None, 1, 0, Wb, D, D * S,
                               None, 1, 0, info)
        out = [Wb[b].reshape((D, S), order="F") for b in range(nb)]
    bad = np.flatnonzero(info > 0)
    if bad.size:
        e = _abi.PosDefException(int(info[bad[0]]))
        e.index = int(bad[0])
        raise e
    return out


def rand_map(rng, fs, S):
    """``[rand(rng, f, S) for f in fs]`` in one library call (blr_rand_batched_*), with the normals drawn from rng in exactly that
    order (problem by problem: Z1_b, then Z2_b -- reference :51-52).  A list of FiniteGPs gives a list of N_b x S arrays; a list of
    regressors (BayesianLinearRegressor / BasisFunctionRegressor) gives a list of arrays of S BLRFunctionSamples.  The first problem
    whose prior (or noise) is not positive definite raises PosDefException; its position is the exception's ``index``."""
    fs, S = list(fs), int(S)
    if not fs:
        return []
    finite = isinstance(fs[0], FiniteGP)
    if any(isinstance(f, FiniteGP) != finite for f in fs):
        raise TypeError("rand_map takes a list of FiniteGPs or a list of regressors, not a mixture")
    qs = []
    for b, f in enumerate(fs):
        try:
            qs.append(_draw_problem(rng, f, S, finite))
        except _abi.PosDefException as e:
            e.index = b
            raise
    res = _draw_many(qs, S)
    if finite:
        return res
    out = []
    for f, W in zip(fs, res):
        _, phi = _blr_and_mapping(f)
        arr = np.empty(S, dtype=object)
        for i in range(S):
            arr[i] = BLRFunctionSample(W[:, i].copy(), phi)
        out.append(arr)
    return out


# ---------------------------------------------------------------------------------------------------
# draws from the S column posteriors of a matrix target in ONE library call (blr_rand_multi_batched_*): the columns share one
# factor, so it is read once and X is projected once for all S R draws
# ---------------------------------------------------------------------------------------------------
def _draw_columns_problem(rng, fxs, R):
    """The S columns of one matrix target -> dict(qs = their draw problems, normals taken from rng in the reference's order: per
    column Z1_c, then Z2_c for a FiniteGP; joint = they can share one call: one precision object, one basis and, for FiniteGPs, one
    x object and equal isotropic / diagonal noise)."""
    fxs = list(fxs)
    if not fxs:
        raise ValueError("at least one column is needed")
    finite = isinstance(fxs[0], FiniteGP)
    if any(isinstance(f, FiniteGP) != finite for f in fxs):
        raise TypeError("rand_columns takes the FiniteGPs or the regressors of one matrix target, not a mixture")
    qs = [_draw_problem(rng, f, R, finite) for f in fxs]
    pairs = [_blr_and_mapping(f.f if finite else f) for f in fxs]
    q0, (blr0, phi0) = qs[0], pairs[0]
    joint = all(b.Lw is blr0.Lw and ph is phi0 for b, ph in pairs) and all(q["dtype"] == q0["dtype"] for q in qs)
    if joint and finite:
        joint = (q0["noise_kind"] != _abi.NOISE_DENSE and q0["N"] > 0 and all(f.x is fxs[0].x for f in fxs)
                 and all(q["noise_kind"] == q0["noise_kind"] and np.array_equal(q["s"], q0["s"]) for q in qs))
    return dict(qs=qs, joint=joint, finite=finite, phi=phi0, x_src=fxs[0].x if finite else None, phis=[ph for _, ph in pairs])


def _draw_columns_call(probs, R):
    """Equally shaped joint problems through ONE blr_rand_multi_batched_* call -> per problem the list of S arrays (N x R draws of a
    FiniteGP, D x R weights of a regressor).  Inputs that are one object (and one basis) for every problem are passed once."""
    q0, finite = probs[0]["qs"][0], probs[0]["finite"]
    dt, D, N, nb, S = q0["dtype"], q0["D"], q0["N"], len(probs), len(probs[0]["qs"])
    Mb = np.stack([np.stack([q["mw"] for q in p["qs"]], axis=1).reshape(-1, order="F") for p in probs])  # D x S column-major, ldm = D
    Lb = np.stack([p["qs"][0]["Lw"].reshape(-1, order="A") for p in probs])
    Z1b = np.stack([np.concatenate([q["Z1"].reshape(-1, order="F") for q in p["qs"]]) for p in probs])  # D x S R, draw j = c R + r
    info = np.zeros(nb, dtype=np.int32)
    if finite:
        if all(p["x_src"] is probs[0]["x_src"] and p["phi"] is probs[0]["phi"] for p in probs):
            Xb, strideX = q0["X"], 0
        else:
            Xb = np.stack([p["qs"][0]["X"].reshape(-1, order="A") for p in probs])
            strideX = Xb.shape[1]
        sb = np.stack([p["qs"][0]["s"] for p in probs])
        Z2b = np.stack([np.concatenate([q["Z2"].reshape(-1, order="F") for q in p["qs"]]) for p in probs])
        out, rows = np.empty((nb, N * S * R), dtype=dt), N
        _handle().rand_multi_batched(dt, _abi.MEM_HOST, q0["layout"], nb, D, N, S, R, Xb, q0["ldx"], strideX, q0["noise_kind"], sb,
                                     sb.shape[1], q0["prior_kind"], Mb, D, D * S, Lb, q0["ldl"], Lb.shape[1], Z1b, D, D * S * R,
                                     Z2b, N, N * S * R, None, D, D * S * R, out, N, N * S * R, info)
    else:
        out, rows = np.empty((nb, D * S * R), dtype=dt), D
        _handle().rand_multi_batched(dt, _abi.MEM_HOST, _abi.LAYOUT_COLVECS, nb, D, 0, S, R, None, D, 0, _abi.NOISE_ISOTROPIC, None, 0,
                                     q0["prior_kind"], Mb, D, D * S, Lb, q0["ldl"], Lb.shape[1], Z1b, D, D * S * R, None, 1, 0,
                                     out, D, D * S * R, None, 1, 0, info)
    bad = np.flatnonzero(info > 0)
    if bad.size:
        e = _abi.PosDefException(int(info[bad[0]]))
        e.index = int(bad[0])
        raise e
    return [[out[b].reshape((rows, S * R), order="F")[:, c * R:(c + 1) * R] for c in range(S)] for b in range(nb)]


def _draw_columns_wrap(p, arrays, R):
    """FiniteGPs: the N x R arrays themselves; regressors: arrays of R BLRFunctionSamples, as rand_map returns them."""
    if p["finite"]:
        return [np.asfortranarray(a) for a in arrays]
    out = []
    for W, phi in zip(arrays, p["phis"]):
        arr = np.empty(R, dtype=object)
        for i in range(R):
            arr[i] = BLRFunctionSample(W[:, i].copy(), phi)
        out.append(arr)
    return out


def rand_columns_map(rng, fxss, R):
    """``[[rand(rng, fx, R) for fx in fxs] for fxs in fxss]`` for lists of the S columns of matrix targets (FiniteGPs, e.g.
    ``[p(x, Sy) for p in posterior_columns(...)]``, or regressors), with the normals drawn from rng in exactly that order.  Problems
    whose columns share one precision object (and, for FiniteGPs, one x object and equal noise) and that have one shape go through
    ONE blr_rand_multi_batched_* call (the grouping of rand_map); otherwise problem by problem, a problem with mixed columns through
    the route of rand_map.  The first problem whose prior (or noise) is not positive definite raises PosDefException; its position
    is the exception's ``index``."""
    fxss, R = [list(fxs) for fxs in fxss], int(R)
    if not fxss:
        return []
    probs = []
    for b, fxs in enumerate(fxss):
        try:
            probs.append(_draw_columns_problem(rng, fxs, R))
        except _abi.PosDefException as e:
            e.index = b
            raise
    sig = {(p["finite"], len(p["qs"])) + tuple((q["dtype"], None if q["X"] is None else (q["X"].shape, q["X"].flags.f_contiguous),
                                                 q["layout"], q["D"], q["N"], q["noise_kind"], q["prior_kind"],
                                                 None if q["s"] is None else q["s"].shape) for q in p["qs"][:1]) for p in probs}
    if len(sig) == 1 and all(p["joint"] for p in probs):
        return [_draw_columns_wrap(p, arrays, R) for p, arrays in zip(probs, _draw_columns_call(probs, R))]
    out = []
    for b, p in enumerate(probs):
        try:
            arrays = _draw_columns_call([p], R)[0] if p["joint"] else _draw_many(p["qs"], R)
        except _abi.PosDefException as e:
            e.index = b
            raise
        out.append(_draw_columns_wrap(p, arrays, R))
    return out


def rand_columns(rng, fxs, R):
    """``[rand(rng, fx, R) for fx in fxs]`` for the S columns of ONE matrix target -- FiniteGPs, e.g.
    ``[p(x, Sy) for p in posterior_columns(...)]``, or the regressors themselves (arrays of BLRFunctionSamples) -- with the same RNG
    order (per column Z1_c, then Z2_c).  One blr_rand_multi_batched_* call when the columns share one precision object and, for
    FiniteGPs, one x object and equal noise: the factor is read once and X is projected once for all S R draws.  Otherwise the route
    of rand_map."""
    R = int(R)
    p = _draw_columns_problem(rng, fxs, R)
    arrays = _draw_columns_call([p], R)[0] if p["joint"] else _draw_many(p["qs"], R)
    return _draw_columns_wrap(p, arrays, R)
