"""The calls of tests/test_tall_sweep_gpu.py: the four routes that go through the tall-matrix panel sweep (TallSweep, blr_abi.hip),
through the C ABI in host memspace, every output allocated with NaN beyond the extent the library may write.

Each run_* returns {name: whole array, sentinels included}; the test looks at the used part and at the sentinels."""
import numpy as np

from oracle import blr_oracle as O

S_COLS = 5


def problem(dtype, D, N, seed):
    """One regressor with a well-conditioned dense prior; the fp64 master copy is rounded once, the oracle sees the rounded values."""
    rng = np.random.Generator(np.random.PCG64(424200 + seed))
    X = rng.standard_normal((D, N)).astype(dtype)
    mw = (0.3 * rng.standard_normal(D)).astype(dtype)
    Bm = rng.standard_normal((D, D)) / np.sqrt(D)
    Lw = (Bm @ Bm.T + np.eye(D)).astype(dtype)
    Lw = ((Lw + Lw.T) / 2).astype(dtype)
    U = np.triu(O.chol_upper(Lw.astype(float))).astype(dtype)
    s = np.exp(0.3 * rng.standard_normal(N)).astype(dtype)
    Y = rng.standard_normal((N, S_COLS)).astype(dtype)
    return dict(D=D, N=N, X=X, mw=mw, Lw=Lw, U=U, s=s, y=np.ascontiguousarray(Y[:, 0]), Y=Y)


def f64(a):
    return np.asarray(a, dtype=np.float64)


def _x(abi, P, layout):
    """(array in memory order, ldx): ColVecs D x N column-major, RowVecs N x D column-major"""
    if layout == abi.LAYOUT_COLVECS:
        return np.ascontiguousarray(P["X"].T), P["D"]
    return np.ascontiguousarray(P["X"]), P["N"]


def _prior(abi, P, prior):
    """prior: "dense", "factor", or an upper factor given as an array (the bitwise job's zero-diagonal factor)"""
    if isinstance(prior, np.ndarray):
        return np.asfortranarray(prior), abi.PRIOR_UPPER_FACTOR
    if prior == "dense":
        return np.asfortranarray(P["Lw"]), abi.PRIOR_DENSE
    return np.asfortranarray(P["U"]), abi.PRIOR_UPPER_FACTOR


def _nan(shape, dtype):
    return np.full(shape, np.nan, dtype=dtype)


def run_marginals(h, abi, dtype, layout, P, prior):
    D, N = P["D"], P["N"]
    X, ldx = _x(abi, P, layout)
    Lw, kind = _prior(abi, P, prior)
    mean, var = _nan(N + 4, dtype), _nan(N + 4, dtype)
    info = np.full(2, -77, dtype=np.int32)
    try:
        h.marginals_batched(dtype, abi.MEM_HOST, layout, 1, D, N, X, ldx, 0, abi.NOISE_DIAGONAL, P["s"], 0, kind, P["mw"], 0, Lw, D, 0,
                            mean, N + 4, var, N + 4, info)
    except abi.PosDefException:
        pass  # (the status word says which pivot)
    return dict(mean=mean, var=var, info=info)


def run_cov(h, abi, dtype, layout, P, prior):
    D, N = P["D"], P["N"]
    X, ldx = _x(abi, P, layout)
    Lw, kind = _prior(abi, P, prior)
    ldc = N + 3
    mean, Cv = _nan(N + 4, dtype), _nan((N, ldc), dtype)  # (row j of the numpy array = column j of the column-major matrix)
    info = np.full(2, -77, dtype=np.int32)
    try:
        h.mean_and_cov(dtype, abi.MEM_HOST, layout, D, N, X, ldx, abi.NOISE_DIAGONAL, P["s"], N, kind, P["mw"], Lw, D, mean, Cv, ldc, info)
    except abi.PosDefException:
        pass
    return dict(mean=mean, cov=Cv, info=info)


def run_grad(h, abi, dtype, layout, Ps, prior, with_ainv):
    """len(Ps) regressors of one shape in one call"""
    G, D, N = len(Ps), Ps[0]["D"], Ps[0]["N"]
    xs = [_x(abi, P, layout) for P in Ps]
    ldx = xs[0][1]
    X = np.stack([x for x, _ in xs])
    y = np.stack([P["y"] for P in Ps])
    s = np.stack([P["s"] for P in Ps])
    mw = np.stack([P["mw"] for P in Ps])
    pr = [_prior(abi, P, prior) for P in Ps]
    Lw = np.stack([np.ascontiguousarray(L.T) for L, _ in pr])  # [G][column][row]
    kind = pr[0][1]
    lddx = ldx + 2
    ncol = X.shape[1]
    dX = _nan((G, ncol + 1, lddx), dtype)
    dy, ds = _nan((G, N + 4), dtype), _nan((G, N + 4), dtype)
    dmw, mwp = _nan((G, D + 4), dtype), _nan((G, D + 4), dtype)
    ldai = D + 3
    Ai = _nan((G, D + 1, ldai), dtype) if with_ainv else None
    lp = _nan(G + 1, np.float64)
    info = np.full(G + 1, -77, dtype=np.int32)
    try:
        h.logpdf_grad_batched(dtype, abi.MEM_HOST, layout, G, D, N, X, ldx, X[0].size, y, N, abi.NOISE_DIAGONAL, s, N, kind, mw, D,
                              Lw, D, D * D, lp, dX, lddx, dX[0].size, dy, N + 4, ds, N + 4, dmw, D + 4, mwp, D + 4,
                              Ai, ldai, (D + 1) * ldai if with_ainv else 0, info)
    except abi.PosDefException:
        pass
    out = dict(lp=lp, dX=dX, dy=dy, ds=ds, dmw=dmw, mw_post=mwp, info=info)
    if with_ainv:
        out["Ainv"] = Ai
    return out


def run_multi(h, abi, dtype, layout, P, prior):
    D, N, S = P["D"], P["N"], S_COLS
    X, ldx = _x(abi, P, layout)
    Lw, kind = _prior(abi, P, prior)
    Y = np.ascontiguousarray(P["Y"].T)  # [column][n]: N x S column-major
    ldmp = D + 2
    lp = _nan(S + 2, np.float64)
    M = _nan((S + 1, ldmp), dtype)
    info = np.full(2, -77, dtype=np.int32)
    try:
        h.logpdf_multi(dtype, abi.MEM_HOST, layout, D, N, S, X, ldx, Y, N, abi.NOISE_DIAGONAL, P["s"], kind, P["mw"], Lw, D, lp, M, ldmp,
                       info)
    except abi.PosDefException:
        pass
    return dict(lp=lp, means=M, info=info)
