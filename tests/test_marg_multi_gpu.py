"""blr_marginals_multi_batched_* on the device: S mean columns and one variance per input for B regressors in one
call, through the C ABI.  Every column of every regressor is held to the oracle (O.mean per column, O.var) at the bounds
test_marginals_vs_oracle holds blr_marginals_batched_* to -- fp64 rtol = atol = 1e-10, fp32 2e-4 against the fp64 oracle on the
fp32-rounded inputs, problems from O.generate_toy_problem(..., dense_noise_cov=False) -- and the header's bit promises with
assert_array_equal.  Outputs are padded with gaps that hold NaN and must still hold it afterwards."""
import numpy as np
import pytest

import blr_amd
from blr_amd import _abi
from oracle import blr_oracle as O

pytestmark = pytest.mark.gpu

W = _abi.MARG_COLS_PER_PASS
S_MAX = 2 * W + 2
KIND = {"diag": _abi.PRIOR_DIAGONAL, "dense": _abi.PRIOR_DENSE, "factor": _abi.PRIOR_UPPER_FACTOR}
NB = 3


@pytest.fixture(scope="module")
def h():
    hd = _abi.Handle()
    yield hd
    hd.close()


_CACHE = {}


def _data(D, N, dtype, xkind, prior, noise, shared_x=False):
    """NB toy regressors with S_MAX weight columns each (a call uses some of them); the oracle's mean of every column and var, once.
    xkind: "col16" (ColVecs, ldx = D rounded up to 16 bytes), "colodd" (ColVecs, odd ldx > D), "row" (RowVecs, ldx = N + 3);
    padding holds NaN."""
    key = (D, N, np.dtype(dtype).name, xkind, prior, noise, shared_x)
    if key in _CACHE:
        return _CACHE[key]
    rng = np.random.Generator(np.random.PCG64(9000 + 131 * D + N))
    toys = [O.generate_toy_problem(rng, N, D, dense_noise_cov=False, dtype=dtype) for _ in range(NB)]
    if shared_x:
        toys = [(toys[0][0],) + t[1:] for t in toys]
    Xd = np.stack([t[0] for t in toys])  # [b][d][n]
    Md = rng.standard_normal((NB, D, S_MAX)).astype(dtype)
    per16 = 16 // np.dtype(dtype).itemsize
    nx = 1 if shared_x else NB
    if xkind == "row":
        layout, ldx = _abi.LAYOUT_ROWVECS, N + 3
        Xp = np.full((nx, D, ldx), np.nan, dtype=dtype)
        Xp[:, :, :N] = Xd[:nx]
    else:
        layout = _abi.LAYOUT_COLVECS
        ldx = (D + 1) | 1 if xkind == "colodd" else -(-D // per16) * per16
        Xp = np.full((nx, N, ldx), np.nan, dtype=dtype)
        Xp[:, :, :D] = np.swapaxes(Xd[:nx], 1, 2)
    if noise == "diag":
        s = np.stack([t[3] for t in toys])
        noise_kind, strides = _abi.NOISE_DIAGONAL, N
    else:
        s = np.stack([t[3][:1] for t in toys])
        noise_kind, strides = _abi.NOISE_ISOTROPIC, 1
    f64 = lambda a: np.asarray(a, dtype=np.float64)  # noqa: E731
    if prior == "diag":
        Lw = np.exp(rng.standard_normal((NB, D))).astype(dtype)
        ldl, mats = 1, [np.diag(f64(Lw[b])) for b in range(NB)]
    else:
        Lw, mats = np.zeros((NB, D * D), dtype=dtype), []
        for b in range(NB):
            if prior == "factor":
                U = np.triu(O.chol_upper(f64(toys[b][2]))).astype(dtype)
                Lw[b] = U.reshape(-1, order="F")
                mats.append(f64(U).T @ f64(U))
            else:
                A = toys[b][2]
                Lw[b] = A.reshape(-1, order="F")
                mats.append(f64(np.triu(A) + np.triu(A, 1).T))
        ldl = D
    mean_o = np.stack([np.stack([O.mean(f64(Md[b, :, c]), f64(Xd[b])) for c in range(S_MAX)], axis=1) for b in range(NB)])  # [b][n][c]
    var_o = np.stack([O.var(f64(Md[b, :, 0]), mats[b], f64(Xd[b]), f64(s[b]) if noise == "diag" else float(s[b, 0])) for b in range(NB)])
    q = dict(D=D, N=N, dtype=dtype, layout=layout, ldx=ldx, X=Xp, strideX=0 if shared_x else Xp[0].size, Md=Md, s=s, noise_kind=noise_kind,
             strides=strides, prior_kind=KIND[prior], Lw=Lw, ldl=ldl, mean_o=mean_o, var_o=var_o)
    _CACHE[key] = q
    return q


def _pack_M(q, cols, regs):
    """the chosen columns as D x S column-major blocks with ldm = D + 1 and a gap of two elements between regressors"""
    D, S = q["D"], len(cols)
    ldm = D + 1
    M = np.full((len(regs), ldm * S + 2), np.nan, dtype=q["dtype"])
    for pos, b in enumerate(regs):
        for j, c in enumerate(cols):
            M[pos, j * ldm:j * ldm + D] = q["Md"][b, :, c]
    return M, ldm, ldm * S + 2


def _call(hd, q, cols, regs=None, mean=True, var=True, memspace=_abi.MEM_HOST, Lw=None, prior_kind=None, ldl=None):
    """-> (mean [pos][n][j] or None, var [pos][n] or None, info); asserts that every element outside a result still holds NaN"""
    regs = list(range(NB)) if regs is None else regs
    nb, N, S, dt = len(regs), q["N"], len(cols), q["dtype"]
    M, ldm, strideM = _pack_M(q, cols, regs)
    ldmean, stridevar = N + 2, N + 1
    stridemean = ldmean * S + 3
    mo = np.full(nb * stridemean, np.nan, dtype=dt) if mean else None
    vo = np.full(nb * stridevar, np.nan, dtype=dt) if var else None
    info = np.full(nb, -7, dtype=np.int32)
    X = q["X"][0:1] if q["strideX"] == 0 else q["X"][regs]
    Lw = q["Lw"][regs] if Lw is None else Lw
    a = [np.ascontiguousarray(X), np.ascontiguousarray(q["s"][regs]), M, np.ascontiguousarray(Lw), mo, vo, info]
    if memspace == _abi.MEM_DEVICE:
        host, a = a, []
        for arr in host:
            p = hd.device_alloc(arr.nbytes) if arr is not None else None
            if p:
                hd.memcpy_h2d(p, arr)
            a.append(p)
    rc = hd.marginals_multi_batched(dt, memspace, q["layout"], nb, q["D"], N, S, a[0], q["ldx"], q["strideX"], q["noise_kind"],
                                    a[1] if var else None, q["strides"], q["prior_kind"] if prior_kind is None else prior_kind,
                                    a[2] if S else None, ldm, strideM, a[3] if var else None, q["ldl"] if ldl is None else ldl, Lw.shape[1],
                                    a[4], ldmean, stridemean, a[5], stridevar, a[6])
    assert rc == 0
    if memspace == _abi.MEM_DEVICE:
        hd.synchronize()
        for arr, p in zip(host, a):
            if arr is not None and p:
                hd.memcpy_d2h(arr, p)
                hd.device_free(p)
    m_out = v_out = None
    if mean:
        blocks = mo.reshape(nb, stridemean)
        cols_ = blocks[:, :ldmean * S].reshape(nb, S, ldmean)
        m_out = np.swapaxes(cols_[:, :, :N], 1, 2).copy()
        assert np.isnan(cols_[:, :, N:]).all() and np.isnan(blocks[:, ldmean * S:]).all(), "mean: a gap was written"
    if var:
        blocks = vo.reshape(nb, stridevar)
        v_out = blocks[:, :N].copy()
        assert np.isnan(blocks[:, N:]).all(), "var: a gap was written"
    return m_out, v_out, info


def _check(q, cols, m, v, regs=None):
    regs = list(range(NB)) if regs is None else regs
    rt = 1e-10 if q["dtype"] == np.float64 else 2e-4
    for pos, b in enumerate(regs):
        if m is not None:
            for j, c in enumerate(cols):
                np.testing.assert_allclose(m[pos, :, j], q["mean_o"][b, :, c], rtol=rt, atol=rt, err_msg=f"mean, regressor {b} column {c}")
        if v is not None:
            np.testing.assert_allclose(v[pos], q["var_o"][b], rtol=rt, err_msg=f"var, regressor {b}")


CASES = [
    (3, 1, 1, "col16", "diag", "iso"), (16, 31, 2, "colodd", "dense", "diag"), (33, 33, 15, "row", "factor", "diag"),
    (64, 70, 17, "col16", "factor", "iso"), (113, 130, W, "colodd", "factor", "diag"), (128, 130, W + 1, "col16", "factor", "diag"),
    (128, 70, 2 * W + 2, "row", "dense", "iso"), (113, 31, W + 1, "row", "diag", "diag"), (128, 33, 2, "colodd", "diag", "iso"),
    (33, 130, 2 * W + 2, "col16", "dense", "diag"), (16, 70, 15, "row", "factor", "iso"), (3, 130, 17, "colodd", "dense", "iso"),
    (64, 1, W, "row", "dense", "diag"),
]


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("D,N,S,xkind,prior,noise", CASES)
def test_every_column_matches_the_oracle(h, D, N, S, xkind, prior, noise, dtype):
    q = _data(D, N, dtype, xkind, prior, noise)
    cols = list(range(S))
    m, v, info = _call(h, q, cols)
    assert (info == 0).all() and m.dtype == dtype and v.dtype == dtype
    _check(q, cols, m, v)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_one_candidate_set_for_every_regressor(h, dtype):
    q = _data(33, 70, dtype, "col16", "factor", "diag", shared_x=True)
    cols = list(range(W + 1))
    m, v, info = _call(h, q, cols)
    assert q["strideX"] == 0 and (info == 0).all()
    _check(q, cols, m, v)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_other_output_combinations(h, dtype):
    q = _data(64, 70, dtype, "col16", "factor", "iso")
    cols = list(range(17))
    m, v, _ = _call(h, q, cols, var=False)  # mean only: s and Lw are NULL
    assert v is None
    _check(q, cols, m, None)
    m, v, _ = _call(h, q, [], mean=True)  # S = 0: var only, M and mean ignored
    _check(q, [], None, v)
    m, v, _ = _call(h, q, cols, mean=False)  # mean == NULL with S > 0
    assert m is None
    _check(q, cols, None, v)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_bit_properties(h, dtype):
    q = _data(113, 130, dtype, "colodd", "factor", "diag")
    cols = list(range(W + 1))
    m, v, _ = _call(h, q, cols)
    m2, v2, _ = _call(h, q, cols)  # repeat call
    np.testing.assert_array_equal(m, m2)
    np.testing.assert_array_equal(v, v2)
    for b in range(NB):  # B = 3 against three B = 1 calls
        m1, v1, _ = _call(h, q, cols, regs=[b])
        np.testing.assert_array_equal(m1[0], m[b])
        np.testing.assert_array_equal(v1[0], v[b])
    mr, vr, _ = _call(h, q, cols, regs=[2, 1, 0])  # reversed batch
    np.testing.assert_array_equal(mr[::-1], m)
    np.testing.assert_array_equal(vr[::-1], v)
    perm = [W] + list(range(1, W)) + [0]  # column W moves from pass 1 to pass 0, column 0 the other way
    mp, vp, _ = _call(h, q, perm)
    np.testing.assert_array_equal(mp, m[:, :, perm])
    np.testing.assert_array_equal(vp, v)
    # column c unchanged when the other columns are replaced by garbage
    for j in (3, W):
        keep = q["Md"]
        try:
            Mg = np.full_like(keep, 1e30)
            Mg[:, :, j] = keep[:, :, j]
            q["Md"] = Mg
            mg, vg, _ = _call(h, q, cols)
        finally:
            q["Md"] = keep
        np.testing.assert_array_equal(mg[:, :, j], m[:, :, j])
        np.testing.assert_array_equal(vg, v)
    # var does not depend on S or on whether the means are wanted
    _, v_s1, _ = _call(h, q, [0])
    _, v_s0, _ = _call(h, q, [])
    _, v_nomean, _ = _call(h, q, cols, mean=False)
    np.testing.assert_array_equal(v_s1, v)
    np.testing.assert_array_equal(v_s0, v)
    np.testing.assert_array_equal(v_nomean, v)
    # one column alone: its bits do not depend on S
    m_one, _, _ = _call(h, q, [5])
    np.testing.assert_array_equal(m_one[:, :, 0], m[:, :, 5])
    # host against device memspace
    md, vd, infod = _call(h, q, cols, memspace=_abi.MEM_DEVICE)
    np.testing.assert_array_equal(md, m)
    np.testing.assert_array_equal(vd, v)
    assert (infod == 0).all()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("prior", ["factor", "diag"])
@pytest.mark.parametrize("xkind", ["colodd", "row"])
def test_a_workgroup_that_walks_several_tiles(h, xkind, prior, dtype):
    """600 regressors that share every input (all strides 0), D = 20, N = 130 (two full tiles and a tail of two), S = 17 (two passes):
    regressors x passes >= 2 x CUs, so one workgroup per (regressor, pass) commits a tile and prefetches the next while it
    multiplies, three times over.  At B = 1 every workgroup takes one tile: the bits must not depend on which of the two it was."""
    Bn, D, N, S = 600, 20, 130, 17
    q = _data(D, N, dtype, xkind, prior, "diag")
    cols = list(range(S))
    m1, v1, info1 = _call(h, q, cols, regs=[0])
    assert info1[0] == 0
    _check(q, cols, m1, v1, regs=[0])
    M, ldm, _ = _pack_M(q, cols, [0])
    mo = np.full((Bn, N * S), np.nan, dtype=dtype)
    vo = np.full((Bn, N), np.nan, dtype=dtype)
    info = np.full(Bn, -7, dtype=np.int32)
    rc = h.marginals_multi_batched(dtype, _abi.MEM_HOST, q["layout"], Bn, D, N, S, np.ascontiguousarray(q["X"][0]), q["ldx"], 0, q["noise_kind"],
                                   np.ascontiguousarray(q["s"][0]), 0, q["prior_kind"], M, ldm, 0, np.ascontiguousarray(q["Lw"][0]), q["ldl"], 0,
                                   mo, N, N * S, vo, N, info)
    assert rc == 0 and (info == 0).all()
    m = np.swapaxes(mo.reshape(Bn, S, N), 1, 2)
    np.testing.assert_array_equal(m, np.broadcast_to(m1[0], m.shape))
    np.testing.assert_array_equal(vo, np.broadcast_to(v1[0], vo.shape))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_a_prior_that_is_not_positive_definite(h, dtype):
    q = _data(33, 70, dtype, "col16", "dense", "diag")
    D, cols = q["D"], list(range(3))
    Lw = q["Lw"].copy()
    bad = np.eye(D)
    bad[4, 4] = -1.0  # the leading minor of order 5 is the first that is not positive
    Lw[1] = bad.reshape(-1, order="F").astype(dtype)
    regs = list(range(NB))
    N, S = q["N"], len(cols)
    M, ldm, strideM = _pack_M(q, cols, regs)
    mo = np.full((NB, N * S), -777.0, dtype=dtype)
    vo = np.full((NB, N), -777.0, dtype=dtype)
    info = np.full(NB, -7, dtype=np.int32)
    rc = h.marginals_multi_batched(dtype, _abi.MEM_HOST, q["layout"], NB, D, N, S, q["X"], q["ldx"], q["strideX"], q["noise_kind"], q["s"],
                                   q["strides"], q["prior_kind"], M, ldm, strideM, Lw, q["ldl"], Lw.shape[1], mo, N, N * S, vo, N, info)
    assert rc == 0 and info.tolist() == [0, 5, 0]
    assert (mo[1] == -777.0).all() and (vo[1] == -777.0).all()  # the outputs of that regressor are left untouched
    m = np.swapaxes(mo.reshape(NB, S, N), 1, 2)
    for b in (0, 2):
        _check(q, cols, m[b:b + 1], vo[b:b + 1], regs=[b])


def test_round_trip_with_the_fit(h):
    """blr_posterior_multi_batched_f64 writes mw_post / T_post; they go straight into the new call (UPPER_FACTOR, ldm = ldmp)."""
    B, D, N, S = 2, 33, 70, 3
    rng = np.random.Generator(np.random.PCG64(4242))
    toys = [O.generate_toy_problem(rng, N, D, dense_noise_cov=False) for _ in range(B)]
    X = np.stack([np.asfortranarray(t[0]).reshape(-1, order="F") for t in toys])
    Y = rng.standard_normal((B, N, S))
    Yp = np.stack([np.asfortranarray(Y[b]).reshape(-1, order="F") for b in range(B)])
    s = np.stack([t[3] for t in toys])
    mw = np.stack([t[1] for t in toys])
    Lw = np.stack([t[2].reshape(-1, order="F") for t in toys])
    ldmp, ldt = D + 1, D + 2
    mp = np.full((B, ldmp * S + 2), np.nan)
    Tp = np.full((B, ldt * D + 5), np.nan)
    lp, info = np.zeros((B, S)), np.full(B, -7, dtype=np.int32)
    h.posterior_multi_batched(np.float64, _abi.MEM_HOST, _abi.LAYOUT_COLVECS, B, D, N, S, X, D, D * N, Yp, N, N * S, _abi.NOISE_DIAGONAL, s, N,
                              _abi.PRIOR_DENSE, mw, D, Lw, D, D * D, mp, ldmp, mp.shape[1], Tp, ldt, Tp.shape[1], None, D, D * D, lp, S, info)
    assert (info == 0).all()
    mean = np.full((B, N * S), np.nan)
    var = np.full((B, N), np.nan)
    info2 = np.full(B, -7, dtype=np.int32)
    rc = h.marginals_multi_batched(np.float64, _abi.MEM_HOST, _abi.LAYOUT_COLVECS, B, D, N, S, X, D, D * N, _abi.NOISE_DIAGONAL, s, N,
                                   _abi.PRIOR_UPPER_FACTOR, mp, ldmp, mp.shape[1], Tp, ldt, Tp.shape[1], mean, N, N * S, var, N, info2)
    assert rc == 0 and (info2 == 0).all()
    for b in range(B):
        Xb, _, Lb, sb = toys[b]
        for c in range(S):
            mw_post, _, Lw_post = O.posterior_literal(mw[b], Lb, Xb, sb, Y[b, :, c])
            np.testing.assert_allclose(mean[b, c * N:(c + 1) * N], O.mean(mw_post, Xb), rtol=1e-10, atol=1e-10)
        np.testing.assert_allclose(var[b], O.var(mw_post, Lw_post, Xb, sb), rtol=1e-10)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_large_d_route(h, dtype):
    q = _data(144, 40, dtype, "col16", "dense", "diag")
    cols = list(range(3))
    m, v, info = _call(h, q, cols)
    assert (info == 0).all()
    _check(q, cols, m, v)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_python_columns_against_a_loop_of_mean_and_var(dtype):
    rng = np.random.Generator(np.random.PCG64(77))
    D, N, S = 33, 70, W + 1
    X, mw, Lw, s = O.generate_toy_problem(rng, N, D, dense_noise_cov=False, dtype=dtype)
    Y = rng.standard_normal((N, S)).astype(dtype)
    xs = rng.standard_normal((D, 50)).astype(dtype)
    Sy = np.exp(rng.standard_normal(50)).astype(dtype)
    f = blr_amd.BayesianLinearRegressor(mw, Lw)
    posts = blr_amd.posterior_columns(f(blr_amd.ColVecs(np.asfortranarray(X)), s), Y)
    x = blr_amd.ColVecs(np.asfortranarray(xs))
    m, v = blr_amd.mean_and_var_columns(posts, x, Sy)
    assert m.shape == (50, S) and v.shape == (50,) and m.dtype == dtype and v.dtype == dtype
    rt = 1e-10 if dtype == np.float64 else 2e-4
    for j, p in enumerate(posts):
        mj, vj = blr_amd.mean_and_var(p(x, Sy))
        np.testing.assert_allclose(m[:, j], mj, rtol=rt, atol=rt)
        np.testing.assert_allclose(v, vj, rtol=rt)
    np.testing.assert_array_equal(blr_amd.mean_columns(posts, x), m)
    (m2, v2), (m3, v3) = blr_amd.mean_and_var_columns_map([posts, posts], [x, x], Sy=[Sy, Sy])
    np.testing.assert_array_equal(m2, m)
    np.testing.assert_array_equal(v3, v)
