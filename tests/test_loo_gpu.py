"""Exact leave-one-out predictives (blr_loo_batched_*, loo, loo_map, ResidentPosterior.loo) against the CPU oracle: brute-force
refits, the N x N formulas, the merged downdate, and the fused / composed routes against each other.  All tests need an MI355X."""
import math

import numpy as np
import pytest

from oracle import blr_oracle as O

pytestmark = pytest.mark.gpu

LOG2PI = math.log(2.0 * math.pi)


@pytest.fixture(scope="module")
def B():
    import blr_amd

    blr_amd._abi.default_handle()  # raises if the extension or the GPU is missing: no silent fallback
    return blr_amd


def _rng(i=0):
    return np.random.Generator(np.random.PCG64(777 + i))


def _nxn(mw, Lw, X, s, y):
    """LOO mean / var / logpdf from K = X'Lw^-1 X + S (N x N, numpy): [K^-1]_nn, [K^-1 delta]_n (R&W eq. 5.12)."""
    N = X.shape[1]
    K = X.T @ np.linalg.solve(Lw, X) + np.diag(np.broadcast_to(s, (N,)))
    Ki = np.linalg.inv((K + K.T) / 2)
    a = Ki @ (y - X.T @ mw)
    d = np.diag(Ki)
    var = 1.0 / d
    mean = y - a / d
    lp = -0.5 * (LOG2PI + np.log(var) + (y - mean) ** 2 / var)
    return mean, var, lp


def _state(rng, D, N, scale=0.7):
    """A resident posterior with N observations of dimension D (PDMat prior) and those observations."""
    U = np.triu(rng.standard_normal((D, D))) * (0.3 / np.sqrt(D))
    U[np.diag_indices(D)] = 1.0 + np.abs(U[np.diag_indices(D)])
    mw = rng.standard_normal(D)
    X = np.asfortranarray(rng.standard_normal((D, N)) * (scale / np.sqrt(D)))
    s = np.exp(0.3 * rng.standard_normal(N))
    y = rng.standard_normal(N)
    return mw, U, X, s, y


# ---- 1. brute force on toy problems --------------------------------------------------------------------------------------
@pytest.mark.parametrize("prior", ["diagonal", "dense", "pdmat"])
@pytest.mark.parametrize("noise", ["isotropic", "diagonal"])
def test_brute_force_toy(B, prior, noise):
    rng = _rng(1)
    N, D = 13, 7
    X, mw, Lw, s = O.generate_toy_problem(rng, N, D, dense_noise_cov=False)
    if noise == "isotropic":
        s = np.float64(0.8)
    if prior == "diagonal":
        Lw = np.exp(0.3 * rng.standard_normal(D))
        Lw_b, Lw_d = B.Diagonal(Lw), np.diag(Lw)
    elif prior == "dense":
        Lw_b, Lw_d = Lw, Lw
    else:
        U = np.linalg.cholesky(Lw).T
        Lw_b, Lw_d = B.PDMat(U), U.T @ U
    f = B.BayesianLinearRegressor(mw, Lw_b)
    y = rng.standard_normal(N)
    Sy = B.Diagonal(s) if noise == "diagonal" else s
    r = B.loo(f(X, Sy), y)
    assert r.logpdf.dtype == np.float64 and r.mean.shape == (N,) and r.var.shape == (N,)
    sv = np.broadcast_to(s, (N,))
    full = O.logpdf_literal(mw, Lw_d, X, np.diag(sv), y)
    for n in range(N):
        rest = [i for i in range(N) if i != n]
        lp_o = full - O.logpdf_literal(mw, Lw_d, X[:, rest], np.diag(sv[rest]), y[rest])
        assert r.logpdf[n] == pytest.approx(lp_o, rel=1e-9, abs=1e-12)
    m_o, v_o, lp_o = _nxn(mw, Lw_d, X, sv, y)
    np.testing.assert_allclose(r.mean, m_o, rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(r.var, v_o, rtol=1e-9)
    np.testing.assert_allclose(r.logpdf, lp_o, rtol=1e-9)
    assert r.total == pytest.approx(math.fsum(r.logpdf), rel=1e-12)


# ---- 2. against the merged downdate ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,N,layout", [(7, 40, "col"), (64, 150, "col"), (128, 200, "col"), (128, 200, "row"), (200, 90, "col"),
                                        (200, 90, "row"), (1024, 1100, "col")])
def test_resident_loo_matches_forget(B, D, N, layout):
    rng = _rng(2 + D)
    mw, U, X, s, y = _state(rng, D, N)
    st = B.ResidentPosterior(B.BayesianLinearRegressor(mw, B.PDMat(U)))
    xin = B.ColVecs(X) if layout == "col" else B.RowVecs(np.asfortranarray(X.T))
    st.condition(xin, B.Diagonal(s), y)
    m0, T0 = st.state()
    r = st.loo(xin, B.Diagonal(s), y)
    m1, T1 = st.state()
    assert np.array_equal(m0, m1) and np.array_equal(T0, T1)  # the state is not modified
    assert r.total == pytest.approx(math.fsum(r.logpdf), rel=1e-12)
    picks = range(N) if D <= 200 else rng.choice(N, 4, replace=False)
    picks = list(picks)[:40]
    for n in picks:
        cp = B.ResidentPosterior(B.BayesianLinearRegressor(m0, B.PDMat(T0)))
        lp = cp.forget(X[:, n:n + 1], B.Diagonal(s[n:n + 1]), y[n:n + 1])
        assert r.logpdf[n] == pytest.approx(lp, rel=1e-9, abs=1e-10)


# ---- 3. the c2 shape (D = 128, N = 4096) ----------------------------------------------------------------------------------
def _c2(rng, dtype=np.float64):
    D, N = 128, 4096
    X = rng.standard_normal((D, N)).astype(dtype)
    mw = rng.standard_normal(D).astype(dtype)
    Lw = np.exp(0.2 * rng.standard_normal(D)).astype(dtype)
    s = dtype(0.5)
    y = (X.T @ rng.standard_normal(D) / np.sqrt(D) + rng.standard_normal(N)).astype(dtype)
    return D, N, X, mw, Lw, s, y


def _lapack_loo(X, mw, Lw, s, y):
    X, mw, Lw, y = (np.asarray(a, dtype=np.float64) for a in (X, mw, Lw, y))
    s = float(s)
    A = np.diag(Lw) + (X @ X.T) / s
    T = np.linalg.cholesky(A).T
    mp = np.linalg.solve(A, Lw * mw + X @ y / s)
    Z = np.linalg.solve(T.T, X)
    sig2 = np.sum(Z * Z, axis=0)
    m = X.T @ mp
    omh = (s - sig2) / s
    r = y - m
    return y - r / omh, s / omh, -0.5 * (LOG2PI + np.log(s) - np.log(omh) + r * r / (s * omh)), 1.0 - omh


def test_c2_fp64(B):
    D, N, X, mw, Lw, s, y = _c2(_rng(3))
    r = B.loo(B.BayesianLinearRegressor(mw, B.Diagonal(Lw))(np.asfortranarray(X), s), y)
    m_o, v_o, lp_o, h = _lapack_loo(X, mw, Lw, s, y)
    ok = h <= 0.999
    assert ok.sum() > N // 2
    np.testing.assert_allclose(r.logpdf[ok], lp_o[ok], rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(r.mean[ok], m_o[ok], rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(r.var[ok], v_o[ok], rtol=1e-9)


def test_c2_fp32(B):
    D, N, X, mw, Lw, s, y = _c2(_rng(4), np.float32)
    r = B.loo(B.BayesianLinearRegressor(mw, B.Diagonal(Lw))(np.asfortranarray(X), s), y)
    assert r.mean.dtype == np.float32 and r.logpdf.dtype == np.float64
    m_o, v_o, lp_o, h = _lapack_loo(X, mw, Lw, s, y)
    ok = h <= 0.99
    np.testing.assert_allclose(r.logpdf[ok], lp_o[ok], rtol=1e-3, atol=1e-3)
    np.testing.assert_allclose(r.mean[ok], m_o[ok], rtol=1e-3, atol=1e-3)
    np.testing.assert_allclose(r.var[ok], v_o[ok], rtol=1e-3)


# ---- 4. routes ------------------------------------------------------------------------------------------------------------
def _raw(B, dtype, layout, X, ldx, y, s, mw, T, Bn=1, strideX=0):
    """blr_loo_batched_* in the host memspace on one state (mw, T)."""
    D, N = mw.shape[0], y.shape[-1]
    lm, lv, ll = (np.full((Bn, N), 7.0, dtype=dt) for dt in (dtype, dtype, np.float64))
    tot, info = np.full(Bn, 7.0), np.zeros(Bn, dtype=np.int32)
    s = np.atleast_1d(np.asarray(s, dtype=dtype))
    kind = B._abi.NOISE_DIAGONAL if s.shape[-1] == N and N > 1 else B._abi.NOISE_ISOTROPIC
    B._abi.default_handle().loo(dtype, B._abi.MEM_HOST, layout, Bn, D, N, X, ldx, strideX, y, N if y.ndim > 1 else 0, kind, s,
                                s.shape[-1] if s.ndim > 1 else 0, mw, D if mw.ndim > 1 else 0, T, D, D * D if T.ndim > 2 else 0,
                                lm, N, lv, N, ll, N, tot, info)
    return lm, lv, ll, tot, info


def _posterior_state(B, mw, U, X, s, y):
    st = B.ResidentPosterior(B.BayesianLinearRegressor(mw, B.PDMat(U)))
    st.condition(B.ColVecs(X), B.Diagonal(s), y)
    m, T = st.state()
    return m, np.asfortranarray(T)


def test_colvecs_rowvecs_same_bits_and_fused_vs_composed(B):
    rng = _rng(5)
    D, N = 128, 300
    mw, U, X, s, y = _state(rng, D, N)
    m, T = _posterior_state(B, mw, U, X, s, y)
    col = _raw(B, np.float64, B._abi.LAYOUT_COLVECS, X, D, y, s, m, T)
    row = _raw(B, np.float64, B._abi.LAYOUT_ROWVECS, np.asfortranarray(X.T), N, y, s, m, T)
    for a, b in zip(col, row):
        assert np.array_equal(a, b)
    # an odd leading dimension takes the composed route (sweep marginals + epilogue kernel)
    Xo = np.asfortranarray(np.vstack([X, np.zeros((1, N))]))
    odd = _raw(B, np.float64, B._abi.LAYOUT_COLVECS, Xo, D + 1, y, s, m, T)
    for a, b in zip(col[:4], odd[:4]):
        np.testing.assert_allclose(a, b, rtol=1e-12, atol=1e-12)
    assert col[4][0] == 0 and odd[4][0] == 0


@pytest.mark.parametrize("layout", ["col", "row"])  # D > 128: block substitution (ColVecs) / tall TRSM (RowVecs)
def test_large_d_routes_against_lapack(B, layout):
    rng = _rng(6)
    D, N = 256, 500
    mw, U, X, s, y = _state(rng, D, N)
    m, T = _posterior_state(B, mw, U, X, s, y)
    if layout == "col":
        got = _raw(B, np.float64, B._abi.LAYOUT_COLVECS, X, D, y, s, m, T)
    else:
        got = _raw(B, np.float64, B._abi.LAYOUT_ROWVECS, np.asfortranarray(X.T), N, y, s, m, T)
    m_o, v_o, lp_o = _nxn(mw, U.T @ U, X, s, y)
    assert got[4][0] == 0
    np.testing.assert_allclose(got[0][0], m_o, rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(got[1][0], v_o, rtol=1e-9)
    np.testing.assert_allclose(got[2][0], lp_o, rtol=1e-9, atol=1e-9)


# ---- 5. batches -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,N", [(16, 50), (128, 256)])
def test_loo_map_bit_identical_to_single_calls(B, D, N):
    rng = _rng(7 + D)
    fxs, ys = [], []
    for _ in range(5):
        mw, U, X, s, y = _state(rng, D, N)
        fxs.append(B.BayesianLinearRegressor(mw, B.PDMat(U))(B.ColVecs(X), B.Diagonal(s)))
        ys.append(y)
    many = B.loo_map(fxs, ys)
    for b in range(5):
        one = B.loo(fxs[b], ys[b])
        for a, c in zip(many[b], one):
            assert np.array_equal(a, c)
    # a different position in a different batch gives the same bits
    again = B.loo_map(fxs[::-1], ys[::-1])
    for b in range(5):
        for a, c in zip(again[4 - b], many[b]):
            assert np.array_equal(a, c)


def test_shared_inputs_stride_zero(B):
    rng = _rng(8)
    D, N, nb = 128, 128, 3
    X = np.asfortranarray(rng.standard_normal((D, N)) / np.sqrt(D))
    s = np.exp(0.3 * rng.standard_normal(N))
    ms, Ts, ys = [], [], []
    for _ in range(nb):
        mw, U, _, _, y = _state(rng, D, N)
        m, T = _posterior_state(B, mw, U, X, s, y)
        ms.append(m); Ts.append(T); ys.append(y)
    mwb, Tb, yb = np.stack(ms), np.stack([t.reshape(-1, order="F") for t in Ts]), np.stack(ys)
    lm, lv, ll, tot, info = (np.full((nb, N), 7.0), np.full((nb, N), 7.0), np.full((nb, N), 7.0), np.full(nb, 7.0),
                             np.zeros(nb, dtype=np.int32))
    B._abi.default_handle().loo(np.float64, B._abi.MEM_HOST, B._abi.LAYOUT_COLVECS, nb, D, N, X, D, 0, yb, N,
                                B._abi.NOISE_DIAGONAL, s, 0, mwb, D, Tb, D, D * D, lm, N, lv, N, ll, N, tot, info)
    assert not info.any()
    for b in range(nb):
        one = _raw(B, np.float64, B._abi.LAYOUT_COLVECS, X, D, ys[b], s, ms[b], Ts[b])
        assert np.array_equal(ll[b], one[2][0]) and np.array_equal(lm[b], one[0][0]) and tot[b] == one[3][0]


# ---- 6. totals ------------------------------------------------------------------------------------------------------------
def test_total_fixed_order_and_reproducible(B):
    rng = _rng(9)
    D, N = 40, 5000
    mw, U, X, s, y = _state(rng, D, N)
    m, T = _posterior_state(B, mw, U, X, s, y)
    a = _raw(B, np.float64, B._abi.LAYOUT_COLVECS, X, D, y, s, m, T)
    b = _raw(B, np.float64, B._abi.LAYOUT_COLVECS, X, D, y, s, m, T)
    assert a[3][0] == pytest.approx(math.fsum(a[2][0]), rel=1e-12)
    for u, v in zip(a, b):
        assert np.array_equal(u, v)
    # only the total asked for: the same bits through the workspace
    tot, info = np.full(1, 7.0), np.zeros(1, dtype=np.int32)
    B._abi.default_handle().loo(np.float64, B._abi.MEM_HOST, B._abi.LAYOUT_COLVECS, 1, D, N, X, D, 0, y, 0, B._abi.NOISE_DIAGONAL,
                                s, 0, m, 0, T, D, 0, None, N, None, N, None, N, tot, info)
    assert tot[0] == a[3][0]


# ---- 7. status and NaN ----------------------------------------------------------------------------------------------------
def test_status_and_untouched_outputs(B):
    rng = _rng(10)
    D, N = 128, 100
    mw, U, X, s, y = _state(rng, D, N)
    m, T = _posterior_state(B, mw, U, X, s, y)
    Tz = T.copy()
    Tz[5, 5] = 0.0
    got = _raw(B, np.float64, B._abi.LAYOUT_COLVECS, X, D, y, s, m, Tz)
    assert got[4][0] == 6
    for a in got[:4]:
        assert np.all(a == 7.0)
    sb = s.copy()
    sb[17] = -1.0
    got = _raw(B, np.float64, B._abi.LAYOUT_COLVECS, X, D, y, sb, m, T)
    assert got[4][0] == 18
    for a in got[:4]:
        assert np.all(a == 7.0)
    # a bad factor wins over a bad variance
    assert _raw(B, np.float64, B._abi.LAYOUT_COLVECS, X, D, y, sb, m, Tz)[4][0] == 6
    with pytest.raises(B.PosDefException):
        st = B.ResidentPosterior(B.BayesianLinearRegressor(m, B.PDMat(T)))
        st.loo(B.ColVecs(X), B.Diagonal(sb), y)


@pytest.mark.parametrize("D", [16, 128])
def test_degenerate_leverage_gives_nan_and_counts(B, D):
    rng = _rng(11 + D)
    N = 80
    mw, U, X, s, y = _state(rng, D, N)
    h = B._abi.default_handle()
    st = B.ResidentPosterior(B.BayesianLinearRegressor(mw, B.PDMat(U)))
    st.condition(B.ColVecs(X), B.Diagonal(s), y)
    # a high-leverage observation the state does NOT contain: sigma2 > s, so 1 - h < 0
    xo = np.asfortranarray(np.concatenate([X, 40.0 * rng.standard_normal((D, 1))], axis=1))
    so = np.concatenate([s, [1e-3]])
    yo = np.concatenate([y, [0.3]])
    before = h.get_stat("loo_degenerate")
    r = st.loo(B.ColVecs(xo), B.Diagonal(so), yo)
    assert h.get_stat("loo_degenerate") - before == 1
    assert np.isnan(r.mean[N]) and np.isnan(r.var[N]) and np.isnan(r.logpdf[N]) and math.isnan(r.total)
    assert np.all(np.isfinite(r.logpdf[:N]))


# ---- 8. basis functions ---------------------------------------------------------------------------------------------------
def test_basis_function_regressor_callable_phi(B):
    rng = _rng(12)
    N, Din = 13, 3
    Xin = rng.standard_normal((Din, N))
    blr = B.BayesianLinearRegressor(rng.standard_normal(2), B.Diagonal(np.array([1.3, 0.7])))
    phi = lambda x: B.ColVecs(O.phi_test(O.ColVecs(x.X)).X)  # noqa: E731  (the oracle's basis on the package's container)
    bfr = B.BasisFunctionRegressor(blr, phi)
    s = np.exp(0.3 * rng.standard_normal(N))
    y = rng.standard_normal(N)
    r = B.loo(bfr(B.ColVecs(Xin), B.Diagonal(s)), y)
    F = O.phi_test(Xin)
    m_o, v_o, lp_o = _nxn(blr.mw, np.diag([1.3, 0.7]), F, s, y)
    np.testing.assert_allclose(r.logpdf, lp_o, rtol=1e-9)
    np.testing.assert_allclose(r.mean, m_o, rtol=1e-9, atol=1e-12)


def test_resident_random_fourier_features(B):
    rng = _rng(13)
    Din, D, N = 3, 64, 200
    rff = B.RandomFourierFeatures(rng.standard_normal((Din, D)), rng.uniform(0, 2 * np.pi, D))
    Xin = np.asfortranarray(rng.standard_normal((Din, N)))
    s = np.float64(0.3)
    y = rng.standard_normal(N)
    mw, Lw = np.zeros(D), np.ones(D)
    st = B.ResidentPosterior(B.BasisFunctionRegressor(B.BayesianLinearRegressor(mw, B.Diagonal(Lw)), rff))
    st.condition(B.ColVecs(Xin), s, y)
    r = st.loo(B.ColVecs(Xin), s, y)
    F = rff(B.ColVecs(Xin)).X
    m_o, v_o, lp_o = _nxn(mw, np.diag(Lw), np.asarray(F, dtype=np.float64), np.full(N, s), y)
    np.testing.assert_allclose(r.logpdf, lp_o, rtol=1e-8, atol=1e-9)
    np.testing.assert_allclose(r.mean, m_o, rtol=1e-8, atol=1e-9)
