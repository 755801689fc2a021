"""blr_mean_and_cov_batched_* on the device: the mean and the full N x N predictive covariance of B regressors in one
call, through the C ABI and through cov_map / mean_and_cov_map / ResidentPosterior.cov / ResidentColumnsPosterior.cov.  Every
regressor is held to the oracle (O.mean, O.cov) on well-conditioned priors (O.generate_toy_problem, as tests/test_marg_multi_gpu.py
builds them): fp64 at the rtol = 1e-9, atol = 1e-10 of test_finitegp_interface_cov, fp32 at the rtol = atol = 2e-4 the header states
for the marginals, against the fp64 oracle on the fp32-rounded inputs.  The header's bit promises are checked with
assert_array_equal.  Outputs are padded with gaps that hold NaN and must still hold it afterwards."""
import numpy as np
import pytest

import blr_amd
from blr_amd import _abi
from oracle import blr_oracle as O

pytestmark = pytest.mark.gpu

KIND = {"diag": _abi.PRIOR_DIAGONAL, "dense": _abi.PRIOR_DENSE, "factor": _abi.PRIOR_UPPER_FACTOR}
NOISE = {"iso": _abi.NOISE_ISOTROPIC, "diag": _abi.NOISE_DIAGONAL, "dense": _abi.NOISE_DENSE}
TOL = {np.float64: dict(rtol=1e-9, atol=1e-10), np.float32: dict(rtol=2e-4, atol=2e-4)}
DTYPES = [np.float64, np.float32]


@pytest.fixture(scope="module")
def h():
    hd = _abi.Handle()
    yield hd
    hd.close()


_CACHE = {}


def _f64(a):
    return np.asarray(a, dtype=np.float64)


def _data(D, N, dtype, xkind, prior, noise, B=3):
    """B toy regressors and the oracle's mean and covariance of each, once.  xkind: "col" (ColVecs, ldx = D + 1), "row" (RowVecs,
    ldx = N + 1); the padding of X holds NaN, and so does the strict lower triangle of a dense Sigma_y (only the upper one is read)."""
    key = (D, N, np.dtype(dtype).name, xkind, prior, noise, B)
    if key in _CACHE:
        return _CACHE[key]
    rng = np.random.Generator(np.random.PCG64(7000 + 131 * D + N))
    toys = [O.generate_toy_problem(rng, N, D, dense_noise_cov=(noise == "dense"), dtype=dtype) for _ in range(B)]
    Xd = np.stack([t[0] for t in toys])  # [b][d][n]
    mw = np.stack([t[1] for t in toys])
    if xkind == "row":
        layout, ldx = _abi.LAYOUT_ROWVECS, N + 1
        Xp = np.full((B, D, ldx), np.nan, dtype=dtype)
        Xp[:, :, :N] = Xd
    else:
        layout, ldx = _abi.LAYOUT_COLVECS, D + 1
        Xp = np.full((B, N, ldx), np.nan, dtype=dtype)
        Xp[:, :, :D] = np.swapaxes(Xd, 1, 2)
    if noise == "dense":
        s = np.stack([np.where(np.tril(np.ones((N, N), dtype=bool), -1), np.nan, t[3]).reshape(-1, order="F") for t in toys]).astype(dtype)
        Sy = [_f64(np.triu(t[3]) + np.triu(t[3], 1).T) for t in toys]
    elif noise == "diag":
        s = np.stack([t[3] for t in toys])
        Sy = [_f64(s[b]) for b in range(B)]
    else:
        s = np.stack([t[3][:1] for t in toys])
        Sy = [float(s[b, 0]) for b in range(B)]
    if prior == "diag":
        Lw = np.exp(rng.standard_normal((B, D))).astype(dtype)
        ldl, mats = 1, [np.diag(_f64(Lw[b])) for b in range(B)]
    else:
        Lw, mats = np.zeros((B, D * D), dtype=dtype), []
        for b in range(B):
            if prior == "factor":
                U = np.triu(O.chol_upper(_f64(toys[b][2]))).astype(dtype)
                Lw[b] = U.reshape(-1, order="F")
                mats.append(_f64(U).T @ _f64(U))
            else:
                A = toys[b][2]
                Lw[b] = A.reshape(-1, order="F")
                mats.append(_f64(np.triu(A) + np.triu(A, 1).T))
        ldl = D
    mean_o = np.stack([O.mean(_f64(mw[b]), _f64(Xd[b])) for b in range(B)])
    cov_o = np.stack([O.cov(_f64(mw[b]), mats[b], _f64(Xd[b]), Sy[b]) for b in range(B)])
    q = dict(D=D, N=N, B=B, dtype=dtype, layout=layout, ldx=ldx, X=Xp, Xd=Xd, mw=mw, s=s, noise_kind=NOISE[noise], lds=N,
             prior_kind=KIND[prior], Lw=Lw, ldl=ldl, mats=mats, Sy=Sy, mean_o=mean_o, cov_o=cov_o)
    _CACHE[key] = q
    return q


def _call(hd, q, regs=None, mean=True, cov=True, memspace=_abi.MEM_HOST, Lw=None, prior_kind=None, shareX=False, shareLw=False, fill=np.nan):
    """-> (mean [pos][n] or None, C [pos][m][n] or None, info); asserts that every element outside a result still holds the fill"""
    regs = list(range(q["B"])) if regs is None else regs
    nb, N, dt = len(regs), q["N"], q["dtype"]
    ldc, stridemean = N + 2, N + 1
    strideC = ldc * N + 3
    mo = np.full(nb * stridemean, fill, dtype=dt) if mean else None
    Co = np.full(nb * strideC, fill, dtype=dt) if cov else None
    info = np.full(nb, -7, dtype=np.int32)
    X = q["X"][regs[:1]] if shareX else q["X"][regs]
    Lw = q["Lw"][regs] if Lw is None else Lw
    Lw = Lw[:1] if shareLw else Lw
    a = [np.ascontiguousarray(X), np.ascontiguousarray(q["s"][regs]), np.ascontiguousarray(q["mw"][regs]), np.ascontiguousarray(Lw), mo, Co, info]
    if memspace == _abi.MEM_DEVICE:
        host, a = a, []
        for arr in host:
            p = hd.device_alloc(arr.nbytes) if arr is not None else None
            if p:
                hd.memcpy_h2d(p, arr)
            a.append(p)
    rc = hd.mean_and_cov_batched(dt, memspace, q["layout"], nb, q["D"], N, a[0], q["ldx"], 0 if shareX else X[0].size, q["noise_kind"],
                                 a[1] if cov else None, q["lds"], q["s"].shape[1], q["prior_kind"] if prior_kind is None else prior_kind,
                                 a[2] if mean else None, q["D"], a[3] if cov else None, q["ldl"], 0 if shareLw else Lw.shape[1],
                                 a[4], stridemean, a[5], ldc, strideC, a[6])
    assert rc == 0
    if memspace == _abi.MEM_DEVICE:
        hd.synchronize()
        for arr, p in zip(host, a):
            if arr is not None and p:
                hd.memcpy_d2h(arr, p)
                hd.device_free(p)
    same = (lambda g: np.all(np.isnan(g))) if np.isnan(fill) else (lambda g: np.all(g == dt(fill)))
    m_out = C_out = None
    if mean:
        blocks = mo.reshape(nb, stridemean)
        assert same(blocks[:, N:])
        m_out = blocks[:, :N].copy()
    if cov:
        blocks = Co.reshape(nb, strideC)
        assert same(blocks[:, ldc * N:])
        cols = blocks[:, :ldc * N].reshape(nb, N, ldc)  # [pos][column][row]
        assert same(cols[:, :, N:])
        C_out = np.swapaxes(cols[:, :, :N], 1, 2).copy()
    return m_out, C_out, info


def _check(q, m, C, info, regs=None):
    regs = list(range(q["B"])) if regs is None else regs
    assert np.array_equal(info, np.zeros(len(regs), dtype=np.int32))
    tol = TOL[q["dtype"]]
    for pos, b in enumerate(regs):
        if m is not None:
            np.testing.assert_allclose(_f64(m[pos]), q["mean_o"][b], **tol)
        if C is not None:
            np.testing.assert_allclose(_f64(C[pos]), q["cov_o"][b], **tol)
            assert np.array_equal(C[pos], C[pos].T)


# every D of {3, 16, 100, 128}, every N of {1, 64, 65, 130}, both layouts, both noise kinds and all three prior kinds, in both element types
LATTICE = [
    (3, 1, "col", "iso", "diag"),
    (16, 64, "row", "diag", "factor"),
    (100, 65, "col", "diag", "dense"),
    (128, 130, "row", "iso", "factor"),
    (128, 130, "col", "diag", "factor"),
    (16, 130, "col", "iso", "dense"),
    (100, 64, "row", "iso", "diag"),
    (3, 65, "row", "diag", "dense"),
    (128, 1, "col", "iso", "factor"),
]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D,N,xkind,noise,prior", LATTICE)
def test_lattice_against_the_oracle(h, D, N, xkind, noise, prior, dtype):
    q = _data(D, N, dtype, xkind, prior, noise)
    m, C, info = _call(h, q)
    _check(q, m, C, info)
    if dtype == np.float64:
        assert all(np.linalg.eigvalsh(C[b]).min() > 0 for b in range(q["B"]))


@pytest.mark.parametrize("dtype", DTYPES)
def test_dense_noise_reads_the_upper_triangle_only(h, dtype):
    q = _data(16, 65, dtype, "col", "factor", "dense", B=2)
    assert np.isnan(q["s"]).sum() == 2 * (65 * 64 // 2)  # the strict lower triangles are poisoned
    m, C, info = _call(h, q)
    _check(q, m, C, info)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("xkind,prior", [("col", "factor"), ("row", "diag")])
def test_diagonal_and_mean_agree_with_the_batched_marginals(h, dtype, xkind, prior):
    q = _data(100, 130, dtype, xkind, prior, "diag")
    m, C, info = _call(h, q)
    _check(q, m, C, info)
    B, N = q["B"], q["N"]
    mm, vv, inf2 = np.empty((B, N), dtype=dtype), np.empty((B, N), dtype=dtype), np.zeros(B, dtype=np.int32)
    h.marginals_batched(dtype, _abi.MEM_HOST, q["layout"], B, q["D"], N, q["X"], q["ldx"], q["X"][0].size, q["noise_kind"], q["s"], N,
                        q["prior_kind"], q["mw"], q["D"], q["Lw"], q["ldl"], q["Lw"].shape[1], mm, N, vv, N, inf2)
    assert not inf2.any()
    for b in range(B):
        np.testing.assert_allclose(np.diag(C[b]), vv[b], **TOL[dtype])
        np.testing.assert_allclose(m[b], mm[b], **TOL[dtype])


@pytest.mark.parametrize("dtype", DTYPES)
def test_shared_inputs_give_the_bits_of_replicated_ones(h, dtype):
    q = _data(100, 65, dtype, "col", "factor", "iso")
    rep = dict(q, X=np.repeat(q["X"][:1], q["B"], axis=0), Lw=np.repeat(q["Lw"][:1], q["B"], axis=0))
    m0, C0, _ = _call(h, rep)
    m1, C1, i1 = _call(h, dict(rep, Lw=q["Lw"]), shareX=True)
    m2, C2, _ = _call(h, dict(rep, Lw=q["Lw"], X=rep["X"]))
    np.testing.assert_array_equal(m1, m2)
    np.testing.assert_array_equal(C1, C2)
    assert not i1.any()
    m3, C3, i3 = _call(h, dict(rep, X=q["X"]), shareLw=True)
    m4, C4, _ = _call(h, dict(rep, X=q["X"]))
    np.testing.assert_array_equal(m3, m4)
    np.testing.assert_array_equal(C3, C4)
    assert not i3.any()
    # and the shared call is right: regressor 0 of the replicated batch is regressor 0 of the plain one
    np.testing.assert_allclose(_f64(C0[0]), q["cov_o"][0], **TOL[dtype])
    m5, C5, _ = _call(h, rep, shareX=True, shareLw=True)
    np.testing.assert_array_equal(C5, C0)
    np.testing.assert_array_equal(m5, m0)


@pytest.mark.parametrize("dtype", DTYPES)
def test_bit_promises(h, dtype):
    q = _data(128, 130, dtype, "col", "factor", "diag", B=5)
    m, C, info = _call(h, q)
    _check(q, m, C, info)
    m3, C3, _ = _call(h, q, regs=[3])  # regressor 3 alone
    np.testing.assert_array_equal(m3[0], m[3])
    np.testing.assert_array_equal(C3[0], C[3])
    ma, Ca, _ = _call(h, q)  # a second call
    np.testing.assert_array_equal(ma, m)
    np.testing.assert_array_equal(Ca, C)
    md, Cd, infd = _call(h, q, memspace=_abi.MEM_DEVICE)  # device memspace
    np.testing.assert_array_equal(md, m)
    np.testing.assert_array_equal(Cd, C)
    assert not infd.any()
    _, Cn, _ = _call(h, q, mean=False)  # without the mean
    np.testing.assert_array_equal(Cn, C)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("prior", ["factor", "diag", "dense"])
def test_chunk_seams(dtype, prior):
    q = _data(16, 65, dtype, "row", prior, "iso", B=5)
    hd = _abi.Handle()
    try:
        m, C, info = _call(hd, q)
        assert hd.get_stat("last_chunks") == 1
        _check(q, m, C, info)
        hd.set_option("MAX_CHUNK", 2)
        m2, C2, info2 = _call(hd, q)
        assert hd.get_stat("last_chunks") == 3
        np.testing.assert_array_equal(m2, m)
        np.testing.assert_array_equal(C2, C)
        assert not info2.any()
        hd.set_option("MAX_CHUNK", None)
        assert hd.get_stat("workspace_bytes") > 0
        hd.release_workspace()
        _, C3, _ = _call(hd, q)  # the workspace comes back
        np.testing.assert_array_equal(C3, C)
    finally:
        hd.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("prior,k", [("dense", 2), ("factor", 3), ("diag", 1)])
def test_status_of_a_failed_regressor(h, dtype, prior, k):
    D, N = 16, 65
    q = _data(D, N, dtype, "col", prior, "diag")
    Lw = q["Lw"].copy()
    if prior == "dense":
        Lw[1, 1 * D + 1] = -1.0  # A[1, 1] < 0: indefinite at leading minor 2
    elif prior == "factor":
        Lw[1, 2 * D + 2] = 0.0   # a zero at diagonal entry 3
    else:
        Lw[1, 0] = -1.0          # a negative entry 1
    fill = 123.5
    m, C, info = _call(h, q, Lw=Lw, fill=fill)
    assert info.tolist() == [0, k, 0]
    assert np.all(m[1] == dtype(fill)) and np.all(C[1] == dtype(fill))  # untouched, bit for bit
    for b in (0, 2):
        np.testing.assert_allclose(_f64(m[b]), q["mean_o"][b], **TOL[dtype])
        np.testing.assert_allclose(_f64(C[b]), q["cov_o"][b], **TOL[dtype])


@pytest.mark.parametrize("dtype", DTYPES)
def test_mean_only_and_cov_only(h, dtype):
    q = _data(100, 65, dtype, "col", "dense", "diag")
    m, C, info = _call(h, q)
    mo, none, info_m = _call(h, q, cov=False)  # C = NULL: s and Lw are not passed either
    assert none is None and not info_m.any()
    np.testing.assert_array_equal(mo, m)
    none, Co, info_c = _call(h, q, mean=False)  # mean = NULL with mw = NULL
    assert none is None and not info_c.any()
    np.testing.assert_array_equal(Co, C)
    _check(q, mo, Co, info)


@pytest.mark.parametrize("prior,noise", [("factor", "diag"), ("dense", "iso")])
def test_slow_route_above_128(h, prior, noise):
    q = _data(130, 70, np.float64, "col", prior, noise, B=2)
    m, C, info = _call(h, q)
    assert np.array_equal(info, [0, 0])
    for b in range(2):
        np.testing.assert_allclose(m[b], q["mean_o"][b], **TOL[np.float64])
        np.testing.assert_allclose(C[b], q["cov_o"][b], **TOL[np.float64])
    mo, _, _ = _call(h, q, cov=False)
    np.testing.assert_allclose(mo, q["mean_o"], **TOL[np.float64])


def _problems(rng, D, N, nb, shared_x):
    x = blr_amd.ColVecs(np.asfortranarray(rng.standard_normal((D, N))))
    fxs = []
    for _ in range(nb):
        X, mw, Lw, Sy = O.generate_toy_problem(rng, N, D, dense_noise_cov=False)
        f = blr_amd.BayesianLinearRegressor(mw, blr_amd.Symmetric(Lw))
        fxs.append(f(x if shared_x else blr_amd.ColVecs(np.asfortranarray(X)), blr_amd.Diagonal(Sy)))
    return fxs


@pytest.mark.parametrize("shared_x", [False, True])
def test_cov_map_equals_the_loop(shared_x):
    rng = np.random.default_rng(11)
    fxs = _problems(rng, 20, 70, 4, shared_x)
    tol = TOL[np.float64]
    covs = blr_amd.cov_map(fxs)
    both = blr_amd.mean_and_cov_map(fxs)
    for fx, Cm, (m2, C2) in zip(fxs, covs, both):
        m1, C1 = blr_amd.mean_and_cov(fx)
        np.testing.assert_allclose(Cm, C1, **tol)
        np.testing.assert_allclose(C2, C1, **tol)
        np.testing.assert_allclose(m2, m1, **tol)
        np.testing.assert_allclose(Cm, O.cov(fx.f.mw, fx.f.Lw.data, fx.x.X, fx.Sy.diag), **tol)


def test_resident_posteriors():
    rng = np.random.default_rng(12)
    D, N, Nt, S = 20, 30, 70, 3
    X, mw, Lw, Sy = O.generate_toy_problem(rng, N, D, dense_noise_cov=False)
    Xt = np.asfortranarray(rng.standard_normal((D, Nt)))
    st_noise = np.exp(rng.standard_normal(Nt))
    y = rng.standard_normal(N)
    st = blr_amd.ResidentPosterior(blr_amd.BayesianLinearRegressor(mw, blr_amd.Symmetric(Lw)))
    st.condition(blr_amd.ColVecs(np.asfortranarray(X)), blr_amd.Diagonal(Sy), y)
    mw_o, _, A_o = O.posterior_literal(mw, Lw, X, Sy, y)
    tol = TOL[np.float64]
    C = st.cov(blr_amd.ColVecs(Xt), blr_amd.Diagonal(st_noise))
    np.testing.assert_allclose(C, O.cov(mw_o, A_o, Xt, st_noise), **tol)
    assert np.array_equal(C, C.T)
    m, C2 = st.mean_and_cov(blr_amd.ColVecs(Xt), blr_amd.Diagonal(st_noise))
    np.testing.assert_array_equal(C2, C)
    np.testing.assert_allclose(m, O.mean(mw_o, Xt), rtol=1e-8, atol=1e-9)  # (the posterior mean itself went through a solve)
    # the S columns of a matrix target share the factor: one covariance, the same as the single-output state's for that factor
    f = st.regressor()
    cols = blr_amd.ResidentColumnsPosterior([blr_amd.BayesianLinearRegressor(rng.standard_normal(D), f.Lw) for _ in range(S)])
    Cc = cols.cov(blr_amd.ColVecs(Xt), blr_amd.Diagonal(st_noise))
    np.testing.assert_array_equal(Cc, C)
