"""Downdate of a resident posterior (blr_downdate_factor_*, ResidentPosterior.forget) against the CPU oracle on the data that
remains.  All tests need an MI355X."""
import numpy as np
import pytest

from oracle import blr_oracle as O

pytestmark = pytest.mark.gpu

RTOL = 1e-9


@pytest.fixture(scope="module")
def B():
    import blr_amd

    blr_amd._abi.default_handle()  # raises if the extension or the GPU is missing: no silent fallback
    return blr_amd


@pytest.fixture
def opt(B):
    """blr_set_option on the process-wide handle, restored to the default after the test."""
    h = B._abi.default_handle()
    touched = []

    def set_(key, value):
        h.set_option(key, value)
        touched.append(key)

    yield set_
    for key in touched:
        h.set_option(key, None)


def _rng(i=0):
    return np.random.Generator(np.random.PCG64(4242 + i))


def _upper(A):
    return np.linalg.cholesky(A).T


def _prior(rng, D):
    U = np.triu(rng.standard_normal((D, D))) * (0.3 / np.sqrt(D))
    U[np.diag_indices(D)] = 1.0 + np.abs(U[np.diag_indices(D)])
    return rng.standard_normal(D), U


def _assert_state(mw_got, T_got, mw_o, A_o, rtol=RTOL):
    T_got = np.triu(np.asarray(T_got, dtype=np.float64))
    assert np.all(np.diag(T_got) > 0)
    np.testing.assert_allclose(T_got.T @ T_got, A_o, rtol=rtol, atol=rtol * np.abs(A_o).max())
    np.testing.assert_allclose(mw_got, mw_o, rtol=50 * rtol, atol=rtol * np.abs(mw_o).max())


# ---- 1. retraction -------------------------------------------------------------------------------------------------------
def test_forget_three_of_thirteen(B):
    rng = _rng(1)
    N, D = 13, 7
    X, mw, Lw, s = O.generate_toy_problem(rng, N, D, dense_noise_cov=False)
    f = B.BayesianLinearRegressor(mw, Lw)
    y = B.rand(rng, f(X, s))
    idx = [1, 6, 10]
    rest = [i for i in range(N) if i not in idx]
    st = B.ResidentPosterior(B.posterior(f(X, s), y))
    lp = st.forget(X[:, idx], s[idx], y[idx])
    mw_o, _, L_o = O.posterior_literal(mw, Lw, X[:, rest], s[rest], y[rest])
    m1, T1 = st.state()
    _assert_state(m1, T1, mw_o, L_o)
    f2 = st.regressor()
    Xp = rng.standard_normal((D, 9))
    np.testing.assert_allclose(B.mean(f2(Xp, s[:9])), O.mean(mw_o, Xp), rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(B.cov(f2(Xp, s[:9])), O.cov(mw_o, L_o, Xp, s[:9]), rtol=1e-9, atol=1e-12)
    lp_o = O.logpdf_literal(mw, Lw, X, s, y) - O.logpdf_literal(mw, Lw, X[:, rest], s[rest], y[rest])
    assert lp == pytest.approx(lp_o, rel=1e-9, abs=1e-10)


# ---- 2. round trip -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [7, 64, 128, 200])
def test_condition_then_forget_round_trip(B, D):
    rng = _rng(2 + D)
    mw, U = _prior(rng, D)
    k = 5
    X = rng.standard_normal((D, k)) * (0.7 / np.sqrt(D))
    y = rng.standard_normal(k)
    s = np.exp(0.3 * rng.standard_normal(k))
    st = B.ResidentPosterior(B.BayesianLinearRegressor(mw, B.PDMat(U)))
    m0, T0 = st.state()
    lp_up = st.condition(B.ColVecs(np.asfortranarray(X)), B.Diagonal(s), y)
    lp_dn = st.forget(B.ColVecs(np.asfortranarray(X)), B.Diagonal(s), y)
    m1, T1 = st.state()
    _assert_state(m1, T1, m0, T0.T @ T0)
    assert lp_dn == pytest.approx(lp_up, rel=1e-9, abs=1e-10)
    assert lp_up == pytest.approx(O.logpdf_literal(mw, U.T @ U, X, s, y), rel=1e-9)


# ---- 3. sliding window ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [16, 128])
def test_sliding_window_does_not_drift(B, D):
    rng = _rng(3 + D)
    W, kstep, steps = 40, 2, 50
    N = W + kstep * steps
    mw = rng.standard_normal(D)
    Lw = np.exp(0.2 * rng.standard_normal(D))
    X = rng.standard_normal((D, N)) / np.sqrt(D)
    s = np.exp(0.3 * rng.standard_normal(N))
    y = rng.standard_normal(N)
    f = B.BayesianLinearRegressor(mw, B.Diagonal(Lw))
    st = B.ResidentPosterior(B.posterior(f(X[:, :W], B.Diagonal(s[:W])), y[:W]))
    for t in range(steps):
        new = slice(W + kstep * t, W + kstep * (t + 1))
        old = slice(kstep * t, kstep * (t + 1))
        st.condition(X[:, new], B.Diagonal(s[new]), y[new])
        lp = st.forget(X[:, old], B.Diagonal(s[old]), y[old])
        assert np.isfinite(lp)
    last = slice(N - W, N)
    mw_o, _, L_o = O.posterior_literal(mw, Lw, X[:, last], s[last], y[last])
    m1, T1 = st.state()
    _assert_state(m1, T1, mw_o, L_o)
    # the last step's value: log p(y_old | the window without it)
    old = slice(kstep * (steps - 1), kstep * steps)
    win = slice(N - W, N)
    lo = O.logpdf_literal(mw, Lw, np.hstack([X[:, old], X[:, win]]), np.concatenate([s[old], s[win]]), np.concatenate([y[old], y[win]]))
    assert lp == pytest.approx(lo - O.logpdf_literal(mw, Lw, X[:, win], s[win], y[win]), rel=1e-8, abs=1e-9)


# ---- 4. device-batched sweep ---------------------------------------------------------------------------------------------
def _batch_problem(rng, nb, D, k, noise, shared_x=False):
    """prior states (m0_b, U0_b); the posterior state after the k observations, from the oracle; X [nb or 1, D, k]."""
    nx = 1 if shared_x else nb
    X = rng.standard_normal((nx, D, k)) * (0.7 / np.sqrt(max(k, 1)))
    y = rng.standard_normal((nb, k))
    s = np.exp(0.3 * rng.standard_normal((nb, k))) if noise == "diagonal" else np.full((1,), 0.37)
    prior, post = [], []
    for b in range(nb):
        m0, U0 = _prior(rng, D)
        sb = s[b] if noise == "diagonal" else np.full(k, s[0])
        mp, _, Ap = O.posterior_literal(m0, U0.T @ U0, X[0 if shared_x else b], sb, y[b])
        prior.append((m0, U0.T @ U0))
        post.append((mp, _upper(Ap)))
    return X, y, s, prior, post


def _exact_downdate(mp, Tp, X, s, y):
    """fp64 downdate of the (rounded) inputs: the posterior without (X, s, y)."""
    A = Tp.T @ Tp - (X / s) @ X.T
    m = np.linalg.solve(A, Tp.T @ (Tp @ mp) - (X / s) @ y)
    return m, A


def _fp32_check(mp32, Tp32, X32, s32, y32, got_m, got_T, got_lp, what):
    f64 = lambda a: np.asarray(a, dtype=np.float64)
    m_ex, A_ex = _exact_downdate(f64(mp32), f64(Tp32), f64(X32), f64(s32), f64(y32))
    lp_ex = O.logpdf_literal(m_ex, A_ex, f64(X32), f64(s32), f64(y32))
    # yardstick: the same downdate in fp32 LAPACK (explicit precision, Cholesky, solves) on the same fp32 inputs
    A32 = Tp32.T @ Tp32 - (X32 / s32) @ X32.T
    m32 = np.linalg.solve(A32, Tp32.T @ (Tp32 @ mp32) - (X32 / s32) @ y32)
    lp32 = O.logpdf_literal(m32, A32, X32, s32.astype(np.float32), y32)
    rel = lambda a, b: float(np.abs(f64(a) - b).max() / max(np.abs(b).max(), 1e-30))
    Tg = np.triu(f64(got_T))
    e_m, e_A = rel(got_m, m_ex), rel(Tg.T @ Tg, A_ex)
    y_m, y_A = rel(m32, m_ex), rel(A32, A_ex)
    assert e_A <= 8 * y_A + 2e-6, (what, e_A, y_A)
    assert e_m <= 8 * y_m + 4e-6, (what, e_m, y_m)
    scale = abs(lp_ex) + len(y32) * 2.0 + float(np.abs(np.log(f64(s32))).sum())
    assert abs(got_lp - lp_ex) <= 8 * abs(float(lp32) - lp_ex) + 4e-6 * scale, (what, got_lp, lp_ex, lp32)


_SWEEP_D = [1, 5, 16, 64, 100, 128, 129, 200, 512]


def _kernels(D):
    return ["lds", "global"] if D <= 128 else ["global"]


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("noise", ["diagonal", "isotropic"])
@pytest.mark.parametrize("k", [1, 3, 16, 40])
@pytest.mark.parametrize("D,kernel", [(D, kn) for D in _SWEEP_D for kn in _kernels(D)])
def test_downdate_device_batched(B, opt, D, kernel, k, noise, dtype):
    import torch

    opt("NO_DOWNDATE_LDS", "1" if kernel == "global" else None)
    a = B._abi
    h = a.default_handle()
    rng = _rng(40 + D + 7 * k)
    nb = 3
    X, y, s, prior, post = _batch_problem(rng, nb, D, k, noise)
    dev = torch.device("cuda:0")
    tdt = torch.float64 if dtype == np.float64 else torch.float32
    Xd = torch.tensor(np.transpose(X, (0, 2, 1)).copy(), dtype=tdt, device=dev)  # [nb, k, D] row-major == D x k ColVecs
    yd = torch.tensor(y, dtype=tdt, device=dev)
    sd = torch.tensor(s, dtype=tdt, device=dev)
    mwd = torch.tensor(np.stack([p[0] for p in post]), dtype=tdt, device=dev)
    Td = torch.tensor(np.stack([p[1].T for p in post]), dtype=tdt, device=dev)  # column-major upper factors
    mp32 = mwd.cpu().numpy().copy()
    Tp32 = np.transpose(Td.cpu().numpy(), (0, 2, 1)).copy()
    lp = torch.zeros(nb, dtype=torch.float64, device=dev)
    info = torch.full((nb,), 7, dtype=torch.int32, device=dev)
    kind = a.NOISE_DIAGONAL if noise == "diagonal" else a.NOISE_ISOTROPIC
    torch.cuda.synchronize()
    h.downdate_factor(dtype, a.MEM_DEVICE, a.LAYOUT_COLVECS, nb, D, k, Xd.data_ptr(), D, k * D, yd.data_ptr(), k, kind,
                      sd.data_ptr(), k if noise == "diagonal" else 0, mwd.data_ptr(), D, Td.data_ptr(), D, D * D, lp.data_ptr(),
                      info.data_ptr())
    torch.cuda.synchronize()
    assert info.cpu().tolist() == [0] * nb
    for b in range(nb):
        sb = s[b] if noise == "diagonal" else np.full(k, s[0])
        Tg = Td[b].cpu().numpy().T
        if dtype == np.float32:
            sb32 = sb.astype(np.float32)
            _fp32_check(mp32[b], np.triu(Tp32[b]), X[b].astype(np.float32), sb32, y[b].astype(np.float32), mwd[b].cpu().numpy(), Tg,
                        lp[b].item(), f"D={D} k={k} {noise} {kernel}")
            continue
        m0, A0 = prior[b]
        _assert_state(mwd[b].cpu().numpy(), Tg, m0, A0)
        assert lp[b].item() == pytest.approx(O.logpdf_literal(m0, A0, X[b], sb, y[b]), rel=1e-9, abs=1e-9)


@pytest.mark.parametrize("kernel", ["lds", "global"])
@pytest.mark.parametrize("case", ["rowvecs", "shared_x", "host"])
def test_downdate_layouts_and_memspaces(B, opt, kernel, case):
    import torch

    opt("NO_DOWNDATE_LDS", "1" if kernel == "global" else None)
    a = B._abi
    h = a.default_handle()
    rng = _rng(90 + len(case))
    nb, D, k = 3, 24, 5
    X, y, s, prior, post = _batch_problem(rng, nb, D, k, "diagonal", shared_x=case == "shared_x")
    mw = np.stack([p[0] for p in post])
    T = np.stack([p[1].T for p in post])  # [nb, D, D]: row-major transpose == column-major factor
    lp = np.zeros(nb)
    info = np.full(nb, 7, dtype=np.int32)
    if case == "rowvecs":
        Xa = np.ascontiguousarray(X)  # [nb, D, k] row-major == k x D column-major (RowVecs), ldx = k
        layout, ldx, sX = a.LAYOUT_ROWVECS, k, D * k
    else:
        Xa = np.ascontiguousarray(np.transpose(X, (0, 2, 1)))
        layout, ldx, sX = a.LAYOUT_COLVECS, D, (0 if case == "shared_x" else D * k)
    if case == "host":
        mw_h, T_h = mw.copy(), T.copy()
        h.downdate_factor(np.float64, a.MEM_HOST, layout, nb, D, k, Xa, ldx, sX, y, k, a.NOISE_DIAGONAL, s, k, mw_h, D, T_h, D,
                          D * D, lp, info)
        got_m, got_T = mw_h, T_h
    else:
        dev = torch.device("cuda:0")
        t = lambda v: torch.tensor(v, dtype=torch.float64, device=dev)
        Xd, yd, sd, mwd, Td = t(Xa), t(y), t(s), t(mw), t(T)
        lpd = torch.zeros(nb, dtype=torch.float64, device=dev)
        infod = torch.full((nb,), 7, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        h.downdate_factor(np.float64, a.MEM_DEVICE, layout, nb, D, k, Xd.data_ptr(), ldx, sX, yd.data_ptr(), k, a.NOISE_DIAGONAL,
                          sd.data_ptr(), k, mwd.data_ptr(), D, Td.data_ptr(), D, D * D, lpd.data_ptr(), infod.data_ptr())
        torch.cuda.synchronize()
        got_m, got_T, lp, info = mwd.cpu().numpy(), Td.cpu().numpy(), lpd.cpu().numpy(), infod.cpu().numpy()
    assert info.tolist() == [0] * nb
    for b in range(nb):
        m0, A0 = prior[b]
        Xb = X[0 if case == "shared_x" else b]
        _assert_state(got_m[b], got_T[b].T, m0, A0)
        assert lp[b] == pytest.approx(O.logpdf_literal(m0, A0, Xb, s[b], y[b]), rel=1e-9, abs=1e-9)


def test_downdate_zero_observations_is_a_no_op(B, opt):
    import torch

    a = B._abi
    h = a.default_handle()
    rng = _rng(95)
    for kernel, D in (("lds", 33), ("global", 33), ("global", 150)):
        opt("NO_DOWNDATE_LDS", "1" if kernel == "global" else None)
        m0, U = _prior(rng, D)
        mwd = torch.tensor(m0, device="cuda:0")
        Td = torch.tensor(U.T.copy(), device="cuda:0")
        m_before, T_before = mwd.clone(), Td.clone()
        lp = torch.full((1,), 5.0, dtype=torch.float64, device="cuda:0")
        info = torch.full((1,), 7, dtype=torch.int32, device="cuda:0")
        sd = torch.ones(1, dtype=torch.float64, device="cuda:0")
        torch.cuda.synchronize()
        h.downdate_factor(np.float64, a.MEM_DEVICE, a.LAYOUT_COLVECS, 1, D, 0, None, D, 0, None, 0, a.NOISE_ISOTROPIC, sd.data_ptr(),
                          0, mwd.data_ptr(), 0, Td.data_ptr(), D, 0, lp.data_ptr(), info.data_ptr())
        torch.cuda.synchronize()
        assert info.item() == 0 and lp.item() == 0.0
        assert torch.equal(mwd, m_before) and torch.equal(Td, T_before)


# ---- 5. failure ----------------------------------------------------------------------------------------------------------
def _single(B, h, D, T, x, s, y=None, mw=None, kind=None):
    import torch

    a = B._abi
    k = x.shape[1]
    dev = torch.device("cuda:0")
    Td = torch.tensor(T.T.copy(), dtype=torch.float64, device=dev)
    mwd = torch.tensor(np.zeros(D) if mw is None else mw, dtype=torch.float64, device=dev)
    Xd = torch.tensor(x.T.copy(), dtype=torch.float64, device=dev)
    yd = torch.tensor(np.zeros(k) if y is None else y, dtype=torch.float64, device=dev)
    sd = torch.tensor(s, dtype=torch.float64, device=dev)
    lp = torch.zeros(1, dtype=torch.float64, device=dev)
    info = torch.full((1,), 77, dtype=torch.int32, device=dev)
    T0, m0 = Td.clone(), mwd.clone()
    torch.cuda.synchronize()
    h.downdate_factor(np.float64, a.MEM_DEVICE, a.LAYOUT_COLVECS, 1, D, k, Xd.data_ptr(), D, 0, yd.data_ptr(), 0,
                      kind if kind is not None else a.NOISE_DIAGONAL, sd.data_ptr(), 0, mwd.data_ptr(), 0, Td.data_ptr(), D, 0,
                      lp.data_ptr(), info.data_ptr())
    torch.cuda.synchronize()
    return info.item(), lp.item(), torch.equal(Td, T0) and torch.equal(mwd, m0)


@pytest.mark.parametrize("kernel", ["lds", "global"])
def test_downdate_failure_codes_and_untouched_state(B, opt, kernel):
    opt("NO_DOWNDATE_LDS", "1" if kernel == "global" else None)
    h = B._abi.default_handle()
    D = 9
    x = np.array([[0.5, 0.5, 0.5, 0.6, 0.1, 0.0, 0.0, 0.0, 0.0]]).T  # prefix sums of x^2: .25 .5 .75 1.11 ...
    info, lp, same = _single(B, h, D, np.eye(D), x, np.ones(1))
    assert (info, np.isnan(lp), same) == (4, True, True)
    # the failure of a LATER observation leaves the state as it was too (the first one alone would succeed)
    x2 = np.hstack([0.3 * np.eye(D)[:, :1], x])
    info, lp, same = _single(B, h, D, np.eye(D), x2, np.ones(2))
    assert (info, np.isnan(lp), same) == (4, True, True)
    # a bad variance: its 1-based index, checked before any removal
    x3 = 0.1 * np.ones((D, 3))
    info, lp, same = _single(B, h, D, 2 * np.eye(D), x3, np.array([0.5, 1.0, -0.2]))
    assert (info, np.isnan(lp), same) == (3, True, True)
    # a bad diagonal entry of the factor: its index, and it wins over the bad variance
    Tbad = 2 * np.eye(D)
    Tbad[5, 5] = -1.0
    info, lp, same = _single(B, h, D, Tbad, x3, np.array([0.5, 1.0, -0.2]))
    assert (info, np.isnan(lp), same) == (6, True, True)


@pytest.mark.parametrize("kernel", ["lds", "global"])
def test_downdate_failing_regressor_in_a_batch(B, opt, kernel):
    import torch

    opt("NO_DOWNDATE_LDS", "1" if kernel == "global" else None)
    a = B._abi
    h = a.default_handle()
    rng = _rng(96)
    nb, D, k = 5, 12, 2
    X, y, s, prior, post = _batch_problem(rng, nb, D, k, "diagonal")
    X[2] *= 40.0  # regressor 2 removes far more than it holds
    dev = torch.device("cuda:0")
    t = lambda v: torch.tensor(v, dtype=torch.float64, device=dev)
    Xd, yd, sd = t(np.transpose(X, (0, 2, 1)).copy()), t(y), t(s)
    mwd = t(np.stack([p[0] for p in post]))
    Td = t(np.stack([p[1].T for p in post]))
    T2, m2 = Td[2].clone(), mwd[2].clone()
    lp = torch.zeros(nb, dtype=torch.float64, device=dev)
    info = torch.zeros(nb, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    h.downdate_factor(np.float64, a.MEM_DEVICE, a.LAYOUT_COLVECS, nb, D, k, Xd.data_ptr(), D, k * D, yd.data_ptr(), k,
                      a.NOISE_DIAGONAL, sd.data_ptr(), k, mwd.data_ptr(), D, Td.data_ptr(), D, D * D, lp.data_ptr(), info.data_ptr())
    torch.cuda.synchronize()
    inf = info.cpu().tolist()
    assert inf[2] > 0 and [inf[b] for b in (0, 1, 3, 4)] == [0] * 4
    assert np.isnan(lp[2].item()) and torch.equal(Td[2], T2) and torch.equal(mwd[2], m2)
    for b in (0, 1, 3, 4):
        m0, A0 = prior[b]
        _assert_state(mwd[b].cpu().numpy(), Td[b].cpu().numpy().T, m0, A0)
        assert lp[b].item() == pytest.approx(O.logpdf_literal(m0, A0, X[b], s[b], y[b]), rel=1e-9, abs=1e-9)


def test_forget_raises_and_keeps_the_state(B):
    D = 9
    st = B.ResidentPosterior(B.BayesianLinearRegressor(np.zeros(D), B.Diagonal(np.ones(D))))
    m0, T0 = st.state()
    x = np.array([[0.5, 0.5, 0.5, 0.6, 0.1, 0.0, 0.0, 0.0, 0.0]]).T
    with pytest.raises(B._abi.PosDefException) as e:
        st.forget(x, 1.0, np.zeros(1))
    assert e.value.info == 4
    m1, T1 = st.state()
    assert np.array_equal(m0, m1) and np.array_equal(T0, T1)
    with pytest.raises(NotImplementedError):
        st.forget(0.1 * np.ones((D, 2)), np.eye(2), np.zeros(2))


# ---- 6. reproducibility --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,kernel", [(100, "lds"), (100, "global"), (200, "global")])
def test_downdate_bits_do_not_depend_on_the_batch(B, opt, D, kernel):
    import torch

    opt("NO_DOWNDATE_LDS", "1" if kernel == "global" else None)
    a = B._abi
    h = a.default_handle()
    rng = _rng(97 + D)
    nb, k = 8, 3
    X, y, s, prior, post = _batch_problem(rng, nb, D, k, "diagonal")
    dev = torch.device("cuda:0")
    t = lambda v: torch.tensor(v, dtype=torch.float64, device=dev)
    Xd, yd, sd = t(np.transpose(X, (0, 2, 1)).copy()), t(y), t(s)
    mw0 = t(np.stack([p[0] for p in post]))
    T0 = t(np.stack([p[1].T for p in post]))

    def run(sl):
        n = len(range(nb)[sl])
        mwd, Td = mw0[sl].clone(), T0[sl].clone()
        lp = torch.zeros(n, dtype=torch.float64, device=dev)
        info = torch.zeros(n, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        h.downdate_factor(np.float64, a.MEM_DEVICE, a.LAYOUT_COLVECS, n, D, k, Xd[sl].contiguous().data_ptr(), D, k * D,
                          yd[sl].contiguous().data_ptr(), k, a.NOISE_DIAGONAL, sd[sl].contiguous().data_ptr(), k, mwd.data_ptr(), D,
                          Td.data_ptr(), D, D * D, lp.data_ptr(), info.data_ptr())
        torch.cuda.synchronize()
        assert info.cpu().tolist() == [0] * n
        return mwd, Td, lp

    m_a, T_a, lp_a = run(slice(0, nb))
    m_b, T_b, lp_b = run(slice(0, nb))
    assert torch.equal(m_a, m_b) and torch.equal(T_a, T_b) and torch.equal(lp_a, lp_b)
    m_1, T_1, lp_1 = run(slice(3, 4))
    assert torch.equal(m_1[0], m_a[3]) and torch.equal(T_1[0], T_a[3]) and torch.equal(lp_1[0], lp_a[3])


# ---- 7. basis functions --------------------------------------------------------------------------------------------------
def test_forget_through_random_fourier_features(B):
    rng = _rng(98)
    D, Din, N = 24, 3, 15
    Xin = rng.standard_normal((Din, N))
    Om = rng.standard_normal((Din, D))
    beta = 2 * np.pi * rng.random(D)
    rff = B.RandomFourierFeatures(Om, beta)
    mw = 0.1 * rng.standard_normal(D)
    dvec = np.exp(0.2 * rng.standard_normal(D))
    s = np.exp(0.3 * rng.standard_normal(N))
    y = rng.standard_normal(N)
    bfr = B.BasisFunctionRegressor(B.BayesianLinearRegressor(mw, B.Diagonal(dvec)), rff)
    st = B.ResidentPosterior(bfr)
    st.condition(B.ColVecs(np.asfortranarray(Xin)), B.Diagonal(s), y)
    idx = [0, 4, 5, 12]
    rest = [i for i in range(N) if i not in idx]
    lp = st.forget(B.ColVecs(np.asfortranarray(Xin[:, idx])), B.Diagonal(s[idx]), y[idx])
    Phi = rff(B.ColVecs(np.asfortranarray(Xin))).X
    mw_o, _, L_o = O.posterior_literal(mw, dvec, Phi[:, rest], s[rest], y[rest])
    m1, T1 = st.state()
    _assert_state(m1, T1, mw_o, L_o)
    lp_o = O.logpdf_literal(mw, dvec, Phi, s, y) - O.logpdf_literal(mw, dvec, Phi[:, rest], s[rest], y[rest])
    assert lp == pytest.approx(lp_o, rel=1e-9, abs=1e-10)
    assert isinstance(st.regressor(), B.BasisFunctionRegressor)
