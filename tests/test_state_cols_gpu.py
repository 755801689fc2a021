"""Update / downdate of a resident multi-output state (blr_update_multi_factor_*, blr_downdate_multi_factor_*,
ResidentColumnsPosterior) against the CPU oracle per column, the single-column entry points bit for bit on column 0,
and the bit promises of the header.  All tests need an MI355X."""
import numpy as np
import pytest

from oracle import blr_oracle as O

pytestmark = pytest.mark.gpu

RTOL = 1e-9  # tests/test_downdate_gpu.py


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
    return np.random.Generator(np.random.PCG64(9191 + i))


def _upper(A):
    return np.linalg.cholesky(A).T


def _prior(rng, D, S):
    U = np.triu(rng.standard_normal((D, D))) * (0.3 / np.sqrt(D))
    U[np.diag_indices(D)] = 1.0 + np.abs(U[np.diag_indices(D)])
    return rng.standard_normal((S, D)), U


def _assert_state(mw_got, T_got, mw_o, A_o, rtol=RTOL):
    T_got = np.triu(np.asarray(T_got, dtype=np.float64))
    assert np.all(np.diag(T_got) > 0)
    np.testing.assert_allclose(T_got.T @ T_got, A_o, rtol=rtol, atol=rtol * np.abs(A_o).max())
    np.testing.assert_allclose(mw_got, mw_o, rtol=50 * rtol, atol=rtol * np.abs(mw_o).max())


_PROBLEMS = {}


def _problem(seed, nb, D, k, S, noise, shared_x=False):
    """Per regressor b: the state WITHOUT the k observations (means m0[b] (S, D), factor U0[b]) and the state WITH them, from the
    oracle (mp[b] (S, D), Tp[b]); X [nb or 1, D, k], Y [nb, S, k], s [nb, k] or [1]; lp[b, c] = log p(Y_c | state without).  The
    reference is computed once per shape and shared (callers copy what they change)."""
    key = (seed, nb, D, k, S, noise, shared_x)
    if key in _PROBLEMS:
        return _PROBLEMS[key]
    rng = _rng(seed)
    nx = 1 if shared_x else nb
    X = rng.standard_normal((nx, D, k)) * (0.7 / np.sqrt(max(k, 1)))
    Y = rng.standard_normal((nb, S, k))
    s = np.exp(0.3 * rng.standard_normal((nb, k))) if noise == "diagonal" else np.full((1,), 0.37)
    m0, U0, mp, Tp, lp = [], [], [], [], np.zeros((nb, S))
    for b in range(nb):
        m, U = _prior(rng, D, S)
        sb = s[b] if noise == "diagonal" else np.full(k, s[0])
        Xb = X[0 if shared_x else b]
        A0 = U.T @ U
        cols = [O.posterior_literal(m[c], A0, Xb, sb, Y[b, c]) for c in range(S)]
        lp[b] = [O.logpdf_literal(m[c], A0, Xb, sb, Y[b, c]) for c in range(S)]
        m0.append(m); U0.append(U)
        mp.append(np.stack([c[0] for c in cols])); Tp.append(_upper(cols[0][2]))
    out = dict(X=X, Y=Y, s=s, m0=np.stack(m0), U0=np.stack(U0), mp=np.stack(mp), Tp=np.stack(Tp), lp=lp)
    for v in out.values():
        v.setflags(write=False)
    _PROBLEMS[key] = out
    return out


def _run(B, down, dtype, X, Y, s, M, T, S=None, memspace="device", layout="col", logpdf=True, pad=0, info_fill=7, asynchronous=False):
    """One call.  X [nx, D, k], Y [nb, >= S, k], s [nb, k] | [1], M [nb, >= S, D] (means as rows), T [nb, D, D] upper factors.  The
    first S columns are used.  `pad` widens ldx, ldY, ldm and ldt.  -> (M (nb, S, D), T (nb, D, D) upper, lp (nb, S), info (nb,))"""
    import torch

    a = B._abi
    h = a.default_handle()
    nb, D = M.shape[0], M.shape[2]
    k = X.shape[2]
    S = M.shape[1] if S is None else S
    nx = X.shape[0]
    diag = s.ndim == 2
    ldx = (D if layout == "col" else max(k, 1)) + pad
    ldY, ldm, ldt = max(k, 1) + pad, D + pad, D + pad
    fill = -77.0
    if layout == "col":
        Xa = np.full((nx, max(k, 1), ldx), fill); Xa[:, :k, :D] = np.transpose(X, (0, 2, 1))
    else:
        Xa = np.full((nx, D, ldx), fill); Xa[:, :, :k] = X
    Ya = np.full((nb, max(S, 1), ldY), fill); Ya[:, :S, :k] = Y[:, :S]
    Ma = np.full((nb, max(S, 1), ldm), fill); Ma[:, :S, :D] = M[:, :S]
    Ta = np.full((nb, D, ldt), fill); Ta[:, :, :D] = np.transpose(np.triu(T), (0, 2, 1))
    # (the strictly-lower part of the stored factor is not read: give it a value that would be found in the results)
    low = np.tril(np.ones((D, D), dtype=bool), -1)  # T[i, j], i > j, lives at Ta[:, j, i]
    for b in range(nb):
        Ta[b, :, :D][low.T] = fill
    Xa, Ya, Ma, Ta, sa = (np.ascontiguousarray(v, dtype=dtype) for v in (Xa, Ya, Ma, Ta, s))
    lp = np.full((nb, max(S, 1)), 5.0)
    info = np.full(nb, info_fill, dtype=np.int32)
    args = lambda p: (dtype, a.MEM_HOST if memspace == "host" else a.MEM_DEVICE, a.LAYOUT_COLVECS if layout == "col" else a.LAYOUT_ROWVECS,
                      nb, D, k, S, p(Xa), ldx, 0 if nx == 1 and nb > 1 else Xa[0].size, p(Ya), ldY, Ya[0].size, a.NOISE_DIAGONAL if diag else a.NOISE_ISOTROPIC,
                      p(sa), k if diag else 0, p(Ma), ldm, Ma[0].size, p(Ta), ldt, Ta[0].size, p(lp) if logpdf else None, lp[0].size, p(info))
    fn = h.downdate_multi_factor if down else h.update_multi_factor
    if memspace == "host":
        fn(*args(lambda v: v))
    else:
        keep = []

        def up(v):
            keep.append(torch.tensor(v, device="cuda:0"))
            return keep[-1].data_ptr()

        torch.cuda.synchronize()
        if asynchronous:
            h.set_async(True)
        try:
            fn(*args(up))
        finally:
            if asynchronous:
                h.synchronize()
                h.set_async(False)
        torch.cuda.synchronize()
        got = [t.cpu().numpy() for t in keep]
        Ma, Ta = got[3], got[4]
        lp = got[5] if logpdf else lp
        info = got[-1]
    assert np.all(Ma[:, :S, D:] == dtype(fill)) and np.all(Ta[:, :, D:] == dtype(fill))  # the padding keeps its bits
    for b in range(nb):  # the strictly-lower part keeps its bits or is zeroed (the update's re-factorisation route, blr_update_factor_*)
        assert np.all((Ta[b, :, :D][low.T] == dtype(fill)) | (Ta[b, :, :D][low.T] == 0))
    Tg = np.triu(np.transpose(Ta[:, :, :D], (0, 2, 1)))
    return Ma[:, :S, :D].copy(), Tg, lp[:, :S].copy(), info.copy()


def _start_and_goal(p, down):
    return (p["mp"], p["Tp"], p["m0"], p["U0"]) if down else (p["m0"], p["U0"], p["mp"], p["Tp"])


def _exact_step(sign, m, T, X, s, y):
    """fp64 update (+1) / downdate (-1) of the (rounded) inputs"""
    A0 = T.T @ T
    A = A0 + sign * (X / s) @ X.T
    return np.linalg.solve(A, A0 @ m + sign * (X / s) @ y), A


def _fp32_check(sign, m32, T32, X32, s32, y32, got_m, got_T, got_lp, what):
    """tests/test_downdate_gpu.py's yardstick, for either direction: 8 x the error of the same step in fp32 LAPACK plus its floors"""
    f64 = lambda v: np.asarray(v, dtype=np.float64)
    m_ex, A_ex = _exact_step(sign, f64(m32), f64(T32), f64(X32), f64(s32), f64(y32))
    A32 = T32.T @ T32 + np.float32(sign) * (X32 / s32) @ X32.T
    m32n = np.linalg.solve(A32, (T32.T @ T32) @ m32 + np.float32(sign) * (X32 / s32) @ y32)
    if sign > 0:  # log p(y | state before the call)
        lp_ex = O.logpdf_literal(f64(m32), f64(T32).T @ f64(T32), f64(X32), f64(s32), f64(y32))
        lp32 = O.logpdf_literal(m32, T32.T @ T32, X32, s32, y32)
    else:  # log p(y | state after the call)
        lp_ex = O.logpdf_literal(m_ex, A_ex, f64(X32), f64(s32), f64(y32))
        lp32 = O.logpdf_literal(m32n, A32, X32, s32, y32)
    rel = lambda u, v: float(np.abs(f64(u) - v).max() / max(np.abs(v).max(), 1e-30))
    Tg = np.triu(f64(got_T))
    e_m, e_A = rel(got_m, m_ex), rel(Tg.T @ Tg, A_ex)
    y_m, y_A = rel(m32n, m_ex), rel(A32, A_ex)
    print(what, "e_A", e_A, "y_A", y_A, "e_m", e_m, "y_m", y_m, "lp", got_lp, lp_ex, float(lp32))
    assert e_A <= 8 * y_A + 2e-6, (what, e_A, y_A)
    assert e_m <= 8 * y_m + 4e-6, (what, e_m, y_m)
    scale = abs(lp_ex) + len(y32) * 2.0 + float(np.abs(np.log(f64(s32))).sum())
    assert abs(got_lp - lp_ex) <= 8 * abs(float(lp32) - lp_ex) + 4e-6 * scale, (what, got_lp, lp_ex, lp32)


def _check_against_oracle(p, down, dtype, S, got, what, regs=None):
    Mg, Tg, lp, info = got
    nb = Mg.shape[0]
    m_start, T_start, m_goal, T_goal = _start_and_goal(p, down)
    for b in (range(nb) if regs is None else regs):
        assert info[b] == 0, (what, b, info)
        Xb = p["X"][0 if p["X"].shape[0] == 1 else b]
        sb = p["s"][b] if p["s"].ndim == 2 else np.full(Xb.shape[1], p["s"][0])
        for c in range(S):
            if dtype == np.float32:
                f32 = lambda v: np.asarray(v, dtype=np.float32)
                _fp32_check(-1.0 if down else 1.0, f32(m_start[b, c]), f32(np.triu(T_start[b])), f32(Xb), f32(sb), f32(p["Y"][b, c]), Mg[b, c],
                            Tg[b], lp[b, c], f"{what} b={b} c={c}")
            else:
                _assert_state(Mg[b, c], Tg[b], m_goal[b, c], T_goal[b].T @ T_goal[b])
                assert lp[b, c] == pytest.approx(p["lp"][b, c], rel=1e-9, abs=1e-9), (what, b, c)


# ---- 1. every column against the oracle ------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("noise", ["diagonal", "isotropic"])
@pytest.mark.parametrize("k", [1, 3, 16, 17, 40])
@pytest.mark.parametrize("D", [1, 33, 100, 128])
@pytest.mark.parametrize("down", [False, True])
def test_columns_against_the_oracle(B, opt, down, D, k, noise, dtype):
    W = B._abi.STATE_COLS_PER_PASS
    p = _problem(100 + D + 7 * k, 3, D, k, W + 1, noise)
    m_start, T_start, _, _ = _start_and_goal(p, down)
    sweeps = ["always", "never"] if (not down and k <= 16) else [None]  # (can_sweep: D <= 128 and k <= 16)
    for sweep in sweeps:
        opt("SWEEP", sweep)
        for S in (1, 2, W, W + 1):
            got = _run(B, down, dtype, p["X"], p["Y"], p["s"], m_start, T_start, S=S)
            _check_against_oracle(p, down, dtype, S, got, f"down={down} D={D} k={k} S={S} {noise} sweep={sweep}")


# ---- 2. round trip and drift ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [7, 128])
def test_condition_then_forget_round_trip(B, D):
    p = _problem(200 + D, 3, D, 5, 5, "diagonal")
    M1, T1, lp_up, info = _run(B, False, np.float64, p["X"], p["Y"], p["s"], p["m0"], p["U0"])
    assert info.tolist() == [0] * 3
    M2, T2, lp_dn, info = _run(B, True, np.float64, p["X"], p["Y"], p["s"], M1, T1)
    assert info.tolist() == [0] * 3
    for b in range(3):
        for c in range(5):
            _assert_state(M2[b, c], T2[b], p["m0"][b, c], p["U0"][b].T @ p["U0"][b])
    np.testing.assert_allclose(lp_dn, lp_up, rtol=1e-9, atol=1e-10)
    np.testing.assert_allclose(lp_up, p["lp"], rtol=1e-9, atol=1e-9)


@pytest.mark.parametrize("D", [16, 128])
def test_sliding_window_does_not_drift(B, D):
    """40 steps of (newest observation in, oldest out) with S = 5; bound: tests/test_downdate_gpu.py::test_sliding_window_does_not_drift"""
    rng = _rng(300 + D)
    W, steps, S = 40, 40, 5
    N = W + steps
    mw = rng.standard_normal(D)
    Lw = np.exp(0.2 * rng.standard_normal(D))
    X = rng.standard_normal((D, N)) / np.sqrt(D)
    s = np.exp(0.3 * rng.standard_normal(N))
    Y = rng.standard_normal((N, S))
    f = B.BayesianLinearRegressor(mw, B.Diagonal(Lw))
    st = B.ResidentColumnsPosterior(B.posterior_columns(f(X[:, :W], B.Diagonal(s[:W])), Y[:W]))
    for t in range(steps):
        new, old = slice(W + t, W + t + 1), slice(t, t + 1)
        st.condition(X[:, new], B.Diagonal(s[new]), Y[new])
        lp = st.forget(X[:, old], B.Diagonal(s[old]), Y[old])
        assert lp.shape == (S,) and np.all(np.isfinite(lp))
    Mg, Tg = st.state()
    old, win = slice(steps - 1, steps), slice(N - W, N)
    for c in range(S):
        mw_o, _, L_o = O.posterior_literal(mw, Lw, X[:, win], s[win], Y[win, c])
        _assert_state(Mg[:, c], Tg, mw_o, L_o)
        # the last step's value: log p(y_old | the window without it)
        lo = O.logpdf_literal(mw, Lw, np.hstack([X[:, old], X[:, win]]), np.concatenate([s[old], s[win]]), np.concatenate([Y[old, c], Y[win, c]]))
        assert lp[c] == pytest.approx(lo - O.logpdf_literal(mw, Lw, X[:, win], s[win], Y[win, c]), rel=1e-8, abs=1e-9)


# ---- 3. column 0 is the single-column entry point, bit for bit -------------------------------------------------------------------
def _single(B, down, dtype, X, y, s, m, T):
    """blr_update_factor_* / blr_downdate_factor_* on device operands: X [nb, D, k], y [nb, k], m [nb, D], T [nb, D, D] upper"""
    import torch

    a = B._abi
    h = a.default_handle()
    nb, D, k = X.shape
    diag = s.ndim == 2
    t = lambda v: torch.tensor(np.ascontiguousarray(v, dtype=dtype), device="cuda:0")
    Xd, yd, sd, md, Td = t(np.transpose(X, (0, 2, 1))), t(y), t(s), t(m), t(np.transpose(np.triu(T), (0, 2, 1)))
    lp = torch.zeros(nb, dtype=torch.float64, device="cuda:0")
    info = torch.full((nb,), 7, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    (h.downdate_factor if down else h.update_factor)(dtype, a.MEM_DEVICE, a.LAYOUT_COLVECS, nb, D, k, Xd.data_ptr(), D, D * k, yd.data_ptr(), k,
                                                     a.NOISE_DIAGONAL if diag else a.NOISE_ISOTROPIC, sd.data_ptr(), k if diag else 0,
                                                     md.data_ptr(), D, Td.data_ptr(), D, D * D, lp.data_ptr(), info.data_ptr())
    torch.cuda.synchronize()
    return md.cpu().numpy(), np.triu(np.transpose(Td.cpu().numpy(), (0, 2, 1))), lp.cpu().numpy(), info.cpu().numpy()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("D,k", [(33, 1), (128, 1), (100, 5), (200, 3)])
@pytest.mark.parametrize("down", [False, True])
def test_column_zero_is_the_single_column_entry_point(B, down, D, k, dtype):
    p = _problem(400 + D + k, 3, D, k, 9, "diagonal")
    m_start, T_start, _, _ = _start_and_goal(p, down)
    m1, T1, lp1, info1 = _single(B, down, dtype, p["X"], p["Y"][:, 0], p["s"], m_start[:, 0], T_start)
    for S in (1, 9):
        Mg, Tg, lp, info = _run(B, down, dtype, p["X"], p["Y"], p["s"], m_start, T_start, S=S)
        assert np.array_equal(Mg[:, 0], m1) and np.array_equal(Tg, T1) and np.array_equal(info, info1) and info.tolist() == [0] * 3
        assert np.array_equal(lp[:, 0], lp1)


# ---- 4. bit promises -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [100, 200])
@pytest.mark.parametrize("down", [False, True])
def test_bits_do_not_depend_on_the_batch_the_position_or_the_other_columns(B, down, D):
    W = B._abi.STATE_COLS_PER_PASS
    S = 2 * W + 3
    p = _problem(500 + D, 4, D, 3, S, "diagonal")
    m_start, T_start, _, _ = _start_and_goal(p, down)
    run = lambda X, Y, s, M, T, **kw: _run(B, down, np.float64, X, Y, s, M, T, **kw)
    ref = run(p["X"], p["Y"], p["s"], m_start, T_start)
    again = run(p["X"], p["Y"], p["s"], m_start, T_start)  # restored state, repeated call
    assert all(np.array_equal(u, v) for u, v in zip(ref, again))
    # a regressor alone against the same regressor inside the batch
    one = run(p["X"][2:3], p["Y"][2:3], p["s"][2:3], m_start[2:3], T_start[2:3])
    assert all(np.array_equal(u[0], v[2]) for u, v in zip(one, ref))
    # column 1 moved into the last pass (and S changed): the same bits
    perm = np.arange(S)
    perm[1], perm[S - 1] = S - 1, 1
    moved = run(p["X"], p["Y"][:, perm], p["s"], m_start[:, perm], T_start)
    assert np.array_equal(moved[0][:, S - 1], ref[0][:, 1]) and np.array_equal(moved[2][:, S - 1], ref[2][:, 1])
    short = run(p["X"], p["Y"], p["s"], m_start, T_start, S=3)
    assert np.array_equal(short[0], ref[0][:, :3]) and np.array_equal(short[2], ref[2][:, :3]) and np.array_equal(short[1], ref[1])
    # the other columns' data changed (column 0 included: its factor does not involve Y)
    Y2 = p["Y"].copy()
    Y2[:, :5] += 1.0
    Y2[:, 6:] *= -2.0
    other = run(p["X"], Y2, p["s"], m_start, T_start)
    assert np.array_equal(other[0][:, 5], ref[0][:, 5]) and np.array_equal(other[2][:, 5], ref[2][:, 5]) and np.array_equal(other[1], ref[1])
    # host memspace, and an asynchronous handle, against the synchronous device call
    host = run(p["X"], p["Y"], p["s"], m_start, T_start, memspace="host")
    assert all(np.array_equal(u, v) for u, v in zip(ref, host))
    if D <= 128:
        asy = run(p["X"], p["Y"], p["s"], m_start, T_start, asynchronous=True)
        assert all(np.array_equal(u, v) for u, v in zip(ref, asy))


# ---- 5. failures -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [12, 150])
@pytest.mark.parametrize("case", ["factor", "noise", "indefinite"])
def test_a_failing_regressor_keeps_its_bits(B, case, D):
    down = case == "indefinite"
    S, k = 4, 2
    p = _problem(600 + D, 3, D, k, S, "diagonal")
    m_start, T_start, _, _ = (np.array(v) for v in _start_and_goal(p, down))
    X, s = np.array(p["X"]), np.array(p["s"])
    if case == "factor":
        T_start[1, 4, 4] = -1.0
        want = 5
    elif case == "noise":
        s[1, 1] = -0.2
        want = 2
    else:
        X[1] *= 40.0  # regressor 1 removes far more than it holds
        want = None
    for d in ([False, True] if case != "indefinite" else [True]):
        ms, Ts = (m_start, T_start) if d == down else (np.array(v) for v in _start_and_goal(p, d)[:2])
        if d != down and case == "factor":
            Ts[1, 4, 4] = -1.0
        Mg, Tg, lp, info = _run(B, d, np.float64, X, p["Y"], s, ms, Ts)
        m1, T1, lp1, info1 = _single(B, d, np.float64, X, p["Y"][:, 0], s, ms[:, 0], Ts)
        assert info.tolist() == info1.tolist() and info[1] > 0 and info[0] == 0 and info[2] == 0
        assert want is None or info[1] == want
        assert np.array_equal(Mg[1], ms[1]) and np.array_equal(Tg[1], np.triu(Ts[1])) and np.all(np.isnan(lp[1]))
        _check_against_oracle(p, d, np.float64, S, (Mg, Tg, lp, info), f"{case} down={d}", regs=(0, 2))


# ---- 6. no-ops and layouts -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("down", [False, True])
def test_no_ops_and_layouts(B, down):
    D, k, S = 24, 5, 4
    p = _problem(700, 3, D, k, S, "diagonal")
    m_start, T_start, _, _ = _start_and_goal(p, down)
    for memspace in ("device", "host"):
        # k = 0: every evidence 0, status 0, the state keeps its bits
        Mg, Tg, lp, info = _run(B, down, np.float64, p["X"][:, :, :0], p["Y"][:, :, :0], p["s"], m_start, T_start, memspace=memspace)
        assert np.array_equal(Mg, m_start) and np.array_equal(Tg, np.triu(T_start)) and np.all(lp == 0.0) and info.tolist() == [0] * 3
        # S = 0: nothing is touched, the status included
        Mg, Tg, lp, info = _run(B, down, np.float64, p["X"], p["Y"], p["s"], m_start, T_start, S=0, memspace=memspace, info_fill=7)
        assert np.array_equal(Tg, np.triu(T_start)) and info.tolist() == [7] * 3
        # RowVecs and padded ldx / ldY / ldm / ldt
        for layout in ("col", "row"):
            got = _run(B, down, np.float64, p["X"], p["Y"], p["s"], m_start, T_start, layout=layout, pad=3, memspace=memspace)
            _check_against_oracle(p, down, np.float64, S, got, f"{layout} padded {memspace}")
    # NULL logpdf
    Mg, Tg, lp, info = _run(B, down, np.float64, p["X"], p["Y"], p["s"], m_start, T_start, logpdf=False)
    _check_against_oracle(p, down, np.float64, S, (Mg, Tg, p["lp"], info), "NULL logpdf")
    # strideX = 0 with strideY != 0: one design matrix, a target block per regressor
    q = _problem(701, 3, D, k, S, "diagonal", shared_x=True)
    ms, Ts, _, _ = _start_and_goal(q, down)
    _check_against_oracle(q, down, np.float64, S, _run(B, down, np.float64, q["X"], q["Y"], q["s"], ms, Ts), "shared X")


# ---- 7. large D: the slow route ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("k", [1, 5])
@pytest.mark.parametrize("down", [False, True])
def test_large_d(B, down, k, dtype):
    p = _problem(800 + k, 3, 200, k, 3, "diagonal")
    m_start, T_start, _, _ = _start_and_goal(p, down)
    _check_against_oracle(p, down, dtype, 3, _run(B, down, dtype, p["X"], p["Y"], p["s"], m_start, T_start), f"D=200 k={k} down={down}")


# ---- 8. ResidentColumnsPosterior -----------------------------------------------------------------------------------------------
def test_resident_columns_posterior_against_the_columns(B):
    rng = _rng(900)
    D, N, S, k = 20, 30, 4, 3
    X = rng.standard_normal((D, N)) / np.sqrt(D)
    s = np.exp(0.3 * rng.standard_normal(N))
    Y = rng.standard_normal((N, S))
    f = B.BayesianLinearRegressor(rng.standard_normal(D), B.Diagonal(np.exp(0.2 * rng.standard_normal(D))))
    first, new = slice(0, N - k), slice(N - k, N)
    fs = B.posterior_columns(f(X[:, first], B.Diagonal(s[first])), Y[first])
    st = B.ResidentColumnsPosterior(fs)
    singles = [B.ResidentPosterior(fc) for fc in fs]
    lp = st.condition(X[:, new], B.Diagonal(s[new]), Y[new])
    lp1 = [r.condition(X[:, new], B.Diagonal(s[new]), Y[new, c]) for c, r in enumerate(singles)]
    np.testing.assert_allclose(lp, lp1, rtol=1e-9, atol=1e-12)
    Xt = rng.standard_normal((D, 7))
    m, v = st.mean_and_var(Xt, 0.1)
    for c, r in enumerate(singles):
        mc, vc = B.mean_and_var(r.regressor()(Xt, 0.1))
        np.testing.assert_allclose(m[:, c], mc, rtol=1e-9, atol=1e-12)
        np.testing.assert_allclose(v, vc, rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(st.mean(Xt), m, rtol=1e-12, atol=1e-14)
    old = slice(0, 2)
    lp = st.forget(X[:, old], B.Diagonal(s[old]), Y[old])
    lp1 = [r.forget(X[:, old], B.Diagonal(s[old]), Y[old, c]) for c, r in enumerate(singles)]
    np.testing.assert_allclose(lp, lp1, rtol=1e-9, atol=1e-12)
    regs = st.regressors()
    assert len(regs) == S and all(r.Lw is regs[0].Lw for r in regs) and isinstance(regs[0].Lw, B.PDMat)
    Mg, Tg = st.state()
    for c, r in enumerate(singles):
        m1, T1 = r.state()
        np.testing.assert_allclose(Mg[:, c], m1, rtol=1e-9, atol=1e-12)
        np.testing.assert_allclose(Tg.T @ Tg, T1.T @ T1, rtol=1e-9, atol=1e-12)
    # a prior regressor plus S; columns that do not share their precision are refused
    pr = B.ResidentColumnsPosterior(f, S=3)
    assert pr.state()[0].shape == (D, 3)
    with pytest.raises(ValueError, match="share one precision"):
        B.ResidentColumnsPosterior([B.BayesianLinearRegressor(np.zeros(D), B.Diagonal(np.ones(D))) for _ in range(2)])


def test_resident_columns_posterior_through_random_fourier_features(B):
    rng = _rng(901)
    D, Din, N, S = 24, 3, 15, 3
    Xin = rng.standard_normal((Din, N))
    rff = B.RandomFourierFeatures(rng.standard_normal((Din, D)), 2 * np.pi * rng.random(D))
    mw = 0.1 * rng.standard_normal(D)
    dvec = np.exp(0.2 * rng.standard_normal(D))
    s = np.exp(0.3 * rng.standard_normal(N))
    Y = rng.standard_normal((N, S))
    bfr = B.BasisFunctionRegressor(B.BayesianLinearRegressor(mw, B.Diagonal(dvec)), rff)
    st = B.ResidentColumnsPosterior(bfr, S=S)
    cv = lambda idx: B.ColVecs(np.asfortranarray(Xin[:, idx]))
    everything = list(range(N))
    lp = st.condition(cv(everything), B.Diagonal(s), Y)
    Phi = rff(cv(everything)).X
    idx = [0, 4, 5, 12]
    rest = [i for i in everything if i not in idx]
    lp_dn = st.forget(cv(idx), B.Diagonal(s[idx]), Y[idx])
    Mg, Tg = st.state()
    for c in range(S):
        assert lp[c] == pytest.approx(O.logpdf_literal(mw, dvec, Phi, s, Y[:, c]), rel=1e-9, abs=1e-10)
        mw_o, _, L_o = O.posterior_literal(mw, dvec, Phi[:, rest], s[rest], Y[rest, c])
        _assert_state(Mg[:, c], Tg, mw_o, L_o)
        lp_o = O.logpdf_literal(mw, dvec, Phi, s, Y[:, c]) - O.logpdf_literal(mw, dvec, Phi[:, rest], s[rest], Y[rest, c])
        assert lp_dn[c] == pytest.approx(lp_o, rel=1e-9, abs=1e-10)
    assert all(isinstance(r, B.BasisFunctionRegressor) for r in st.regressors())
    m, _ = st.mean_and_var(cv(idx), 0.1)
    np.testing.assert_allclose(m, Phi[:, idx].T @ Mg, rtol=1e-9, atol=1e-12)


def test_pos_def_exception_leaves_the_state_unchanged(B):
    D, S = 9, 3
    st = B.ResidentColumnsPosterior(B.BayesianLinearRegressor(np.zeros(D), B.Diagonal(np.ones(D))), S=S)
    M0, T0 = st.state()
    x = np.array([[0.5, 0.5, 0.5, 0.6, 0.1, 0.0, 0.0, 0.0, 0.0]]).T
    with pytest.raises(B._abi.PosDefException) as e:
        st.forget(x, 1.0, np.zeros((1, S)))
    assert e.value.info == 4
    M1, T1 = st.state()
    assert np.array_equal(M0, M1) and np.array_equal(T0, T1)
    with pytest.raises(NotImplementedError):
        st.condition(0.1 * np.ones((D, 2)), np.eye(2), np.zeros((2, S)))
    with pytest.raises(NotImplementedError):
        st.forget(0.1 * np.ones((D, 2)), np.eye(2), np.zeros((2, S)))
