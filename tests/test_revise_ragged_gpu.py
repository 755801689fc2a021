"""Condition and forget on resident states with unequal observation counts (blr_update_factor_ragged_*, blr_downdate_factor_ragged_*,
ResidentPosteriorBatch): every regressor against the CPU oracle by the repeated-conditioning restatement and the
tolerances of tests/test_gpu_parity.py and tests/test_downdate_gpu.py, and bit for bit against the B = 1 entry point the header
names.  All tests need an MI355X."""
import functools

import numpy as np
import pytest

from oracle import blr_oracle as O

import _revise_ragged_data as R
from _yardsticks import _assert_fp32_within_lapack
from test_downdate_gpu import RTOL, _assert_state, _fp32_check

pytestmark = pytest.mark.gpu


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


@functools.lru_cache(maxsize=None)
def batch(D, counts=R.COUNTS, dtype=np.float64, seed=0):
    return R.Batch(D, counts, dtype, seed)


def _stats(h):
    return [h.get_stat(k) for k in ("ragged_sweep", "ragged_refit", "ragged_idle")]


def _check_oracle(P, direction, kind, b, m0, T0, got_m, got_T, got_lp, what):
    """regressor b against the oracle: from the state (m0, T0 upper) it started at, on its slice"""
    X, y, s = P.X[:, P.sl(b)], P.y[P.sl(b)], P.noise(kind, b)
    Tg = np.triu(np.asarray(got_T, dtype=np.float64))
    f32 = lambda v: np.asarray(v, dtype=np.float32)
    if direction == "update":
        if P.dtype == np.float32:
            _assert_fp32_within_lapack(f32(m0), f32(T0.T @ T0), np.asfortranarray(f32(X)), f32(s), f32(y), got_m, Tg.T @ Tg, got_lp,
                                       floor=(4e-6, 2e-6, 2e-6), what=what)
            return
        mw_o, _, L_o = O.posterior_literal(m0, T0.T @ T0, X, s, y)
        np.testing.assert_allclose(Tg.T @ Tg, L_o, rtol=RTOL, atol=RTOL * np.abs(L_o).max())
        np.testing.assert_allclose(got_m, mw_o, rtol=50 * RTOL, atol=RTOL * np.abs(mw_o).max())
        assert got_lp == pytest.approx(O.logpdf_literal(m0, T0.T @ T0, X, s, y), rel=10 * RTOL, abs=10 * RTOL)
        return
    if P.dtype == np.float32:
        _fp32_check(f32(m0), f32(T0), f32(X), f32(s), f32(y), got_m, Tg, got_lp, what)
        return
    mb, Tb = P.base[b]
    _assert_state(got_m, Tg, mb, Tb.T @ Tb)
    assert got_lp == pytest.approx(O.logpdf_literal(mb, Tb.T @ Tb, X, s, y), rel=1e-9, abs=1e-9)


def _upper_bits(T):
    return np.triu(T.T).tobytes()  # T: a column-major factor as a row-major array


def _run_and_hold(B, opt, P, direction, mode, layout, kind, oracle=True, order=None):
    """One ragged call; every regressor held to its B = 1 yardstick bit for bit and (oracle) to the CPU oracle -> (mw, T, lp, info)"""
    a, h = B._abi, B._abi.default_handle()
    sweep, refit, idle = R.routes(P.counts, P.D, direction, mode)
    states = P.start(direction, kind)
    mw0, T0 = P.state_operands(states)
    opt("SWEEP", "always")  # the yardstick of the sweep route: blr_update_factor_* on a SWEEP=always handle
    yard = {b: R.yardstick(a, h, "sweep" if direction == "update" else "downdate", P, kind, b, mw0[b], T0[b], layout) for b in sweep}
    yard.update({b: R.yardstick(a, h, "refit", P, kind, b, mw0[b], T0[b], layout) for b in refit})
    opt("SWEEP", None if mode == "auto" else mode)
    mw, T = mw0.copy(), T0.copy()
    lp, info = R.call(a, h, direction, P, layout, kind, mw, T)
    assert _stats(h) == [len(sweep), len(refit), len(idle)]
    assert info.tolist() == [0] * P.nb
    for b in idle:
        assert R.same_bits(mw[b], mw0[b]) and R.same_bits(T[b], T0[b]) and lp[b] == 0.0
    for b in sweep + refit:
        ym, yT, ylp, yinfo = yard[b]
        what = f"{direction} {mode} D={P.D} {P.dtype.__name__} {layout} {kind} b={b} k={P.counts[b]}"
        assert yinfo == 0, what
        assert R.same_bits(mw[b], ym) and _upper_bits(T[b]) == _upper_bits(yT) and R.same_bits(lp[b], ylp), what
        if b in sweep:
            assert R.same_bits(T[b], yT), what  # (the sweep and the downdate leave the strictly-lower part alone: NaN still)
        if oracle:
            _check_oracle(P, direction, kind, b, *states[b], mw[b], T[b].T, lp[b], what)
    return mw, T, lp, info


# ---- parity and bits -----------------------------------------------------------------------------------------------------------------
CASES = [("update", "auto"), ("update", "always"), ("downdate", "auto")]


@pytest.mark.parametrize("kind", ["iso0", "iso1", "diag"])
@pytest.mark.parametrize("layout", ["colvecs", "colvecs_odd", "rowvecs"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("D", [5, 64, 65, 128])
@pytest.mark.parametrize("direction,mode", CASES)
def test_parity_and_bits(B, opt, direction, mode, D, dtype, layout, kind):
    """NaN fills the padding rows of X (RowVecs: the rows beyond offsets[B]) and the strictly-lower part of every factor"""
    _run_and_hold(B, opt, batch(D, dtype=dtype), direction, mode, layout, kind)


def test_sweep_never_refits_every_active_regressor(B, opt):
    _run_and_hold(B, opt, batch(40), "update", "never", "colvecs", "diag")


# ---- permutation, repetition, chunking --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("direction,mode", CASES)
def test_permutation_and_second_call_give_the_same_bits(B, opt, direction, mode):
    D, kind = 65, "diag"
    P = batch(D)
    mw, T, lp, _ = _run_and_hold(B, opt, P, direction, mode, "colvecs", kind, oracle=False)
    mw2, T2, lp2, _ = _run_and_hold(B, opt, P, direction, mode, "colvecs", kind, oracle=False)
    assert R.same_bits(mw, mw2) and R.same_bits(T, T2) and R.same_bits(lp, lp2)
    # the same regressors in another order, as a batch of its own
    a, h = B._abi, B._abi.default_handle()
    perm = [8, 0, 3, 7, 1, 6, 4, 2, 5]
    Q = R.Batch(D, [P.counts[b] for b in perm], P.dtype)
    for j, b in enumerate(perm):
        Q.X[:, Q.sl(j)], Q.y[Q.sl(j)], Q.s_diag[Q.sl(j)] = P.X[:, P.sl(b)], P.y[P.sl(b)], P.s_diag[P.sl(b)]
    Q.base = [P.base[b] for b in perm]
    states = [P.start(direction, kind)[b] for b in perm]
    mq, Tq = Q.state_operands(states)
    opt("SWEEP", None if mode == "auto" else mode)
    lq, iq = R.call(a, h, direction, Q, "colvecs", kind, mq, Tq)
    assert iq.tolist() == [0] * Q.nb
    for j, b in enumerate(perm):
        assert R.same_bits(mq[j], mw[b]) and _upper_bits(Tq[j]) == _upper_bits(T[b]) and R.same_bits(lq[j], lp[b]), (j, b)


@pytest.mark.parametrize("direction,mode", CASES)
def test_max_chunk_gives_the_same_bits(B, opt, direction, mode):
    P = batch(40)
    h = B._abi.default_handle()
    mw, T, lp, _ = _run_and_hold(B, opt, P, direction, mode, "colvecs", "iso1", oracle=False)
    sweep, refit, _ = R.routes(P.counts, P.D, direction, mode)
    assert h.get_stat("last_chunks") == (1 if sweep else 0) + (1 if refit else 0)
    opt("MAX_CHUNK", 2)
    mw2, T2, lp2, _ = _run_and_hold(B, opt, P, direction, mode, "colvecs", "iso1", oracle=False)
    assert h.get_stat("last_chunks") == -(-len(sweep) // 2) + -(-len(refit) // 2)
    assert R.same_bits(mw, mw2) and R.same_bits(T, T2) and R.same_bits(lp, lp2)


# ---- failures in a batch -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("direction,mode", CASES)
def test_failures_leave_their_state_and_the_others_alone(B, opt, direction, mode):
    """regressor 3 (k = 16): a non-positive diagonal entry of T; regressor 5 (k = 3): s = 0 at its 3rd observation; downdate only,
    regressor 4 (k = 17): its first observation scaled so that 1 - a'a < 0 -- an observation the state never held"""
    a, h = B._abi, B._abi.default_handle()
    D, kind = 40, "diag"
    P = batch(D)
    clean_m, clean_T, clean_lp, _ = _run_and_hold(B, opt, P, direction, mode, "colvecs", kind, oracle=False)
    Q = R.Batch(D, P.counts, P.dtype)  # (the same seed: the same data)
    Q.s_diag[Q.sl(5).start + 2] = 0.0
    bad = {3: 7, 5: 3}
    if direction == "downdate":
        Q.X[:, Q.sl(4).start] *= 40.0
        bad[4] = None  # the leading minor that fails: some j in 1 .. D
    mw0, T0 = Q.state_operands(P.start(direction, kind))
    T0[3][6, 6] = -T0[3][6, 6]
    mw, T = mw0.copy(), T0.copy()
    opt("SWEEP", None if mode == "auto" else mode)
    lp, info = R.call(a, h, direction, Q, "colvecs", kind, mw, T)
    for b in range(P.nb):
        if b in bad:
            assert info[b] == bad[b] if bad[b] is not None else 1 <= info[b] <= D, (b, info[b])
            assert np.isnan(lp[b]) and R.same_bits(mw[b], mw0[b]) and R.same_bits(T[b], T0[b]), b
        else:
            assert info[b] == 0
            assert R.same_bits(mw[b], clean_m[b]) and _upper_bits(T[b]) == _upper_bits(clean_T[b]) and R.same_bits(lp[b], clean_lp[b]), b


# ---- padding: gaps of the state are never written ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("direction,mode", CASES)
def test_gaps_of_the_state_are_never_written(B, opt, direction, mode):
    a, h = B._abi, B._abi.default_handle()
    D, kind = 65, "iso1"
    P = batch(D)
    dense_m, dense_T, dense_lp, _ = _run_and_hold(B, opt, P, direction, mode, "colvecs_odd", kind, oracle=False)
    ldt, smw = D + 1, D + 2
    sT = ldt * D + 7
    mw0, T0 = P.state_operands(P.start(direction, kind))
    mbuf = np.full(P.nb * smw, np.nan)
    Tbuf = np.full(P.nb * sT, np.nan)
    state = np.zeros(P.nb * sT, dtype=bool)  # where factor b keeps its D x D block
    for b in range(P.nb):
        mbuf[b * smw:b * smw + D] = mw0[b]
        blk = Tbuf[b * sT:b * sT + ldt * D].reshape(D, ldt)
        blk[:, :D] = T0[b]
        state[b * sT:b * sT + ldt * D].reshape(D, ldt)[:, :D] = True
    m_in, T_in = mbuf.copy(), Tbuf.copy()
    Xa, lay, ldx = P.x_operand("colvecs_odd")
    s, nk, strides = P.s_operand(kind)
    lp, info = np.full(P.nb, -7.0), np.full(P.nb, 7, dtype=np.int32)
    fn = h.update_factor_ragged if direction == "update" else h.downdate_factor_ragged
    fn(P.dtype, a.MEM_HOST, getattr(a, lay), P.nb, D, P.offsets, Xa, ldx, P.y, getattr(a, nk), s, strides, mbuf, smw, Tbuf, ldt, sT, lp, info)
    assert info.tolist() == [0] * P.nb and R.same_bits(lp, dense_lp)
    assert R.same_bits(Tbuf[~state], T_in[~state])
    for b in range(P.nb):
        assert R.same_bits(mbuf[b * smw + D:(b + 1) * smw], m_in[b * smw + D:(b + 1) * smw])
        assert R.same_bits(mbuf[b * smw:b * smw + D], dense_m[b])
        got = Tbuf[b * sT:b * sT + ldt * D].reshape(D, ldt)[:, :D]
        assert _upper_bits(got) == _upper_bits(dense_T[b])


# ---- more workgroups than are resident at once ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("direction", ["update", "downdate"])
def test_many_workgroups(B, opt, direction):
    D, nb, kind = 8, 3000, "diag"
    rng = np.random.Generator(np.random.PCG64(31))
    P = batch(D, counts=tuple(int(c) for c in rng.choice([0, 0, 0, 1, 2, 3], size=nb)))
    a, h = B._abi, B._abi.default_handle()
    states = P.start(direction, kind)
    mw0, T0 = P.state_operands(states)
    mw, T = mw0.copy(), T0.copy()
    lp, info = R.call(a, h, direction, P, "colvecs", kind, mw, T)
    sweep, refit, idle = R.routes(P.counts, D, direction, "auto")
    assert _stats(h) == [len(sweep), len(refit), len(idle)] and not info.any()
    for b in range(nb):
        mb, Tb = P.base[b]
        want = O.logpdf_literal(mb, Tb.T @ Tb, P.X[:, P.sl(b)], P.noise(kind, b), P.y[P.sl(b)]) if P.counts[b] else 0.0
        assert lp[b] == pytest.approx(want, rel=1e-9, abs=1e-9), b
        if P.counts[b] == 0:
            assert R.same_bits(mw[b], mw0[b]) and R.same_bits(T[b], T0[b])
        elif b % 97 == 0:
            _check_oracle(P, direction, kind, b, *states[b], mw[b], T[b].T, lp[b], f"many b={b}")


# ---- round trip ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["auto", "always"])
@pytest.mark.parametrize("D", [7, 64, 128])
def test_update_then_downdate_round_trip(B, opt, D, mode):
    a, h = B._abi, B._abi.default_handle()
    P = batch(D)
    opt("SWEEP", None if mode == "auto" else mode)
    mw0, T0 = P.state_operands(P.base)
    mw, T = mw0.copy(), T0.copy()
    lp_up, info = R.call(a, h, "update", P, "colvecs", "diag", mw, T)
    assert not info.any()
    lp_dn, info = R.call(a, h, "downdate", P, "colvecs", "diag", mw, T)
    assert not info.any()
    for b in range(P.nb):
        mb, Tb = P.base[b]
        _assert_state(mw[b], T[b].T, mb, Tb.T @ Tb)
        assert lp_dn[b] == pytest.approx(lp_up[b], rel=1e-9, abs=1e-10)


# ---- memspaces -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("direction,mode", CASES)
def test_device_memspace_sync_and_async_give_the_host_bits(B, opt, direction, mode):
    import torch

    a, h = B._abi, B._abi.default_handle()
    D, kind = 64, "diag"
    P = batch(D)
    mw_h, T_h, lp_h, _ = _run_and_hold(B, opt, P, direction, mode, "colvecs", kind, oracle=False)
    dev = torch.device("cuda:0")
    mw0, T0 = P.state_operands(P.start(direction, kind))
    Xa, lay, ldx = P.x_operand("colvecs")
    s, nk, strides = P.s_operand(kind)
    fn = h.update_factor_ragged if direction == "update" else h.downdate_factor_ragged
    for asynchronous in (False, True):
        t = lambda v: torch.tensor(np.asarray(v).reshape(-1, order="A"), device=dev)  # (memory order)
        Xd, yd, sd, md, Td = t(Xa), t(P.y), t(s), t(mw0), t(T0)
        lpd = torch.full((P.nb,), -7.0, dtype=torch.float64, device=dev)
        infod = torch.full((P.nb,), 7, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        offsets = P.offsets.copy()
        h.set_async(asynchronous)
        try:
            fn(P.dtype, a.MEM_DEVICE, getattr(a, lay), P.nb, D, offsets, Xd.data_ptr(), ldx, yd.data_ptr(), getattr(a, nk), sd.data_ptr(), strides,
               md.data_ptr(), D, Td.data_ptr(), D, D * D, lpd.data_ptr(), infod.data_ptr())
            offsets[:] = -1  # the caller's offsets array is free when the call returns
            h.synchronize()
        finally:
            h.set_async(False)
        assert infod.cpu().tolist() == [0] * P.nb and R.same_bits(lpd.cpu().numpy(), lp_h)
        assert R.same_bits(md.cpu().numpy().reshape(P.nb, D), mw_h)
        Tg = Td.cpu().numpy().reshape(P.nb, D, D)
        assert all(_upper_bits(Tg[b]) == _upper_bits(T_h[b]) for b in range(P.nb))


# ---- D > 128 and NO_DOWNDATE_LDS: correct, not fast ------------------------------------------------------------------------------------
@pytest.mark.parametrize("direction", ["update", "downdate"])
def test_large_d_goes_one_by_one(B, opt, direction):
    a, h = B._abi, B._abi.default_handle()
    P = batch(160, counts=(0, 2, 5))
    states = P.start(direction, "diag")
    mw0, T0 = P.state_operands(states)
    mw, T = mw0.copy(), T0.copy()
    lp, info = R.call(a, h, direction, P, "colvecs", "diag", mw, T)
    assert info.tolist() == [0, 0, 0] and lp[0] == 0.0 and R.same_bits(mw[0], mw0[0]) and R.same_bits(T[0], T0[0])
    assert _stats(h) == ([0, 2, 1] if direction == "update" else [2, 0, 1]) and h.get_stat("last_chunks") == 2
    for b in (1, 2):
        _check_oracle(P, direction, "diag", b, *states[b], mw[b], T[b].T, lp[b], f"D=160 {direction} b={b}")


def test_no_downdate_lds_goes_one_by_one(B, opt):
    a, h = B._abi, B._abi.default_handle()
    P = batch(40)
    opt("NO_DOWNDATE_LDS", "1")
    states = P.start("downdate", "iso1")
    mw, T = P.state_operands(states)
    lp, info = R.call(a, h, "downdate", P, "rowvecs", "iso1", mw, T)
    assert not info.any()
    for b in range(P.nb):
        if P.counts[b]:
            _check_oracle(P, "downdate", "iso1", b, *states[b], mw[b], T[b].T, lp[b], f"global b={b}")
        else:
            assert lp[b] == 0.0


# ---- argument errors -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["update", "downdate"])
def test_argument_errors(B, name):
    a, h = B._abi, B._abi.default_handle()
    lib = a.load_library()
    D = 4
    p = a._ptr
    for suf, dt in (("f64", np.float64), ("f32", np.float32)):
        fn = getattr(lib, f"blr_{name}_factor_ragged_{suf}")

        def go(handle, offsets=(0, 3, 5), nk=a.NOISE_ISOTROPIC, nb=2):
            off = np.array(offsets, dtype=np.int64)
            X, y, s = np.zeros((D, 5), dtype=dt, order="F"), np.zeros(5, dtype=dt), np.ones(5, dtype=dt)
            mw, T = np.zeros((2, D), dtype=dt), np.stack([np.eye(D, dtype=dt)] * 2)
            lp, info = np.zeros(2), np.zeros(2, dtype=np.int32)
            return fn(handle, a.MEM_HOST, a.LAYOUT_COLVECS, nb, D, p(off), p(X), D, p(y), nk, p(s), 1, p(mw), D, p(T), D, D * D, p(lp), p(info))

        assert go(h._h, offsets=(0, 3, 2)) == -6       # decreasing offsets
        assert go(h._h, nk=a.NOISE_DENSE) == -10       # dense noise
        assert go(None) == -1                          # valid arguments and a NULL handle
        assert go(None, offsets=(0, 3, 2)) == -6       # (the argument checks come first)
        assert go(h._h, nb=0) == 0 and go(None, nb=0) == 0
        assert go(h._h) == 0


# ---- Python ----------------------------------------------------------------------------------------------------------------------------
def test_resident_posterior_batch_against_resident_posteriors(B):
    P = batch(24, counts=(0, 1, 4, 2, 0, 1))
    fs = [B.BayesianLinearRegressor(m, B.PDMat(T)) for m, T in P.base]
    st = B.ResidentPosteriorBatch(fs)
    singles = [B.ResidentPosterior(f) for f in fs]
    x = B.ColVecs(np.asfortranarray(P.X))
    for method in ("condition", "forget"):
        lp = getattr(st, method)(x, P.offsets, B.Diagonal(P.s_diag), P.y)
        mw, T = st.state()
        assert lp.shape == (P.nb,) and mw.shape == (P.nb, P.D) and T.shape == (P.nb, P.D, P.D)
        for b, one in enumerate(singles):
            if P.counts[b] == 0:
                assert lp[b] == 0.0
                continue
            sl = P.sl(b)
            want = getattr(one, method)(B.ColVecs(np.asfortranarray(P.X[:, sl])), B.Diagonal(P.s_diag[sl]), P.y[sl])
            m1, T1 = one.state()
            assert lp[b] == pytest.approx(want, rel=1e-9, abs=1e-10)
            _assert_state(mw[b], T[b], m1, T1.T @ T1)
    regs = st.regressors()
    assert len(regs) == P.nb and isinstance(regs[0].Lw, B.PDMat)
    # a failed regressor raises with its position; a variance per regressor is read at s + b
    with pytest.raises(B.PosDefException) as e:
        st.condition(x, P.offsets, np.array([0.1, 0.1, 0.1, -1.0, 0.1, 0.1]), P.y)
    assert e.value.index == 3
