"""Exact leave-one-out predictives of multi-output states (blr_loo_multi_batched_*, loo_columns, loo_columns_map,
ResidentColumnsPosterior.loo) against the CPU oracle: brute-force refits and the N x N formulas per column, the
single-column entry point, the bit promises of the header, status, NaN rule, the D > 128 route and the Python surface.  All tests
need an MI355X.

The states come from the generator of tests/test_loo_gpu.py (`_state`): its largest leverage over five seeds is 0.54 for the shapes
used here, and every oracle comparison asserts max h_n <= 0.9 on the oracle side, so nothing is masked and no case is left out."""
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
    return np.random.Generator(np.random.PCG64(2020 + i))


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


def _nxn_cols(M0, Lw, X, s, Y):
    """-> (mean N x S, var N, logpdf N x S) of the oracle, with the leverage bound of this file asserted on the oracle side"""
    cols = [_nxn(M0[:, c], Lw, X, s, Y[:, c]) for c in range(Y.shape[1])]
    var = cols[0][1]
    h = 1.0 - np.broadcast_to(s, var.shape) / var
    assert h.max() <= 0.9, h.max()
    return np.stack([c[0] for c in cols], axis=1), var, np.stack([c[2] for c in cols], axis=1)


def _state(rng, D, N, scale=0.7):
    """A resident posterior with N observations of dimension D (PDMat prior) and those observations."""
    U = np.triu(rng.standard_normal((D, D))) * (0.3 / np.sqrt(D))
    U[np.diag_indices(D)] = 1.0 + np.abs(U[np.diag_indices(D)])
    mw = rng.standard_normal(D)
    X = np.asfortranarray(rng.standard_normal((D, N)) * (scale / np.sqrt(D)))
    s = np.exp(0.3 * rng.standard_normal(N))
    y = rng.standard_normal(N)
    return mw, U, X, s, y


_CACHE = {}


def _multi_state(B, D, N, S, noise="diagonal", seed=0, dtype=np.float64):
    """(M0, U, X, s, Y, M, T): the generator's state with S columns of prior means and targets, conditioned on the device through
    ResidentColumnsPosterior; computed once per key and never modified (the tests copy what they change)."""
    key = (D, N, S, noise, seed, np.dtype(dtype).name)
    if key not in _CACHE:
        rng = _rng(1000 * seed + D + N + S)
        _, U, X, s, _ = _state(rng, D, N)
        if noise == "isotropic":
            s = np.float64(0.8)
        M0 = rng.standard_normal((D, S))
        Y = np.asfortranarray(rng.standard_normal((N, S)))
        U, X, M0, Y = (np.asfortranarray(a.astype(dtype)) for a in (U, X, M0, Y))
        s = np.asarray(s, dtype=dtype)
        Lw = B.PDMat(U)
        st = B.ResidentColumnsPosterior([B.BayesianLinearRegressor(M0[:, c].copy(), Lw) for c in range(S)])
        st.condition(B.ColVecs(X), B.Diagonal(s) if noise == "diagonal" else s, Y)
        M, T = st.state()
        _CACHE[key] = (M0, U, X, s, Y, np.asfortranarray(M), np.asfortranarray(T))
    return _CACHE[key]


def _raw(B, dtype, layout, X, ldx, Y, s, M, T, Bn=1, strideX=0, strideY=0, strides=0, strideM=0, strideT=0, want="mvlt",
         memspace=None, N=None, S=None):
    """blr_loo_multi_batched_* (host memspace by default) -> (mean [Bn, N, S], var [Bn, N], logpdf [Bn, N, S], total [Bn, S], info);
    outputs not in `want` are passed as NULL and come back as None; the others start as the sentinel 7.0."""
    D = M.shape[-2] if M.ndim > 1 else None
    N = Y.shape[-2] if N is None else N
    S = Y.shape[-1] if S is None else S
    D = T.shape[-1] if T.ndim >= 2 and T.shape[-1] == T.shape[-2] else D
    lm = np.full((Bn, S, N), 7.0, dtype=dtype) if "m" in want else None
    lv = np.full((Bn, N), 7.0, dtype=dtype) if "v" in want else None
    ll = np.full((Bn, S, N), 7.0) if "l" in want else None
    tot = np.full((Bn, S), 7.0) if "t" in want else None
    info = np.zeros(Bn, dtype=np.int32)
    s = np.atleast_1d(np.asarray(s, dtype=dtype))
    kind = B._abi.NOISE_DIAGONAL if s.shape[-1] == N and N > 1 else B._abi.NOISE_ISOTROPIC
    h = B._abi.default_handle()
    Yf = np.ascontiguousarray(np.swapaxes(Y, -1, -2))  # N x S column-major per regressor = (S, N) C-order
    Mf = np.ascontiguousarray(np.swapaxes(M, -1, -2))
    Tf = np.ascontiguousarray(np.swapaxes(T, -1, -2))
    h.loo_multi_batched(dtype, B._abi.MEM_HOST if memspace is None else memspace, layout, Bn, D, N, S, X, ldx, strideX, Yf, N, strideY,
                        kind, s, strides, Mf, D, strideM, Tf, D, strideT, lm, N, N * S, lv, N, ll, N, N * S, tot, S, info)
    sw = lambda a: None if a is None else np.swapaxes(a, 1, 2)  # noqa: E731
    return sw(lm), lv, sw(ll), tot, info


def _x_of(B, X, layout):
    D, N = X.shape
    if layout == "col":
        return B._abi.LAYOUT_COLVECS, X, D
    return B._abi.LAYOUT_ROWVECS, np.asfortranarray(X.T), N


# ---- 1. oracle, fp64 ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prior", ["diagonal", "dense", "pdmat"])
@pytest.mark.parametrize("noise", ["isotropic", "diagonal"])
def test_brute_force_toy_per_column(B, prior, noise):
    rng = _rng(1)
    N, D, S = 13, 7, 3
    X, _, Lw, s = O.generate_toy_problem(rng, N, D, dense_noise_cov=False)
    mw = rng.standard_normal(D)
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
    Y = rng.standard_normal((N, S))
    Sy = B.Diagonal(s) if noise == "diagonal" else s
    r = B.loo_columns(f(X, Sy), Y)
    assert r.logpdf.dtype == np.float64 and r.mean.shape == (N, S) and r.var.shape == (N,) and r.total.shape == (S,)
    sv = np.broadcast_to(s, (N,))
    for c in range(S):
        full = O.logpdf_literal(mw, Lw_d, X, np.diag(sv), Y[:, c])
        for n in range(N):
            rest = [i for i in range(N) if i != n]
            lp_o = full - O.logpdf_literal(mw, Lw_d, X[:, rest], np.diag(sv[rest]), Y[rest, c])
            assert r.logpdf[n, c] == pytest.approx(lp_o, rel=1e-9, abs=1e-12)
    m_o, v_o, lp_o = _nxn_cols(np.repeat(mw[:, None], S, axis=1), Lw_d, X, sv, Y)
    np.testing.assert_allclose(r.mean, m_o, rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(r.var, v_o, rtol=1e-9)
    np.testing.assert_allclose(r.logpdf, lp_o, rtol=1e-9)
    for c in range(S):
        assert r.total[c] == pytest.approx(math.fsum(r.logpdf[:, c]), rel=1e-12)


SHAPES = [(16, 70, 17), (64, 150, 5), (100, 130, 33), (128, 64, 1), (128, 200, 16), (128, 200, 17), (128, 300, 40)]


@pytest.mark.parametrize("D,N,S", SHAPES)
@pytest.mark.parametrize("layout", ["col", "row"])
@pytest.mark.parametrize("noise", ["isotropic", "diagonal"])
def test_against_nxn_formulas(B, D, N, S, layout, noise):
    M0, U, X, s, Y, M, T = _multi_state(B, D, N, S, noise)
    lay, Xl, ldx = _x_of(B, X, layout)
    lm, lv, ll, tot, info = _raw(B, np.float64, lay, Xl, ldx, Y, s, M, T)
    assert info[0] == 0
    m_o, v_o, lp_o = _nxn_cols(M0, U.T @ U, X, s, Y)
    np.testing.assert_allclose(lm[0], m_o, rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(lv[0], v_o, rtol=1e-9)  # once per input
    np.testing.assert_allclose(ll[0], lp_o, rtol=1e-9)
    for c in range(S):
        assert tot[0, c] == pytest.approx(math.fsum(ll[0][:, c]), rel=1e-12)


# ---- 2. against the single-column entry point ---------------------------------------------------------------------------------
@pytest.mark.parametrize("D,N,S", [(16, 70, 17), (64, 150, 5), (128, 200, 17)])
def test_every_column_equals_the_single_column_entry_point(B, D, N, S):
    """The same mathematics with a different product order: rtol 1e-12 on every output.  The means alone also get atol 1e-12, the
    pair of bounds tests/test_loo_gpu.py holds between two routes of blr_loo_batched_*: mean = y - r / (1 - h) is a difference of
    O(1) terms and can cancel to nothing (measured here: -6.6e-6 at (128, 200, 17), where the two entry points differ by 2.2e-16,
    one ulp of the terms, i.e. 3.3e-12 of the result), and the two orders of x'm differ by up to gamma_D |x| |m| / (1 - h), about
    1e-13 for these states (D = 128, eps = 1.1e-16, |x| |m| < 10, h <= 0.54)."""
    M0, U, X, s, Y, M, T = _multi_state(B, D, N, S)
    lm, lv, ll, tot, info = _raw(B, np.float64, B._abi.LAYOUT_COLVECS, X, D, Y, s, M, T)
    h = B._abi.default_handle()
    for c in range(S):
        m1, v1, l1 = np.full(N, 7.0), np.full(N, 7.0), np.full(N, 7.0)
        t1, i1 = np.full(1, 7.0), np.zeros(1, dtype=np.int32)
        h.loo(np.float64, B._abi.MEM_HOST, B._abi.LAYOUT_COLVECS, 1, D, N, X, D, 0, np.ascontiguousarray(Y[:, c]), 0,
              B._abi.NOISE_DIAGONAL, s, 0, np.ascontiguousarray(M[:, c]), 0, T, D, 0, m1, N, v1, N, l1, N, t1, i1)
        assert i1[0] == 0
        np.testing.assert_allclose(lm[0][:, c], m1, rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(lv[0], v1, rtol=1e-12)
        np.testing.assert_allclose(ll[0][:, c], l1, rtol=1e-12)
        assert tot[0, c] == pytest.approx(t1[0], rel=1e-12)


# ---- 3. fp32 ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,N,S", [(128, 200, 17), (64, 150, 5)])
@pytest.mark.parametrize("layout", ["col", "row"])
def test_fp32_against_the_fp64_formulas(B, D, N, S, layout):
    M0, U, X, s, Y, M, T = _multi_state(B, D, N, S, dtype=np.float32)
    assert M.dtype == np.float32 and T.dtype == np.float32
    lay, Xl, ldx = _x_of(B, X, layout)
    lm, lv, ll, tot, info = _raw(B, np.float32, lay, Xl, ldx, Y, s, M, T)
    assert info[0] == 0 and lm.dtype == np.float32 and lv.dtype == np.float32 and ll.dtype == np.float64 and tot.dtype == np.float64
    U64, X64, M64, Y64, s64 = (np.asarray(a, dtype=np.float64) for a in (U, X, M0, Y, s))
    m_o, v_o, lp_o = _nxn_cols(M64, U64.T @ U64, X64, s64, Y64)
    np.testing.assert_allclose(ll[0], lp_o, rtol=1e-3, atol=1e-3)
    np.testing.assert_allclose(lm[0], m_o, rtol=1e-3, atol=1e-3)
    np.testing.assert_allclose(lv[0], v_o, rtol=1e-3)


# ---- 4. bits --------------------------------------------------------------------------------------------------------------
def _same(a, b):
    return all(np.array_equal(u, v) for u, v in zip(a, b))


def test_bits_repeat_batch_position_and_shared_inputs(B):
    D, N, S, nb = 128, 200, 17, 3
    sts = [_multi_state(B, D, N, S, seed=k) for k in range(nb)]
    ones = [_raw(B, np.float64, B._abi.LAYOUT_COLVECS, q[2], D, q[4], q[3], q[5], q[6]) for q in sts]
    again = _raw(B, np.float64, B._abi.LAYOUT_COLVECS, sts[0][2], D, sts[0][4], sts[0][3], sts[0][5], sts[0][6])
    assert _same(ones[0], again)  # a repeat call
    for order in (range(nb), range(nb - 1, -1, -1)):
        order = list(order)
        Xb = np.stack([sts[k][2].reshape(-1, order="F") for k in order])
        Yb, sb = np.stack([sts[k][4] for k in order]), np.stack([sts[k][3] for k in order])
        Mb, Tb = np.stack([sts[k][5] for k in order]), np.stack([sts[k][6] for k in order])
        got = _raw(B, np.float64, B._abi.LAYOUT_COLVECS, Xb, D, Yb, sb, Mb, Tb, Bn=nb, strideX=D * N, strideY=N * S, strides=N,
                   strideM=D * S, strideT=D * D)
        assert not got[4].any()
        for pos, k in enumerate(order):
            assert _same([a[pos] for a in got[:4]], [a[0] for a in ones[k][:4]])
    # strideX = 0 and strideY = 0: three states over the same inputs and targets
    q = sts[0]
    Mb, Tb = np.stack([sts[k][5] for k in range(nb)]), np.stack([sts[k][6] for k in range(nb)])
    got = _raw(B, np.float64, B._abi.LAYOUT_COLVECS, q[2], D, q[4], q[3], Mb, Tb, Bn=nb, strideM=D * S, strideT=D * D)
    assert not got[4].any()
    for k in range(nb):
        one = _raw(B, np.float64, B._abi.LAYOUT_COLVECS, q[2], D, q[4], q[3], sts[k][5], sts[k][6])
        assert _same([a[k] for a in got[:4]], [a[0] for a in one[:4]])


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("layout", ["col", "row"])
@pytest.mark.parametrize("noise", ["isotropic", "diagonal"])
def test_a_workgroup_that_walks_several_tiles(B, noise, layout, dtype):
    """600 regressors over the same inputs, targets and state (all strides 0), D = 20, N = 130 (two full tiles and a tail of two),
    S = 17 (two passes): regressors >= 2 x CUs, so one workgroup per regressor commits a tile and prefetches the next while it
    multiplies, three times over.  At B = 1 every workgroup takes one tile: the bits must not depend on which of the two it was.
    The B = 1 outputs are held to the oracle at the bounds of test_against_nxn_formulas / test_fp32_against_the_fp64_formulas."""
    Bn, D, N, S = 600, 20, 130, 17
    M0, U, X, s, Y, M, T = _multi_state(B, D, N, S, noise, dtype=dtype)
    lay, Xl, ldx = _x_of(B, X, layout)
    one = _raw(B, dtype, lay, Xl, ldx, Y, s, M, T)
    lm, lv, ll, tot, info = one
    assert info[0] == 0
    U64, X64, M64, Y64, s64 = (np.asarray(a, dtype=np.float64) for a in (U, X, M0, Y, s))
    m_o, v_o, lp_o = _nxn_cols(M64, U64.T @ U64, X64, s64, Y64)
    if dtype == np.float64:
        np.testing.assert_allclose(lm[0], m_o, rtol=1e-9, atol=1e-12)
        np.testing.assert_allclose(lv[0], v_o, rtol=1e-9)
        np.testing.assert_allclose(ll[0], lp_o, rtol=1e-9)
    else:
        np.testing.assert_allclose(ll[0], lp_o, rtol=1e-3, atol=1e-3)
        np.testing.assert_allclose(lm[0], m_o, rtol=1e-3, atol=1e-3)
        np.testing.assert_allclose(lv[0], v_o, rtol=1e-3)
    for c in range(S):
        assert tot[0, c] == pytest.approx(math.fsum(ll[0][:, c]), rel=1e-12)
    got = _raw(B, dtype, lay, Xl, ldx, Y, s, M, T, Bn=Bn)
    assert not got[4].any()
    for a, a1 in zip(got[:4], one[:4]):
        np.testing.assert_array_equal(a, np.broadcast_to(a1[0], a.shape))


@pytest.mark.parametrize("layout", ["col", "row"])
def test_bits_of_a_column_do_not_depend_on_the_others(B, layout):
    D, N, S = 100, 130, 33
    M0, U, X, s, Y, M, T = _multi_state(B, D, N, S)
    lay, Xl, ldx = _x_of(B, X, layout)
    base = _raw(B, np.float64, lay, Xl, ldx, Y, s, M, T)
    perm = np.roll(np.arange(S), 5)[::-1].copy()  # columns move across the 16-column pass boundaries
    assert any(perm[c] // 16 != c // 16 for c in range(S))
    got = _raw(B, np.float64, lay, Xl, ldx, np.asfortranarray(Y[:, perm]), s, np.asfortranarray(M[:, perm]), T)
    assert np.array_equal(got[0][0], base[0][0][:, perm]) and np.array_equal(got[2][0], base[2][0][:, perm])
    assert np.array_equal(got[3][0], base[3][0][perm]) and np.array_equal(got[1], base[1])
    # garbage in the other columns of Y and M; a single column alone (S = 1)
    rng = _rng(44)
    for c in (0, 15, 16, 32):
        Yg, Mg = 1e3 * rng.standard_normal((N, S)), 1e3 * rng.standard_normal((D, S))
        Yg[:, c], Mg[:, c] = Y[:, c], M[:, c]
        got = _raw(B, np.float64, lay, Xl, ldx, np.asfortranarray(Yg), s, np.asfortranarray(Mg), T)
        assert np.array_equal(got[0][0][:, c], base[0][0][:, c]) and np.array_equal(got[2][0][:, c], base[2][0][:, c])
        assert got[3][0, c] == base[3][0, c] and np.array_equal(got[1], base[1])
        alone = _raw(B, np.float64, lay, Xl, ldx, np.asfortranarray(Y[:, c:c + 1]), s, np.asfortranarray(M[:, c:c + 1]), T)
        assert np.array_equal(alone[0][0][:, 0], base[0][0][:, c]) and np.array_equal(alone[2][0][:, 0], base[2][0][:, c])
        assert alone[3][0, 0] == base[3][0, c]


def test_bits_of_var_total_only_and_memspaces(B):
    D, N, S = 128, 200, 17
    M0, U, X, s, Y, M, T = _multi_state(B, D, N, S)
    lay = B._abi.LAYOUT_COLVECS
    base = _raw(B, np.float64, lay, X, D, Y, s, M, T)
    for S1 in (1, 16, 17):
        Ys, Ms = np.asfortranarray(Y[:, :S1]), np.asfortranarray(M[:, :S1])
        assert np.array_equal(_raw(B, np.float64, lay, X, D, Ys, s, Ms, T)[1], base[1])
        only = _raw(B, np.float64, lay, X, D, Ys, s, Ms, T, want="v")
        assert np.array_equal(only[1], base[1]) and only[0] is None and only[2] is None and only[3] is None
    # total only: the log densities go through the handle's workspace, the same bits
    tot = _raw(B, np.float64, lay, X, D, Y, s, M, T, want="t")
    assert np.array_equal(tot[3], base[3])
    # device memspace on staged operands
    h = B._abi.default_handle()
    from blr_amd.regressor import _DeviceBuffer

    Yf, Mf, Tf = (np.ascontiguousarray(a.T) for a in (Y, M, T))
    ins = [_DeviceBuffer.of(h, a) for a in (X, Yf, s, Mf, Tf)]
    outs = [_DeviceBuffer(h, N * S * 8), _DeviceBuffer(h, N * 8), _DeviceBuffer(h, N * S * 8), _DeviceBuffer(h, S * 8),
            _DeviceBuffer.of(h, np.zeros(1, dtype=np.int32))]
    try:
        h.loo_multi_batched(np.float64, B._abi.MEM_DEVICE, lay, 1, D, N, S, ins[0].ptr, D, 0, ins[1].ptr, N, 0, B._abi.NOISE_DIAGONAL,
                            ins[2].ptr, 0, ins[3].ptr, D, 0, ins[4].ptr, D, 0, outs[0].ptr, N, 0, outs[1].ptr, 0, outs[2].ptr, N, 0,
                            outs[3].ptr, 0, outs[4].ptr)
        lm, lv, ll, tt = np.empty((S, N)), np.empty(N), np.empty((S, N)), np.empty(S)
        for host, b in zip((lm, lv, ll, tt), outs):
            h.memcpy_d2h(host, b.ptr)
    finally:
        for b in ins + outs:
            b.free()
    assert np.array_equal(lm.T, base[0][0]) and np.array_equal(lv, base[1][0]) and np.array_equal(ll.T, base[2][0])
    assert np.array_equal(tt, base[3][0])


# ---- 5. totals ------------------------------------------------------------------------------------------------------------
def test_totals_are_fixed_order_sums(B):
    D, N, S = 40, 5000, 3
    M0, U, X, s, Y, M, T = _multi_state(B, D, N, S)
    lm, lv, ll, tot, info = _raw(B, np.float64, B._abi.LAYOUT_COLVECS, X, D, Y, s, M, T)
    assert info[0] == 0
    for c in range(S):
        assert tot[0, c] == pytest.approx(math.fsum(ll[0][:, c]), rel=1e-12)
    # N = 0: every requested total is 0, info 0
    got = _raw(B, np.float64, B._abi.LAYOUT_COLVECS, np.zeros((D, 1)), D, np.zeros((0, S)), 1.0, M, T, want="t", N=0, S=S)
    assert got[4][0] == 0 and np.all(got[3] == 0.0)


# ---- 6. status ------------------------------------------------------------------------------------------------------------
def test_status_and_untouched_outputs(B):
    D, N, S = 128, 100, 3
    M0, U, X, s, Y, M, T = _multi_state(B, D, N, S)
    lay = B._abi.LAYOUT_COLVECS
    Tz = T.copy()
    Tz[5, 5] = 0.0
    sb = s.copy()
    sb[17] = -1.0
    for Tq, sq, code in ((Tz, s, 6), (T, sb, 18), (Tz, sb, 6)):  # a bad factor wins over a bad variance
        got = _raw(B, np.float64, lay, X, D, Y, sq, M, Tq)
        assert got[4][0] == code
        for a in got[:4]:
            assert np.all(a == 7.0)
    # the batch's other regressor is filled
    good = _raw(B, np.float64, lay, X, D, Y, s, M, T)
    got = _raw(B, np.float64, lay, X, D, Y, s, M, np.stack([Tz, T]), Bn=2, strideT=D * D)
    assert got[4].tolist() == [6, 0]
    for a, g in zip(got[:4], good[:4]):
        assert np.all(a[0] == 7.0) and np.array_equal(a[1], g[0])
    with pytest.raises(B.PosDefException):
        st = B.ResidentColumnsPosterior([B.BayesianLinearRegressor(M[:, c].copy(), Lw) for Lw in [B.PDMat(T)] for c in range(S)])
        st.loo(B.ColVecs(X), B.Diagonal(sb), Y)


# ---- 7. degenerate leverage -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [16, 128])
def test_degenerate_leverage_gives_nan_and_counts_once(B, D):
    N, S = 80, 3
    M0, U, X, s, Y, M, T = _multi_state(B, D, N, S)
    rng = _rng(11 + D)
    h = B._abi.default_handle()
    Lw = B.PDMat(T)
    st = B.ResidentColumnsPosterior([B.BayesianLinearRegressor(M[:, c].copy(), Lw) for c in range(S)])
    # a high-leverage input the state does NOT contain: sigma2 > s, so 1 - h < 0
    xo = np.asfortranarray(np.concatenate([X, 40.0 * rng.standard_normal((D, 1))], axis=1))
    so = np.concatenate([s, [1e-3]])
    Yo = np.concatenate([Y, np.full((1, S), 0.3)], axis=0)
    before = h.get_stat("loo_degenerate")
    r = st.loo(B.ColVecs(xo), B.Diagonal(so), Yo)
    assert h.get_stat("loo_degenerate") - before == 1  # once, not S times
    assert np.isnan(r.var[N]) and np.all(np.isnan(r.mean[N])) and np.all(np.isnan(r.logpdf[N])) and np.all(np.isnan(r.total))
    assert np.all(np.isfinite(r.logpdf[:N])) and np.all(np.isfinite(r.mean[:N])) and np.all(np.isfinite(r.var[:N]))


# ---- 8. D > 128 -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,N,S,layout", [(200, 90, 3, "col"), (200, 90, 3, "row"), (256, 500, 18, "col")])
def test_large_d_against_nxn_formulas(B, D, N, S, layout):
    M0, U, X, s, Y, M, T = _multi_state(B, D, N, S)
    lay, Xl, ldx = _x_of(B, X, layout)
    lm, lv, ll, tot, info = _raw(B, np.float64, lay, Xl, ldx, Y, s, M, T)
    assert info[0] == 0
    m_o, v_o, lp_o = _nxn_cols(M0, U.T @ U, X, s, Y)
    np.testing.assert_allclose(lm[0], m_o, rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(lv[0], v_o, rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(ll[0], lp_o, rtol=1e-9, atol=1e-9)
    for c in range(S):
        assert tot[0, c] == pytest.approx(math.fsum(ll[0][:, c]), rel=1e-12)


# ---- 9. Python ------------------------------------------------------------------------------------------------------------
def test_loo_columns_against_a_loop_of_loo(B):
    rng = _rng(9)
    D, N, S = 64, 150, 5
    fxs, Ys = [], []
    for _ in range(3):
        mw, U, X, s, _ = _state(rng, D, N)
        fxs.append(B.BayesianLinearRegressor(mw, B.PDMat(U))(B.ColVecs(X), B.Diagonal(s)))
        Ys.append(rng.standard_normal((N, S)))
    many = B.loo_columns_map(fxs, Ys)
    one = B.loo_columns(fxs[1], Ys[1])
    for a, b in zip(one, many[1]):
        assert np.array_equal(a, b)
    for fx, Y, r in zip(fxs, Ys, many):
        assert r.mean.shape == (N, S) and r.var.shape == (N,) and r.logpdf.shape == (N, S) and r.total.shape == (S,)
        for c in range(S):
            ref = B.loo(fx, Y[:, c])
            np.testing.assert_allclose(r.mean[:, c], ref.mean, rtol=1e-9, atol=1e-12)
            np.testing.assert_allclose(r.var, ref.var, rtol=1e-9)
            np.testing.assert_allclose(r.logpdf[:, c], ref.logpdf, rtol=1e-9)
            assert r.total[c] == pytest.approx(ref.total, rel=1e-9)
    # unequal shapes: the loop route gives the same numbers
    mixed = B.loo_columns_map([fxs[0], fxs[1]], [Ys[0], Ys[1][:, :2]])
    assert np.array_equal(mixed[0].logpdf, many[0].logpdf) and np.array_equal(mixed[1].logpdf, many[1].logpdf[:, :2])


def test_resident_loo_leaves_the_state_and_matches_forget(B):
    D, N, S = 128, 200, 5
    rng = _rng(10)
    _, U, X, s, _ = _state(rng, D, N)
    M0, Y = rng.standard_normal((D, S)), rng.standard_normal((N, S))
    Lw = B.PDMat(U)
    st = B.ResidentColumnsPosterior([B.BayesianLinearRegressor(M0[:, c].copy(), Lw) for c in range(S)])
    st.condition(B.ColVecs(X), B.Diagonal(s), Y)
    M1, T1 = st.state()
    r = st.loo(B.ColVecs(X), B.Diagonal(s), Y)
    M2, T2 = st.state()
    assert np.array_equal(M1, M2) and np.array_equal(T1, T2)  # bit-identical: the state is not modified
    for n in rng.choice(N, 10, replace=False):
        Lc = B.PDMat(T1)
        cp = B.ResidentColumnsPosterior([B.BayesianLinearRegressor(M1[:, c].copy(), Lc) for c in range(S)])
        lp = cp.forget(B.ColVecs(X[:, n:n + 1]), B.Diagonal(s[n:n + 1]), Y[n:n + 1])
        for c in range(S):
            assert r.logpdf[n, c] == pytest.approx(lp[c], rel=1e-9, abs=1e-10)
