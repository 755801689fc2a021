"""Evidence over a grid of (prior scale, noise scale) settings (blr_logpdf_grid_*, logpdf_grid, posterior_best, logpdf_grid_map)
against the CPU oracle setting by setting, against blr_posterior_batched_* on the scaled operands, and against itself (argmax,
position independence, determinism, local failures).  All tests need an MI355X."""
import numpy as np
import pytest

from oracle import blr_oracle as O
from _yardsticks import _assert_fp32_within_lapack

pytestmark = pytest.mark.gpu

# fp64 bounds: the project's own (header of blr_posterior_batched_*, tests/test_gpu_parity.py)
TOL_LP, TOL_MW, TOL_A = 1e-10, 1e-9, 1e-9
SCALES = 10.0 ** np.linspace(-2, 2, 5)


@pytest.fixture(scope="module")
def B():
    import blr_amd

    blr_amd._abi.default_handle()  # raises if the extension or the GPU is missing: no silent fallback
    return blr_amd


def _problem(seed, D, N, noise, prior, zero_mean, nb=1):
    """nb data sets of one shape, drawn as the issue states: X ~ N(0,1), w ~ N(0,I), mw ~ 0.3 N(0,I), base noise 0.1 or
    exp(0.5 N(0,1)), y = X'w + sqrt(s0) N(0,1), base prior Diagonal(exp(0.3 N(0,1))) or BB'/D + I."""
    rng = np.random.Generator(np.random.PCG64(seed))
    out = []
    for _ in range(nb):
        X = np.asfortranarray(rng.standard_normal((D, N)))
        w = rng.standard_normal(D)
        mw = np.zeros(D) if zero_mean else 0.3 * rng.standard_normal(D)
        s0 = np.exp(0.5 * rng.standard_normal(N)) if noise == "diag" else np.float64(0.1)
        y = X.T @ w + np.sqrt(s0) * rng.standard_normal(N)
        if prior == "dense":
            Bm = rng.standard_normal((D, D))
            L0 = Bm @ Bm.T / D + np.eye(D)
        else:
            L0 = np.exp(0.3 * rng.standard_normal(D))
        out.append((X, y, s0, mw, L0))
    return out


def _grid(nb, shared, seed=5):
    """(alpha [nb, 25], tau [nb, 25]): the 5 x 5 grid of 10^(-2..2), prior scale slowest; per regressor a permutation of it"""
    a, t = np.repeat(SCALES, 5), np.tile(SCALES, 5)
    if shared:
        return np.tile(a, (nb, 1)), np.tile(t, (nb, 1))
    rng = np.random.Generator(np.random.PCG64(seed))
    perms = [rng.permutation(25) for _ in range(nb)]
    return np.stack([a[p] for p in perms]), np.stack([t[p] for p in perms])


def _call(B, probs, alpha, tau, layout="col", dtype=np.float64, shared=False, want_post=True, want_best=True, sentinel=None):
    """blr_logpdf_grid_* through the Handle, host memspace -> (logpdf [nb, G], info, best, mw_best [nb, D], T_best [nb, D, D])"""
    A = B._abi
    nb = len(probs)
    D, N = probs[0][0].shape
    G = alpha.shape[1]
    if layout == "col":
        Xb = np.stack([np.asfortranarray(p[0], dtype=dtype).reshape(-1, order="F") for p in probs])
        lay, ldx = A.LAYOUT_COLVECS, max(D, 1)
    else:  # N x D column-major
        Xb = np.stack([np.asfortranarray(p[0].T, dtype=dtype).reshape(-1, order="F") for p in probs])
        lay, ldx = A.LAYOUT_ROWVECS, max(N, 1)
    yb = np.stack([np.asarray(p[1], dtype=dtype) for p in probs])
    diag = np.ndim(probs[0][2]) == 1
    sb = np.stack([np.asarray(p[2], dtype=dtype).reshape(-1) for p in probs])
    mwb = np.stack([np.asarray(p[3], dtype=dtype) for p in probs])
    dense = np.ndim(probs[0][4]) == 2
    Lb = np.stack([np.asfortranarray(p[4], dtype=dtype).reshape(-1, order="F") for p in probs])
    al = np.ascontiguousarray(alpha[0] if shared else alpha, dtype=dtype)
    ta = np.ascontiguousarray(tau[0] if shared else tau, dtype=dtype)
    lp = np.full((nb, G), 12345.0)
    info = np.full((nb, G), -7, dtype=np.int32)
    best = np.full(nb, -9, dtype=np.int64) if want_best else None
    fill = np.nan if sentinel is None else sentinel
    mwp = np.full((nb, D), fill, dtype=dtype) if want_post else None
    Tp = np.full((nb, D * D), fill, dtype=dtype) if want_post else None
    B._abi.default_handle().logpdf_grid(
        dtype, A.MEM_HOST, lay, nb, D, N, Xb, ldx, Xb.shape[1], yb, yb.shape[1], A.NOISE_DIAGONAL if diag else A.NOISE_ISOTROPIC, sb,
        sb.shape[1], A.PRIOR_DENSE if dense else A.PRIOR_DIAGONAL, mwb, D, Lb, max(D, 1), Lb.shape[1], G, al, 0 if shared else G, ta,
        0 if shared else G, lp, G, best, mwp, D, Tp, max(D, 1), D * D, info, G)
    Tm = Tp.reshape(nb, D, D).transpose(0, 2, 1) if want_post else None  # column-major D x D per regressor
    return lp, info, best, mwp, Tm


def _oracle(p, a, t):
    X, y, s0, mw, L0 = p
    lp = O.logpdf_literal(mw, a * L0, X, t * s0, y)
    m, T, A = O.posterior_literal(mw, a * L0, X, t * s0, y)
    return lp, m, T, A


def _assert_conditioned(p, a, t):
    """the issue's precondition, on the CPU: the oracle's two formulations agree to a tenth of the bounds at this setting"""
    X, y, s0, mw, L0 = p
    lp, m, _, A = _oracle(p, a, t)
    md, _, Ad, lpd = O.posterior_logpdf_direct(mw, a * L0, X, t * s0 if np.ndim(s0) else np.float64(t * s0), y)
    assert abs(lpd - lp) <= 0.1 * TOL_LP * abs(lp), ("ill-conditioned case: re-draw", a, t)
    assert np.linalg.norm(md - m) <= 0.1 * TOL_MW * np.linalg.norm(m), ("ill-conditioned case: re-draw", a, t)
    assert np.max(np.abs(Ad - A)) <= 0.1 * TOL_A * np.max(np.abs(A)), ("ill-conditioned case: re-draw", a, t)
    return lp, m, A


# (D, N, layout, noise, prior, zero mean, nb, shared grid): every shape of the issue; layouts, noise and prior kinds, means, B in
# {1, 5} and shared / per-regressor grids rotate over them; 40, 72 and 90 are the widths of 3, 5 and 6 blocks of 16 rows, which
# no other shape runs (grid_small_nb<T, NB>)
CASES = [
    (7, 13, "col", "iso", "diag", True, 1, True),
    (7, 13, "row", "diag", "dense", False, 5, False),
    (3, 11, "col", "diag", "dense", False, 5, True),
    (3, 11, "row", "iso", "diag", True, 1, False),
    (32, 150, "col", "diag", "dense", False, 1, True),
    (32, 150, "row", "iso", "diag", False, 5, False),
    (40, 150, "col", "iso", "dense", False, 5, True),
    (40, 150, "row", "diag", "diag", True, 1, False),
    (64, 700, "col", "diag", "dense", True, 5, True),
    (64, 700, "row", "iso", "dense", False, 1, True),
    (72, 700, "col", "diag", "diag", False, 1, True),
    (72, 700, "row", "iso", "dense", False, 5, False),
    (90, 150, "col", "iso", "diag", True, 5, False),
    (90, 150, "row", "diag", "dense", False, 1, True),
    (100, 150, "col", "iso", "dense", False, 1, True),
    (100, 150, "row", "diag", "diag", True, 5, False),
    (128, 700, "col", "iso", "diag", False, 5, False),
    (128, 700, "row", "diag", "dense", False, 1, True),
    (128, 4096, "col", "iso", "dense", False, 1, True),
    (128, 4096, "col", "diag", "diag", True, 1, True),
    (128, 4096, "row", "diag", "dense", False, 5, False),
    (200, 400, "col", "diag", "dense", False, 1, True),
    (200, 400, "row", "iso", "diag", False, 5, False),
]
_IDS = ["-".join(map(str, c)) for c in CASES]


def _batched_reference(B, p, a_row, t_row):
    """blr_posterior_batched_f64 with strideX = 0, stridey = 0 and the G scaled (s, Lw) pairs: the parent's way to the same numbers"""
    A = B._abi
    X, y, s0, mw, L0 = p
    D, N = X.shape
    G = a_row.size
    diag, dense = np.ndim(s0) == 1, np.ndim(L0) == 2
    sb = np.stack([np.asarray(t * s0, dtype=np.float64).reshape(-1) for t in t_row])
    Lb = np.stack([np.asfortranarray(a * L0).reshape(-1, order="F") for a in a_row])
    lp, info = np.zeros(G), np.zeros(G, dtype=np.int32)
    B._abi.default_handle().posterior_batched(
        np.float64, A.MEM_HOST, A.LAYOUT_COLVECS, G, D, N, np.asfortranarray(X), D, 0, np.ascontiguousarray(y), 0,
        A.NOISE_DIAGONAL if diag else A.NOISE_ISOTROPIC, sb, sb.shape[1], A.PRIOR_DENSE if dense else A.PRIOR_DIAGONAL,
        np.ascontiguousarray(mw), 0, Lb, D, Lb.shape[1], None, D, None, D, D * D, None, D, D * D, lp, info)
    return lp, info


@pytest.mark.parametrize("case", CASES, ids=_IDS)
def test_grid_against_oracle_and_library_f64(B, case):
    """1, 2 and the oracle half of 3: every setting against logpdf_literal / posterior_literal (1e-10 / 1e-9 / 1e-9) after the CPU
    conditioning check, against blr_posterior_batched_f64 on the scaled operands (1e-10), the winner's posterior against the oracle."""
    D, N, layout, noise, prior, zero_mean, nb, shared = case
    probs = _problem(1000 + D * 7 + N + nb, D, N, noise, prior, zero_mean, nb)
    alpha, tau = _grid(nb, shared)
    lp, info, best, mwp, Tm = _call(B, probs, alpha, tau, layout=layout, shared=shared)
    assert np.all(info == 0)
    for b, p in enumerate(probs):
        ref = np.empty(25)
        for g in range(25):
            ref[g], m_o, A_o = _assert_conditioned(p, alpha[b, g], tau[b, g])
            assert abs(lp[b, g] - ref[g]) <= TOL_LP * abs(ref[g]), (b, g, lp[b, g], ref[g])
        k = int(best[b])
        assert k == int(np.argmax(np.where(np.isnan(lp[b]), -np.inf, lp[b])))
        _, m_o, _, A_o = _oracle(p, alpha[b, k], tau[b, k])
        T = Tm[b]
        assert np.all(np.tril(T, -1) == 0)
        e_m = np.linalg.norm(mwp[b] - m_o) / np.linalg.norm(m_o)
        e_A = np.max(np.abs(T.T @ T - A_o)) / np.max(np.abs(A_o))
        assert e_m <= TOL_MW and e_A <= TOL_A, (b, k, e_m, e_A)
        lib, lib_info = _batched_reference(B, p, alpha[b], tau[b])
        assert np.all(lib_info == 0)
        assert np.max(np.abs(lp[b] - lib) / np.abs(lib)) <= TOL_LP


def test_grid_d1024_against_oracle_f64(B):
    """(1024, 1100), G = 4: the D > 128 route, same bounds; the conditioning check decides whether the case stands"""
    p = _problem(4321, 1024, 1100, "diag", "dense", False)[0]
    alpha = np.array([[0.1, 1.0, 1.0, 10.0]])
    tau = np.array([[1.0, 1.0, 10.0, 0.1]])
    lp, info, best, mwp, Tm = _call(B, [p], alpha, tau)
    assert np.all(info == 0)
    for g in range(4):
        ref, _, _ = _assert_conditioned(p, alpha[0, g], tau[0, g])
        assert abs(lp[0, g] - ref) <= TOL_LP * abs(ref)
    k = int(best[0])
    assert k == int(np.argmax(lp[0]))
    _, m_o, _, A_o = _oracle(p, alpha[0, k], tau[0, k])
    assert np.linalg.norm(mwp[0] - m_o) <= TOL_MW * np.linalg.norm(m_o)
    assert np.max(np.abs(Tm[0].T @ Tm[0] - A_o)) <= TOL_A * np.max(np.abs(A_o))


def _fp32(p):
    return (p[0].astype(np.float32), p[1].astype(np.float32), np.asarray(p[2], dtype=np.float32), p[3].astype(np.float32),
            p[4].astype(np.float32))


def _fp32_one_setting(B, p32, a32, t32, layout, what):
    """a one-setting fp32 grid -- the entry's (mw_best, T_best, evidence) are this setting's -- held to 4 x fp32 LAPACK's error"""
    X32, y32, s32, mw32, L32 = p32
    lp, info, best, mwp, Tm = _call(B, [p32], np.array([[a32]]), np.array([[t32]]), layout=layout, dtype=np.float32)
    assert info[0, 0] == 0 and best[0] == 0
    T = np.triu(Tm[0].astype(np.float64))
    _assert_fp32_within_lapack(mw32, a32 * L32, X32, np.asarray(t32 * s32, dtype=np.float32), y32, mwp[0], T.T @ T, lp[0, 0],
                               got_T=Tm[0], what=what)
    return lp[0, 0], mwp[0], Tm[0]


# every shape of the issue's list in fp32, the same rotation of layouts / kinds as the fp64 cases; (1024, 1100) with G = 4
FP32_CASES = [c[:6] for c in CASES if c[6] == 1 or c[0] in (3, 40, 72, 90, 100, 200)] + [(1024, 1100, "col", "diag", "dense", False)]


@pytest.mark.parametrize("case", FP32_CASES, ids=lambda c: "-".join(map(str, c)))
def test_grid_fp32_within_lapack(B, case):
    """fp32: per setting, 4 x the error fp32 LAPACK makes on the same fp32-rounded inputs (tests/_yardsticks.py, unchanged)"""
    D, N, layout, noise, prior, zero_mean = case
    p32 = _fp32(_problem(2000 + D + N, D, N, noise, prior, zero_mean)[0])
    a_all, t_all = _grid(1, True)
    if D > 128 and N > 1000:
        a_all, t_all = np.array([[0.1, 1.0, 1.0, 10.0]]), np.array([[1.0, 1.0, 10.0, 0.1]])
    for g in range(a_all.shape[1]):
        _fp32_one_setting(B, p32, np.float32(a_all[0, g]), np.float32(t_all[0, g]), layout, (case, g))


@pytest.mark.parametrize("case", [(100, 150, "row", "diag", "dense", False), (128, 2100, "col", "iso", "diag", False)],
                         ids=lambda c: "-".join(map(str, c)))
def test_grid_fp32_full_grid_batch(B, case):
    """fp32 with the B axis, per-regressor 25-setting grids (stride_alpha / stride_tau = G), argmax and refit at best[b] != 0: every
    evidence of the full call is, bit for bit, that of the one-setting call which is held to the fp32 yardstick together with its
    posterior; the winner's posterior is that call's too."""
    D, N, layout, noise, prior, zero_mean = case
    probs = [_fp32(p) for p in _problem(2500 + D, D, N, noise, prior, zero_mean, 5)]
    alpha, tau = _grid(5, False)
    lp, info, best, mwp, Tm = _call(B, probs, alpha, tau, layout=layout, dtype=np.float32)
    assert np.all(info == 0) and np.any(best != 0)
    for b, p32 in enumerate(probs):
        k = int(best[b])
        assert k == int(np.argmax(lp[b]))
        for g in range(25):
            lp1, mw1, T1 = _fp32_one_setting(B, p32, np.float32(alpha[b, g]), np.float32(tau[b, g]), layout, (case, b, g))
            assert lp1 == lp[b, g]
            if g == k:
                assert np.array_equal(mw1, mwp[b]) and np.array_equal(T1, Tm[b])


def test_argmax_ties_and_refit_position_independence(B):
    p = _problem(31, 128, 700, "iso", "diag", False)[0]
    alpha, tau = _grid(1, True)
    lp, info, best, mwp, Tm = _call(B, [p], alpha, tau)
    k = int(best[0])
    assert k == int(np.argmax(np.where(np.isnan(lp[0]), -np.inf, lp[0])))
    assert 5 <= k < 20 and k % 5 not in (0, 4)  # the maximum sits inside the 5 x 5 grid
    # the winner alone: same bits of evidence and posterior
    lp1, _, best1, mw1, T1 = _call(B, [p], alpha[:, k:k + 1], tau[:, k:k + 1])
    assert best1[0] == 0 and lp1[0, 0] == lp[0, k]
    assert np.array_equal(mw1, mwp) and np.array_equal(T1, Tm)
    # a repeated setting: the first one wins
    a2 = np.concatenate([alpha[0, :3], alpha[0, k:k + 1], alpha[0, 3:]])[None]
    t2 = np.concatenate([tau[0, :3], tau[0, k:k + 1], tau[0, 3:]])[None]
    lp2, _, best2, mw2, T2 = _call(B, [p], a2, t2)
    assert best2[0] == 3 and lp2[0, 3] == lp[0, k] and lp2[0, k + 1] == lp[0, k]
    assert np.array_equal(mw2, mwp) and np.array_equal(T2, Tm)


@pytest.mark.parametrize("shape", [(32, 150), (128, 4096), (200, 400)], ids=str)
def test_independence_and_determinism(B, shape):
    D, N = shape
    probs = _problem(77, D, N, "diag", "dense", False, 5)
    alpha, tau = _grid(5, False)
    r1 = _call(B, probs, alpha, tau)
    r2 = _call(B, probs, alpha, tau)
    for x, y in zip(r1, r2):
        assert np.array_equal(x, y)  # same bits on a second call
    one = _call(B, [probs[3]], alpha[3:4], tau[3:4])
    for x, y in zip(r1, one):
        assert np.array_equal(x[3:4], y)  # regressor 3 of B = 5 equals the same data at B = 1
    g = 11
    alone = _call(B, [probs[3]], alpha[3:4, g:g + 1], tau[3:4, g:g + 1])
    assert alone[0][0, 0] == r1[0][3, g] and alone[1][0, 0] == r1[1][3, g]  # setting g of G = 25 equals the same setting alone


def test_host_and_device_memspace_same_bits(B):
    A = B._abi
    from blr_amd.regressor import _DeviceBuffer

    D, N, G = 64, 700, 25
    p = _problem(55, D, N, "diag", "diag", False)[0]
    alpha, tau = _grid(1, True)
    host = _call(B, [p], alpha, tau)
    h = A.default_handle()
    X, y, s0, mw, L0 = p
    bufs = [_DeviceBuffer.of(h, np.ascontiguousarray(a)) for a in (X.reshape(-1, order="F"), y, s0, mw, L0, alpha[0], tau[0])]
    outs = [_DeviceBuffer(h, G * 8), _DeviceBuffer(h, G * 4), _DeviceBuffer(h, 8), _DeviceBuffer(h, D * 8), _DeviceBuffer(h, D * D * 8)]
    try:
        dX, dy, ds, dmw, dL, da, dt = (b.ptr for b in bufs)
        dlp, dinfo, dbest, dmwp, dT = (b.ptr for b in outs)
        h.logpdf_grid(np.float64, A.MEM_DEVICE, A.LAYOUT_COLVECS, 1, D, N, dX, D, 0, dy, 0, A.NOISE_DIAGONAL, ds, 0, A.PRIOR_DIAGONAL,
                      dmw, 0, dL, 1, 0, G, da, 0, dt, 0, dlp, G, dbest, dmwp, D, dT, D, D * D, dinfo, G)
        lp, info, best = np.empty(G), np.empty(G, dtype=np.int32), np.empty(1, dtype=np.int64)
        mwp, T = np.empty(D), np.empty(D * D)
        for host_a, d in ((lp, dlp), (info, dinfo), (best, dbest), (mwp, dmwp), (T, dT)):
            h.memcpy_d2h(host_a, d)
    finally:
        for b in bufs + outs:
            b.free()
    assert np.array_equal(lp, host[0][0]) and np.array_equal(info, host[1][0]) and best[0] == host[2][0]
    assert np.array_equal(mwp, host[3][0]) and np.array_equal(T.reshape(D, D).T, host[4][0])


@pytest.mark.parametrize("D,N", [(32, 150), (128, 700), (200, 400)])
def test_failures_stay_local(B, D, N):
    probs = _problem(99, D, N, "diag", "dense", False, 3)
    alpha, tau = _grid(3, True)
    a_bad, t_bad = alpha.copy(), tau.copy()
    a_bad[:, 2] = 0.0
    t_bad[:, 7] = -1.0
    t_bad[:, 13] = np.nan
    good = _call(B, probs, alpha, tau)
    bad = _call(B, probs, a_bad, t_bad)
    keep = np.array([g for g in range(25) if g not in (2, 7, 13)])
    for g in (2, 7, 13):
        assert np.all(bad[1][:, g] == 1) and np.all(np.isnan(bad[0][:, g]))
    assert np.array_equal(bad[0][:, keep], good[0][:, keep]) and np.all(bad[1][:, keep] == 0)
    without = _call(B, probs, a_bad[:, keep], t_bad[:, keep])
    assert np.array_equal(without[0], bad[0][:, keep])  # bit-identical to a call without the bad settings
    # a base prior with a negative eigenvalue fails all G settings of that regressor only
    X, y, s0, mw, L0 = probs[1]
    w, V = np.linalg.eigh(L0)
    w[0] = -0.5
    broken = list(probs)
    broken[1] = (X, y, s0, mw, (V * w) @ V.T)
    r = _call(B, broken, alpha, tau, sentinel=-3.25)
    info_o = _batched_reference(B, broken[1], alpha[1, :1], tau[1, :1])[1][0]
    assert info_o > 0 and np.all(r[1][1] == info_o) and np.all(np.isnan(r[0][1]))
    assert r[2][1] == -1 and np.all(r[3][1] == -3.25) and np.all(r[4][1] == -3.25)  # untouched
    for b in (0, 2):
        assert np.array_equal(r[0][b], good[0][b]) and r[2][b] == good[2][b] and np.array_equal(r[3][b], good[3][b])


def test_python_surface(B):
    D, N = 7, 40
    X, y, s0, mw, L0 = _problem(3, D, N, "diag", "dense", False)[0]
    f = B.BayesianLinearRegressor(mw, L0)
    fx = f(B.ColVecs(X), B.Diagonal(s0))
    ps, ns = [0.1, 1.0, 10.0], [0.5, 1.0, 2.0, 4.0]
    g = B.logpdf_grid(fx, y, ps, ns)
    assert g.logpdf.shape == (3, 4)
    for i, a in enumerate(ps):
        for j, t in enumerate(ns):
            ref = O.logpdf_literal(mw, a * L0, X, t * s0, y)
            assert abs(g.logpdf[i, j] - ref) <= TOL_LP * abs(ref)
    assert g.best == tuple(int(v) for v in np.unravel_index(np.argmax(g.logpdf), g.logpdf.shape))
    assert B.logpdf_grid(fx, y).logpdf.shape == (1, 1)
    post, g2 = B.posterior_best(fx, y, ps, ns)
    assert isinstance(post.Lw, B.Symmetric) and np.array_equal(g2.logpdf, g.logpdf)
    m_o, _, A_o = O.posterior_literal(mw, ps[g.best[0]] * L0, X, ns[g.best[1]] * s0, y)
    np.testing.assert_allclose(post.mw, m_o, rtol=1e-9)
    U = np.linalg.cholesky(L0).T
    post_pd, _ = B.posterior_best(B.BayesianLinearRegressor(mw, B.PDMat(U))(B.ColVecs(X), B.Diagonal(s0)), y, ps, ns)
    assert isinstance(post_pd.Lw, B.PDMat)
    np.testing.assert_allclose(post_pd.mw, m_o, rtol=1e-9)
    # many data sets of one shape: the same bits as a loop
    probs = _problem(4, D, N, "diag", "dense", False, 4)
    fxs = [B.BayesianLinearRegressor(q[3], q[4])(B.ColVecs(q[0]), B.Diagonal(q[2])) for q in probs]
    ys = [q[1] for q in probs]
    many = B.logpdf_grid_map(fxs, ys, ps, ns)
    for fx_b, y_b, m in zip(fxs, ys, many):
        one = B.logpdf_grid(fx_b, y_b, ps, ns)
        assert np.array_equal(one.logpdf, m.logpdf) and one.best == m.best
    # basis functions: the oracle's phi_test
    rng = np.random.Generator(np.random.PCG64(8))
    Xin = rng.standard_normal((3, 25))
    yb = rng.standard_normal(25)
    blr2 = B.BayesianLinearRegressor(np.zeros(2), B.Diagonal(np.ones(2)))
    phi = lambda x: B.ColVecs(O.phi_test(x.X))  # noqa: E731
    gb = B.logpdf_grid(B.BasisFunctionRegressor(blr2, phi)(B.ColVecs(Xin), 0.3), yb, ps, ns)
    gp = B.logpdf_grid(blr2(B.ColVecs(O.phi_test(Xin)), 0.3), yb, ps, ns)
    assert np.array_equal(gb.logpdf, gp.logpdf)
    with pytest.raises(ValueError, match="dense"):
        B.logpdf_grid(f(B.ColVecs(X), np.eye(N)), y, ps, ns)


@pytest.mark.parametrize("D,N", [(64, 700), (128, 4096), (200, 400)])
def test_bad_base_noise_fails_every_setting_with_its_index(B, D, N):
    """a non-positive base noise entry s_i: info = i for all G settings (what blr_posterior_batched_* reports), at one and at
    several column blocks of the statistics pass; isotropic: observation 1"""
    probs = _problem(61, D, N, "diag", "diag", False, 2)
    alpha, tau = _grid(2, True)
    good = _call(B, probs, alpha, tau, sentinel=-3.25)
    i = (2 * N) // 3  # (N = 4096: inside the third column block)
    X, y, s0, mw, L0 = probs[1]
    s_bad = s0.copy()
    s_bad[i] = -0.5
    s_bad[i + 7] = 0.0
    r = _call(B, [probs[0], (X, y, s_bad, mw, L0)], alpha, tau, sentinel=-3.25)
    assert _batched_reference(B, (X, y, s_bad, mw, L0), alpha[1, :1], tau[1, :1])[1][0] == i + 1
    assert np.all(r[1][1] == i + 1) and np.all(np.isnan(r[0][1])) and r[2][1] == -1
    assert np.all(r[3][1] == -3.25) and np.all(r[4][1] == -3.25)
    assert np.array_equal(r[0][0], good[0][0]) and np.all(r[1][0] == 0) and np.array_equal(r[3][0], good[3][0])
    iso = [(q[0], q[1], np.float64(-0.1 if b == 1 else 0.1), q[3], q[4]) for b, q in enumerate(probs)]
    r = _call(B, iso, alpha, tau)
    assert np.all(r[1][1] == 1) and np.all(np.isnan(r[0][1])) and np.all(r[1][0] == 0)


@pytest.mark.parametrize("D", [7, 128, 200])
def test_no_observations(B, D):
    """N = 0: the evidence is 0 for every setting (as blr_posterior_batched_* gives: to rounding of the two log-determinants),
    the posterior is the scaled prior"""
    rng = np.random.Generator(np.random.PCG64(17))
    L0 = np.exp(0.3 * rng.standard_normal(D))
    mw = rng.standard_normal(D)
    p = (np.zeros((D, 0), order="F"), np.zeros(0), np.float64(0.1), mw, L0)
    alpha, tau = _grid(1, True)
    lp, info, best, mwp, Tm = _call(B, [p], alpha, tau)
    assert np.all(info == 0)
    lib = _batched_reference(B, p, alpha[0], tau[0])[0]
    assert np.all(np.abs(lp) <= 1e-10) and np.all(np.abs(lib) <= 1e-10)
    k = int(best[0])
    assert k == int(np.argmax(lp[0]))
    np.testing.assert_array_equal(mwp[0], mw)
    np.testing.assert_allclose(np.diag(Tm[0]) ** 2, alpha[0, k] * L0, rtol=1e-10)


def test_null_scales_null_best_and_error_text(B):
    """alpha = NULL / tau = NULL mean all ones; best may be NULL; the factor-prior argument error carries its text"""
    A = B._abi
    D, N, G = 32, 150, 3
    X, y, s0, mw, L0 = _problem(71, D, N, "diag", "dense", False)[0]
    ones = np.ones((1, G))
    ref = _call(B, [(X, y, s0, mw, L0)], ones, ones)
    h = A.default_handle()
    Xf, Lf = np.asfortranarray(X), np.asfortranarray(L0)
    for al, ta in ((None, None), (None, np.ones(G)), (np.ones(G), None)):
        lp, info = np.zeros(G), np.full(G, -7, dtype=np.int32)
        mwp, Tp = np.zeros(D), np.zeros((D, D), order="F")
        h.logpdf_grid(np.float64, A.MEM_HOST, A.LAYOUT_COLVECS, 1, D, N, Xf, D, 0, y, 0, A.NOISE_DIAGONAL, s0, 0, A.PRIOR_DENSE, mw, 0, Lf,
                      D, 0, G, al, 0, ta, 0, lp, G, None, mwp, D, Tp, D, D * D, info, G)
        assert np.array_equal(lp, ref[0][0]) and np.all(info == 0)
        assert np.array_equal(mwp, ref[3][0]) and np.array_equal(Tp, ref[4][0])
    lp_o = O.logpdf_literal(mw, L0, X, s0, y)
    assert abs(ref[0][0, 0] - lp_o) <= TOL_LP * abs(lp_o)
    with pytest.raises(A.BLRError, match="pass a carried-forward factor as U'U") as e:
        h.logpdf_grid(np.float64, A.MEM_HOST, A.LAYOUT_COLVECS, 1, D, N, Xf, D, 0, y, 0, A.NOISE_DIAGONAL, s0, 0, A.PRIOR_UPPER_FACTOR, mw,
                      0, Lf, D, 0, G, None, 0, None, 0, np.zeros(G), G, None, None, D, None, D, D * D, np.zeros(G, dtype=np.int32), G)
    assert e.value.code == -15
    with pytest.raises(A.BLRError) as e:  # one workgroup per (regressor, setting): B max(G, 8) < 2^24, checked before anything runs
        h.logpdf_grid(np.float64, A.MEM_HOST, A.LAYOUT_COLVECS, 1 << 23, D, N, Xf, D, 0, y, 0, A.NOISE_DIAGONAL, s0, 0, A.PRIOR_DENSE, mw,
                      0, Lf, D, 0, G, None, 0, None, 0, np.zeros(G), G, None, None, D, None, D, D * D, np.zeros(G, dtype=np.int32), G)
    assert e.value.code == -21


def test_more_regressors_than_a_grid_dimension_y_holds(B):
    """B > 65535 with several column blocks (N >= 2048): 70000 regressors that share one data set (all strides 0) give, each,
    the bits of the same data at B = 1"""
    A = B._abi
    D, N, G, nb = 7, 2100, 2, 70000
    X, y, s0, mw, L0 = _problem(81, D, N, "diag", "diag", False)[0]
    al, ta = np.array([[0.5, 2.0]]), np.array([[1.0, 3.0]])
    one = _call(B, [(X, y, s0, mw, L0)], al, ta, shared=True)
    lp, info, best = np.zeros((nb, G)), np.full((nb, G), -7, dtype=np.int32), np.full(nb, -9, dtype=np.int64)
    mwp = np.zeros((nb, D))
    A.default_handle().logpdf_grid(np.float64, A.MEM_HOST, A.LAYOUT_COLVECS, nb, D, N, np.asfortranarray(X), D, 0, y, 0, A.NOISE_DIAGONAL,
                                   s0, 0, A.PRIOR_DIAGONAL, mw, 0, L0, 1, 0, G, al[0].copy(), 0, ta[0].copy(), 0, lp, G, best, mwp, D,
                                   None, D, D * D, info, G)
    assert np.all(info == 0) and np.all(best == one[2][0])
    assert np.all(lp == one[0][0][None, :]) and np.all(mwp == one[3][0][None, :])
