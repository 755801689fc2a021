"""Exact leave-fold-out predictives (blr_kfold_batched_*, kfold, kfold_map, ResidentPosterior.kfold) on the GPU:
brute-force refits with the CPU oracle on a toy problem, F = 1 against blr_loo_batched_*, a lattice of (D, N, F, layout) against the
closed form of tests/_kfold_ref.py, the resident round trip, the bit promises of the header, the NaN rule, the status, the D > 128
route and kfold_map.  All tests need an MI355X."""
import math

import numpy as np
import pytest

from oracle import blr_oracle as O

from _kfold_ref import LOG2PI, brute_force, closed_form, fp32_bounds, posterior_state, rng_of, state

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def B():
    import blr_amd

    blr_amd._abi.default_handle()  # raises if the extension or the GPU is missing: no silent fallback
    return blr_amd


@pytest.fixture(scope="module")
def h(B):
    hd = B._abi.Handle(0)
    yield hd
    hd.set_option("MAX_CHUNK", None)


def _problems(nb, D, N, dtype=np.float64, seed=0):
    """nb states (mw', T) that contain their N observations: arrays [nb, ...] of `dtype` (the state from the float64 oracle)"""
    out = []
    for b in range(nb):
        mw, U, X, s, y = state(rng_of(seed + 31 * b + D + N), D, N)
        mwp, T = posterior_state(mw, U, X, s, y)
        out.append((X, y, s, mwp, np.asfortranarray(T)))
    return [np.stack([q[i] for q in out]).astype(dtype) for i in range(5)]


def _run(B, h, X, y, s, mw, T, F, layout="col", memspace="host", want=(True, True, True, True), fill=None):
    """blr_kfold_batched_* on stacked operands X [nb, D, N], y, s [nb, N], mw [nb, D], T [nb, D, D] -> (mean, var, logpdf, total, info)"""
    A, R = B._abi, B.regressor
    nb, D, N = X.shape
    dtype = X.dtype.type
    nf = -(-N // F)
    if layout == "col":
        Xf, lay, ldx = np.stack([x.reshape(-1, order="F") for x in X]), A.LAYOUT_COLVECS, D
    else:
        Xf, lay, ldx = np.stack([x.T.reshape(-1, order="F") for x in X]), A.LAYOUT_ROWVECS, max(N, 1)
    Tf = np.stack([t.reshape(-1, order="F") for t in T])
    outs = [np.full((nb, N), np.nan if fill is None else fill, dtype=dtype), np.full((nb, N), np.nan if fill is None else fill, dtype=dtype),
            np.full((nb, nf), np.nan if fill is None else fill), np.full(nb, np.nan if fill is None else fill)]
    info = np.full(nb, -7, dtype=np.int32)
    ins = [np.ascontiguousarray(a) for a in (Xf, y, s, mw, Tf)]
    if memspace == "host":
        o = [a if w else None for a, w in zip(outs, want)]
        h.kfold(dtype, A.MEM_HOST, lay, nb, D, N, F, ins[0], ldx, D * N, ins[1], N, A.NOISE_DIAGONAL, ins[2], N, ins[3], D, ins[4], D, D * D,
                o[0], N, o[1], N, o[2], nf, o[3], info)
    else:
        bufs = [R._DeviceBuffer.of(h, a) for a in ins + outs + [info]]
        try:
            p = [b.ptr for b in bufs]
            o = [q if w else None for q, w in zip(p[5:9], want)]
            h.kfold(dtype, A.MEM_DEVICE, lay, nb, D, N, F, p[0], ldx, D * N, p[1], N, A.NOISE_DIAGONAL, p[2], N, p[3], D, p[4], D, D * D,
                    o[0], N, o[1], N, o[2], nf, o[3], p[9])
            for host, ptr in zip(outs + [info], p[5:]):
                h.memcpy_d2h(host, ptr)
        finally:
            for b in bufs:
                b.free()
    return outs[0], outs[1], outs[2], outs[3], info


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


# ---- 1. brute force on a toy problem ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [1, 2, 5, 13, 64])
@pytest.mark.parametrize("prior", ["diagonal", "dense", "pdmat"])
@pytest.mark.parametrize("noise", ["isotropic", "diagonal"])
def test_brute_force_toy(B, prior, noise, F):
    rng = rng_of(1)
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
    r = B.kfold(f(X, Sy), y, F)
    nf = -(-N // F)
    assert isinstance(r, B.KFold) and r.logpdf.dtype == np.float64 and r.logpdf.shape == (nf,) and r.mean.shape == (N,) and r.var.shape == (N,)
    m_o, v_o, lp_o = brute_force(mw, Lw_d, np.asarray(X), np.array(np.broadcast_to(s, (N,))), y, F)
    print("toy", prior, noise, F, np.max(np.abs(r.mean - m_o)), np.max(np.abs(r.var / v_o - 1)), np.max(np.abs(r.logpdf / lp_o - 1)))
    np.testing.assert_allclose(r.mean, m_o, rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(r.var, v_o, rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(r.logpdf, lp_o, rtol=1e-9, atol=1e-12)
    assert r.total == pytest.approx(math.fsum(r.logpdf), rel=1e-12)


# ---- 2. F = 1 against blr_loo_batched_* ------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,N", [(64, 150), (128, 200)])
def test_fold_size_one_is_loo(B, h, D, N):
    X, y, s, mw, T = _problems(1, D, N)
    m, v, lp, tot, info = _run(B, h, X, y, s, mw, T, 1)
    A = B._abi
    lm, lv, ll, lt, li = np.empty(N), np.empty(N), np.empty(N), np.empty(1), np.zeros(1, dtype=np.int32)
    h.loo(np.float64, A.MEM_HOST, A.LAYOUT_COLVECS, 1, D, N, np.ascontiguousarray(X[0].reshape(-1, order="F")), D, 0, y[0], 0,
          A.NOISE_DIAGONAL, s[0], 0, mw[0], 0, np.ascontiguousarray(T[0].reshape(-1, order="F")), D, 0, lm, N, lv, N, ll, N, lt, li)
    assert info[0] == 0 and li[0] == 0
    np.testing.assert_allclose(m[0], lm, rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(v[0], lv, rtol=1e-9)
    np.testing.assert_allclose(lp[0], ll, rtol=1e-9, atol=1e-12)
    assert tot[0] == pytest.approx(lt[0], rel=1e-9)


# ---- 3. the lattice against the closed form ---------------------------------------------------------------------------------
def _lattice():
    """A pairwise-covering subset of D x N x F x layout (every pair of values of two factors occurs): 5 x 5 = 25 (D, N) pairs, F and the
    layout walking through their values at coprime steps, plus the cases the walk misses."""
    Ds, Ns, Fs, Ls = [1, 16, 17, 100, 128], [1, 63, 64, 65, 200], [1, 3, 16, 17, 33, 64], ["col", "row"]
    facs = [Ds, Ns, Fs, Ls]
    cases = set()
    for i, D in enumerate(Ds):
        for j, N in enumerate(Ns):
            cases.add((D, N, Fs[(i + j) % 6], Ls[(i + 2 * j) % 2]))
    # a partial last fold inside a partial last pack (N = 200, F = 3: packs of 63 rows, the last with 11 = 3 + 3 + 3 + 2), a fold of
    # 33 (one fold per pack, 31 rows idle), full packs with a partial last fold (N = 65, F = 16)
    cases |= {(128, 200, 3, "col"), (100, 200, 33, "row"), (17, 65, 16, "col"), (128, 200, 64, "row"), (128, 200, 17, "col")}

    def missing():
        return [(a, x, b, y) for a in range(4) for b in range(a + 1, 4) for x in facs[a] for y in facs[b]
                if not any(c[a] == x and c[b] == y for c in cases)]

    k = 0
    while True:  # complete greedily: a case for the first missing pair, its other two factors from the next missing pairs they fit
        miss = missing()
        if not miss:
            break
        a, x, b, y = miss[0]
        case = {a: x, b: y}
        for a2, x2, b2, y2 in miss[1:]:
            if all(case.get(f, v) == v for f, v in ((a2, x2), (b2, y2))):
                case.update({a2: x2, b2: y2})
        for f in range(4):
            case.setdefault(f, facs[f][k % len(facs[f])])
        k += 1
        cases.add(tuple(case[f] for f in range(4)))
    return sorted(cases)


LATTICE = _lattice()
assert len(LATTICE) <= 60


def test_lattice_is_pairwise_covering():
    cols = list(zip(*LATTICE))
    vals = [sorted(set(c), key=str) for c in cols]
    for a in range(4):
        for b in range(a + 1, 4):
            assert {(x, y) for x in vals[a] for y in vals[b]} <= set(zip(cols[a], cols[b])), (a, b)
    assert any(N % F and (N % ((64 // F) * F)) for _, N, F, _ in LATTICE)


@pytest.mark.parametrize("D,N,F,layout", LATTICE)
def test_lattice_fp64(B, h, D, N, F, layout):
    X, y, s, mw, T = _problems(2, D, N)
    m, v, lp, tot, info = _run(B, h, X, y, s, mw, T, F, layout=layout)
    assert not info.any()
    for b in range(2):
        m_o, v_o, lp_o, _ = closed_form(mw[b], T[b], X[b], s[b], y[b], F)
        np.testing.assert_allclose(m[b], m_o, rtol=1e-9, atol=1e-12)
        np.testing.assert_allclose(v[b], v_o, rtol=1e-9, atol=1e-12)
        np.testing.assert_allclose(lp[b], lp_o, rtol=1e-9, atol=1e-12)
        assert tot[b] == pytest.approx(math.fsum(lp[b]), rel=1e-12)


@pytest.mark.parametrize("D,N,F,layout", LATTICE)
def test_lattice_fp32(B, h, D, N, F, layout):
    """fp32 against the float64 closed form on the fp32-rounded inputs: 4 x the error of the same closed form in NumPy float32 on them
    plus a floor of 8 eps32 of the output's scale (tests/_kfold_ref.py fp32_bounds)."""
    X, y, s, mw, T = _problems(1, D, N, dtype=np.float32)
    m, v, lp, tot, info = _run(B, h, X, y, s, mw, T, F, layout=layout)
    assert not info.any() and m.dtype == np.float32 and lp.dtype == np.float64
    truth, bounds = fp32_bounds(mw[0], T[0], X[0], s[0], y[0], F)
    for got, t, bd, name in zip((m[0], v[0], lp[0]), truth, bounds, ("mean", "var", "logpdf")):
        err = float(np.max(np.abs(got.astype(np.float64) - t)))
        print("fp32", D, N, F, layout, name, err, bd)
        assert err <= bd, (name, err, bd)
    assert tot[0] == pytest.approx(math.fsum(lp[0]), rel=1e-12)


# ---- 4. the resident round trip ----------------------------------------------------------------------------------------------
def test_resident_kfold_matches_forget_predict_condition(B):
    D, N, F = 64, 150, 25
    mw, U, X, s, y = state(rng_of(4), D, N)
    st = B.ResidentPosterior(B.BayesianLinearRegressor(mw, B.PDMat(U)))
    st.condition(B.ColVecs(X), B.Diagonal(s), y)
    m0, T0 = st.state()
    r = st.kfold(B.ColVecs(X), B.Diagonal(s), y, F)
    m1, T1 = st.state()
    assert np.array_equal(m0, m1) and np.array_equal(T0, T1)  # the state is not modified
    assert r.logpdf.shape == (6,) and r.total == pytest.approx(math.fsum(r.logpdf), rel=1e-12)
    for f in range(6):
        a, b = f * F, min((f + 1) * F, N)
        xf, sf, yf = B.ColVecs(np.asfortranarray(X[:, a:b])), B.Diagonal(s[a:b]), y[a:b]
        st.forget(xf, sf, yf)
        m, C = st.mean_and_cov(xf, sf)
        st.condition(xf, sf, yf)
        L = np.linalg.cholesky(C)
        u = np.linalg.solve(L, yf - m)
        lp = -0.5 * ((b - a) * LOG2PI + 2 * np.sum(np.log(np.diag(L))) + u @ u)
        np.testing.assert_allclose(r.mean[a:b], m, rtol=1e-8, atol=1e-10)
        np.testing.assert_allclose(r.var[a:b], np.diag(C), rtol=1e-8)
        assert r.logpdf[f] == pytest.approx(lp, rel=1e-8)


# ---- 5. bit promises -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_bits_do_not_depend_on_batch_position_chunks_memspace_or_outputs(B, h, dtype):
    nb, D, N, F = 7, 33, 150, 8
    X, y, s, mw, T = _problems(nb, D, N, dtype=dtype)
    h.set_option("MAX_CHUNK", None)
    ref = _run(B, h, X, y, s, mw, T, F)
    assert not ref[4].any() and not any(np.isnan(a).any() for a in ref[:4])
    assert h.get_stat("last_chunks") == 1
    again = _run(B, h, X, y, s, mw, T, F)
    assert all(_same(a, b) for a, b in zip(ref, again))                       # call to call
    for b in (0, 3, 6):                                                       # B = 7 against B = 1
        one = _run(B, h, *(a[b:b + 1] for a in (X, y, s, mw, T)), F)
        assert all(_same(a[b:b + 1], o) for a, o in zip(ref[:4], one[:4])), b
    perm = np.array([4, 0, 6, 2, 5, 1, 3])                                    # a permuted batch
    pr = _run(B, h, *(a[perm] for a in (X, y, s, mw, T)), F)
    assert all(_same(a[perm], o) for a, o in zip(ref[:4], pr[:4]))
    for cap, chunks in ((1, 7), (2, 4), (3, 3)):                              # chunk seams
        h.set_option("MAX_CHUNK", str(cap))
        try:
            got = _run(B, h, X, y, s, mw, T, F)
            assert h.get_stat("last_chunks") == chunks
        finally:
            h.set_option("MAX_CHUNK", None)
        assert all(_same(a, o) for a, o in zip(ref, got)), cap
    dev = _run(B, h, X, y, s, mw, T, F, memspace="device")                    # host against device memspace
    assert all(_same(a, o) for a, o in zip(ref, dev))
    for k in range(4):                                                        # each output alone
        want = tuple(i == k for i in range(4))
        alone = _run(B, h, X, y, s, mw, T, F, want=want)
        assert _same(alone[k], ref[k]), k
        assert all(np.isnan(alone[i]).all() for i in range(4) if i != k)      # the others are not touched


def test_a_fold_depends_on_its_own_data_only(B, h):
    """F = 8: eight folds share a workgroup.  New X, y and s in fold 2 alone: every other fold keeps its bits; and a fold keeps its bits
    when N shrinks (its pack then holds fewer folds) or when it lands elsewhere in a workgroup."""
    D, N, F = 33, 150, 8
    X, y, s, mw, T = _problems(1, D, N)
    ref = _run(B, h, X, y, s, mw, T, F)
    X2, y2, s2 = X.copy(), y.copy(), s.copy()
    rng = rng_of(9)
    X2[0][:, 16:24] *= 0.5
    y2[0][16:24] = rng.standard_normal(8)
    s2[0][16:24] *= 1.5
    got = _run(B, h, X2, y2, s2, mw, T, F)
    keep = np.r_[0:16, 24:N]
    assert _same(got[0][0][keep], ref[0][0][keep]) and _same(got[1][0][keep], ref[1][0][keep])
    assert _same(np.delete(got[2][0], 2), np.delete(ref[2][0], 2))
    assert not _same(got[2][0][2], ref[2][0][2]) and not np.isnan(got[2]).any()
    # the first 5 folds alone (N = 40: one pack of five folds instead of eight)
    short = _run(B, h, X[:, :, :40], y[:, :40], s[:, :40], mw, T, F)
    assert _same(short[0][0], ref[0][0][:40]) and _same(short[1][0], ref[1][0][:40]) and _same(short[2][0], ref[2][0][:5])
    # folds 3 .. 9 as folds 0 .. 6: another place in the workgroup
    moved = _run(B, h, X[:, :, 24:80], y[:, 24:80], s[:, 24:80], mw, T, F)
    assert _same(moved[0][0], ref[0][0][24:80]) and _same(moved[2][0], ref[2][0][3:10])


# ---- 6. a degenerate fold -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_degenerate_fold_is_nan_and_alone(B, h, dtype):
    nb, D, N, F = 3, 33, 150, 8
    X, y, s, mw, T = _problems(nb, D, N, dtype=dtype)
    ref = _run(B, h, X, y, s, mw, T, F)
    s2 = s.copy()
    s2[:, 24:32] *= dtype(1e-6)  # the state holds these observations with 1e6 times less weight: I - H~ is not positive definite
    before = h.get_stat("kfold_degenerate")
    got = _run(B, h, X, y, s2, mw, T, F)
    assert h.get_stat("kfold_degenerate") - before == nb
    assert not got[4].any()
    keep = np.r_[0:24, 32:N]
    for b in range(nb):
        assert np.isnan(got[0][b][24:32]).all() and np.isnan(got[1][b][24:32]).all() and np.isnan(got[2][b][3]) and np.isnan(got[3][b])
        assert _same(got[0][b][keep], ref[0][b][keep]) and _same(got[1][b][keep], ref[1][b][keep])
        assert _same(np.delete(got[2][b], 3), np.delete(ref[2][b], 3)) and not np.isnan(np.delete(got[2][b], 3)).any()


# ---- 7. status -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,N", [(33, 70), (192, 70)])
def test_status_leaves_the_outputs_untouched(B, h, D, N):
    nb, F = 3, 8
    X, y, s, mw, T = _problems(nb, D, N)
    T[0][4, 4] = -1.0   # diagonal entry 5 of the first factor
    s[2][10] = 0.0      # variance 11 of the third regressor
    m, v, lp, tot, info = _run(B, h, X, y, s, mw, T, F, fill=-123.0)
    assert list(info) == [5, 0, 11]
    for b in (0, 2):
        assert (m[b] == -123.0).all() and (v[b] == -123.0).all() and (lp[b] == -123.0).all() and tot[b] == -123.0
    m_o, v_o, lp_o, _ = closed_form(mw[1], T[1], X[1], s[1], y[1], F)
    np.testing.assert_allclose(m[1], m_o, rtol=1e-8, atol=1e-10)
    np.testing.assert_allclose(lp[1], lp_o, rtol=1e-8)
    assert tot[1] == pytest.approx(math.fsum(lp[1]), rel=1e-12)
    # N = 0: an empty sum
    z = _run(B, h, X[:, :, :0], y[:, :0], s[:, :0], mw[1:2].repeat(nb, 0), T[1:2].repeat(nb, 0), F)
    assert not z[4].any() and (z[3] == 0.0).all()


# ---- 8. the D > 128 route ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["col", "row"])
def test_large_d_route(B, h, layout):
    D, N, F = 192, 150, 48
    X, y, s, mw, T = _problems(2, D, N)
    m, v, lp, tot, info = _run(B, h, X, y, s, mw, T, F, layout=layout)
    assert not info.any()
    for b in range(2):
        m_o, v_o, lp_o, _ = closed_form(mw[b], T[b], X[b], s[b], y[b], F)
        np.testing.assert_allclose(m[b], m_o, rtol=1e-8, atol=1e-10)
        np.testing.assert_allclose(v[b], v_o, rtol=1e-8)
        np.testing.assert_allclose(lp[b], lp_o, rtol=1e-8)
        assert tot[b] == pytest.approx(math.fsum(lp[b]), rel=1e-12)
    only = _run(B, h, X, y, s, mw, T, F, layout=layout, want=(False, False, False, True))
    assert _same(only[3], tot)


# ---- 9. kfold_map, perm, a basis-function regressor ------------------------------------------------------------------------------
def test_kfold_map_is_bit_identical_to_single_calls(B):
    rng = rng_of(11)
    D, N, F, nb = 16, 70, 16, 4
    fxs, ys = [], []
    for _ in range(nb):
        mw, U, X, s, y = state(rng, D, N)
        fxs.append(B.BayesianLinearRegressor(mw, B.PDMat(U))(B.ColVecs(X), B.Diagonal(s)))
        ys.append(y)
    many = B.kfold_map(fxs, ys, F)
    for r, fx, y in zip(many, fxs, ys):
        one = B.kfold(fx, y, F)
        assert _same(r.mean, one.mean) and _same(r.var, one.var) and _same(r.logpdf, one.logpdf) and r.total == one.total
    # unequal shapes: one call per problem, the same numbers
    mw, U, X, s, y = state(rng, D, 50)
    fxs[1], ys[1] = B.BayesianLinearRegressor(mw, B.PDMat(U))(B.ColVecs(X), B.Diagonal(s)), y
    mixed = B.kfold_map(fxs, ys, F)
    assert mixed[1].logpdf.shape == (4,) and _same(mixed[0].mean, many[0].mean) and _same(mixed[3].logpdf, many[3].logpdf)
    # random folds: the same as the gathered problem, scattered back
    perm = rng.permutation(50)
    rp = B.kfold(fxs[1], ys[1], F, perm=perm)
    g = B.kfold(B.BayesianLinearRegressor(mw, B.PDMat(U))(B.ColVecs(np.asfortranarray(X[:, perm])), B.Diagonal(s[perm])), y[perm], F)
    assert _same(rp.mean[perm], g.mean) and _same(rp.var[perm], g.var) and _same(rp.logpdf, g.logpdf)


def test_basis_function_regressor_with_a_callable(B):
    rng = rng_of(12)
    N, F = 40, 8
    x = rng.standard_normal((1, N))
    phi = lambda xs: B.ColVecs(np.asfortranarray(np.vstack([np.ones(len(xs)), xs.X[0], xs.X[0] ** 2])))  # noqa: E731
    blr = B.BayesianLinearRegressor(np.zeros(3), B.Diagonal(np.ones(3)))
    y = 0.3 * x[0] ** 2 + 0.1 * rng.standard_normal(N)
    r = B.kfold(B.BasisFunctionRegressor(blr, phi)(B.ColVecs(x), 0.05), y, F)
    Phi = phi(B.ColVecs(x)).X
    m_o, v_o, lp_o = brute_force(np.zeros(3), np.eye(3), Phi, np.full(N, 0.05), y, F)
    np.testing.assert_allclose(r.mean, m_o, rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(r.var, v_o, rtol=1e-9)
    np.testing.assert_allclose(r.logpdf, lp_o, rtol=1e-9, atol=1e-12)
    (r2,) = B.kfold_map([B.BasisFunctionRegressor(blr, phi)(B.ColVecs(x), 0.05)], [y], F)
    assert _same(r2.logpdf, r.logpdf)
