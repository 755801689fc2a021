"""blr_posterior_multi_batched_* on the device: B regressors with S target columns each in one call, through the
C ABI.  Every column of every regressor is held to the oracle (posterior_literal / logpdf_literal on that column) -- fp64 at the
header's bounds for the route column 0 took, fp32 at _assert_fp32_within_lapack -- and column 0, the factor, the precision and
the status to the bits of blr_posterior_batched_* on the same handle."""
import numpy as np
import pytest

from _yardsticks import _assert_fp32_within_lapack
from blr_amd import _abi
from oracle import blr_oracle as O

pytestmark = pytest.mark.gpu

W = _abi.MULTI_COLS_PER_PASS
S_MAX = W + 1
KIND = {"diag": _abi.PRIOR_DIAGONAL, "dense": _abi.PRIOR_DENSE, "factor": _abi.PRIOR_UPPER_FACTOR}


@pytest.fixture(scope="module")
def h():
    hd = _abi.Handle()
    yield hd
    hd.close()


def _data(D, N, dtype, xkind, noise, prior, nb=3, smax=S_MAX, shared_x=False, seed=0, xscale=1.0):
    """nb regressors with smax target columns each (a call uses the first S of them).  xkind: "col16" (ColVecs, ldx = D rounded up
    to 16 bytes), "colodd" (ColVecs, odd ldx > D), "row" (RowVecs, ldx = N + 3); padding holds NaN."""
    rng = np.random.Generator(np.random.PCG64(7000 + 131 * D + N + seed))
    nx = 1 if shared_x else nb
    Xd = (xscale * rng.standard_normal((nx, D, N))).astype(dtype)
    per16 = 16 // np.dtype(dtype).itemsize
    if xkind == "row":
        layout, ldx = _abi.LAYOUT_ROWVECS, N + 3
        Xp = np.full((nx, D, ldx), np.nan, dtype=dtype)  # [d][n] with ldx per d: N x D column-major
        Xp[:, :, :N] = Xd
    else:
        layout = _abi.LAYOUT_COLVECS
        ldx = (D + 1) | 1 if xkind == "colodd" else -(-D // per16) * per16
        Xp = np.full((nx, max(N, 1), ldx), np.nan, dtype=dtype)  # [n][d] with ldx per n: D x N column-major
        Xp[:, :N, :D] = np.swapaxes(Xd, 1, 2)
    Wt = rng.standard_normal((nb, D, smax)) / np.sqrt(D) / xscale
    Yd = (np.einsum("bdn,bds->bns", np.broadcast_to(Xd.astype(float), (nb, D, N)), Wt) + 0.8 * rng.standard_normal((nb, N, smax))).astype(dtype)
    if noise == "diag":
        s = np.exp(0.3 * rng.standard_normal((nb, max(N, 1)))).astype(dtype)
        noise_kind, strides, s_of = _abi.NOISE_DIAGONAL, max(N, 1), (lambda b: s[b, :N])
    else:
        s = np.exp(0.3 * rng.standard_normal((nb, 1))).astype(dtype)
        noise_kind, strides, s_of = _abi.NOISE_ISOTROPIC, 1, (lambda b: s[b, 0])
    mw = (0.2 * rng.standard_normal((nb, D)) / xscale).astype(dtype)
    if prior == "diag":
        Lw = (np.exp(0.3 * rng.standard_normal((nb, D))) * xscale**2).astype(dtype)
        ldl, mats = 1, [Lw[b] for b in range(nb)]
    else:
        Lw, mats = np.zeros((nb, D * D), dtype=dtype), []
        for b in range(nb):
            if prior == "factor":  # entries that are multiples of 1/8: U'U is exact in fp32 too
                U = np.triu(rng.integers(-1, 2, size=(D, D)) / 8.0, 1) + np.diag(1.0 + rng.integers(0, 5, size=D) / 8.0)
                Lw[b] = U.reshape(-1, order="F")
                mats.append((U.T @ U).astype(dtype))
            else:
                Bm = rng.standard_normal((D, D)) / np.sqrt(D)
                M = (Bm @ Bm.T + np.eye(D)).astype(dtype)
                M = np.triu(M) + np.triu(M, 1).T
                Lw[b] = M.reshape(-1, order="F")
                mats.append(M)
        ldl = D
    return dict(D=D, N=N, dtype=dtype, nb=nb, layout=layout, ldx=ldx, X=Xp, strideX=0 if shared_x else Xp[0].size, Xd=Xd, Yd=Yd, s=s,
                s_of=s_of, noise_kind=noise_kind, strides=strides, prior_kind=KIND[prior], mw=mw, Lw=Lw, ldl=ldl, mats=mats, cache={},
                x_of=(lambda b: Xd[0 if shared_x else b]))


def _pack_Y(q, cols):
    """the chosen columns of every regressor as N x S column-major blocks with ldY = N + 2 and a gap of one element between regressors"""
    N, S = q["N"], len(cols)
    ldY = N + 2
    Y = np.full((q["nb"], ldY * S + 1), np.nan, dtype=q["dtype"])
    for j, c in enumerate(cols):
        Y[:, j * ldY:j * ldY + N] = q["Yd"][:, :, c]
    return Y, ldY, ldY * S + 1


def _outputs(q, S, fill=np.nan, gaps=True, nb=None):
    D, nb = q["D"], nb or q["nb"]
    g = 1 if gaps else 0
    ldmp, ldt, st_lp = D + g, D + 2 * g, S + g
    st_m, st_T = ldmp * S + 2 * g, ldt * D + 5 * g
    return dict(ldmp=ldmp, st_m=st_m, ldt=ldt, st_T=st_T, st_lp=st_lp, M=np.full(nb * st_m, fill, dtype=q["dtype"]),
                T=np.full(nb * st_T, fill, dtype=q["dtype"]), A=np.full(nb * st_T, fill, dtype=q["dtype"]), lp=np.full(nb * st_lp, fill),
                info=np.full(nb, -7, dtype=np.int32))


def _multi(hd, q, cols, o, regs=None, memspace=_abi.MEM_HOST, arrays=None, T=True):
    regs = list(range(q["nb"])) if regs is None else regs
    Y, ldY, strideY = _pack_Y(q, cols)
    sl = slice(regs[0], regs[-1] + 1)
    a = dict(X=q["X"][0:1] if q["strideX"] == 0 else q["X"][sl], Y=Y[sl], s=q["s"][sl], mw=q["mw"][sl], Lw=q["Lw"][sl], M=o["M"],
             T=o["T"] if T else None, A=o["A"], lp=o["lp"], info=o["info"])
    if arrays is not None:
        a = arrays(a)
    rc = hd.posterior_multi_batched(q["dtype"], memspace, q["layout"], len(regs), q["D"], q["N"], len(cols), a["X"], q["ldx"], q["strideX"],
                                    a["Y"], ldY, strideY, q["noise_kind"], a["s"], q["strides"], q["prior_kind"], a["mw"], q["D"], a["Lw"],
                                    q["ldl"], q["Lw"].shape[1], a["M"], o["ldmp"], o["st_m"], a["T"], o["ldt"], o["st_T"], a["A"], o["ldt"],
                                    o["st_T"], a["lp"], o["st_lp"], a["info"])
    return rc, a


def _batched_col0(hd, q, col, nb=None):
    """blr_posterior_batched_* on one column of every regressor, into outputs without gaps"""
    D, N, nb = q["D"], q["N"], nb or q["nb"]
    Y, ldY, strideY = _pack_Y(q, [col])
    mp, T, A = (np.full(nb * D, np.nan, dtype=q["dtype"]), np.full(nb * D * D, np.nan, dtype=q["dtype"]), np.full(nb * D * D, np.nan, dtype=q["dtype"]))
    lp, info = np.full(nb, np.nan), np.full(nb, -7, dtype=np.int32)
    hd.posterior_batched(q["dtype"], _abi.MEM_HOST, q["layout"], nb, D, N, q["X"], q["ldx"], q["strideX"], Y, strideY, q["noise_kind"], q["s"],
                         q["strides"], q["prior_kind"], q["mw"], D, q["Lw"], q["ldl"], q["Lw"].shape[1], mp, D, T, D, D * D, A, D, D * D, lp, info)
    return mp.reshape(nb, D), T.reshape(nb, D, D), A.reshape(nb, D, D), lp, info


def _mean(o, b, j, D):
    return o["M"][b * o["st_m"] + j * o["ldmp"]:b * o["st_m"] + j * o["ldmp"] + D]


def _mat(buf, b, D, ld, stride):
    return buf[b * stride + np.arange(D)[None, :] * ld + np.arange(D)[:, None]]


def _check(q, cols, o, i8=False, regs=None, T=True):
    """every column of every regressor against the oracle; every element outside a result must still hold NaN"""
    D, N = q["D"], q["N"]
    regs = list(range(q["nb"])) if regs is None else regs
    f64 = lambda a: np.asarray(a, dtype=np.float64)  # noqa: E731
    written = {k: np.zeros(o[k].shape, dtype=bool) for k in ("M", "T", "lp")}
    for pos, b in enumerate(regs):
        assert o["info"][pos] == 0
        Tb, Ab = _mat(o["T"], pos, D, o["ldt"], o["st_T"]), _mat(o["A"], pos, D, o["ldt"], o["st_T"])
        Xb, sb = q["x_of"](b), q["s_of"](b)
        for c in range(D):
            written["T"][pos * o["st_T"] + c * o["ldt"]:pos * o["st_T"] + c * o["ldt"] + D] = True
        for j, c in enumerate(cols):
            m, lp = _mean(o, pos, j, D), float(o["lp"][pos * o["st_lp"] + j])
            written["M"][pos * o["st_m"] + j * o["ldmp"]:pos * o["st_m"] + j * o["ldmp"] + D] = True
            written["lp"][pos * o["st_lp"] + j] = True
            yb = q["Yd"][b, :, c]
            if q["dtype"] == np.float32:
                _assert_fp32_within_lapack(q["mw"][b], q["mats"][b], np.asfortranarray(Xb), np.asarray(sb, dtype=np.float32), yb, m, Ab, lp,
                                           got_T=Tb if (j == 0 and T) else None, what=f"regressor {b} column {c}")
                continue
            if (b, c) not in q["cache"]:
                args = (f64(q["mw"][b]), f64(q["mats"][b]), f64(Xb), f64(sb), f64(yb))
                q["cache"][(b, c)] = O.posterior_literal(*args) + (O.logpdf_literal(*args),)
            mw_o, T_o, A_o, lp_o = q["cache"][(b, c)]
            if i8:  # the int8 route's error model (include/blr_mi355x.h), as tests/test_gpu_parity.py test_i8_* hold it
                dlt = f64(yb) - f64(Xb).T @ f64(q["mw"][b])
                assert abs(lp - lp_o) <= 1e-11 * abs(lp_o) + 1e-14 * float(np.sum(dlt * dlt / sb)), (b, c, lp, lp_o)
                dA = np.sqrt(np.diag(A_o))
                np.testing.assert_allclose(m * dA, mw_o * dA, rtol=1e-8, atol=1e-9 * np.abs(mw_o * dA).max())
                if j == 0:
                    assert (np.abs(Ab - A_o) / np.outer(dA, dA)).max() <= 1e-12
                continue
            assert abs(lp - lp_o) <= 1e-10 * max(1.0, abs(lp_o)), (b, c, lp, lp_o)
            np.testing.assert_allclose(m, mw_o, rtol=1e-9, atol=1e-11, err_msg=f"mean of regressor {b} column {c}")
            if j == 0:
                if T:
                    np.testing.assert_allclose(Tb, T_o, rtol=1e-9, atol=1e-11, err_msg=f"T of regressor {b}")
                np.testing.assert_allclose(Ab, A_o, rtol=1e-9, atol=1e-11, err_msg=f"Lw' of regressor {b}")
    for k in ("M", "T", "lp"):
        if k == "T" and not T:
            continue
        assert np.all(np.isfinite(o[k][written[k]])) and np.all(np.isnan(o[k][~written[k]])), k
    assert np.all(np.isnan(o["A"][~written["T"]]))


# D -> (layout / alignment, noise, prior): RowVecs, diagonal noise and every prior kind are in the lattice
VARIANT = {1: ("colodd", "iso", "diag"), 33: ("row", "diag", "dense"), 100: ("col16", "iso", "factor"), 128: ("col16", "diag", "diag")}


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("N", [0, 1, 29, 131])
@pytest.mark.parametrize("D", [1, 33, 100, 128])
def test_every_column_matches_the_oracle(h, D, N, dtype):
    q = _data(D, N, dtype, *VARIANT[D])
    for S in (1, 2, 17, W + 1):
        o = _outputs(q, S)
        rc, _ = _multi(h, q, list(range(S)), o)
        assert rc == 0
        _check(q, list(range(S)), o)


def test_int8_route_for_column_0(h):
    q = _data(128, 543, np.float64, "col16", "iso", "diag", nb=2, smax=3)
    o = _outputs(q, 3)
    assert _multi(h, q, [0, 1, 2], o)[0] == 0
    assert h.last_route().startswith("fused_i8_kernel")
    _check(q, [0, 1, 2], o, i8=True)
    ref = _batched_col0(h, q, 0)
    assert h.last_route().startswith("fused_i8_kernel")
    for b in range(2):
        assert np.array_equal(_mean(o, b, 0, 128), ref[0][b]) and o["lp"][b * o["st_lp"]] == ref[3][b]
        assert np.array_equal(_mat(o["T"], b, 128, o["ldt"], o["st_T"]), ref[1][b].T)


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_one_wave_route_and_shared_x(h, dtype):
    q = _data(64, 77, dtype, "col16", "iso", "diag", smax=5)
    o = _outputs(q, 5)
    assert _multi(h, q, list(range(5)), o)[0] == 0
    assert h.last_route().startswith("fused_wave_kernel")
    _check(q, list(range(5)), o)
    qs = _data(40, 50, dtype, "col16", "diag", "dense", smax=4, shared_x=True)
    o = _outputs(qs, 4)
    assert _multi(h, qs, list(range(4)), o)[0] == 0
    _check(qs, list(range(4)), o)


def _bits(q, o, pos, j):
    D = q["D"]
    return _mean(o, pos, j, D).tobytes() + o["lp"][pos * o["st_lp"] + j].tobytes()


@pytest.mark.parametrize("D,N,dtype,variant", [(100, 131, np.float64, ("col16", "diag", "dense")), (33, 29, np.float32, ("row", "iso", "factor")),
                                               (128, 70, np.float64, ("colodd", "iso", "diag"))])
def test_bits(h, D, N, dtype, variant):
    q = _data(D, N, dtype, *variant, smax=5)
    o = _outputs(q, 5)
    assert _multi(h, q, [0, 1, 2, 3, 4], o)[0] == 0
    # two identical calls agree
    o2 = _outputs(q, 5)
    assert _multi(h, q, [0, 1, 2, 3, 4], o2)[0] == 0
    for k in ("M", "T", "A", "lp", "info"):
        assert np.array_equal(o[k], o2[k], equal_nan=True), k
    # column 0, T_post, Lw_post and info are blr_posterior_batched_* on the same handle; S = 1 is that call entirely
    mp, T, A, lp, info = _batched_col0(h, q, 0)
    o1 = _outputs(q, 1)
    assert _multi(h, q, [0], o1)[0] == 0
    for b in range(q["nb"]):
        for oo in (o, o1):
            assert np.array_equal(_mean(oo, b, 0, D), mp[b]) and oo["lp"][b * oo["st_lp"]] == lp[b] and oo["info"][b] == info[b] == 0
            assert np.array_equal(_mat(oo["T"], b, D, oo["ldt"], oo["st_T"]), T[b].T)
            assert np.array_equal(_mat(oo["A"], b, D, oo["ldt"], oo["st_T"]), A[b].T)
    # regressor 1 alone reproduces its bits in the batch
    oa = _outputs(q, 5, nb=1)
    assert _multi(h, q, [0, 1, 2, 3, 4], oa, regs=[1])[0] == 0
    for j in range(5):
        assert _bits(q, oa, 0, j) == _bits(q, o, 1, j), j
    assert np.array_equal(_mat(oa["T"], 0, D, oa["ldt"], oa["st_T"]), _mat(o["T"], 1, D, o["ldt"], o["st_T"]))
    # column 3 of the S = 5 call reproduces its bits in an S = 2 call built from columns {0, 3}
    ob = _outputs(q, 2)
    assert _multi(h, q, [0, 3], ob)[0] == 0
    for b in range(q["nb"]):
        assert _bits(q, ob, b, 1) == _bits(q, o, b, 3) and _bits(q, ob, b, 0) == _bits(q, o, b, 0)


def test_a_column_in_a_later_pass_keeps_its_bits(h):
    """column W + 2 of an S = W + 4 call (second pass) against an S = 2 call built from columns {0, W + 2} (first pass)"""
    q = _data(33, 29, np.float64, "col16", "diag", "diag", smax=W + 4)
    o, ob = _outputs(q, W + 4), _outputs(q, 2)
    assert _multi(h, q, list(range(W + 4)), o)[0] == 0 and _multi(h, q, [0, W + 2], ob)[0] == 0
    for b in range(q["nb"]):
        assert _bits(q, ob, b, 1) == _bits(q, o, b, W + 2)


def test_a_bad_regressor_leaves_the_others_alone(h):
    D, N, S = 24, 40, 4
    good = _data(D, N, np.float64, "col16", "diag", "dense", nb=4, smax=S)
    og = _outputs(good, S)
    assert _multi(h, good, list(range(S)), og)[0] == 0
    for which in ("prior", "noise"):
        bad = _data(D, N, np.float64, "col16", "diag", "dense", nb=4, smax=S)
        if which == "prior":
            bad["Lw"][1, 2 * D + 2] = -1.0  # regressor 1: leading minor 3 of the prior is not positive
            want = 3
        else:
            bad["s"][1, 10] = 0.0           # regressor 1: the variance of observation 11
            want = 11
        ob = _outputs(bad, S, fill=-5.0, gaps=False)
        ok = _outputs(good, S, fill=-5.0, gaps=False)
        assert _multi(h, bad, list(range(S)), ob)[0] == 0 and _multi(h, good, list(range(S)), ok)[0] == 0
        assert ob["info"].tolist() == [0, want, 0, 0]
        assert np.all(np.isnan(ob["lp"][S:2 * S])) and np.all(ob["M"][ob["st_m"]:2 * ob["st_m"]] == -5.0)
        assert np.all(ob["T"][ob["st_T"]:2 * ob["st_T"]] == -5.0)
        for b in (0, 2, 3):
            for k, st in (("M", "st_m"), ("T", "st_T"), ("A", "st_T"), ("lp", "st_lp")):
                assert np.array_equal(ob[k][b * ob[st]:(b + 1) * ob[st]], ok[k][b * ok[st]:(b + 1) * ok[st]]), (which, b, k)


@pytest.mark.parametrize("use_async", [False, True], ids=["sync", "async"])
def test_device_memspace_gives_the_host_memspace_bits(h, use_async):
    q = _data(40, 57, np.float64, "col16", "diag", "dense", smax=4)
    o, od = _outputs(q, 4), _outputs(q, 4)
    assert _multi(h, q, [0, 1, 2, 3], o)[0] == 0
    dev, host = {}, {}

    def to_device(a):
        host.update(a)
        for k, v in a.items():
            dev[k] = h.device_alloc(v.nbytes)
            h.memcpy_h2d(dev[k], v)
        return dev

    try:
        h.set_async(use_async)
        assert _multi(h, q, [0, 1, 2, 3], od, memspace=_abi.MEM_DEVICE, arrays=to_device)[0] == 0
        if use_async:
            h.synchronize()
        for k in ("M", "T", "A", "lp", "info"):
            h.memcpy_d2h(host[k], dev[k])
    finally:
        h.set_async(False)
        for p in dev.values():
            h.device_free(p)
    for k in ("M", "T", "A", "lp", "info"):
        assert np.array_equal(o[k], od[k], equal_nan=True), k


def test_large_d_takes_the_slow_route(h):
    q = _data(160, 90, np.float64, "col16", "diag", "diag", nb=2, smax=3)
    o = _outputs(q, 3)
    assert _multi(h, q, [0, 1, 2], o)[0] == 0
    _check(q, [0, 1, 2], o)


def test_without_t_post_the_factor_lives_in_the_workspace(h):
    q = _data(48, 60, np.float64, "col16", "iso", "diag", smax=3)
    h.release_workspace()
    before = h.get_stat("workspace_bytes")
    o = _outputs(q, 3)
    assert _multi(h, q, [0, 1, 2], o, T=False)[0] == 0
    assert h.get_stat("workspace_bytes") >= before + q["nb"] * 48 * 48 * 8
    _check(q, [0, 1, 2], o, T=False)
    assert np.all(np.isnan(o["T"]))
    h.release_workspace()
    assert h.get_stat("workspace_bytes") <= before


def test_python_maps_give_the_per_column_results():
    import blr_amd as B

    rng = np.random.Generator(np.random.PCG64(11))
    D, N, S = 24, 50, 3
    fxs, Ys = [], []
    for _ in range(3):
        f = B.BayesianLinearRegressor(0.2 * rng.standard_normal(D), B.Diagonal(np.exp(0.3 * rng.standard_normal(D))))
        fxs.append(f(B.ColVecs(np.asfortranarray(rng.standard_normal((D, N)))), np.exp(0.2 * rng.standard_normal(N))))
        Ys.append(rng.standard_normal((N, S)))
    lps = B.logpdf_columns_map(fxs, Ys)
    posts = B.posterior_columns_map(fxs, Ys)
    assert lps.shape == (3, S) and [len(p) for p in posts] == [S] * 3
    for fx, Y, lp, ps in zip(fxs, Ys, lps, posts):
        for j in range(S):
            one = B.posterior(fx, Y[:, j])
            assert lp[j] == pytest.approx(B.logpdf(fx, Y[:, j]), rel=1e-10, abs=1e-10)
            np.testing.assert_allclose(ps[j].mw, one.mw, rtol=1e-9, atol=1e-11)
            np.testing.assert_allclose(ps[j].Lw.toarray(), one.Lw.toarray(), rtol=1e-9, atol=1e-10)
    assert [len(p) for p in B.posterior_columns_map(fxs[:1], Ys[:1])] == [S] and len(B.posterior_columns(fxs[0], Ys[0])) == S
