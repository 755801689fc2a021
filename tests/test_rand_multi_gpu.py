"""blr_rand_multi_batched_* (R draws from each of the S column posteriors of B regressors in one call),
ResidentColumnsPosterior.rand, rand_columns and rand_columns_map against the CPU oracle per column (reference
src/bayesian_linear_regression.jl:49-53, src/sampling_functions.jl:16-49) with mw = M[:, c].  References, generator and tolerances
are those of tests/test_rand_batched_gpu.py.  All tests need an MI355X."""
import numpy as np
import pytest

from oracle import blr_oracle as O
from test_rand_batched_gpu import ATOL64, RTOL32, RTOL64, SENTINEL, _problem

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def B():
    import blr_amd

    blr_amd._abi.default_handle()
    return blr_amd


def _rng(i=0):
    return np.random.Generator(np.random.PCG64(77101 + i))


def _make(nb, D, N, S, R, prior_kind=1, noise_kind=0, share_x=False, share_prior=False, share_m=False, seed=0, bad=None):
    """nb problems in float64: per regressor (X D x N, M D x S, Lw in the library's form, the oracle's precision, s, Z1 D x S R,
    Z2 N x S R); shared inputs are the same arrays in every problem"""
    from blr_amd import _abi

    rng = _rng(seed)
    base = _problem(rng, D, N, prior_kind, noise_kind)
    M0 = rng.standard_normal((D, S))
    probs = []
    for b in range(nb):
        X, _, Lw, prec, s = _problem(rng, D, N, prior_kind, noise_kind)
        M = rng.standard_normal((D, S))
        if share_x:
            X = base[0]
        if share_prior:
            Lw, prec = base[2], base[3]
        if share_m:
            M = M0
        if bad is not None and b == bad[0]:  # a prior that fails at index bad[1]
            k = bad[1]
            Lw = Lw.copy()
            if prior_kind == _abi.PRIOR_DIAGONAL:
                Lw[k - 1] = -1.0
            elif prior_kind == _abi.PRIOR_UPPER_FACTOR:
                Lw[k - 1, k - 1] = 0.0
            else:
                Lw[k - 1, k - 1] = -50.0
        probs.append(dict(X=X, M=M, Lw=Lw, prec=prec, s=s, Z1=rng.standard_normal((D, S * R)), Z2=rng.standard_normal((N, S * R))))
    return probs


def _oracle(p, S, R, noise_kind, noisy):
    """(Y N x S R, W D x S R) per column with mw = M[:, c]"""
    Ws, Ys = [], []
    for c in range(S):
        z1, z2 = p["Z1"][:, c * R:(c + 1) * R], p["Z2"][:, c * R:(c + 1) * R]
        W = O.sample_weights(p["M"][:, c], p["prec"], z1)
        s_full = p["s"] if noise_kind == 1 else float(p["s"][0])
        Ys.append(O.rand(p["M"][:, c], p["prec"], p["X"], s_full, z1, z2) if noisy else p["X"].T @ W)
        Ws.append(W)
    D, N = p["X"].shape
    return (np.hstack(Ys) if Ys else np.zeros((N, 0))), (np.hstack(Ws) if Ws else np.zeros((D, 0)))


def _call(probs, S, R, dtype=np.float64, layout=0, prior_kind=1, noise_kind=0, noisy=True, want_W=True, want_Y=True, share_x=False,
          share_prior=False, share_m=False, ldx_pad=0, memspace=0, async_=False, handle=None):
    """Packs the problems, calls blr_rand_multi_batched_*, returns (Y [nb] of N x S R or None, W [nb] of D x S R or None, info)."""
    from blr_amd import _abi

    nb = len(probs)
    D, N = probs[0]["X"].shape
    SR = S * R
    if layout == _abi.LAYOUT_COLVECS:
        ldx = D + ldx_pad
        xs = [np.vstack([p["X"], np.full((ldx_pad, N), 9.0)]).astype(dtype).reshape(-1, order="F") for p in probs]
    else:
        ldx = N + ldx_pad
        xs = [np.vstack([p["X"].T, np.full((ldx_pad, D), 9.0)]).astype(dtype).reshape(-1, order="F") for p in probs]
    Xb = xs[0] if share_x else np.stack(xs)
    ls = [p["Lw"].astype(dtype).reshape(-1, order="F") for p in probs]
    Lb = ls[0] if share_prior else np.stack(ls)
    ms = [p["M"].astype(dtype).reshape(-1, order="F") for p in probs]
    Mb = ms[0] if share_m else np.stack(ms)
    ldl = 1 if prior_kind == _abi.PRIOR_DIAGONAL else D
    sb = np.stack([p["s"] for p in probs]).astype(dtype)
    Z1b = np.stack([p["Z1"].reshape(-1, order="F") for p in probs]).astype(dtype)
    Z2b = np.stack([p["Z2"].reshape(-1, order="F") for p in probs]).astype(dtype)
    Wb = np.full((nb, D * SR), SENTINEL, dtype=dtype) if want_W else None
    Yb = np.full((nb, N * SR), SENTINEL, dtype=dtype) if want_Y else None
    info = np.full(nb, -5, dtype=np.int32)
    h = handle or _abi.default_handle()
    args = dict(X=Xb, s=sb, M=Mb, Lw=Lb, Z1=Z1b, Z2=Z2b if noisy else None, W=Wb, Y=Yb, info=info)
    if memspace == _abi.MEM_DEVICE:
        import torch

        dev = {k: (torch.from_numpy(np.ascontiguousarray(v)).cuda() if v is not None and v.size else None) for k, v in args.items()}
        ptr = {k: (v.data_ptr() if v is not None else None) for k, v in dev.items()}
        torch.cuda.synchronize()  # (torch's copies run on its own stream, the library on the handle's)
    else:
        ptr = args
    if async_:
        h.set_async(1)
    try:
        rc = h.rand_multi_batched(dtype, memspace, layout, nb, D, N, S, R, ptr["X"], ldx, 0 if share_x else Xb.shape[-1], noise_kind,
                                  ptr["s"], sb.shape[1], prior_kind, ptr["M"], D, 0 if share_m else D * S, ptr["Lw"], ldl,
                                  0 if share_prior else Lb.shape[-1], ptr["Z1"], D, D * SR, ptr["Z2"], N, N * SR, ptr["W"], D, D * SR,
                                  ptr["Y"], N, N * SR, ptr["info"])
        assert rc == 0
        if async_:
            h.synchronize()
    finally:
        if async_:
            h.set_async(0)
    if memspace == _abi.MEM_DEVICE:
        Yb = dev["Y"].cpu().numpy() if dev["Y"] is not None else Yb
        Wb = dev["W"].cpu().numpy() if dev["W"] is not None else Wb
        info = dev["info"].cpu().numpy()
    Ys = [Yb[b].reshape((N, SR), order="F") for b in range(nb)] if want_Y else None
    Ws = [Wb[b].reshape((D, SR), order="F") for b in range(nb)] if want_W else None
    return Ys, Ws, info


def _check(probs, Ys, Ws, info, S, R, dtype, noise_kind, noisy, skip=None):
    for b, p in enumerate(probs):
        if b == skip:
            continue
        assert info[b] == 0, (b, info[b])
        Y_o, W_o = _oracle(p, S, R, noise_kind, noisy)
        for got, ref in ((Ys, Y_o), (Ws, W_o)):
            if got is None:
                continue
            assert got[b].shape == ref.shape
            if dtype == np.float64:
                np.testing.assert_allclose(got[b], ref, rtol=RTOL64, atol=ATOL64)
            elif ref.size:
                err = np.max(np.abs(got[b] - ref))
                assert err <= RTOL32 * max(1.0, np.max(np.abs(ref))), (b, err)


# (nb, D, N, S, R, dtype, layout, prior_kind, noise_kind, noisy, want_W, want_Y, ldx_pad): every value of every axis of the issue's
# grid at least once in both element types
CASES = [
    (3, 1, 1, 1, 1, np.float64, 0, 1, 0, True, True, True, 0),
    (37, 5, 17, 3, 7, np.float64, 1, 0, 1, True, True, True, 3),
    (1, 17, 64, 2, 16, np.float64, 0, 2, 0, False, False, True, 0),
    (3, 100, 65, 5, 1, np.float64, 1, 1, 1, True, True, True, 0),
    (3, 128, 130, 1, 33, np.float64, 0, 0, 0, True, True, True, 3),
    (1, 128, 0, 3, 7, np.float64, 0, 1, 0, True, True, True, 0),
    (3, 17, 17, 3, 7, np.float64, 0, 2, 1, True, True, False, 0),
    (3, 129, 17, 3, 2, np.float64, 0, 1, 1, True, True, True, 0),
    (3, 300, 17, 3, 2, np.float64, 1, 0, 0, False, True, True, 3),
    (37, 1, 1, 1, 1, np.float32, 1, 2, 1, True, True, True, 0),
    (3, 5, 17, 3, 7, np.float32, 0, 1, 0, False, True, True, 3),
    (3, 17, 65, 2, 16, np.float32, 1, 0, 1, True, False, True, 3),
    (1, 100, 64, 5, 1, np.float32, 0, 2, 0, True, True, True, 0),
    (3, 128, 130, 1, 33, np.float32, 1, 1, 1, True, True, True, 0),
    (3, 128, 0, 3, 7, np.float32, 0, 0, 0, True, True, True, 0),
    (3, 100, 17, 5, 1, np.float32, 0, 1, 0, True, True, False, 0),
    (3, 129, 17, 3, 2, np.float32, 1, 2, 0, True, True, True, 0),
    (1, 300, 17, 3, 2, np.float32, 0, 1, 1, False, True, True, 0),
]


@pytest.mark.parametrize("case", CASES, ids=[f"B{c[0]}-D{c[1]}-N{c[2]}-S{c[3]}-R{c[4]}-{np.dtype(c[5]).name}-L{c[6]}-P{c[7]}-n{c[8]}"
                                             f"{'' if c[9] else '-free'}{'' if c[10] else '-noW'}{'' if c[11] else '-noY'}-pad{c[12]}"
                                             for c in CASES])
def test_rand_multi_vs_oracle(B, case):
    nb, D, N, S, R, dt, layout, pk, nk, noisy, want_W, want_Y, pad = case
    probs = _make(nb, D, N, S, R, pk, nk, seed=D + N + S)
    Ys, Ws, info = _call(probs, S, R, dt, layout, pk, nk, noisy, want_W, want_Y, ldx_pad=pad)
    _check(probs, Ys, Ws, info, S, R, dt, nk, noisy)


@pytest.mark.parametrize("D,N", [(64, 16), (128, 130)])
def test_rand_multi_shared_inputs(B, D, N):
    S, R = 3, 7
    for sx, sp, sm in ((True, False, False), (False, True, False), (False, False, True), (True, True, True)):
        for pk in (0, 1, 2):
            probs = _make(5, D, N, S, R, pk, 0, share_x=sx, share_prior=sp, share_m=sm, seed=7)
            Ys, Ws, info = _call(probs, S, R, np.float64, 0, pk, 0, False, True, True, share_x=sx, share_prior=sp, share_m=sm)
            _check(probs, Ys, Ws, info, S, R, np.float64, 0, False)


@pytest.mark.parametrize("D", [5, 128, 150])
@pytest.mark.parametrize("pk", [0, 1, 2])
def test_rand_multi_info_leaves_failed_outputs(B, D, pk):
    S, R, N, k = 3, 2, 17, 3
    probs = _make(3, D, N, S, R, pk, 0, seed=11, bad=(1, k))
    Ys, Ws, info = _call(probs, S, R, np.float64, 0, pk, 0, True, True, True)
    assert list(info) == [0, k, 0]
    assert np.all(Ys[1] == SENTINEL) and np.all(Ws[1] == SENTINEL)
    _check(probs, Ys, Ws, info, S, R, np.float64, 0, True, skip=1)


@pytest.mark.parametrize("D,N", [(128, 130), (37, 17)])
@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_rand_multi_bit_promises(B, D, N, dt):
    S, R, nb = 3, 7, 64
    probs = _make(nb, D, N, S, R, 0, 1, seed=21)
    kw = dict(dtype=dt, layout=0, prior_kind=0, noise_kind=1)

    def call(idx, **over):
        Ys, Ws, info = _call([probs[i] for i in idx], S, R, **dict(kw, **over))
        assert not info.any()
        return Ys, Ws

    Y_all, W_all = call(range(nb))
    Y_again, W_again = call(range(nb))  # repeatable
    assert all(np.array_equal(a, b) for a, b in zip(Y_all + W_all, Y_again + W_again))
    for b in (0, 17, 63):  # independent of B and of the position in the batch
        Y1, W1 = call([b])
        assert np.array_equal(Y1[0], Y_all[b]) and np.array_equal(W1[0], W_all[b])
    Y_rev, W_rev = call(range(nb)[::-1])
    assert all(np.array_equal(a, b) for a, b in zip(Y_rev[::-1] + W_rev[::-1], Y_all + W_all))
    # column independence: draw for draw against three S = 1 calls, and against an R = 1 call on one draw (another pass and slot)
    p = probs[17]
    for c in range(S):
        sl = slice(c * R, (c + 1) * R)
        one = dict(p, M=p["M"][:, c:c + 1], Z1=p["Z1"][:, sl], Z2=p["Z2"][:, sl])
        Ys, Ws, info = _call([one], 1, R, **kw)
        assert info[0] == 0 and np.array_equal(Ys[0], Y_all[17][:, sl]) and np.array_equal(Ws[0], W_all[17][:, sl])
    j = 1 * R + 5  # column 1, draw 5: slot 12 of pass 0 there, slot 0 of pass 0 here
    one = dict(p, M=p["M"][:, 1:2], Z1=p["Z1"][:, j:j + 1], Z2=p["Z2"][:, j:j + 1])
    Ys, Ws, info = _call([one], 1, 1, **kw)
    assert info[0] == 0 and np.array_equal(Ys[0][:, 0], Y_all[17][:, j]) and np.array_equal(Ws[0][:, 0], W_all[17][:, j])
    j = 2 * R + 6  # the last draw: slot 4 of pass 1 there
    one = dict(p, M=p["M"][:, 2:3], Z1=p["Z1"][:, j:j + 1], Z2=p["Z2"][:, j:j + 1])
    Ys, Ws, info = _call([one], 1, 1, **kw)
    assert info[0] == 0 and np.array_equal(Ys[0][:, 0], Y_all[17][:, j]) and np.array_equal(Ws[0][:, 0], W_all[17][:, j])
    # Y does not depend on whether W is requested; host and device memspace agree
    Y_now, _ = call(range(5), want_W=False)
    assert all(np.array_equal(a, b) for a, b in zip(Y_now, Y_all[:5]))
    Y_dev, W_dev = call(range(5), memspace=1)
    assert all(np.array_equal(a, b) for a, b in zip(Y_dev + W_dev, Y_all[:5] + W_all[:5]))


@pytest.mark.parametrize("D,N", [(5, 17), (128, 130)])
def test_rand_multi_device_memspace_and_async(B, D, N):
    S, R = 3, 7
    probs = _make(3, D, N, S, R, 1, 0, seed=3)
    for async_ in (False, True):
        Ys, Ws, info = _call(probs, S, R, np.float64, 0, 1, 0, True, True, True, memspace=1, async_=async_)
        _check(probs, Ys, Ws, info, S, R, np.float64, 0, True)


@pytest.mark.parametrize("share_x", [False, True])
def test_rand_multi_chunk_seams(B, share_x):
    from blr_amd import _abi

    h = _abi.default_handle()
    S, R, D, N, nb = 3, 7, 37, 70, 7
    probs = _make(nb, D, N, S, R, 0, 1, share_x=share_x, seed=5)
    kw = dict(dtype=np.float64, layout=0, prior_kind=0, noise_kind=1, share_x=share_x)
    Y0, W0, info0 = _call(probs, S, R, **kw)
    assert h.get_stat("last_chunks") == 1
    h.set_option("MAX_CHUNK", "3")
    try:
        Y1, W1, info1 = _call(probs, S, R, **kw)
        assert h.get_stat("last_chunks") == 3
    finally:
        h.set_option("MAX_CHUNK", None)
    assert not info0.any() and not info1.any()
    assert all(np.array_equal(a, b) for a, b in zip(Y0 + W0, Y1 + W1))
    _check(probs, Y1, W1, info1, S, R, np.float64, 1, True)


def _state(B, rng, D, S, phi=None):
    A = rng.standard_normal((D, D)) / np.sqrt(D)
    Lw = B.PDMat(np.triu(O.chol_upper(A @ A.T + np.eye(D))))
    fs = [B.BayesianLinearRegressor(rng.standard_normal(D), Lw) for _ in range(S)]
    return B.ResidentColumnsPosterior([B.BasisFunctionRegressor(f, phi) for f in fs] if phi is not None else fs)


def test_resident_columns_rand_equals_host_round_trip(B):
    rng = _rng(41)
    D, S, R, N = 12, 3, 6, 9
    st = _state(B, rng, D, S)
    Xc, Yc = rng.standard_normal((D, 5)), rng.standard_normal((5, S))
    st.condition(Xc, 0.3, rng.standard_normal((5, S)))
    st.condition(Xc, 0.4, Yc)
    st.forget(Xc, 0.4, Yc)
    x = rng.standard_normal((D, N))
    for Sy in (0.25, B.Diagonal(np.exp(rng.standard_normal(N) * 0.3))):
        got = st.rand(np.random.Generator(np.random.PCG64(1)), x, R, Sy=Sy)
        r = np.random.Generator(np.random.PCG64(1))
        want = [B.rand(r, f(x, Sy), R) for f in st.regressors()]
        assert got.shape == (N, S, R) and got.flags.f_contiguous
        for c in range(S):
            np.testing.assert_allclose(got[:, c, :], want[c], rtol=1e-9, atol=1e-10)
    got = st.rand(np.random.Generator(np.random.PCG64(2)), x, R)  # noise-free function values: Z1_c only
    r = np.random.Generator(np.random.PCG64(2))
    for c, f in enumerate(st.regressors()):
        np.testing.assert_allclose(got[:, c, :], B.evaluate(B.rand(r, f, R), x), rtol=1e-9, atol=1e-10)
    # with a basis: condition and rand both map the inputs through phi
    phi = lambda z: np.vstack([z, z ** 2])  # noqa: E731
    st2 = _state(B, rng, 2 * D, S, phi)
    st2.condition(rng.standard_normal((D, 5)), 0.5, rng.standard_normal((5, S)))
    got = st2.rand(np.random.Generator(np.random.PCG64(3)), x, 4, Sy=0.1)
    r = np.random.Generator(np.random.PCG64(3))
    for c, f in enumerate(st2.regressors()):
        np.testing.assert_allclose(got[:, c, :], B.rand(r, f(x, 0.1), 4), rtol=1e-9, atol=1e-10)


def _columns(B, rng, D, N, S, k=6):
    X = B.ColVecs(np.asfortranarray(rng.standard_normal((D, k))))
    f = B.BayesianLinearRegressor(np.zeros(D), B.Diagonal(np.ones(D)))
    return B.posterior_columns(f(X, 0.3), rng.standard_normal((k, S)))


def test_rand_columns_and_map_equal_the_per_column_loop(B):
    rng = _rng(51)
    D, N, S, R = 10, 14, 3, 5
    x = B.ColVecs(np.asfortranarray(rng.standard_normal((D, N))))
    sy = B.Diagonal(np.exp(rng.standard_normal(N) * 0.3))

    def close(got, want):
        assert len(got) == len(want)
        for g, w in zip(got, want):
            assert g.shape == w.shape
            np.testing.assert_allclose(g, w, rtol=1e-9, atol=1e-10)

    posts = _columns(B, rng, D, N, S)
    fxs = [p(x, sy) for p in posts]
    got = B.rand_columns(np.random.Generator(np.random.PCG64(4)), fxs, R)
    r = np.random.Generator(np.random.PCG64(4))
    close(got, [B.rand(r, fx, R) for fx in fxs])
    # regressors: arrays of function samples
    got = B.rand_columns(np.random.Generator(np.random.PCG64(5)), posts, R)
    r = np.random.Generator(np.random.PCG64(5))
    want = [B.rand(r, p, R) for p in posts]
    Xq = rng.standard_normal((D, 4))
    for a, b in zip(got, want):
        assert a.shape == b.shape == (R,)
        for sa, sb in zip(a, b):
            np.testing.assert_allclose(sa.w, sb.w, rtol=1e-9, atol=1e-10)
            np.testing.assert_allclose(sa(Xq), sb(Xq), rtol=1e-9, atol=1e-10)
    # a map over equally shaped problems (one shared x object), then with one problem of another shape and one with mixed columns
    fxss = [[p(x, sy) for p in _columns(B, rng, D, N, S)] for _ in range(4)]
    got = B.rand_columns_map(np.random.Generator(np.random.PCG64(6)), fxss, R)
    r = np.random.Generator(np.random.PCG64(6))
    for g, fxs_b in zip(got, fxss):
        close(g, [B.rand(r, fx, R) for fx in fxs_b])
    x2 = B.ColVecs(np.asfortranarray(rng.standard_normal((D, 9))))
    mixed = [fxss[0][0], fxss[1][1], fxss[0][2]]  # two precision objects
    fxss2 = [fxss[0], [p(x2, 0.2) for p in _columns(B, rng, D, 9, S)], mixed]
    got = B.rand_columns_map(np.random.Generator(np.random.PCG64(7)), fxss2, R)
    r = np.random.Generator(np.random.PCG64(7))
    for g, fxs_b in zip(got, fxss2):
        close(g, [B.rand(r, fx, R) for fx in fxs_b])
    # a prior that is not positive definite: the problem's position
    badL = np.eye(D)
    badL[4, 4] = -1.0
    bad = [B.BayesianLinearRegressor(rng.standard_normal(D), badL)(x, sy) for _ in range(S)]
    bad = [B.FiniteGP(B.BayesianLinearRegressor(f.f.mw, bad[0].f.Lw), f.x, f.Sy) for f in bad]  # one precision object
    with pytest.raises(B.PosDefException) as e:
        B.rand_columns_map(np.random.Generator(np.random.PCG64(8)), [fxss[0], fxss[1], bad, fxss[2]], R)
    assert e.value.index == 2 and e.value.info == 5
