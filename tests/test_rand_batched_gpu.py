"""blr_rand_batched_* (draws from B regressors in one call), rand_map and ResidentPosterior.rand against the CPU oracle, per
regressor (reference src/bayesian_linear_regression.jl:49-53, src/sampling_functions.jl:16-49).  All tests need an MI355X."""
import numpy as np
import pytest

import _draw_problems as DP
from oracle import blr_oracle as O

pytestmark = pytest.mark.gpu

RTOL64, ATOL64 = 1e-10, 1e-11
RTOL32 = 2e-4
SENTINEL = -777.0


@pytest.fixture(scope="module")
def B():
    import blr_amd

    blr_amd._abi.default_handle()
    return blr_amd


def _rng(i=0):
    return np.random.Generator(np.random.PCG64(55501 + i))


def _problem(rng, D, N, prior_kind, noise_kind):
    """one well-conditioned regressor: X (D x N), mw, Lw in the library's form, the oracle's precision, s"""
    from blr_amd import _abi

    X = rng.standard_normal((D, N)) / np.sqrt(D)
    mw = rng.standard_normal(D)
    if prior_kind == _abi.PRIOR_DIAGONAL:
        Lw = np.exp(rng.standard_normal(D) * 0.3)
        prec = Lw
    else:
        A = rng.standard_normal((D, D)) / np.sqrt(D)
        prec = A @ A.T + np.eye(D)
        Lw = np.triu(O.chol_upper(prec)) if prior_kind == _abi.PRIOR_UPPER_FACTOR else prec
    s = np.exp(rng.standard_normal(N) * 0.3) if noise_kind == _abi.NOISE_DIAGONAL else np.array([0.3])
    return X, mw, Lw, prec, s


def _run(B, nb, D, N, S, dtype=np.float64, layout=0, prior_kind=1, noise_kind=0, noisy=True, want_W=True, share_x=False,
         share_prior=False, ldx_pad=0, memspace=0, seed=0, bad=None, async_=False):
    """Packs nb problems, calls blr_rand_batched_*, returns (Y[nb], W[nb], info, per-problem oracle (Y, W), raw operands)."""
    from blr_amd import _abi

    rng = _rng(seed)
    probs = [_problem(rng, D, N, prior_kind, noise_kind) for _ in range(1 if share_x and share_prior else nb)]
    if share_x or share_prior:
        base = probs[0]
        fresh = [_problem(rng, D, N, prior_kind, noise_kind) for _ in range(nb)]
        probs = [(base[0] if share_x else p[0], p[1], base[2] if share_prior else p[2], base[3] if share_prior else p[3], p[4])
                 for p in fresh]
    if bad is not None:  # regressor `bad[0]` gets a prior that fails at index bad[1]
        b, k = bad
        X, mw, Lw, prec, s = probs[b]
        Lw = Lw.copy()
        if prior_kind == _abi.PRIOR_DIAGONAL:
            Lw[k - 1] = -1.0
        elif prior_kind == _abi.PRIOR_UPPER_FACTOR:
            Lw[k - 1, k - 1] = 0.0
        else:
            Lw[k - 1, k - 1] = -50.0
        probs[b] = (X, mw, Lw, prec, s)
    Z1 = [rng.standard_normal((D, S)) for _ in range(nb)]
    Z2 = [rng.standard_normal((N, S)) for _ in range(nb)]
    # operands in the batched layout
    if layout == _abi.LAYOUT_COLVECS:
        ldx = D + ldx_pad
        xs = [np.vstack([p[0], np.full((ldx_pad, N), 9.0)]).astype(dtype).reshape(-1, order="F") for p in probs]
    else:
        ldx = N + ldx_pad
        xs = [np.vstack([p[0].T, np.full((ldx_pad, D), 9.0)]).astype(dtype).reshape(-1, order="F") for p in probs]
    Xb = xs[0] if share_x else np.stack(xs)
    strideX = 0 if share_x else Xb.shape[-1]
    ls = [p[2].astype(dtype).reshape(-1, order="F") for p in probs]
    Lb = ls[0] if share_prior else np.stack(ls)
    strideL = 0 if share_prior else Lb.shape[-1]
    ldl = 1 if prior_kind == _abi.PRIOR_DIAGONAL else D
    mwb = np.stack([p[1] for p in probs]).astype(dtype)
    sb = np.stack([p[4] for p in probs]).astype(dtype)
    Z1b = np.stack([z.reshape(-1, order="F") for z in Z1]).astype(dtype)
    Z2b = np.stack([z.reshape(-1, order="F") for z in Z2]).astype(dtype)
    Wb = np.full((nb, D * S), SENTINEL, dtype=dtype) if want_W else None
    Yb = np.full((nb, N * S), SENTINEL, dtype=dtype)
    info = np.full(nb, -5, dtype=np.int32)
    h = _abi.default_handle()
    args = dict(X=Xb, s=sb, mw=mwb, Lw=Lb, Z1=Z1b, Z2=Z2b if noisy else None, W=Wb, Y=Yb, info=info)
    if memspace == _abi.MEM_DEVICE:
        import torch

        dev = {k: (torch.from_numpy(np.ascontiguousarray(v)).cuda() if v is not None else None) for k, v in args.items()}
        ptr = {k: (v.data_ptr() if v is not None else None) for k, v in dev.items()}
        torch.cuda.synchronize()  # (torch's copies run on its own stream, the library on the handle's)
    else:
        ptr = args
    if async_:
        h.set_async(1)
    try:
        h.rand_batched(dtype, memspace, layout, nb, D, N, S, ptr["X"], ldx, strideX, noise_kind, ptr["s"], sb.shape[1], prior_kind,
                       ptr["mw"], D, ptr["Lw"], ldl, strideL, ptr["Z1"], D, D * S, ptr["Z2"], N, N * S, ptr["W"], D, D * S,
                       ptr["Y"], N, N * S, ptr["info"])
        if async_:
            h.synchronize()
    finally:
        if async_:
            h.set_async(0)
    if memspace == _abi.MEM_DEVICE:
        Yb = dev["Y"].cpu().numpy()
        Wb = dev["W"].cpu().numpy() if want_W else None
        info = dev["info"].cpu().numpy()
    Ys = [Yb[b].reshape((N, S), order="F") for b in range(nb)]
    Ws = [Wb[b].reshape((D, S), order="F") for b in range(nb)] if want_W else None
    refs = []
    for b, p in enumerate(probs):
        if bad is not None and b == bad[0]:
            refs.append(None)
            continue
        W_o = O.sample_weights(p[1], p[3], Z1[b])
        s_full = p[4] if noise_kind == _abi.NOISE_DIAGONAL else float(p[4][0])
        Y_o = O.rand(p[1], p[3], p[0], s_full, Z1[b], Z2[b]) if noisy else p[0].T @ W_o
        # the operands as the library saw them (rounded to dtype, in fp64) for the derived bound of _check
        r64 = lambda a: np.asarray(a, dtype=dtype).astype(np.float64)
        kind = {_abi.PRIOR_DENSE: "dense", _abi.PRIOR_UPPER_FACTOR: "factor", _abi.PRIOR_DIAGONAL: "diag"}[prior_kind]
        case = DP.Case("rand_batched", "rand_batched", "f32" if dtype == np.float32 else "f64", D, N=N, S=S, prior=kind,
                       noise=(("diag" if noise_kind == _abi.NOISE_DIAGONAL else "iso") if noisy else None))
        ops = dict(X=[r64(p[0])], mw=[r64(p[1])], L=[r64(p[2])], Z1=[r64(Z1[b])], Z2=[r64(Z2[b])], s=[r64(p[4])])
        refs.append((Y_o, W_o, case, ops))
    return Ys, Ws, info, refs


def _check(Ys, Ws, info, refs, dtype):
    for b, ref in enumerate(refs):
        if ref is None:
            continue
        assert info[b] == 0, (b, info[b])
        Y_o, W_o, case, ops = ref
        if dtype == np.float64:
            np.testing.assert_allclose(Ys[b], Y_o, rtol=RTOL64, atol=ATOL64)
            if Ws is not None:
                np.testing.assert_allclose(Ws[b], W_o, rtol=RTOL64, atol=ATOL64)
        else:
            if Y_o.size:
                # |Y - Y_ref| <= gamma(D + 2) |X|'|W| + 2 eps |sqrt(s) Z2| elementwise, Y_ref the fp64 product of the same rounded
                # inputs with the library's own W; without a W output: the reference weights and their bound through |X|'
                # (tests/_draw_problems.py: projection_bound, weights_tolerance)
                X, noise = ops["X"][0], DP.noise_term(case, ops, 0)
                if Ws is not None:
                    W, slack = Ws[b].astype(np.float64), 0.0
                else:
                    W, wb, _ = DP.weights_tolerance(case, ops, 0)
                    W = np.asarray(W, dtype=np.float64)
                    slack = np.abs(X).T @ np.broadcast_to(np.asarray(wb, dtype=np.float64), W.shape)
                bound = DP.projection_bound(case, X, W, noise) + slack
                assert np.all(np.abs(Ys[b].astype(np.float64) - (X.T @ W + noise)) <= bound), b
            if Ws is not None:
                assert np.max(np.abs(Ws[b] - W_o)) <= RTOL32 * max(1.0, np.max(np.abs(W_o))), b


# (nb, D, N, S, dtype, layout, prior_kind, noise_kind, noisy, want_W, ldx_pad) -- a covering subset of the issue's grid
CASES = [
    (3, 1, 1, 1, np.float64, 0, 1, 0, True, True, 0),
    (37, 5, 17, 7, np.float64, 1, 0, 1, True, True, 3),
    (3, 64, 4096, 7, np.float64, 0, 1, 0, True, False, 0),
    (37, 100, 17, 64, np.float32, 0, 2, 1, False, True, 1),
    (3, 128, 17, 129, np.float64, 0, 0, 0, True, True, 2),
    (37, 128, 1, 1, np.float32, 1, 1, 0, False, True, 0),
    (3, 129, 17, 7, np.float64, 0, 1, 1, True, True, 0),
    (3, 300, 4096, 1, np.float32, 1, 0, 0, True, True, 1),
    (1, 300, 0, 7, np.float64, 0, 2, 0, True, True, 0),
    (37, 64, 0, 64, np.float32, 0, 0, 0, True, True, 0),
    (3, 128, 4096, 129, np.float32, 0, 1, 1, True, True, 0),
    (1, 5, 17, 1, np.float64, 0, 2, 0, False, False, 0),
]


@pytest.mark.parametrize("case", CASES, ids=[f"B{c[0]}-D{c[1]}-N{c[2]}-S{c[3]}-{np.dtype(c[4]).name}-L{c[5]}-P{c[6]}-n{c[7]}"
                                             f"{'' if c[8] else '-free'}{'' if c[9] else '-noW'}-pad{c[10]}" for c in CASES])
def test_rand_batched_vs_oracle(B, case):
    nb, D, N, S, dt, layout, pk, nk, noisy, want_W, pad = case
    Ys, Ws, info, refs = _run(B, nb, D, N, S, dt, layout, pk, nk, noisy, want_W, ldx_pad=pad, seed=D + N)
    _check(Ys, Ws, info, refs, dt)


@pytest.mark.parametrize("D,N,S", [(5, 17, 7), (128, 4096, 16), (300, 17, 1)])
def test_rand_batched_device_memspace_and_async(B, D, N, S):
    for async_ in (False, True):
        Ys, Ws, info, refs = _run(B, 3, D, N, S, np.float64, 0, 1, 0, True, True, memspace=1, seed=3, async_=async_)
        _check(Ys, Ws, info, refs, np.float64)


@pytest.mark.parametrize("D,N,S", [(64, 16, 1), (128, 4096, 16), (200, 17, 3)])
def test_rand_batched_shared_x_and_prior(B, D, N, S):
    for share_x, share_prior in ((True, False), (False, True), (True, True)):
        for pk in (0, 1, 2):
            Ys, Ws, info, refs = _run(B, 5, D, N, S, np.float64, 0, pk, 0, False, True, share_x=share_x, share_prior=share_prior, seed=7)
            _check(Ys, Ws, info, refs, np.float64)


@pytest.mark.parametrize("D,N,S", [(5, 17, 7), (128, 16, 1), (64, 4096, 16), (150, 17, 2)])
@pytest.mark.parametrize("pk", [0, 1, 2])
def test_rand_batched_info_leaves_failed_outputs(B, D, N, S, pk):
    k = 3
    Ys, Ws, info, refs = _run(B, 3, D, N, S, np.float64, 0, pk, 0, True, True, seed=11, bad=(1, k))
    assert list(info) == [0, k, 0]
    assert np.all(Ys[1] == SENTINEL) and np.all(Ws[1] == SENTINEL)
    _check(Ys, Ws, info, refs, np.float64)


@pytest.mark.parametrize("D,N,S,dt", [(128, 16, 1, np.float64), (100, 4096, 16, np.float64), (64, 256, 8, np.float32),
                                      (37, 17, 7, np.float32)])
def test_rand_batched_is_batch_invariant_and_deterministic(B, D, N, S, dt):
    from blr_amd import _abi

    h = _abi.default_handle()
    rng = _rng(21)
    nb = 64
    probs = [_problem(rng, D, N, _abi.PRIOR_DENSE, _abi.NOISE_DIAGONAL) for _ in range(nb)]
    X = np.stack([p[0].astype(dt).reshape(-1, order="F") for p in probs])
    L = np.stack([p[2].astype(dt).reshape(-1, order="F") for p in probs])
    mw = np.stack([p[1] for p in probs]).astype(dt)
    s = np.stack([p[4] for p in probs]).astype(dt)
    Z1 = rng.standard_normal((nb, D * S)).astype(dt)
    Z2 = rng.standard_normal((nb, N * S)).astype(dt)

    def call(idx):
        m = len(idx)
        Y = np.zeros((m, N * S), dtype=dt)
        W = np.zeros((m, D * S), dtype=dt)
        info = np.zeros(m, dtype=np.int32)
        h.rand_batched(dt, _abi.MEM_HOST, _abi.LAYOUT_COLVECS, m, D, N, S, X[idx].copy(), D, D * N, _abi.NOISE_DIAGONAL, s[idx].copy(), N,
                       _abi.PRIOR_DENSE, mw[idx].copy(), D, L[idx].copy(), D, D * D, Z1[idx].copy(), D, D * S, Z2[idx].copy(), N, N * S,
                       W, D, D * S, Y, N, N * S, info)
        assert not info.any()
        return Y, W

    Y_all, W_all = call(list(range(nb)))
    Y_again, W_again = call(list(range(nb)))
    assert np.array_equal(Y_all, Y_again) and np.array_equal(W_all, W_again)
    for b in (0, 17, 63):
        Y1, W1 = call([b])
        assert np.array_equal(Y1[0], Y_all[b]) and np.array_equal(W1[0], W_all[b])
    perm = list(range(nb))[::-1]
    Y_rev, W_rev = call(perm)
    assert np.array_equal(Y_rev[::-1], Y_all) and np.array_equal(W_rev[::-1], W_all)


@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_thompson_shape_full_size_on_device(B, dt):
    """B = 4096, D = 128, one shared set of 16 candidates, S = 1, noise-free, upper-factor priors, device pointers: every regressor
    against a float64 torch reference on the device."""
    import torch
    from blr_amd import _abi

    nb, D, N, S = 4096, 128, 16, 1
    g = torch.Generator(device="cuda").manual_seed(5)
    X = (torch.randn(D, N, generator=g, device="cuda", dtype=torch.float64) / D ** 0.5)
    A = torch.randn(nb, D, D, generator=g, device="cuda", dtype=torch.float64) / D ** 0.5
    U = torch.linalg.cholesky(A @ A.transpose(1, 2) + torch.eye(D, device="cuda", dtype=torch.float64), upper=True)
    mw = torch.randn(nb, D, generator=g, device="cuda", dtype=torch.float64)
    Z1 = torch.randn(nb, D, generator=g, device="cuda", dtype=torch.float64)
    tdt = torch.float64 if dt == np.float64 else torch.float32
    Ud, mwd, Z1d = (t.to(tdt).contiguous() for t in (U.transpose(1, 2), mw, Z1))  # U column-major: the rows of its transpose
    Y = torch.full((nb, N), SENTINEL, device="cuda", dtype=tdt)
    info = torch.full((nb,), -5, device="cuda", dtype=torch.int32)
    h = _abi.default_handle()
    # X as ColVecs: D x N column-major = the (N, D) row-major tensor
    Xc = X.t().contiguous().to(tdt)
    torch.cuda.synchronize()  # the operands are written on torch's stream; the library runs on its handle's own stream
    h.rand_batched(dt, _abi.MEM_DEVICE, _abi.LAYOUT_COLVECS, nb, D, N, S, Xc.data_ptr(), D, 0, _abi.NOISE_ISOTROPIC, None, 0,
                   _abi.PRIOR_UPPER_FACTOR, mwd.data_ptr(), D, Ud.data_ptr(), D, D * D, Z1d.data_ptr(), D, D, None, N, 0, None, D, 0,
                   Y.data_ptr(), N, N, info.data_ptr())
    torch.cuda.synchronize()
    assert int(info.abs().sum()) == 0
    W_ref = mw + torch.linalg.solve_triangular(U, Z1.unsqueeze(-1), upper=True).squeeze(-1)
    Y_ref = W_ref @ X  # (nb, N)
    err = (Y.double() - Y_ref).abs().max(dim=1).values
    scale = Y_ref.abs().max(dim=1).values.clamp(min=1.0)
    tol = 1e-10 if dt == np.float64 else RTOL32
    assert bool((err <= tol * scale).all()), float((err / scale).max())


def test_argument_validation(B):
    from blr_amd import _abi

    h = _abi.default_handle()
    D, N, S, nb = 4, 5, 2, 2
    X = np.zeros((nb, D * N))
    s = np.ones((nb, 1))
    mw = np.zeros((nb, D))
    L = np.ones((nb, D))
    Z1 = np.zeros((nb, D * S))
    Z2 = np.zeros((nb, N * S))
    W = np.zeros((nb, D * S))
    Y = np.zeros((nb, N * S))
    info = np.zeros(nb, dtype=np.int32)
    good = dict(X=X, ldx=D, strideX=D * N, s=s, mw=mw, Lw=L, Z1=Z1, ldz1=D, Z2=Z2, ldz2=N, W=W, ldw=D, strideW=D * S, Y=Y, ldy=N,
                strideY=N * S, info=info)

    def call(**kw):
        a = dict(good, **kw)
        return h.rand_batched(np.float64, _abi.MEM_HOST, _abi.LAYOUT_COLVECS, nb, D, N, S, a["X"], a["ldx"], a["strideX"],
                              _abi.NOISE_ISOTROPIC, a["s"], 1, _abi.PRIOR_DIAGONAL, a["mw"], D, a["Lw"], 1, D, a["Z1"], a["ldz1"], D * S,
                              a["Z2"], a["ldz2"], N * S, a["W"], a["ldw"], a["strideW"], a["Y"], a["ldy"], a["strideY"], a["info"])

    assert call() == 0 and not info.any()
    for kw, pos in ((dict(X=None), 8), (dict(ldx=D - 1), 9), (dict(s=None), 12), (dict(mw=None), 15), (dict(Lw=None), 17),
                    (dict(Z1=None), 20), (dict(ldz1=D - 1), 21), (dict(ldz2=N - 1), 24), (dict(ldw=D - 1), 27),
                    (dict(strideW=D * S - 1), 28), (dict(ldy=N - 1), 30), (dict(strideY=N * S - 1), 31), (dict(info=None), 32)):
        with pytest.raises(_abi.BLRError) as e:
            call(**kw)
        assert e.value.code == -pos, (kw, e.value.code)
    # Z2 = NULL: s is not needed; Y = NULL: X is not needed
    assert call(Z2=None, s=None) == 0
    assert call(Y=None, X=None) == 0


def _fx_list(B, rng, specs):
    fxs = []
    for D, N, dt, kind, layout in specs:
        X, mw, Lw, prec, s = _problem(rng, D, N, {"dense": 0, "factor": 1, "diag": 2}[kind], 1)
        Lw_obj = {"dense": lambda: Lw, "factor": lambda: B.PDMat(Lw), "diag": lambda: B.Diagonal(Lw.astype(dt))}[kind]()
        f = B.BayesianLinearRegressor(mw.astype(dt), Lw_obj)
        x = B.ColVecs(np.asfortranarray(X.astype(dt))) if layout == "col" else B.RowVecs(np.ascontiguousarray(X.T.astype(dt)))
        fxs.append(f(x, B.Diagonal(s.astype(dt))))
    return fxs


def _assert_lists_close(got, want, dt):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.shape == w.shape
        if dt == np.float64:
            np.testing.assert_allclose(g, w, rtol=RTOL64, atol=ATOL64)
        elif w.size:
            assert np.max(np.abs(g - w)) <= RTOL32 * max(1.0, np.max(np.abs(w)))


@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_rand_map_equals_single_rand_calls(B, dt):
    rng = _rng(31)
    for specs in ([(8, 12, dt, "dense", "col")] * 5, [(130, 40, dt, "factor", "row")] * 3,
                  [(6, 12, dt, "diag", "col"), (6, 9, dt, "diag", "col"), (4, 12, dt, "dense", "row")]):  # the last: mixed, falls back
        fxs = _fx_list(B, rng, specs)
        got = B.rand_map(np.random.Generator(np.random.PCG64(3)), fxs, 7)
        r = np.random.Generator(np.random.PCG64(3))
        want = [B.rand(r, fx, 7) for fx in fxs]
        _assert_lists_close(got, want, dt)
    # regressors, a BasisFunctionRegressor among them: arrays of function samples
    f = B.BayesianLinearRegressor(np.ones(3), B.Diagonal(np.full(3, 2.0)))
    g = B.BasisFunctionRegressor(B.BayesianLinearRegressor(np.zeros(3), B.Diagonal(np.ones(3))), lambda x: np.sin(x))
    fs = [f, g, f]
    got = B.rand_map(np.random.Generator(np.random.PCG64(4)), fs, 5)
    r = np.random.Generator(np.random.PCG64(4))
    want = [B.rand(r, h_, 5) for h_ in fs]
    Xq = rng.standard_normal((3, 6))
    for a, b in zip(got, want):
        assert a.shape == b.shape == (5,)
        for sa, sb in zip(a, b):
            np.testing.assert_allclose(sa.w, sb.w, rtol=RTOL64, atol=ATOL64)
            np.testing.assert_allclose(sa(Xq), sb(Xq), rtol=1e-9, atol=1e-10)


def test_rand_map_shared_candidates_and_posdef(B):
    rng = _rng(32)
    X = B.ColVecs(np.asfortranarray(rng.standard_normal((16, 10))))
    fs = [B.BayesianLinearRegressor(rng.standard_normal(16), B.PDMat(np.triu(O.chol_upper(np.eye(16) * (1 + b))))) for b in range(6)]
    fxs = [f(X, 0.2) for f in fs]
    got = B.rand_map(np.random.Generator(np.random.PCG64(8)), fxs, 3)
    r = np.random.Generator(np.random.PCG64(8))
    _assert_lists_close(got, [B.rand(r, fx, 3) for fx in fxs], np.float64)
    bad = np.eye(16)
    bad[4, 4] = -1.0
    fxs[2] = B.BayesianLinearRegressor(np.zeros(16), bad)(X, 0.2)
    with pytest.raises(B.PosDefException) as e:
        B.rand_map(np.random.Generator(np.random.PCG64(8)), fxs, 3)
    assert e.value.index == 2 and e.value.info == 5


def test_resident_posterior_rand_equals_host_round_trip(B):
    rng = _rng(41)
    D = 12
    X1, mw, Lw, prec, s = _problem(rng, D, 30, 0, 1)
    st = B.ResidentPosterior(B.BayesianLinearRegressor(mw, Lw))
    for _ in range(3):
        Xc = rng.standard_normal((D, 4))
        st.condition(Xc, 0.3, rng.standard_normal(4))
    x = rng.standard_normal((D, 9))
    got = st.rand(np.random.Generator(np.random.PCG64(1)), x, 6, Sy=0.25)
    want = B.rand(np.random.Generator(np.random.PCG64(1)), st.regressor()(x, 0.25), 6)
    np.testing.assert_allclose(got, want, rtol=1e-9, atol=1e-10)
    got = st.rand(np.random.Generator(np.random.PCG64(2)), x, 6)
    want = B.evaluate(B.rand(np.random.Generator(np.random.PCG64(2)), st.regressor(), 6), x)
    np.testing.assert_allclose(got, want, rtol=1e-9, atol=1e-10)
    # with a basis: condition and rand both map the inputs through phi
    phi = lambda z: np.vstack([z, z ** 2])  # noqa: E731
    st2 = B.ResidentPosterior(B.BasisFunctionRegressor(B.BayesianLinearRegressor(np.zeros(2 * D), B.Diagonal(np.ones(2 * D))), phi))
    st2.condition(rng.standard_normal((D, 5)), 0.5, rng.standard_normal(5))
    got = st2.rand(np.random.Generator(np.random.PCG64(3)), x, 4, Sy=0.1)
    want = B.rand(np.random.Generator(np.random.PCG64(3)), st2.regressor()(x, 0.1), 4)
    np.testing.assert_allclose(got, want, rtol=1e-9, atol=1e-10)


def test_rand_map_moments(B):
    # reference test/bayesian_linear_regression.jl:11-21 on a small batch: empirical mean / covariance of many draws
    rng = _rng(51)
    N, D, S = 6, 3, 100_000
    fxs = []
    for _ in range(3):
        X, mw, Lw, s = O.generate_toy_problem(rng, N, D, dense_noise_cov=False)
        fxs.append((B.BayesianLinearRegressor(mw, Lw)(X, s), mw, Lw, X, s))
    Ys = B.rand_map(np.random.Generator(np.random.PCG64(9)), [q[0] for q in fxs], S)
    for Y, (fx, mw, Lw, X, s) in zip(Ys, fxs):
        m_emp = Y.mean(axis=1)
        Yc = Y - m_emp[:, None]
        np.testing.assert_allclose(B.mean(fx), m_emp, atol=2e-2, rtol=2e-2)
        np.testing.assert_allclose(O.cov(mw, Lw, X, s), Yc @ Yc.T / S, atol=3e-2, rtol=3e-2)
