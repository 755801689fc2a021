"""Data and call helpers of tests/test_grid_ragged_gpu.py (blr_logpdf_grid_ragged_*): problems drawn as tests/test_grid_gpu.py draws
them, one per observation count; their packed form in the three loaders' layouts; the packed call, and its yardstick -- one call of
blr_logpdf_grid_* with B = 1 per regressor on the slice of the SAME packed arrays."""
import numpy as np

# every seam of grid_splits (1024 / 2048: S = 1 -> 2, a full and a short last block; 9000: S = 8 with a 936-column tail) and of the
# 64-column stages, in scrambled order
COUNTS = (2047, 0, 65, 9000, 1, 2048, 63, 1023, 64, 2049)
SCALES = 10.0 ** np.array([-1.0, 0.0, 1.0])
ALPHA, TAU = np.repeat(SCALES, 3), np.tile(SCALES, 3)  # the 3 x 3 grid, prior scale slowest


def draw(seed, D, counts, noise, prior, zero_mean=False):
    """[(X D x n, y, s0, mw, L0)]: X ~ N(0,1), w ~ N(0,I), mw ~ 0.3 N(0,I), y = X'w + sqrt(s0) N(0,1); base noise 0.1 ("shared"),
    0.1 exp(0.5 N(0,1)) per regressor ("iso") or exp(0.5 N(0,1)) per observation ("diag"); base prior Diagonal(exp(0.3 N(0,1)))
    or BB'/D + I"""
    rng = np.random.Generator(np.random.PCG64(seed))
    out = []
    for n in counts:
        X = np.asfortranarray(rng.standard_normal((D, n)))
        w = rng.standard_normal(D)
        mw = np.zeros(D) if zero_mean else 0.3 * rng.standard_normal(D)
        if noise == "diag":
            s0 = np.exp(0.5 * rng.standard_normal(n))
        else:
            s0 = np.float64(0.1) if noise == "shared" else np.float64(0.1 * np.exp(0.5 * rng.standard_normal()))
        y = X.T @ w + np.sqrt(s0) * rng.standard_normal(n)
        if prior == "dense":
            Bm = rng.standard_normal((D, D))
            L0 = Bm @ Bm.T / D + np.eye(D)
        else:
            L0 = np.exp(0.3 * rng.standard_normal(D))
        out.append((X, y, s0, mw, L0))
    return out


def grids(nb, shared, seed=5):
    """(alpha [nb, 9], tau [nb, 9]): one grid for all, or a permutation of it per regressor"""
    if shared:
        return np.tile(ALPHA, (nb, 1)), np.tile(TAU, (nb, 1))
    rng = np.random.Generator(np.random.PCG64(seed))
    perms = [rng.permutation(9) for _ in range(nb)]
    return np.stack([ALPHA[p] for p in perms]), np.stack([TAU[p] for p in perms])


def pack(A, probs, xkind, noise, dtype):
    """The packed operands: xkind "col" (ColVecs, ldx = D: the LDS-DMA loader when D is a multiple of the vector width), "colpad"
    (ColVecs, ldx = D + 1, the pad row NaN: the generic loader) or "row" (RowVecs)."""
    nb = len(probs)
    D = probs[0][0].shape[0]
    counts = [p[0].shape[1] for p in probs]
    offsets = np.concatenate(([0], np.cumsum(counts))).astype(np.int64)
    total = int(offsets[-1])
    if xkind == "row":
        X = np.asfortranarray(np.concatenate([p[0].T for p in probs], axis=0), dtype=dtype).reshape(-1, order="F")
        layout, ldx = A.LAYOUT_ROWVECS, max(total, 1)
    else:
        ldx = D + (1 if xkind == "colpad" else 0)
        Xm = np.full((ldx, total), np.nan, dtype=dtype, order="F")
        Xm[:D] = np.concatenate([p[0] for p in probs], axis=1)
        X, layout = Xm.reshape(-1, order="F"), A.LAYOUT_COLVECS
    y = np.concatenate([p[1] for p in probs]).astype(dtype)
    if noise == "diag":
        s, noise_kind, strides = np.concatenate([p[2] for p in probs]).astype(dtype), A.NOISE_DIAGONAL, 0
    elif noise == "iso":
        s, noise_kind, strides = np.array([p[2] for p in probs], dtype=dtype), A.NOISE_ISOTROPIC, 1
    else:
        s, noise_kind, strides = np.array([probs[0][2]], dtype=dtype), A.NOISE_ISOTROPIC, 0
    dense = np.ndim(probs[0][4]) == 2
    return dict(dtype=dtype, nb=nb, D=D, counts=counts, offsets=offsets, layout=layout, X=X, ldx=ldx, y=y, s=s, noise_kind=noise_kind,
                strides=strides, mw=np.stack([np.asarray(p[3], dtype=dtype) for p in probs]),
                Lw=np.stack([np.asfortranarray(p[4], dtype=dtype).reshape(-1, order="F") for p in probs]),
                prior_kind=A.PRIOR_DENSE if dense else A.PRIOR_DIAGONAL, ldl=max(D, 1))


def _outputs(pk, G, want_best, want_post, sentinel):
    """want_post: True (both refit outputs), "mw" or "T" (only that one, the other NULL) or False"""
    nb, D, dtype = pk["nb"], pk["D"], pk["dtype"]
    return dict(lp=np.full((nb, G), 12345.0), info=np.full((nb, G), -7, dtype=np.int32),
                best=np.full(nb, -9, dtype=np.int64) if want_best else None,
                mw_best=np.full((nb, D), sentinel, dtype=dtype) if want_post in (True, "mw") else None,
                T_best=np.full((nb, D * D), sentinel, dtype=dtype) if want_post in (True, "T") else None)


def _settings(pk, alpha, tau, shared):
    cast = lambda v: None if v is None else np.ascontiguousarray(v[0] if shared else v, dtype=pk["dtype"])  # noqa: E731
    return cast(alpha), cast(tau)


def _n_settings(alpha, tau):
    return 1 if alpha is None and tau is None else (alpha if alpha is not None else tau).shape[1]


def call_ragged(B, pk, alpha, tau, shared=True, want_best=True, want_post=True, sentinel=np.nan, device=False):
    """blr_logpdf_grid_ragged_* -> dict(lp [nb, G], info, best, mw_best [nb, D], T_best [nb, D * D] column-major each)"""
    A = B._abi
    h = A.default_handle()
    nb, D, dtype = pk["nb"], pk["D"], pk["dtype"]
    G = _n_settings(alpha, tau)
    al, ta = _settings(pk, alpha, tau, shared)
    out = _outputs(pk, G, want_best, want_post, sentinel)
    host = dict(X=pk["X"], y=pk["y"], s=pk["s"], mw=pk["mw"], Lw=pk["Lw"], alpha=al, tau=ta, **out)
    args, bufs = dict(host), {}
    if device:
        from blr_amd.regressor import _DeviceBuffer

        for k, v in host.items():
            if v is not None:
                bufs[k] = _DeviceBuffer.of(h, np.ascontiguousarray(v)) if v.nbytes else None
                args[k] = bufs[k].ptr if v.nbytes else 0
    try:
        h.logpdf_grid_ragged(dtype, A.MEM_DEVICE if device else A.MEM_HOST, pk["layout"], nb, D, pk["offsets"], args["X"], pk["ldx"],
                             args["y"], pk["noise_kind"], args["s"], pk["strides"], pk["prior_kind"], args["mw"], D, args["Lw"],
                             pk["ldl"], pk["Lw"].shape[1], G, args["alpha"], 0 if shared else G, args["tau"], 0 if shared else G,
                             args["lp"], G, args["best"], args["mw_best"], D, args["T_best"], max(D, 1), D * D, args["info"], G)
        if device:
            for k, v in out.items():
                if v is not None:
                    h.memcpy_d2h(v, args[k])
    finally:
        for b in bufs.values():
            if b is not None:
                b.free()
    return out


def call_singles(B, pk, alpha, tau, shared=True, want_best=True, want_post=True, sentinel=np.nan, regs=None):
    """The yardstick: blr_logpdf_grid_* with B = 1, host memspace, on each regressor's slice of the packed arrays (addressed in
    place: base pointer + offset, the packed ldx) -> the outputs of call_ragged, rows of regressors outside ``regs`` untouched."""
    A = B._abi
    h = A.default_handle()
    nb, D, dtype = pk["nb"], pk["D"], pk["dtype"]
    isz = np.dtype(dtype).itemsize
    G = _n_settings(alpha, tau)
    al, ta = _settings(pk, alpha, tau, shared)
    out = _outputs(pk, G, want_best, want_post, sentinel)
    X0, y0, s0 = pk["X"].ctypes.data, pk["y"].ctypes.data, pk["s"].ctypes.data
    colv = pk["layout"] == A.LAYOUT_COLVECS
    diag = pk["noise_kind"] == A.NOISE_DIAGONAL
    for b in (range(nb) if regs is None else regs):
        o, n = int(pk["offsets"][b]), int(pk["counts"][b])
        sub = lambda v: None if v is None else (v if shared else v[b])  # noqa: E731
        h.logpdf_grid(dtype, A.MEM_HOST, pk["layout"], 1, D, n, X0 + isz * (o * pk["ldx"] if colv else o), pk["ldx"], 0, y0 + isz * o, 0,
                      pk["noise_kind"], s0 + isz * (o if diag else b * pk["strides"]), 0, pk["prior_kind"], pk["mw"][b], 0, pk["Lw"][b],
                      pk["ldl"], 0, G, sub(al), 0, sub(ta), 0, out["lp"][b], G, out["best"][b:b + 1] if want_best else None,
                      None if out["mw_best"] is None else out["mw_best"][b], D, None if out["T_best"] is None else out["T_best"][b],
                      max(D, 1), D * D,
                      out["info"][b], G)
    return out


def same_bits(r1, r2, rows1=None, rows2=None):
    """every output of the rows of r1 equals (NaNs equal) that of the rows of r2"""
    for k in r1:
        if r1[k] is None or r2[k] is None:
            assert r1[k] is None and r2[k] is None, k
            continue
        a = r1[k] if rows1 is None else r1[k][rows1]
        b = r2[k] if rows2 is None else r2[k][rows2]
        assert np.array_equal(a, b, equal_nan=a.dtype.kind == "f"), k
