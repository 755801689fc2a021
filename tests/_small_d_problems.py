"""Problems of the fused small-D kernels (D <= 128) for the GPU tests: packed batches with every layout / alignment / noise / prior
kind, strided outputs, the oracle checks at the header's tolerances, and the lattice of fused_small_kernel<T, NB, MODE>
instantiations with the rule that says which one a call runs.  A plain module, not a conftest; importing it needs no GPU."""
import numpy as np

from _yardsticks import _assert_fp32_within_lapack
from blr_amd import _abi
from oracle import blr_oracle as O

# empty, one column, both sides of the 32- and 64-column stage, several stages, a tail that is no multiple of the 4-column k-step
COUNTS = [0, 1, 31, 32, 33, 64, 200, 5, 129]


def _batch(D, dtype, xkind, noise, prior, shared_prior, counts=COUNTS, seed=0, pad_value=np.nan):
    """One packed batch.  xkind: "col16" (ColVecs, ldx = D rounded up to 16 bytes), "colpad" (16 bytes more), "colodd" (ColVecs, odd ldx > D), "row"
    (RowVecs, ldx = offsets[B] + 3).  noise: "iso" (one variance per regressor), "iso0" (one for all), "diag".  prior: "diag",
    "dense", "factor" (entries that are multiples of 1/8: U'U is exact in fp32 too).  Padding elements of X hold pad_value."""
    rng = np.random.Generator(np.random.PCG64(1000 * D + seed))
    nb = len(counts)
    offsets = np.concatenate(([0], np.cumsum(counts))).astype(np.int64)
    total = int(offsets[-1])
    Xd = rng.standard_normal((D, total)).astype(dtype)  # the data, D x total
    if xkind == "row":
        layout, ldx = _abi.LAYOUT_ROWVECS, total + 3
        Xp = np.full((ldx, D), pad_value, dtype=dtype, order="F")
        Xp[:total, :] = Xd.T
    else:
        layout = _abi.LAYOUT_COLVECS
        per16 = 16 // np.dtype(dtype).itemsize
        ldx = (D + 1) | 1 if xkind == "colodd" else -(-D // per16) * per16 + (per16 if xkind == "colpad" else 0)
        Xp = np.full((ldx, total), pad_value, dtype=dtype, order="F")
        Xp[:D, :] = Xd
    w = rng.standard_normal(D) / np.sqrt(D)
    if noise == "diag":
        s = np.exp(0.3 * rng.standard_normal(total)).astype(dtype)
        strides = 0
        s_of = lambda b: s[offsets[b]:offsets[b + 1]]  # noqa: E731
    elif noise == "iso":
        s = np.exp(0.3 * rng.standard_normal(nb)).astype(dtype)
        strides = 1
        s_of = lambda b: s[b]  # noqa: E731
    else:
        s = np.array([0.7], dtype=dtype)
        strides = 0
        s_of = lambda b: s[0]  # noqa: E731
    y = (Xd.astype(float).T @ w + 0.8 * rng.standard_normal(total)).astype(dtype)
    npri = 1 if shared_prior else nb
    mw = (0.2 * rng.standard_normal((npri, D))).astype(dtype)
    if prior == "diag":
        Lw = np.exp(0.3 * rng.standard_normal((npri, D))).astype(dtype)
        ldl, dense_of = 1, lambda p: Lw[p]  # noqa: E731
    else:
        Lw = np.zeros((npri, D * D), dtype=dtype)
        mats = []
        for p in range(npri):
            if prior == "factor":
                U = np.triu(rng.integers(-1, 2, size=(D, D)) / 8.0, 1) + np.diag(1.0 + rng.integers(0, 5, size=D) / 8.0)
                Lw[p] = U.reshape(-1, order="F")
                mats.append((U.T @ U).astype(dtype))
            else:
                Bm = rng.standard_normal((D, D)) / np.sqrt(D)
                M = (Bm @ Bm.T + np.eye(D)).astype(dtype)
                M = np.triu(M) + np.triu(M, 1).T
                Lw[p] = M.reshape(-1, order="F")
                mats.append(M)
        ldl, dense_of = D, lambda p: mats[p]  # noqa: E731
    kind = {"diag": _abi.PRIOR_DIAGONAL, "dense": _abi.PRIOR_DENSE, "factor": _abi.PRIOR_UPPER_FACTOR}[prior]
    return dict(D=D, dtype=dtype, nb=nb, offsets=offsets, layout=layout, ldx=ldx, X=Xp, Xd=Xd, y=y, s=s, strides=strides, s_of=s_of,
                noise_kind=_abi.NOISE_DIAGONAL if noise == "diag" else _abi.NOISE_ISOTROPIC, prior_kind=kind, mw=mw, Lw=Lw, ldl=ldl,
                stridemw=0 if shared_prior else D, strideLw=0 if shared_prior else Lw.shape[1], dense_of=dense_of,
                pri=(lambda b: 0) if shared_prior else (lambda b: b))


def _equal_batch(D, dtype, N, xkind, noise, prior, shared_prior, nb=5, seed=0, pad_value=np.nan):
    """nb regressors of N observations each for blr_posterior_batched_*: the packed batch of _batch with equal counts, which IS a
    strided batch (ColVecs: regressor b starts N columns on, strideX = ldx N; RowVecs: N rows on, strideX = N; y and a diagonal
    noise N elements on).  Layout, alignment, noise and prior kinds are _batch's; shared_prior gives one prior at stride 0."""
    q = _batch(D, dtype, xkind, noise, prior, shared_prior, counts=[N] * nb, seed=seed, pad_value=pad_value)
    q["N"] = N
    q["strideX"] = N if q["layout"] == _abi.LAYOUT_ROWVECS else q["ldx"] * N
    q["stride_s"] = N if q["noise_kind"] == _abi.NOISE_DIAGONAL else q["strides"]
    return q


def _batched(hd, q, o):
    """blr_posterior_batched_* on a batch of _equal_batch, host memspace, into the buffers of _outputs"""
    return hd.posterior_batched(q["dtype"], _abi.MEM_HOST, q["layout"], q["nb"], q["D"], q["N"], q["X"], q["ldx"], q["strideX"], q["y"], q["N"],
                                q["noise_kind"], q["s"], q["stride_s"], q["prior_kind"], q["mw"], q["stridemw"], q["Lw"], q["ldl"],
                                q["strideLw"], o["mw_post"], o["stride_mwpost"], o["T"], o["ldt"], o["strideT"], o["A"], o["ldt"],
                                o["strideT"], o["lp"], o["info"])


def _outputs(nb, D, dtype, gaps=False, fill=np.nan):
    ldt = D + 2 if gaps else D
    st_m = D + 3 if gaps else D
    st_T = ldt * D + (5 if gaps else 0)
    return dict(mw_post=np.full(nb * st_m, fill, dtype=dtype), stride_mwpost=st_m, T=np.full(nb * st_T, fill, dtype=dtype), ldt=ldt,
                strideT=st_T, A=np.full(nb * st_T, fill, dtype=dtype), lp=np.full(nb, 123.0), info=np.full(nb, -7, dtype=np.int32))


def _written(nb, D, o):
    """masks of the elements of (mw_post, T / A) that belong to a result; everything else is a gap"""
    written_m = np.zeros(o["mw_post"].shape, dtype=bool)
    written_T = np.zeros(o["T"].shape, dtype=bool)
    for b in range(nb):
        written_m[b * o["stride_mwpost"]:b * o["stride_mwpost"] + D] = True
        for c in range(D):
            written_T[b * o["strideT"] + c * o["ldt"]:b * o["strideT"] + c * o["ldt"] + D] = True
    return written_m, written_T


def _mat(buf, b, D, ld, stride):
    return buf[b * stride + np.arange(D)[None, :] * ld + np.arange(D)[:, None]]


def _result(q, o, b):
    D = q["D"]
    return (o["mw_post"][b * o["stride_mwpost"]:b * o["stride_mwpost"] + D].copy(), _mat(o["T"], b, D, o["ldt"], o["strideT"]),
            _mat(o["A"], b, D, o["ldt"], o["strideT"]), float(o["lp"][b]), int(o["info"][b]))


def _single(hd, q, b):
    """regressor b alone: blr_posterior_batched_* with B = 1 on its slice of the packed arrays (same ldx, same alignment class)"""
    D, dtype = q["D"], q["dtype"]
    o0, o1 = int(q["offsets"][b]), int(q["offsets"][b + 1])
    Xs = q["X"][o0:, :] if q["layout"] == _abi.LAYOUT_ROWVECS else q["X"][:, o0:]
    s = q["s"][o0:] if q["noise_kind"] == _abi.NOISE_DIAGONAL else q["s"][b * q["strides"]:]
    if s.size == 0:
        s = np.ones(1, dtype=dtype)
    if Xs.size == 0:
        Xs = np.zeros((1, 1), dtype=dtype)
    p = q["pri"](b)
    mw_post, T, A = np.full(D, np.nan, dtype=dtype), np.full((D, D), np.nan, dtype=dtype, order="F"), np.full((D, D), np.nan, dtype=dtype, order="F")
    lp, info = np.zeros(1), np.zeros(1, dtype=np.int32)
    hd.posterior_batched(dtype, _abi.MEM_HOST, q["layout"], 1, D, o1 - o0, Xs, q["ldx"], 0, q["y"][o0:] if o1 > o0 else np.zeros(1, dtype=dtype),
                         0, q["noise_kind"], s, 0, q["prior_kind"], q["mw"][p], 0, q["Lw"][p], q["ldl"], 0, mw_post, D, T, D, D * D, A, D,
                         D * D, lp, info)
    return mw_post, T, A, float(lp[0]), int(info[0])


def _same_bits(r1, r2, what=""):
    for x, y_, name in zip(r1, r2, ("mw'", "T", "Lw'", "logpdf", "info")):
        assert np.array_equal(np.asarray(x), np.asarray(y_), equal_nan=True), (what, name)


def _oracle_inputs(q, b):
    """(mw, Lw, X, s, y) of regressor b as the oracle takes them, in the batch's element type"""
    o0, o1 = int(q["offsets"][b]), int(q["offsets"][b + 1])
    p = q["pri"](b)
    return q["mw"][p], q["dense_of"](p), q["Xd"][:, o0:o1], q["s_of"](b), q["y"][o0:o1]


def _check_oracle(q, b, res):
    """-> the errors that were held to the bounds.  fp64: (evidence: relative to max(1, |.|); mw', T, Lw': largest
    |got - ref| / (1e-11 + 1e-9 |ref|), <= 1 inside the bound).  fp32: what _assert_fp32_within_lapack returns."""
    mw_p, T, A, lp, info = res
    assert info == 0
    mw, Lw, Xb, sb, yb = _oracle_inputs(q, b)
    if q["dtype"] == np.float32:
        return _assert_fp32_within_lapack(mw, Lw, np.asfortranarray(Xb), np.asarray(sb, dtype=np.float32), yb, mw_p, A, lp, got_T=T,
                                          what=f"regressor {b}")
    f64 = lambda a: np.asarray(a, dtype=np.float64)  # noqa: E731
    mw_o, T_o, A_o = O.posterior_literal(f64(mw), f64(Lw), f64(Xb), f64(sb), f64(yb))
    lp_o = O.logpdf_literal(f64(mw), f64(Lw), f64(Xb), f64(sb), f64(yb))
    assert abs(lp - lp_o) <= 1e-10 * max(1.0, abs(lp_o)), (b, lp, lp_o)
    np.testing.assert_allclose(mw_p, mw_o, rtol=1e-9, atol=1e-11, err_msg=f"mw' of regressor {b}")
    np.testing.assert_allclose(T, T_o, rtol=1e-9, atol=1e-11, err_msg=f"T of regressor {b}")
    np.testing.assert_allclose(A, A_o, rtol=1e-9, atol=1e-11, err_msg=f"Lw' of regressor {b}")
    used = lambda got, ref: float(np.max(np.abs(got - ref) / (1e-11 + 1e-9 * np.abs(ref))))  # noqa: E731
    return abs(lp - lp_o) / max(1.0, abs(lp_o)), used(mw_p, mw_o), used(T, T_o), used(A, A_o)


# ---- the lattice of fused_small_kernel<T, NB, MODE> -------------------------------------------------------------------------------
VEC = {np.float64: 2, np.float32: 4}  # elements of a 16-byte vector
TYPE_NAME = {np.float64: "double", np.float32: "float"}
LATTICE_OPTIONS = {"NO_I8_GRAM": "1", "NO_WAVE_KERNEL": "1"}            # the handle of the lattice tests ...
LATTICE_OPTIONS_MODE3 = dict(LATTICE_OPTIONS, NO_LDSDMA="1")            # ... and the one of their mode-3 rows
LATTICE_NS = (29, 64, 131)  # below one stage; one 64-column or two 32-column stages; several stages and a tail that is no multiple of 4
LATTICE_B = 5
ALL_ROUTES = frozenset(f"fused_small_kernel<{t}, {nb}, {m}>" for t in ("double", "float") for nb in range(1, 9) for m in (0, 1, 3, 4))


def expected_route(dtype, D, xkind, options):
    """The kernel dispatch_fused_small launches for a _batch / _equal_batch of this type, width and layout kind on a handle with
    these options (a mapping of the option names that are set to "1").  The int8 and the one-wave kernels take shapes away from
    fused_small_kernel unless NO_I8_GRAM and NO_WAVE_KERNEL are set, so the rule is stated for handles that set both."""
    dtype = np.dtype(dtype).type
    on = lambda key: str(options.get(key, "0")) == "1"  # noqa: E731
    if not (on("NO_I8_GRAM") and on("NO_WAVE_KERNEL")):
        raise ValueError("expected_route speaks of handles with NO_I8_GRAM = 1 and NO_WAVE_KERNEL = 1")
    if not 1 <= D <= 128:
        raise ValueError("the fused small-D kernels take 1 <= D <= 128")
    if xkind == "row":
        mode = 1
    elif xkind in ("col16", "colpad") and D % VEC[dtype] == 0:  # base, ldx and stride are multiples of 16 bytes
        mode = 3 if on("NO_LDSDMA") else 4
    elif xkind in ("col16", "colpad", "colodd"):
        mode = 0
    else:
        raise ValueError(f"unknown layout kind {xkind!r}")
    return f"fused_small_kernel<{TYPE_NAME[dtype]}, {(D + 15) // 16}, {mode}>"


def lattice_widths(dtype, NB):
    """(D_lo, D_mid, D_hi): the first row of the last block (odd: modes 0 and 1 only), the last block short by one vector, a full block"""
    return 16 * NB - 15, 16 * NB - VEC[dtype], 16 * NB


def _lattice():
    noises, priors = ("iso", "iso0", "diag"), ("diag", "dense", "factor")
    rows = []
    for dtype in (np.float64, np.float32):
        for NB in range(1, 9):
            lo, mid, hi = lattice_widths(dtype, NB)
            cells = [(lo, "col16", False), (lo, "row", False)]
            for D in (mid, hi):
                cells += [(D, "colodd", False), (D, "row", False), (D, "col16", True), (D, "col16", False)]
            for i, (D, xkind, no_ldsdma) in enumerate(cells):  # 10 cells: the 9 (noise, prior) pairs, the first one twice
                for N in LATTICE_NS:                           # every cell at every N: the stage pipeline differs with NB
                    rows.append(dict(dtype=dtype, NB=NB, D=D, xkind=xkind, mode3=no_ldsdma, N=N, noise=noises[i % 3],
                                     prior=priors[(i // 3) % 3], shared_prior=(i + NB) % 2 == 1,
                                     options=LATTICE_OPTIONS_MODE3 if no_ldsdma else LATTICE_OPTIONS))
    for r in rows:
        r["route"] = expected_route(r["dtype"], r["D"], r["xkind"], r["options"])
        r["id"] = f"{'f64' if r['dtype'] == np.float64 else 'f32'}-NB{r['NB']}-D{r['D']}-{r['xkind']}{'-noldsdma' if r['mode3'] else ''}-N{r['N']}-" \
                  f"{r['noise']}-{r['prior']}{'-shared' if r['shared_prior'] else ''}"
    return rows


LATTICE = _lattice()


def lattice_batch(row, nb=LATTICE_B, pad_value=np.nan):
    return _equal_batch(row["D"], row["dtype"], row["N"], row["xkind"], row["noise"], row["prior"], row["shared_prior"], nb=nb,
                        pad_value=pad_value)
