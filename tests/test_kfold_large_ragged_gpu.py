"""Ragged large-fold leave-fold-out predictives (blr_kfold_large_ragged_*, kfold_large_ragged, cross_validate_ragged)
on the GPU: parity with the float64 closed form of tests/_kfold_large_ref.py on every slice, bit-equality with
blr_kfold_large_batched_* at B = 1, N = N_b, F = F_b on every slice (the header's main promise), bit-equality of the call with itself
(permutation, subset, chunking, memspace, outputs, repetition), the canaries, the status, the NaN rule and the Python front end.  All
tests need an MI355X.

Tolerances are those tests/test_kfold_large_gpu.py applies to blr_kfold_large_batched_*: fp64 rtol 1e-9 / atol 1e-12 against the
closed form, fp32 the bounds of _kfold_large_ref.fp32_bounds_large; kf_total against math.fsum of the folds at rel 1e-12.  The inputs
are those of tests/_kfold_large_ragged_data.py, whose folds tests/test_kfold_large_ragged_cpu.py shows to be well inside the state."""
import math

import numpy as np
import pytest

from _kfold_large_ref import closed_form_large
import _kfold_large_ragged_data as K

pytestmark = pytest.mark.gpu

CANARY = 7.0
LAYOUTS = ["col", "col_unaligned", "row"]
DTYPES = [np.float64, np.float32]


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


class Packed:
    """The regressors `regs` of batch P (any order, any subset) packed side by side behind LEAD unowned observations, with their
    states under noise `noise` and their fold sizes."""

    def __init__(self, P, noise, dtype, regs=None):
        regs = list(range(P.nb)) if regs is None else list(regs)
        self.P, self.noise, self.dtype, self.regs, self.D = P, noise, dtype, regs, P.D
        self.counts = [P.counts[b] for b in regs]
        self.folds = np.array([P.folds[b] for b in regs], dtype=np.int64)
        self.nb = len(regs)
        self.off = np.concatenate([[K.LEAD], K.LEAD + np.cumsum(self.counts)]).astype(np.int64)
        self.fo = P.fold_offsets(regs)
        self.tot = int(self.off[-1])
        self.X, self.y, self.s_diag = np.zeros((P.D, self.tot)), np.zeros(self.tot), np.ones(self.tot)
        for i, b in enumerate(regs):
            self.X[:, self.sl(i)], self.y[self.sl(i)], self.s_diag[self.sl(i)] = P.X[:, P.sl(b)], P.y[P.sl(b)], P.s_diag[P.sl(b)]
        self.s_reg = P.s_reg[regs] if noise == "per_regressor" else P.s_reg[:1]
        mw, T = P.states(noise, dtype)
        self.mw, self.T = np.ascontiguousarray(mw[regs]), np.ascontiguousarray(T[regs])  # T column-major per regressor

    def sl(self, i):
        return slice(int(self.off[i]), int(self.off[i + 1]))

    def fl(self, i):
        return slice(int(self.fo[i]), int(self.fo[i + 1]))

    def noise_args(self, A):
        if self.noise == "one":
            return A.NOISE_ISOTROPIC, np.ascontiguousarray(self.s_reg[:1], dtype=self.dtype), 0
        if self.noise == "per_regressor":
            return A.NOISE_ISOTROPIC, np.ascontiguousarray(self.s_reg, dtype=self.dtype), 1
        return A.NOISE_DIAGONAL, np.ascontiguousarray(self.s_diag, dtype=self.dtype), 0

    def x_args(self, A, layout):
        """-> (layout constant, X view handed to the library, ldx, the buffer that owns it).  The padding between the columns
        (ColVecs: rows D .. ldx - 1; RowVecs: rows tot .. ldx - 1) holds NaN: a lane that read it would poison its output."""
        D, tot, dtype = self.D, self.tot, self.dtype
        vec = 16 // np.dtype(dtype).itemsize
        if layout == "row":
            ldx = tot + 3
            buf = np.full(ldx * D + 1, np.nan, dtype=dtype)
            M = buf[:ldx * D].reshape((ldx, D), order="F")
            M[:tot, :] = self.X.T
            return A.LAYOUT_ROWVECS, M, ldx, buf
        ldx = D + vec if D % vec == 0 else D + 3
        raw = np.full(ldx * tot + 2 * vec, np.nan, dtype=dtype)
        start = (-raw.ctypes.data // raw.itemsize) % vec  # element index of a 16-byte aligned address
        if layout == "col_unaligned":
            start += 1
        M = raw[start:start + ldx * tot].reshape((ldx, tot), order="F")
        M[:D, :] = self.X
        assert (M.ctypes.data % 16 == 0) == (layout == "col")
        return A.LAYOUT_COLVECS, M, ldx, raw


def _run(B, h, Q, layout="col", want=(True, True, True, True), device=False, mw=None, T=None, y=None, s=None):
    """blr_kfold_large_ragged_* on the pack Q -> (kf_mean, kf_var, kf_logpdf, kf_total, info), canaries where nothing was to be written"""
    A = B._abi
    dtype, D = Q.dtype, Q.D
    lay, X, ldx, own = Q.x_args(A, layout)
    nk, s0, strides = Q.noise_args(A)
    s = s0 if s is None else np.ascontiguousarray(s, dtype=dtype)
    nf = int(Q.fo[-1])
    yv = np.ascontiguousarray(Q.y if y is None else y, dtype=dtype)
    mwv, Tv = (Q.mw if mw is None else mw), (Q.T if T is None else T)
    outs = [np.full(Q.tot + 4, CANARY, dtype=dtype), np.full(Q.tot + 4, CANARY, dtype=dtype), np.full(nf + 4, CANARY), np.full(Q.nb, CANARY)]
    info = np.full(Q.nb, -9, dtype=np.int32)
    if not device:
        o = [a if w else None for a, w in zip(outs, want)]
        h.kfold_large_ragged(dtype, A.MEM_HOST, lay, Q.nb, D, Q.off, Q.folds, X, ldx, yv, nk, s, strides, mwv, D, Tv, D, D * D, o[0], o[1], o[2], o[3],
                             info)
    else:
        from blr_amd.regressor import _DeviceBuffer as DB

        bufs = [DB.of(h, a) for a in [own, yv, s, mwv, Tv] + outs + [info]]
        try:
            p = [b.ptr for b in bufs]
            o = [q if w else None for q, w in zip(p[5:9], want)]
            h.kfold_large_ragged(dtype, A.MEM_DEVICE, lay, Q.nb, D, Q.off, Q.folds, p[0] + (X.ctypes.data - own.ctypes.data), ldx, p[1], nk, p[2],
                                 strides, p[3], D, p[4], D, D * D, o[0], o[1], o[2], o[3], p[9])
            for host, ptr in zip(outs + [info], p[5:]):
                h.memcpy_d2h(host, ptr)
        finally:
            for b in bufs:
                b.free()
    return outs[0], outs[1], outs[2], outs[3], info


def _batched_one(B, h, Q, i, y=None):
    """blr_kfold_large_batched_* with B = 1, N = N_b, F = F_b on the i-th slice of Q (contiguous ColVecs) -> (mean, var, logpdf, total, info)"""
    A = B._abi
    dtype, D, N, F = Q.dtype, Q.D, Q.counts[i], int(Q.folds[i])
    nf = K.nfolds(N, F)
    X = np.ascontiguousarray(Q.X[:, Q.sl(i)].T, dtype=dtype).reshape(-1)  # column n at n D
    yv = np.ascontiguousarray((Q.y if y is None else y)[Q.sl(i)], dtype=dtype)
    if Q.noise == "diagonal":
        nk, s = A.NOISE_DIAGONAL, np.ascontiguousarray(Q.s_diag[Q.sl(i)], dtype=dtype)
    else:
        nk, s = A.NOISE_ISOTROPIC, np.ascontiguousarray(Q.s_reg[i if Q.noise == "per_regressor" else 0:][:1], dtype=dtype)
    m, v, lp, tot = np.full(N, CANARY, dtype=dtype), np.full(N, CANARY, dtype=dtype), np.full(nf, CANARY), np.full(1, CANARY)
    info = np.full(1, -9, dtype=np.int32)
    h.kfold_large(dtype, A.MEM_HOST, A.LAYOUT_COLVECS, 1, D, N, F, X, D, D * N, yv, N, nk, s, 0, np.ascontiguousarray(Q.mw[i]), D,
                  np.ascontiguousarray(Q.T[i]), D, D * D, m, N, v, N, lp, nf, tot, info)
    return m, v, lp, tot[0], info[0]


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def _slices(Q, out):
    """the outputs of a packed call cut per regressor: [(mean, var, logpdf, total)]"""
    m, v, lp, tot, _ = out
    return [(m[Q.sl(i)], v[Q.sl(i)], lp[Q.fl(i)], tot[i]) for i in range(Q.nb)]


def _canaries_intact(Q, out):
    m, v, lp, tot, info = out
    for a in (m, v):
        assert np.all(a[:K.LEAD] == CANARY) and np.all(a[Q.tot:] == CANARY)
    assert np.all(lp[int(Q.fo[-1]):] == CANARY)


def _check_parity(Q, out):
    P = Q.P
    _canaries_intact(Q, out)
    assert not out[4].any()
    for i, (m, v, lp, tot) in enumerate(_slices(Q, out)):
        b = Q.regs[i]
        if Q.counts[i] == 0:
            assert len(m) == len(v) == len(lp) == 0 and tot == 0.0
            continue
        if Q.dtype == np.float64:
            m_o, v_o, lp_o, _ = P.reference(Q.noise, np.float64, b)
            np.testing.assert_allclose(m, m_o, rtol=1e-9, atol=1e-12)
            np.testing.assert_allclose(v, v_o, rtol=1e-9, atol=1e-12)
            np.testing.assert_allclose(lp, lp_o, rtol=1e-9, atol=1e-12)
        else:
            truth, bounds = P.bounds32(Q.noise, b)
            for got, t, bd, name in zip((m, v, lp), truth, bounds, ("mean", "var", "logpdf")):
                err = float(np.max(np.abs(got.astype(np.float64) - t)))
                print("fp32", Q.D, b, name, err, bd)
                assert err <= bd, (b, name, err, bd)
        assert tot == pytest.approx(math.fsum(lp), rel=1e-12)


# ---- 1. parity with the float64 closed form -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D,layout,noise", [(5, "col", "one"), (5, "row", "diagonal"), (5, "col_unaligned", "per_regressor"),
                                            (17, "row", "one"), (17, "col_unaligned", "diagonal"), (17, "col", "per_regressor")])
def test_parity(B, h, D, layout, noise, dtype):
    Q = Packed(K.batch(D), noise, dtype)
    _check_parity(Q, _run(B, h, Q, layout=layout))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("layout,noise", [("col", "diagonal"), ("row", "per_regressor"), ("col_unaligned", "one")])
def test_parity_d128(B, h, layout, noise, dtype):
    Q = Packed(K.batch(K.BIG_D, K.BIG_COUNTS, K.BIG_FOLDS), noise, dtype)
    _check_parity(Q, _run(B, h, Q, layout=layout))


# ---- 2. the main promise: every output of every slice has the bits of the equal-count entry point at B = 1 -------------------------
def _check_b1(B, h, Q, out):
    for i, (m, v, lp, tot) in enumerate(_slices(Q, out)):
        m1, v1, lp1, tot1, info1 = _batched_one(B, h, Q, i)
        assert info1 == out[4][i] == 0
        assert _same(m, m1) and _same(v, v1) and _same(lp, lp1), (i, Q.counts[i], int(Q.folds[i]))
        assert tot == tot1 if Q.counts[i] else tot == 0.0, (i, tot, tot1)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("noise", K.NOISES)
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("D", K.DS)
def test_bits_of_b1(B, h, D, layout, noise, dtype):
    Q = Packed(K.batch(D), noise, dtype)
    _check_b1(B, h, Q, _run(B, h, Q, layout=layout))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("layout,noise", [("col", "diagonal"), ("row", "per_regressor"), ("col_unaligned", "one")])
def test_bits_of_b1_d128(B, h, layout, noise, dtype):
    Q = Packed(K.batch(K.BIG_D, K.BIG_COUNTS, K.BIG_FOLDS), noise, dtype)
    _check_b1(B, h, Q, _run(B, h, Q, layout=layout))


# ---- 3. the call against itself ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_bits_permutation_subset_chunking_memspace_outputs_repetition(B, h, dtype):
    P = K.batch(17)
    Q = Packed(P, "diagonal", dtype)
    base = _run(B, h, Q, layout="row")
    ref = {b: s for b, s in zip(Q.regs, _slices(Q, base))}
    assert h.get_stat("last_chunks") == 1

    def agrees(R, out):
        _canaries_intact(R, out)
        for b, (m, v, lp, tot) in zip(R.regs, _slices(R, out)):
            m0, v0, lp0, tot0 = ref[b]
            assert _same(m, m0) and _same(v, v0) and _same(lp, lp0) and tot == tot0, b

    assert all(_same(a, b) for a, b in zip(base, _run(B, h, Q, layout="row")))          # repetition
    perm = [8, 0, 3, 7, 1, 6, 2, 5, 4]
    R = Packed(P, "diagonal", dtype, perm)
    agrees(R, _run(B, h, R, layout="row"))                                                 # a permuted batch
    agrees(R, _run(B, h, R, layout="col"))                                                 # ... and another layout
    S = Packed(P, "diagonal", dtype, [7, 4])
    agrees(S, _run(B, h, S, layout="col_unaligned"))                                       # a subset
    for cap, chunks in ((1, 9), (2, 5)):
        h.set_option("MAX_CHUNK", cap)
        try:
            out = _run(B, h, Q, layout="row")
            assert h.get_stat("last_chunks") == chunks
        finally:
            h.set_option("MAX_CHUNK", None)
        assert all(_same(a, b) for a, b in zip(base, out))
    assert all(_same(a, b) for a, b in zip(base, _run(B, h, Q, layout="row", device=True)))  # device memspace
    for k in range(4):                                                                     # each output alone
        want = tuple(j == k for j in range(4))
        out = _run(B, h, Q, layout="row", want=want)
        for j in range(4):
            assert _same(out[j], base[j]) if j == k else np.all(out[j] == CANARY), (k, j)
        assert _same(out[4], base[4])


# ---- 4. canaries and N_b = 0 ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_empty_regressors_and_gaps(B, h, dtype):
    P = K.batch(5)
    Q = Packed(P, "per_regressor", dtype, [0, 4, 0, 0, 2, 0])   # empty regressors at both ends and side by side
    out = _run(B, h, Q, layout="col")
    _canaries_intact(Q, out)
    m, v, lp, tot, info = out
    assert not info.any()
    assert tot[[0, 2, 3, 5]].tolist() == [0.0] * 4 and len(lp) - 4 == 2 + 7
    R = Packed(P, "per_regressor", dtype, [4, 2])
    for a, b in zip(_slices(Q, out)[1::3], _slices(R, _run(B, h, R, layout="col"))):
        assert all(_same(x, y) for x, y in zip(a, b))
    E = Packed(P, "one", dtype, [0, 0])                         # no observation at all
    m, v, lp, tot, info = _run(B, h, E)
    assert np.all(m == CANARY) and np.all(v == CANARY) and np.all(lp == CANARY) and tot.tolist() == [0.0, 0.0] and info.tolist() == [0, 0]
    Tbad = E.T.copy()
    Tbad[1, 2, 2] = -1.0                                        # the state's status is reported, the total left alone
    m, v, lp, tot, info = _run(B, h, E, T=Tbad)
    assert info.tolist() == [0, 3] and tot.tolist() == [0.0, CANARY]


# ---- 5. the status ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_status_leaves_outputs_untouched_and_neighbours_alone(B, h, dtype):
    P = K.batch(5)
    Q = Packed(P, "diagonal", dtype, [4, 5, 6, 2])
    good = _run(B, h, Q)
    Tbad = Q.T.copy()
    Tbad[1, 3, 3] = 0.0                       # regressor 1: diagonal entry j = 4 (one-based) of its factor
    sbad = np.ascontiguousarray(Q.s_diag, dtype=dtype).copy()
    sbad[int(Q.off[2]) + 10] = -1.0           # regressor 2: s_i <= 0 at i = 11 counted WITHIN its slice
    out = _run(B, h, Q, T=Tbad, s=sbad)
    _canaries_intact(Q, out)
    assert out[4].tolist() == [0, 4, 11, 0]
    for i, (a, b) in enumerate(zip(_slices(Q, out), _slices(Q, good))):
        if i in (1, 2):
            assert all(np.all(np.asarray(x) == CANARY) for x in a), i   # untouched, kf_total included
        else:
            assert all(_same(x, y) for x, y in zip(a, b)), i            # the neighbours keep their bits


# ---- 6. the NaN rule -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_nan_rule_one_fold(B, h, dtype):
    """A fold the state does not contain: fold 1 of the (1100, 550) regressor gets inputs scaled by 40 the state was not conditioned
    on, so that A - G_f has a negative pivot in the float64 reference.  NaN in that fold only, one count, the other folds' bits."""
    P = K.batch(5)
    Q = Packed(P, "diagonal", dtype, [5, 6, 4])
    good = _run(B, h, Q)
    lo = int(Q.off[1]) + 550
    R = Packed(P, "diagonal", dtype, [5, 6, 4])
    R.X = Q.X.copy()
    R.X[:, lo:lo + 550] *= 40.0
    mwp, Tu, X, s, y = (np.asarray(a).astype(dtype).astype(np.float64) for a in (R.mw[1], R.T[1].T, R.X[:, R.sl(1)], R.s_diag[R.sl(1)], R.y[R.sl(1)]))
    Af = Tu.T @ Tu - (X[:, 550:] / s[550:]) @ X[:, 550:].T
    assert np.min(np.linalg.eigvalsh(Af)) < 0                                 # no factor in the reference
    with pytest.raises(np.linalg.LinAlgError):
        closed_form_large(mwp, Tu, X, s, y, 550)
    before = h.get_stat("kfold_degenerate")
    out = _run(B, h, R)
    assert h.get_stat("kfold_degenerate") - before == 1 and not out[4].any()
    _canaries_intact(R, out)
    (m, v, lp, tot), (m0, v0, lp0, _) = _slices(R, out)[1], _slices(Q, good)[1]
    assert np.all(np.isnan(m[550:])) and np.all(np.isnan(v[550:])) and np.isnan(lp[1]) and np.isnan(tot)
    assert _same(m[:550], m0[:550]) and _same(v[:550], v0[:550]) and lp[0] == lp0[0]   # fold 0 does not read fold 1's rows
    for i in (0, 2):
        assert all(_same(x, y) for x, y in zip(_slices(R, out)[i], _slices(Q, good)[i]))


# ---- 7. the Python front end ---------------------------------------------------------------------------------------------------------
def test_python_front_end(B):
    """kfold_large_ragged / cross_validate_ragged against a list of kfold_large / cross_validate on the slices.  The handle options
    NO_I8_GRAM = 1 and NO_WAVE_KERNEL = 1 make the states of blr_posterior_ragged_* and of `posterior` bit-equal (`kfold_ragged`'s
    docstring), so the large-fold results are; a slice whose F_b <= 64 goes through `kfold` in cross_validate -- another route --
    and is compared at the fp64 tolerance."""
    P = K.batch(17)
    regs = [4, 6, 2, 0, 7]
    Q = Packed(P, "diagonal", np.float64, regs)
    X, y, s = np.asfortranarray(Q.X[:, K.LEAD:]), Q.y[K.LEAD:].copy(), Q.s_diag[K.LEAD:].copy()
    off = Q.off - K.LEAD
    f = B.BayesianLinearRegressor(P.mw[4], B.PDMat(P.U[4]))
    hd = B._abi.default_handle()
    hd.set_option("NO_I8_GRAM", "1")
    hd.set_option("NO_WAVE_KERNEL", "1")
    try:
        got = B.kfold_large_ragged(f, B.ColVecs(X), off, B.Diagonal(s), y, Q.folds)
        cv = B.cross_validate_ragged(f, B.ColVecs(X), off, B.Diagonal(s), y, 2)
        one = B.kfold_large_ragged(f, B.ColVecs(X), off, B.Diagonal(s), y, 70)
        assert len(got) == len(cv) == len(one) == len(regs)
        for i, n in enumerate(Q.counts):
            sl = slice(int(off[i]), int(off[i + 1]))
            fx = f(B.ColVecs(np.asfortranarray(X[:, sl])), B.Diagonal(s[sl]))
            if n == 0:
                assert got[i].mean.shape == (0,) and got[i].logpdf.shape == (0,) and got[i].total == 0.0 and cv[i].total == 0.0
                continue
            for r, want in ((got[i], B.kfold_large(fx, y[sl], int(Q.folds[i]))), (one[i], B.kfold_large(fx, y[sl], 70))):
                assert isinstance(r, B.KFold)
                assert _same(r.mean, want.mean) and _same(r.var, want.var) and _same(r.logpdf, want.logpdf) and r.total == want.total
            want = B.cross_validate(fx, y[sl], 2)
            assert cv[i].logpdf.shape == want.logpdf.shape == (min(2, n),)
            if -(-n // 2) > 64:
                assert _same(cv[i].mean, want.mean) and _same(cv[i].var, want.var) and _same(cv[i].logpdf, want.logpdf) and cv[i].total == want.total
            else:
                np.testing.assert_allclose(cv[i].mean, want.mean, rtol=1e-9, atol=1e-12)
                np.testing.assert_allclose(cv[i].var, want.var, rtol=1e-9, atol=1e-12)
                np.testing.assert_allclose(cv[i].logpdf, want.logpdf, rtol=1e-9, atol=1e-12)
    finally:
        hd.set_option("NO_I8_GRAM", None)
        hd.set_option("NO_WAVE_KERNEL", None)
    with pytest.raises(ValueError):
        B.kfold_large_ragged(f, B.ColVecs(X), off, B.Diagonal(s), y, [1, 2])
    with pytest.raises(ValueError):
        B.cross_validate_ragged(f, B.ColVecs(X), off, B.Diagonal(s), y, 0)
