"""Ragged leave-fold-out predictives (blr_kfold_ragged_*, kfold_ragged) on the GPU: parity with the float64 closed form
of tests/_kfold_ref.py on every slice, bit-equality with blr_kfold_batched_* at B = 1 on every slice (the header's main promise),
bit-equality of the call with itself (permutation, B = 1, chunking, item size, memspace, outputs, repetition), the status and the NaN
rule, the Python front end and the D > 128 route.  All tests need an MI355X.

Tolerances are those tests/test_kfold_gpu.py applies to blr_kfold_batched_*: fp64 rtol 1e-9 / atol 1e-12 against the closed form
(D > 128: 1e-8 / 1e-10), fp32 the bounds of _kfold_ref.fp32_bounds; kf_total against math.fsum of the folds at rel 1e-12.  The inputs
are those of tests/_kfold_ragged_data.py, whose folds tests/test_kfold_ragged_cpu.py shows to be well inside the state."""
import math

import numpy as np
import pytest

from _kfold_ref import closed_form, fp32_bounds
import _kfold_ragged_data as K

pytestmark = pytest.mark.gpu

CANARY = 7.0
LAYOUTS = ["col", "col_unaligned", "row"]


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
    hd.set_option("RAGGED_ITEM", None)


class Packed:
    """The regressors `regs` of batch P (any order, any subset) packed side by side behind LEAD unowned observations, with their
    states under noise `noise` -- float64 data as cast to dtype, states from P.states (float64 oracle on the cast data)."""

    def __init__(self, P, noise, dtype, regs=None):
        regs = list(range(P.nb)) if regs is None else list(regs)
        self.P, self.noise, self.dtype, self.regs, self.D = P, noise, dtype, regs, P.D
        self.counts = [P.counts[b] for b in regs]
        self.nb = len(regs)
        self.off = np.concatenate([[K.LEAD], K.LEAD + np.cumsum(self.counts)]).astype(np.int64)
        self.tot = int(self.off[-1])
        self.X, self.y, self.s_diag = np.zeros((P.D, self.tot)), np.zeros(self.tot), np.ones(self.tot)
        for i, b in enumerate(regs):
            self.X[:, self.sl(i)], self.y[self.sl(i)], self.s_diag[self.sl(i)] = P.X[:, P.sl(b)], P.y[P.sl(b)], P.s_diag[P.sl(b)]
        self.s_reg = P.s_reg[regs] if noise == "per_regressor" else P.s_reg[:1]
        mw, T = P.states(noise, dtype)
        self.mw, self.T = np.ascontiguousarray(mw[regs]), np.ascontiguousarray(T[regs])  # T column-major per regressor

    def sl(self, i):
        return slice(int(self.off[i]), int(self.off[i + 1]))

    def fold_offsets(self, F):
        return np.concatenate([[0], np.cumsum([-(-n // F) for n in self.counts])]).astype(np.int64)

    def s_of(self, i):
        """per-observation variances of the i-th regressor of the pack, float64 as cast to dtype"""
        n = self.counts[i]
        if self.noise == "diagonal":
            s = self.s_diag[self.sl(i)]
        else:
            s = np.full(n, self.s_reg[i if self.noise == "per_regressor" else 0])
        return s.astype(self.dtype).astype(np.float64)

    def slice64(self, i):
        """(mw', T upper, X, s, y) of the i-th regressor in float64 as the library sees them"""
        c = lambda a: np.asarray(a).astype(self.dtype).astype(np.float64)  # noqa: E731
        return c(self.mw[i]), c(self.T[i]).T, c(self.X[:, self.sl(i)]), self.s_of(i), c(self.y[self.sl(i)])

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


def _run(B, h, Q, F, layout="col", want=(True, True, True, True), device=False):
    """blr_kfold_ragged_* on the pack Q -> (kf_mean, kf_var, kf_logpdf, kf_total, info), canaries where nothing was to be written"""
    A = B._abi
    dtype, D = Q.dtype, Q.D
    lay, X, ldx, own = Q.x_args(A, layout)
    nk, s, strides = Q.noise_args(A)
    nf = int(Q.fold_offsets(F)[-1])
    yv = np.ascontiguousarray(Q.y, dtype=dtype)
    outs = [np.full(Q.tot + 4, CANARY, dtype=dtype), np.full(Q.tot + 4, CANARY, dtype=dtype), np.full(nf + 4, CANARY), np.full(Q.nb, CANARY)]
    info = np.full(Q.nb, -9, dtype=np.int32)
    if not device:
        o = [a if w else None for a, w in zip(outs, want)]
        h.kfold_ragged(dtype, A.MEM_HOST, lay, Q.nb, D, Q.off, F, X, ldx, yv, nk, s, strides, Q.mw, D, Q.T, D, D * D, o[0], o[1], o[2], o[3], info)
    else:
        from blr_amd.regressor import _DeviceBuffer as DB

        bufs = [DB.of(h, a) for a in [own, yv, s, Q.mw, Q.T] + outs + [info]]
        try:
            p = [b.ptr for b in bufs]
            o = [q if w else None for q, w in zip(p[5:9], want)]
            h.kfold_ragged(dtype, A.MEM_DEVICE, lay, Q.nb, D, Q.off, F, p[0] + (X.ctypes.data - own.ctypes.data), ldx, p[1], nk, p[2], strides,
                           p[3], D, p[4], D, D * D, o[0], o[1], o[2], o[3], p[9])
            for host, ptr in zip(outs + [info], p[5:]):
                h.memcpy_d2h(host, ptr)
        finally:
            for b in bufs:
                b.free()
    return outs[0], outs[1], outs[2], outs[3], info


def _batched_one(B, h, Q, F, i):
    """blr_kfold_batched_* with B = 1 on the i-th slice of Q (contiguous ColVecs) -> (mean [N], var [N], logpdf [nfolds], total, info)"""
    A = B._abi
    dtype, D, N = Q.dtype, Q.D, Q.counts[i]
    nf = -(-N // F)
    X = np.ascontiguousarray(Q.X[:, Q.sl(i)].astype(dtype).reshape(-1, order="F"))
    y = np.ascontiguousarray(Q.y[Q.sl(i)], dtype=dtype)
    if Q.noise == "diagonal":
        nk, s = A.NOISE_DIAGONAL, np.ascontiguousarray(Q.s_diag[Q.sl(i)], dtype=dtype)
    else:
        nk, s = A.NOISE_ISOTROPIC, np.ascontiguousarray(Q.s_reg[[i if Q.noise == "per_regressor" else 0]], dtype=dtype)
    m, v, lp, tot = np.full(N, CANARY, dtype=dtype), np.full(N, CANARY, dtype=dtype), np.full(nf, CANARY), np.full(1, CANARY)
    info = np.full(1, -9, dtype=np.int32)
    h.kfold(dtype, A.MEM_HOST, A.LAYOUT_COLVECS, 1, D, N, F, X, D, 0, y, 0, nk, s, 0, np.ascontiguousarray(Q.mw[i]), 0,
            np.ascontiguousarray(Q.T[i]), D, 0, m, N, v, N, lp, nf, tot, info)
    return m, v, lp, tot[0], int(info[0])


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def _canaries(Q, F, g):
    """nothing outside the slices and the folds was written: the leading slots and the tails"""
    nf = int(Q.fold_offsets(F)[-1])
    for a in g[:2]:
        assert np.all(a[:K.LEAD] == CANARY) and np.all(a[Q.tot:] == CANARY)
    assert np.all(g[2][nf:] == CANARY)


def _check_parity(Q, F, g):
    """every slice against the float64 closed form (fp32: _kfold_ref.fp32_bounds)"""
    fo = Q.fold_offsets(F)
    assert not g[4].any()
    for i, n in enumerate(Q.counts):
        got = (g[0][Q.sl(i)], g[1][Q.sl(i)], g[2][fo[i]:fo[i + 1]])
        if n == 0:
            assert g[3][i] == 0.0
            continue
        mwp, T, X, s, y = Q.slice64(i)
        if Q.dtype == np.float64:
            m_o, v_o, lp_o, _ = closed_form(mwp, T, X, s, y, F)
            np.testing.assert_allclose(got[0], m_o, rtol=1e-9, atol=1e-12)
            np.testing.assert_allclose(got[1], v_o, rtol=1e-9, atol=1e-12)
            np.testing.assert_allclose(got[2], lp_o, rtol=1e-9, atol=1e-12)
        else:
            truth, bounds = fp32_bounds(mwp, T, X, s, y, F)
            for a, t, bd, name in zip(got, truth, bounds, ("mean", "var", "logpdf")):
                err = float(np.max(np.abs(a.astype(np.float64) - t)))
                print("fp32", Q.D, n, F, name, err, bd)
                assert err <= bd, (i, name, err, bd)
        assert g[3][i] == pytest.approx(math.fsum(got[2]), rel=1e-12)


def _check_bits_against_batched(B, h, Q, F, g):
    """THE promise: every output of every slice is what blr_kfold_batched_* with B = 1 writes on it"""
    fo = Q.fold_offsets(F)
    for i in range(Q.nb):
        m, v, lp, tot, info = _batched_one(B, h, Q, F, i)
        assert info == g[4][i] == 0
        assert _same(g[0][Q.sl(i)], m) and _same(g[1][Q.sl(i)], v), (i, Q.counts[i])
        assert _same(g[2][fo[i]:fo[i + 1]], lp) and _same(g[3][i], tot), (i, Q.counts[i])


# ---- 1. / 2. parity and bit-equality with blr_kfold_batched_*: the full F x D grid on one layout ------------------------------------
@pytest.mark.parametrize("F", K.FS)
@pytest.mark.parametrize("D", K.DS)
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_grid_parity_and_bits(B, h, dtype, D, F):
    Q = Packed(K.batch(D), "diagonal", dtype)
    g = _run(B, h, Q, F)
    assert h.last_route() == "kfold_ragged_kernel"
    _canaries(Q, F, g)
    _check_parity(Q, F, g)
    _check_bits_against_batched(B, h, Q, F, g)


# ---- ... and every layout and noise kind, D and F walking through their values -----------------------------------------------------
@pytest.mark.parametrize("noise", K.NOISES)
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_layouts_and_noise_kinds(B, h, dtype, layout, noise):
    k = 3 * LAYOUTS.index(layout) + K.NOISES.index(noise) + (4 if dtype == np.float32 else 0)
    D, F = K.DS[(k + k // 3) % 3], K.FS[k % 5]
    Q = Packed(K.batch(D), noise, dtype)
    g = _run(B, h, Q, F, layout=layout)
    _canaries(Q, F, g)
    _check_parity(Q, F, g)
    _check_bits_against_batched(B, h, Q, F, g)
    if layout != "col":  # the layout changes how X is fetched, nothing of what is computed
        assert all(_same(a, b) for a, b in zip(g, _run(B, h, Q, F)))


# ---- 3. invariance: the call against itself ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_bits_do_not_depend_on_the_batch_the_plan_the_memspace_or_the_outputs(B, h, dtype):
    D, F = 64, 21
    P = K.batch(D)
    Q = Packed(P, "diagonal", dtype)
    h.set_option("MAX_CHUNK", None)
    h.set_option("RAGGED_ITEM", None)
    ref = _run(B, h, Q, F)
    fo = Q.fold_offsets(F)
    assert not ref[4].any() and h.get_stat("last_chunks") == 1
    assert all(_same(a, b) for a, b in zip(ref, _run(B, h, Q, F)))            # a second call
    perm = [8, 0, 10, 3, 9, 5, 1, 7, 2, 6, 4]                                 # a permutation of the batch
    Qp = Packed(P, "diagonal", dtype, regs=perm)
    gp = _run(B, h, Qp, F)
    fop = Qp.fold_offsets(F)
    for i, b in enumerate(perm):
        assert _same(gp[0][Qp.sl(i)], ref[0][Q.sl(b)]) and _same(gp[1][Qp.sl(i)], ref[1][Q.sl(b)]), b
        assert _same(gp[2][fop[i]:fop[i + 1]], ref[2][fo[b]:fo[b + 1]]) and _same(gp[3][i], ref[3][b]), b
    for b in (1, 7, 10):                                                      # B = 1 on a slice
        Q1 = Packed(P, "diagonal", dtype, regs=[b])
        g1 = _run(B, h, Q1, F)
        assert _same(g1[0][Q1.sl(0)], ref[0][Q.sl(b)]) and _same(g1[1][Q1.sl(0)], ref[1][Q.sl(b)])
        assert _same(g1[2][:fo[b + 1] - fo[b]], ref[2][fo[b]:fo[b + 1]]) and _same(g1[3][0], ref[3][b])
    for cap, chunks in ((1, 11), (2, 6)):                                     # chunk seams
        h.set_option("MAX_CHUNK", str(cap))
        try:
            got = _run(B, h, Q, F)
            assert h.get_stat("last_chunks") == chunks
        finally:
            h.set_option("MAX_CHUNK", None)
        assert all(_same(a, o) for a, o in zip(ref, got)), cap
    for item in (64, 128):                                                    # the cut into work items
        h.set_option("RAGGED_ITEM", str(item))
        try:
            got = _run(B, h, Q, F)
        finally:
            h.set_option("RAGGED_ITEM", None)
        assert all(_same(a, o) for a, o in zip(ref, got)), item
    dev = _run(B, h, Q, F, device=True)                                       # host against device memspace
    assert all(_same(a, o) for a, o in zip(ref, dev))
    for k in range(4):                                                        # each output alone
        want = tuple(i == k for i in range(4))
        for device in (False, True):
            alone = _run(B, h, Q, F, want=want, device=device)
            assert _same(alone[k], ref[k]), k
            assert all(np.all(alone[i] == CANARY) for i in range(4) if i != k)  # the others are not touched


# ---- 4. status and degenerate folds --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_status_leaves_outputs_untouched_and_neighbours_unchanged(B, h, dtype):
    D, F = 64, 8
    Q = Packed(K.batch(D), "diagonal", dtype)
    ref = _run(B, h, Q, F)
    fo = Q.fold_offsets(F)
    bad = Packed(K.batch(D), "diagonal", dtype)
    bad.T[3][4, 4] = 0.0                        # diagonal entry 5 of the factor of regressor 3
    bad.s_diag[int(bad.off[8]) + 10] = 0.0      # variance 11 of regressor 8, counted within its slice
    g = _run(B, h, bad, F)
    assert g[4].tolist() == [0, 0, 0, 5, 0, 0, 0, 0, 11, 0, 0]
    _canaries(bad, F, g)
    for b in range(Q.nb):
        if b in (3, 8):
            assert np.all(g[0][Q.sl(b)] == CANARY) and np.all(g[1][Q.sl(b)] == CANARY)
            assert np.all(g[2][fo[b]:fo[b + 1]] == CANARY) and g[3][b] == CANARY
        else:
            assert _same(g[0][Q.sl(b)], ref[0][Q.sl(b)]) and _same(g[1][Q.sl(b)], ref[1][Q.sl(b)]), b
            assert _same(g[2][fo[b]:fo[b + 1]], ref[2][fo[b]:fo[b + 1]]) and _same(g[3][b], ref[3][b]), b
    # an empty regressor reports its state's status and an empty sum
    bad.T[9][0, 0] = -1.0
    g = _run(B, h, bad, F)
    assert g[4][9] == 1 and g[3][9] == CANARY and g[4][0] == 0 and g[3][0] == 0.0


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_a_fold_the_state_does_not_contain_is_nan_and_alone(B, h, dtype):
    D, F, k, f = 64, 8, 8, 3                    # regressor 8 (200 observations), its fold 3: observations 24 .. 31
    P = K.batch(D)
    Q = Packed(P, "diagonal", dtype)
    ref = _run(B, h, Q, F)
    fo = Q.fold_offsets(F)
    deg = Packed(P, "diagonal", dtype)
    mw0, U, X, s, y = (a.astype(dtype).astype(np.float64) for a in (P.mw[k], P.U[k], P.X[:, P.sl(k)], P.s_diag[P.sl(k)], P.y[P.sl(k)]))
    keep = np.r_[0:f * F, (f + 1) * F:P.counts[k]]
    A_ = U.T @ U + (X[:, keep] / s[keep]) @ X[:, keep].T   # the state WITHOUT the fold ...
    deg.T[k] = np.ascontiguousarray(np.linalg.cholesky((A_ + A_.T) / 2), dtype=dtype)  # (column-major T = row-major L)
    deg.mw[k] = np.linalg.solve(A_, U.T @ (U @ mw0) + X[:, keep] @ (y[keep] / s[keep])).astype(dtype)
    lo = int(deg.off[k]) + f * F
    deg.X[:, lo:lo + F] *= 10.0                             # ... and the fold's inputs inflated: its leverages exceed 1
    before = h.get_stat("kfold_degenerate")
    g = _run(B, h, deg, F)
    assert h.get_stat("kfold_degenerate") - before == 1
    assert not g[4].any()
    sk = Q.sl(k)
    inside = np.zeros(P.counts[k], dtype=bool)
    inside[f * F:(f + 1) * F] = True
    assert np.isnan(g[0][sk][inside]).all() and np.isnan(g[1][sk][inside]).all() and np.isnan(g[2][fo[k] + f]) and np.isnan(g[3][k])
    assert np.isfinite(g[0][sk][~inside]).all() and np.isfinite(g[1][sk][~inside]).all()
    assert np.isfinite(np.delete(g[2][fo[k]:fo[k + 1]], f)).all()
    for b in range(Q.nb):                                   # nothing else changed, bit for bit
        if b != k:
            assert _same(g[0][Q.sl(b)], ref[0][Q.sl(b)]) and _same(g[1][Q.sl(b)], ref[1][Q.sl(b)]), b
            assert _same(g[2][fo[b]:fo[b + 1]], ref[2][fo[b]:fo[b + 1]]) and _same(g[3][b], ref[3][b]), b
    _canaries(deg, F, g)


# ---- 5. the Python front end ----------------------------------------------------------------------------------------------------------
@pytest.fixture
def same_posterior_code(B):
    """The states of blr_posterior_ragged_* are bit for bit those of blr_posterior_batched_* on a handle with NO_I8_GRAM = 1 and
    NO_WAVE_KERNEL = 1 (include/blr_mi355x.h, blr_posterior_ragged_*): the front ends' handle for the length of a test."""
    hd = B._abi.default_handle()
    hd.set_option("NO_I8_GRAM", "1")
    hd.set_option("NO_WAVE_KERNEL", "1")
    yield hd
    hd.set_option("NO_I8_GRAM", None)
    hd.set_option("NO_WAVE_KERNEL", None)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_kfold_ragged_equals_the_list_of_kfold_calls(B, same_posterior_code, dtype):
    D, F = 64, 21
    P = K.Batch(D, K.COUNTS, seed=K.SEEDS[D], lead=0)
    X = np.asfortranarray(P.X.astype(dtype))
    y, s = np.ascontiguousarray(P.y, dtype=dtype), np.ascontiguousarray(P.s_diag, dtype=dtype)
    fs = [B.BayesianLinearRegressor(P.mw[b].astype(dtype), B.PDMat(np.asfortranarray(P.U[b].astype(dtype)))) for b in range(P.nb)]
    py = B.kfold_ragged(fs, B.ColVecs(X), P.off, B.Diagonal(s), y, F)
    assert len(py) == P.nb and all(isinstance(r, B.KFold) for r in py)
    for b in range(P.nb):
        n = P.counts[b]
        assert py[b].mean.shape == (n,) and py[b].var.shape == (n,) and py[b].logpdf.shape == (-(-n // F),) and py[b].logpdf.dtype == np.float64
        if n == 0:
            assert py[b].total == 0.0
            continue
        one = B.kfold(fs[b](B.ColVecs(np.asfortranarray(X[:, P.sl(b)])), B.Diagonal(s[P.sl(b)])), y[P.sl(b)], F)
        assert _same(py[b].mean, one.mean) and _same(py[b].var, one.var) and _same(py[b].logpdf, one.logpdf) and py[b].total == one.total
    with pytest.raises(ValueError):
        B.kfold_ragged(fs, B.ColVecs(X), P.off, B.Diagonal(s), y, 65)
    # a prior that is not positive definite: the exception carries the regressor's position
    dense = [B.BayesianLinearRegressor(P.mw[b].astype(dtype), np.asfortranarray((P.U[b].T @ P.U[b]).astype(dtype))) for b in range(P.nb)]
    dense[6] = B.BayesianLinearRegressor(P.mw[6].astype(dtype), np.asfortranarray(-np.eye(D, dtype=dtype)))
    with pytest.raises(B.PosDefException) as e:
        B.kfold_ragged(dense, B.ColVecs(X), P.off, B.Diagonal(s), y, F)
    assert e.value.index == 6


# ---- 6. D > 128: one regressor after the other through blr_kfold_batched_* ----------------------------------------------------------
def test_large_d_route_parity(B, h):
    Q = Packed(K.batch(K.LARGE_D, counts=K.LARGE_COUNTS), "diagonal", np.float64)
    F = K.LARGE_F
    g = _run(B, h, Q, F)
    _canaries(Q, F, g)
    fo = Q.fold_offsets(F)
    assert not g[4].any() and g[3][0] == 0.0
    for i in (1, 2):
        m_o, v_o, lp_o, _ = closed_form(*Q.slice64(i), F)
        np.testing.assert_allclose(g[0][Q.sl(i)], m_o, rtol=1e-8, atol=1e-10)
        np.testing.assert_allclose(g[1][Q.sl(i)], v_o, rtol=1e-8)
        np.testing.assert_allclose(g[2][fo[i]:fo[i + 1]], lp_o, rtol=1e-8)
        assert g[3][i] == pytest.approx(math.fsum(g[2][fo[i]:fo[i + 1]]), rel=1e-12)
