"""Ragged marginals and leave-one-out (blr_marginals_ragged_*, blr_loo_ragged_*, mean_ragged / var_ragged / mean_and_var_ragged /
loo_ragged) against the float64 oracle, against the equal-count entry points, and against themselves bit for bit
(B = 1 on a slice, permutation, neighbours, chunking, item size, memspace, repetition).  All tests need an MI355X.

Tolerances are the project's: marginals rtol = atol = 1e-10 (fp64) / 2e-4 (fp32); LOO the bounds tests/test_loo_gpu.py applies to
blr_loo_batched_*: rtol = atol = 1e-9 on mean and logpdf, rtol = 1e-9 on var (fp64); 1e-3 (fp32)."""
import math

import numpy as np
import pytest

from oracle import blr_oracle as O

pytestmark = pytest.mark.gpu

LOG2PI = math.log(2.0 * math.pi)
COUNTS = [0, 1, 15, 16, 17, 63, 64, 65, 200, 0, 333]
LEAD = 5  # offsets[0]: leading observations of the packed arrays that belong to nobody
CANARY = 7.0
LAYOUTS = ["col", "col_unaligned", "row"]
NOISES = ["one", "per_regressor", "diagonal"]


@pytest.fixture(scope="module")
def B():
    import blr_amd

    blr_amd._abi.default_handle()  # raises if the extension or the GPU is missing: no silent fallback
    return blr_amd


def _tol(dtype, loo):
    if loo:
        return (1e-9, 1e-9) if dtype == np.float64 else (1e-3, 1e-3)
    return (1e-10, 1e-10) if dtype == np.float64 else (2e-4, 2e-4)


class Batch:
    """Packed data of len(counts) regressors (float64 masters, cast on use): inputs scaled as tests/test_loo_gpu.py::_state draws
    them (no degenerate leverage), a well-conditioned factor prior per regressor, and the posterior states for the LOO."""

    def __init__(self, D, counts, seed=0, lead=LEAD):
        rng = np.random.Generator(np.random.PCG64(4242 + seed))
        self.D, self.counts = D, list(counts)
        self.off = np.concatenate([[lead], lead + np.cumsum(counts)]).astype(np.int64)
        nb, tot = len(counts), int(self.off[-1])
        self.nb, self.tot = nb, tot
        self.X = rng.standard_normal((D, tot)) * (0.7 / np.sqrt(D))
        self.y = rng.standard_normal(tot)
        self.s_diag = np.exp(0.3 * rng.standard_normal(tot))
        self.s_reg = np.exp(0.3 * rng.standard_normal(nb))
        self.mw = rng.standard_normal((nb, D))
        U = np.triu(rng.standard_normal((nb, D, D))) * (0.3 / np.sqrt(D))
        for b in range(nb):
            U[b][np.diag_indices(D)] = 1.0 + np.abs(U[b][np.diag_indices(D)])
        self.U = U

    def sl(self, b):
        return slice(int(self.off[b]), int(self.off[b + 1]))

    def noise(self, kind, b):
        """per-observation noise variances of regressor b under noise `kind`"""
        n = self.counts[b]
        if kind == "one":
            return np.full(n, self.s_reg[0])
        if kind == "per_regressor":
            return np.full(n, self.s_reg[b])
        return self.s_diag[self.sl(b)]

    def noise_args(self, B, kind, dtype):
        if kind == "one":
            return B._abi.NOISE_ISOTROPIC, np.ascontiguousarray(self.s_reg[:1], dtype=dtype), 0
        if kind == "per_regressor":
            return B._abi.NOISE_ISOTROPIC, np.ascontiguousarray(self.s_reg, dtype=dtype), 1
        return B._abi.NOISE_DIAGONAL, np.ascontiguousarray(self.s_diag, dtype=dtype), 0

    def x_args(self, B, layout, dtype):
        """-> (layout constant, X view handed to the library, ldx, the buffer that owns it).  The padding between the columns
        (ColVecs: rows D .. ldx - 1; RowVecs: rows tot .. ldx - 1) holds NaN: a lane that read it would poison its output."""
        D, tot = self.D, self.tot
        vec = 16 // np.dtype(dtype).itemsize
        if layout == "row":
            ldx = tot + 3
            buf = np.full(ldx * D + 1, np.nan, dtype=dtype)
            M = buf[:ldx * D].reshape((ldx, D), order="F")
            M[:tot, :] = self.X.T
            return B._abi.LAYOUT_ROWVECS, M, ldx, buf
        ldx = D + vec if D % vec == 0 else D + 3
        raw = np.full(ldx * tot + 2 * vec, np.nan, dtype=dtype)
        start = (-raw.ctypes.data // raw.itemsize) % vec  # element index of a 16-byte aligned address
        if layout == "col_unaligned":
            start += 1
        M = raw[start:start + ldx * tot].reshape((ldx, tot), order="F")
        M[:D, :] = self.X
        assert (M.ctypes.data % 16 == 0) == (layout == "col")
        return B._abi.LAYOUT_COLVECS, M, ldx, raw

    def states(self, noise, dtype):
        """posterior states (mw', T) of every regressor in float64 from the data as cast to dtype, then cast"""
        D = self.D
        mws, Ts = np.empty((self.nb, D)), np.empty((self.nb, D, D))
        for b in range(self.nb):
            X = self.X[:, self.sl(b)].astype(dtype).astype(np.float64)
            y = self.y[self.sl(b)].astype(dtype).astype(np.float64)
            s = self.noise(noise, b).astype(dtype).astype(np.float64)
            U = self.U[b].astype(dtype).astype(np.float64)
            mw = self.mw[b].astype(dtype).astype(np.float64)
            A = U.T @ U + (X / s) @ X.T
            Ts[b] = np.linalg.cholesky((A + A.T) / 2).T
            mws[b] = np.linalg.solve(A, U.T @ (U @ mw) + X @ (y / s))
        return np.ascontiguousarray(mws, dtype=dtype), np.ascontiguousarray(Ts.transpose(0, 2, 1), dtype=dtype)  # T column-major


def _loo_closed_form(X, y, s, mw, T):
    """the header's closed form in float64 / longdouble"""
    Z = np.linalg.solve(T.T, X)
    sig2 = np.sum(Z * Z, axis=0).astype(np.longdouble)
    m = (X.T @ mw).astype(np.longdouble)
    s, y = s.astype(np.longdouble), y.astype(np.longdouble)
    omh = (s - sig2) / s
    r = y - m
    return ((y - r / omh).astype(np.float64), (s / omh).astype(np.float64),
            (-0.5 * (LOG2PI + np.log(s) - np.log(omh) + r * r / (s * omh))).astype(np.float64))


def _dense(P, b, dtype):
    """the dense prior precision of regressor b: U'U of the factor as cast to dtype (float64)"""
    U = P.U[b].astype(dtype).astype(np.float64)
    return U.T @ U.copy()


def _marg(B, P, dtype, layout, noise, prior="factor", want=("mean", "var"), h=None, off=None, regs=None, xa=None, device=False):
    """blr_marginals_ragged_* on batch P -> (mean, var, info), canaries where nothing was to be written.  regs: the regressors of
    the call (default all); off: their offsets (default P's)."""
    h = h or B._abi.default_handle()
    regs = list(range(P.nb)) if regs is None else regs
    off = P.off[[regs[0] + i for i in range(len(regs) + 1)]] if off is None else off
    lay, X, ldx, _own = xa or P.x_args(B, layout, dtype)
    nk, s, strides = P.noise_args(B, noise, dtype)
    if noise == "per_regressor":
        s = s[regs[0]:]
    D = P.D
    if prior == "diagonal":
        pk, Lw, ldl, sl = B._abi.PRIOR_DIAGONAL, np.ascontiguousarray([np.diag(P.U[b]) ** 2 for b in regs], dtype=dtype), 1, D
    elif prior == "dense":
        pk, ldl, sl = B._abi.PRIOR_DENSE, D, D * D
        Lw = np.ascontiguousarray([_dense(P, b, dtype) for b in regs], dtype=dtype)
    else:
        pk, ldl, sl = B._abi.PRIOR_UPPER_FACTOR, D, D * D
        Lw = np.ascontiguousarray([P.U[b].T for b in regs], dtype=dtype)  # (row-major of U' = column-major of U)
    if getattr(P, "Lw_override", None) is not None and prior == "dense":
        Lw = np.ascontiguousarray(P.Lw_override[regs], dtype=dtype)
    mw = np.ascontiguousarray(P.mw[regs], dtype=dtype)
    mean = np.full(P.tot + 4, CANARY, dtype=dtype) if "mean" in want else None
    var = np.full(P.tot + 4, CANARY, dtype=dtype) if "var" in want else None
    info = np.full(len(regs), -9, dtype=np.int32)
    wv = "var" in want
    if not device:
        h.marginals_ragged(dtype, B._abi.MEM_HOST, lay, len(regs), D, off, X, ldx, nk, s if wv else None, strides, pk, mw, D,
                           Lw if wv else None, ldl, sl, mean, var, info)
    else:
        from blr_amd.regressor import _DeviceBuffer as DB
        bufs = {k: DB.of(h, a) for k, a in dict(X=_own, s=s, mw=mw, Lw=Lw, mean=mean, var=var, info=info).items() if a is not None}
        xptr = bufs["X"].ptr + (X.ctypes.data - _own.ctypes.data)
        try:
            h.marginals_ragged(dtype, B._abi.MEM_DEVICE, lay, len(regs), D, off, xptr, ldx, nk, bufs["s"].ptr if wv else None, strides, pk,
                               bufs["mw"].ptr, D, bufs["Lw"].ptr if wv else None, ldl, sl, bufs["mean"].ptr if mean is not None else None,
                               bufs["var"].ptr if wv else None, bufs["info"].ptr)
            for k, a in (("mean", mean), ("var", var), ("info", info)):
                if a is not None:
                    h.memcpy_d2h(a, bufs[k].ptr)
        finally:
            for b in bufs.values():
                b.free()
    return mean, var, info


def _loo(B, P, dtype, layout, noise, state, want=("lm", "lv", "ll", "tot"), h=None, regs=None, xa=None, device=False, y=None):
    """blr_loo_ragged_* on batch P with the states `state` -> (loo_mean, loo_var, loo_logpdf, loo_total, info)"""
    h = h or B._abi.default_handle()
    regs = list(range(P.nb)) if regs is None else regs
    off = P.off[[regs[0] + i for i in range(len(regs) + 1)]]
    lay, X, ldx, _own = xa or P.x_args(B, layout, dtype)
    nk, s, strides = P.noise_args(B, noise, dtype)
    if getattr(P, "s_override", None) is not None and noise == "diagonal":
        s = np.ascontiguousarray(P.s_override, dtype=dtype)
    if noise == "per_regressor":
        s = s[regs[0]:]
    D = P.D
    mw, T = np.ascontiguousarray(state[0][regs]), np.ascontiguousarray(state[1][regs])
    yv = np.ascontiguousarray(P.y if y is None else y, dtype=dtype)
    lm = np.full(P.tot + 4, CANARY, dtype=dtype) if "lm" in want else None
    lv = np.full(P.tot + 4, CANARY, dtype=dtype) if "lv" in want else None
    ll = np.full(P.tot + 4, CANARY, dtype=np.float64) if "ll" in want else None
    tot = np.full(len(regs), CANARY, dtype=np.float64) if "tot" in want else None
    info = np.full(len(regs), -9, dtype=np.int32)
    if not device:
        h.loo_ragged(dtype, B._abi.MEM_HOST, lay, len(regs), D, off, X, ldx, yv, nk, s, strides, mw, D, T, D, D * D, lm, lv, ll, tot, info)
    else:
        from blr_amd.regressor import _DeviceBuffer as DB
        bufs = {k: DB.of(h, a) for k, a in dict(X=_own, y=yv, s=s, mw=mw, T=T, lm=lm, lv=lv, ll=ll, tot=tot, info=info).items() if a is not None}
        xptr = bufs["X"].ptr + (X.ctypes.data - _own.ctypes.data)
        g = lambda k: bufs[k].ptr if k in bufs else None  # noqa: E731
        try:
            h.loo_ragged(dtype, B._abi.MEM_DEVICE, lay, len(regs), D, off, xptr, ldx, g("y"), nk, g("s"), strides, g("mw"), D, g("T"), D, D * D,
                         g("lm"), g("lv"), g("ll"), g("tot"), g("info"))
            for k, a in (("lm", lm), ("lv", lv), ("ll", ll), ("tot", tot), ("info", info)):
                if a is not None:
                    h.memcpy_d2h(a, bufs[k].ptr)
        finally:
            for b in bufs.values():
                b.free()
    return lm, lv, ll, tot, info


def _check_canaries(P, arrays):
    """nothing outside [offsets[0], offsets[B]) was written: the five leading slots and the tail"""
    for a in arrays:
        if a is not None and a.shape[0] > P.nb:
            assert np.all(a[:LEAD] == CANARY) and np.all(a[P.tot:] == CANARY)


_BATCHES = {}


def _batch(D, seed=0, counts=None):
    key = (D, seed, tuple(counts or COUNTS))
    if key not in _BATCHES:
        _BATCHES[key] = Batch(D, counts or COUNTS, seed)
    return _BATCHES[key]


def _marg_reference(P, dtype, noise, prior):
    mean, var = np.zeros(P.tot), np.zeros(P.tot)
    for b in range(P.nb):
        U = P.U[b].astype(dtype).astype(np.float64)
        if prior == "diagonal":
            U = np.diag(np.sqrt((np.diag(P.U[b]) ** 2).astype(dtype).astype(np.float64)))
        elif prior == "dense":
            U = np.linalg.cholesky(_dense(P, b, dtype).astype(dtype).astype(np.float64)).T
        X = P.X[:, P.sl(b)].astype(dtype).astype(np.float64)
        if X.shape[1]:
            mean[P.sl(b)], var[P.sl(b)] = O.marginals_direct(P.mw[b].astype(dtype).astype(np.float64), U, X,
                                                             P.noise(noise, b).astype(dtype).astype(np.float64))
    return mean, var


# ---- the lattice ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("D", [128, 96, 17, 1, 160])
def test_marginals_lattice(B, D, dtype, layout):
    P = _batch(D)
    rtol, atol = _tol(dtype, False)
    xa = P.x_args(B, layout, dtype)
    x_before = xa[3].copy()
    for noise in NOISES:
        for prior in ("factor", "dense", "diagonal"):
            m_o, v_o = _marg_reference(P, dtype, noise, prior)
            both = _marg(B, P, dtype, layout, noise, prior, xa=xa)
            _check_canaries(P, both[:2])
            assert not np.any(both[2])
            live = slice(LEAD, P.tot)
            np.testing.assert_allclose(both[0][live], m_o[live], rtol=rtol, atol=atol)
            np.testing.assert_allclose(both[1][live], v_o[live], rtol=rtol, atol=atol)
            if noise == "diagonal":  # each output alone: the same bits as together
                only_m = _marg(B, P, dtype, layout, noise, prior, want=("mean",), xa=xa)
                only_v = _marg(B, P, dtype, layout, noise, prior, want=("var",), xa=xa)
                assert only_m[1] is None and only_v[0] is None
                if D <= 128:
                    assert np.array_equal(only_m[0], both[0]) and np.array_equal(only_v[1], both[1])
                else:
                    np.testing.assert_allclose(only_m[0][live], m_o[live], rtol=rtol, atol=atol)
                    np.testing.assert_allclose(only_v[1][live], v_o[live], rtol=rtol, atol=atol)
    assert np.array_equal(xa[3], x_before, equal_nan=True)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("D", [128, 96, 17, 1, 160])
def test_loo_lattice(B, D, dtype, layout):
    P = _batch(D)
    rtol, atol = _tol(dtype, True)
    xa = P.x_args(B, layout, dtype)
    live = slice(LEAD, P.tot)
    for noise in NOISES:
        st = P.states(noise, dtype)
        ref = [np.zeros(P.tot) for _ in range(3)]
        for b in range(P.nb):
            if P.counts[b]:
                r = _loo_closed_form(P.X[:, P.sl(b)].astype(dtype).astype(np.float64), P.y[P.sl(b)].astype(dtype).astype(np.float64),
                                     P.noise(noise, b).astype(dtype).astype(np.float64), st[0][b].astype(np.float64),
                                     st[1][b].astype(np.float64).T)
                for k in range(3):
                    ref[k][P.sl(b)] = r[k]
        lm, lv, ll, tot, info = _loo(B, P, dtype, layout, noise, st, xa=xa)
        _check_canaries(P, (lm, lv, ll))
        assert not np.any(info)
        np.testing.assert_allclose(lm[live], ref[0][live], rtol=rtol, atol=atol)
        np.testing.assert_allclose(lv[live], ref[1][live], rtol=rtol)
        np.testing.assert_allclose(ll[live], ref[2][live], rtol=rtol, atol=atol)
        for b in range(P.nb):
            assert tot[b] == pytest.approx(math.fsum(ll[P.sl(b)]), rel=1e-12, abs=1e-12)
            if P.counts[b] == 0:
                assert tot[b] == 0.0
        if noise == "diagonal":  # each output alone, and the total without the log densities (workspace): the same bits
            for k, name in enumerate(("lm", "lv", "ll", "tot")):
                alone = _loo(B, P, dtype, layout, noise, st, want=(name,), xa=xa)
                assert all(alone[j] is None for j in range(4) if j != k)
                if D <= 128:
                    assert np.array_equal(alone[k], (lm, lv, ll, tot)[k])
                else:
                    np.testing.assert_allclose(alone[k][live if k < 3 else slice(None)], (lm, lv, ll, tot)[k][live if k < 3 else slice(None)],
                                               rtol=rtol, atol=atol)


# ---- bits ----------------------------------------------------------------------------------------------------------------------
def _both(B, P, dtype, layout, **kw):
    """marginals (dense prior: the factorisation is part of the promise) and LOO of the whole batch under diagonal noise"""
    st = P.states("diagonal", dtype)
    return _marg(B, P, dtype, layout, "diagonal", "dense", **kw), _loo(B, P, dtype, layout, "diagonal", st, **kw)


def _same(P, got, ref, regs=None, ref_P=None, ref_regs=None):
    """the per-observation outputs and totals of regressors `regs` of `got` equal those of `ref_regs` of `ref`, bit for bit"""
    ref_P = ref_P or P
    regs = range(P.nb) if regs is None else regs
    ref_regs = regs if ref_regs is None else ref_regs
    for (mg, lg), (mr, lr) in [(got, ref)]:
        for b, c in zip(regs, ref_regs):
            for g, r in list(zip(mg[:2], mr[:2])) + list(zip(lg[:3], lr[:3])):
                assert np.array_equal(g[P.sl(b)], r[ref_P.sl(c)]), (b, c)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("D", [128, 17])
def test_bits(B, D, dtype, layout):
    P = _batch(D)
    A = B._abi
    ref = _both(B, P, dtype, layout)
    xa = P.x_args(B, layout, dtype)
    st = P.states("diagonal", dtype)
    # two successive calls on one handle
    again = _both(B, P, dtype, layout)
    _same(P, again, ref)
    assert np.array_equal(again[1][3], ref[1][3])
    # each regressor against a B = 1 call on its slice
    for b in range(P.nb):
        one = (_marg(B, P, dtype, layout, "diagonal", "dense", regs=[b], xa=xa), _loo(B, P, dtype, layout, "diagonal", st, regs=[b], xa=xa))
        _same(P, one, ref, regs=[b])
        assert one[1][3][0] == ref[1][3][b]
    # host against device memspace
    dev = _both(B, P, dtype, layout, device=True)
    _same(P, dev, ref)
    assert np.array_equal(dev[1][3], ref[1][3]) and np.array_equal(dev[1][4], ref[1][4])
    # MAX_CHUNK = 3 and RAGGED_ITEM = 64 (the regressors of 200 and 333 observations then cross item seams)
    for key, val, chunks in (("MAX_CHUNK", 3, 4), ("RAGGED_ITEM", 64, 1)):
        h = A.Handle()
        try:
            h.set_option(key, val)
            got = _both(B, P, dtype, layout, h=h)
            assert h.get_stat("last_chunks") == chunks
        finally:
            h.close()
        _same(P, got, ref)
        assert np.array_equal(got[1][3], ref[1][3])


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("D", [128, 17])
def test_bits_permutation_and_neighbours(B, D, dtype):
    P = _batch(D)
    layout = "col"
    ref = _both(B, P, dtype, layout)
    perm = np.random.Generator(np.random.PCG64(5)).permutation(P.nb)
    Q = Batch(D, [P.counts[i] for i in perm], seed=99)
    for j, i in enumerate(perm):  # regressor j of Q is regressor i of P
        for name in ("X",):
            Q.X[:, Q.sl(j)] = P.X[:, P.sl(i)]
        Q.y[Q.sl(j)], Q.s_diag[Q.sl(j)] = P.y[P.sl(i)], P.s_diag[P.sl(i)]
        Q.mw[j], Q.U[j] = P.mw[i], P.U[i]
    got = _both(B, Q, dtype, layout)
    _same(Q, got, ref, regs=range(Q.nb), ref_P=P, ref_regs=list(perm))
    assert np.array_equal(got[1][3], ref[1][3][perm])
    # a neighbour's data replaced: the others keep their bits
    k = 6
    R2 = Batch(D, P.counts, seed=0)
    R2.X[:, R2.sl(k)] *= 1.5
    R2.y[R2.sl(k)] += 1.0
    # (the states of the other regressors are those of P: computed per regressor from its own slice)
    got = _both(B, R2, dtype, layout)
    others = [b for b in range(P.nb) if b != k]
    _same(R2, got, ref, regs=others, ref_P=P, ref_regs=others)
    assert not np.array_equal(got[0][1][P.sl(k)], ref[0][1][P.sl(k)])


# ---- against the equal-count entry points -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("D", [128, 17])
def test_equal_counts_agree_with_batched_entry_points(B, D, dtype):
    A = B._abi
    nb, N = 5, 80
    P = Batch(D, [N] * nb, seed=3, lead=0)
    h = A.default_handle()
    X = np.asfortranarray(P.X.astype(dtype))
    s = np.ascontiguousarray(P.s_diag, dtype=dtype)
    mw = np.ascontiguousarray(P.mw, dtype=dtype)
    U = np.ascontiguousarray([P.U[b].T for b in range(nb)], dtype=dtype)
    mean, var, info = np.zeros((nb, N), dtype=dtype), np.zeros((nb, N), dtype=dtype), np.zeros(nb, dtype=np.int32)
    h.marginals_batched(dtype, A.MEM_HOST, A.LAYOUT_COLVECS, nb, D, N, X, D, D * N, A.NOISE_DIAGONAL, s, N, A.PRIOR_UPPER_FACTOR, mw, D, U, D,
                        D * D, mean, N, var, N, info)
    xa = (A.LAYOUT_COLVECS, X, D, X)
    gm, gv, gi = _marg(B, P, dtype, "col", "diagonal", "factor", xa=xa)
    rtol, atol = _tol(dtype, False)
    np.testing.assert_allclose(gm[:P.tot], mean.ravel(), rtol=rtol, atol=atol)
    np.testing.assert_allclose(gv[:P.tot], var.ravel(), rtol=rtol, atol=atol)
    st = P.states("diagonal", dtype)
    y = np.ascontiguousarray(P.y, dtype=dtype)
    lm, lv, ll = np.zeros((nb, N), dtype=dtype), np.zeros((nb, N), dtype=dtype), np.zeros((nb, N))
    tot = np.zeros(nb)
    h.loo(dtype, A.MEM_HOST, A.LAYOUT_COLVECS, nb, D, N, X, D, D * N, y, N, A.NOISE_DIAGONAL, s, N, st[0], D, st[1], D, D * D, lm, N, lv, N,
          ll, N, tot, info)
    g = _loo(B, P, dtype, "col", "diagonal", st, xa=xa)
    rtol, atol = _tol(dtype, True)
    np.testing.assert_allclose(g[0][:P.tot], lm.ravel(), rtol=rtol, atol=atol)
    np.testing.assert_allclose(g[1][:P.tot], lv.ravel(), rtol=rtol)
    np.testing.assert_allclose(g[2][:P.tot], ll.ravel(), rtol=rtol, atol=atol)
    np.testing.assert_allclose(g[3], tot, rtol=rtol, atol=atol)


# ---- end to end -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("D", [128, 17])
def test_end_to_end_from_posterior_ragged(B, D, dtype):
    A = B._abi
    P = Batch(D, COUNTS, seed=7, lead=0)
    h = A.default_handle()
    X = np.asfortranarray(P.X.astype(dtype))
    y, s = np.ascontiguousarray(P.y, dtype=dtype), np.ascontiguousarray(P.s_diag, dtype=dtype)
    mw = np.ascontiguousarray(P.mw, dtype=dtype)
    U = np.ascontiguousarray([P.U[b].T for b in range(P.nb)], dtype=dtype)
    mwp, Tp = np.zeros((P.nb, D), dtype=dtype), np.zeros((P.nb, D * D), dtype=dtype)
    info = np.zeros(P.nb, dtype=np.int32)
    h.posterior_ragged(dtype, A.MEM_HOST, A.LAYOUT_COLVECS, P.nb, D, P.off, X, D, y, A.NOISE_DIAGONAL, s, 0, A.PRIOR_UPPER_FACTOR, mw, D, U, D,
                       D * D, mwp, D, Tp, D, D * D, None, D, D * D, None, info)
    assert not np.any(info)
    g = _loo(B, P, dtype, "col", "diagonal", (mwp, Tp.reshape(P.nb, D, D)), xa=(A.LAYOUT_COLVECS, X, D, X))
    rtol, atol = _tol(dtype, True)
    st = P.states("diagonal", dtype)
    fs = [B.BayesianLinearRegressor(mw[b], B.PDMat(np.asfortranarray(P.U[b].astype(dtype)))) for b in range(P.nb)]
    py = B.loo_ragged(fs, B.ColVecs(X), P.off, B.Diagonal(s), y)
    for b in range(P.nb):
        if not P.counts[b]:
            continue
        r = _loo_closed_form(X[:, P.sl(b)].astype(np.float64), y[P.sl(b)].astype(np.float64), s[P.sl(b)].astype(np.float64),
                             st[0][b].astype(np.float64), st[1][b].astype(np.float64).T)
        np.testing.assert_allclose(g[0][P.sl(b)], r[0], rtol=rtol, atol=atol)
        np.testing.assert_allclose(g[1][P.sl(b)], r[1], rtol=rtol)
        np.testing.assert_allclose(g[2][P.sl(b)], r[2], rtol=rtol, atol=atol)
        one = B.loo(fs[b](B.ColVecs(np.asfortranarray(X[:, P.sl(b)])), B.Diagonal(s[P.sl(b)])), y[P.sl(b)])
        np.testing.assert_allclose(py[b].mean, one.mean, rtol=rtol, atol=atol)
        np.testing.assert_allclose(py[b].var, one.var, rtol=rtol)
        np.testing.assert_allclose(py[b].logpdf, one.logpdf, rtol=rtol, atol=atol)
        assert py[b].total == pytest.approx(one.total, rel=rtol, abs=atol * P.counts[b])
    # the marginal front end on the same packed data
    m, v = B.mean_and_var_ragged(fs, B.ColVecs(X), P.off, B.Diagonal(s))
    m_o, v_o = _marg_reference(P, dtype, "diagonal", "factor")
    rtol, atol = _tol(dtype, False)
    np.testing.assert_allclose(m, m_o, rtol=rtol, atol=atol)
    np.testing.assert_allclose(v, v_o, rtol=rtol, atol=atol)
    assert np.array_equal(B.mean_ragged(fs, B.ColVecs(X), P.off), m) and np.array_equal(B.var_ragged(fs, B.ColVecs(X), P.off, B.Diagonal(s)), v)


# ---- status and the NaN rule ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [128, 17])
def test_status_leaves_outputs_untouched(B, D):
    dtype, layout = np.float64, "col"
    P = _batch(D)
    ref = _both(B, P, dtype, layout)
    st = P.states("diagonal", dtype)
    k = 8  # 200 observations
    others = [b for b in range(P.nb) if b != k]
    # a dense prior that is not positive definite
    Q = Batch(D, COUNTS, seed=0)
    Q.Lw_override = np.array([_dense(P, b, dtype) for b in range(P.nb)])
    Q.Lw_override[k][D - 1, D - 1] = -1.0
    m, v, info = _marg(B, Q, dtype, layout, "diagonal", "dense")
    assert info[k] > 0 and not np.any(info[others])
    assert np.all(m[P.sl(k)] == CANARY) and np.all(v[P.sl(k)] == CANARY)
    for b in others:
        assert np.array_equal(m[P.sl(b)], ref[0][0][P.sl(b)]) and np.array_equal(v[P.sl(b)], ref[0][1][P.sl(b)])
    # a state whose T has a zero diagonal entry
    T2 = st[1].copy()
    j = min(3, D - 1)
    T2[k][j, j] = 0.0
    g = _loo(B, P, dtype, layout, "diagonal", (st[0], T2))
    assert g[4][k] == j + 1 and not np.any(g[4][others]) and g[3][k] == CANARY
    assert all(np.all(a[P.sl(k)] == CANARY) for a in g[:3])
    for b in others:
        assert all(np.array_equal(a[P.sl(b)], r[P.sl(b)]) for a, r in zip(g[:3], ref[1][:3])) and g[3][b] == ref[1][3][b]
    # a diagonal s that is non-positive inside one regressor's slice: the index is slice-relative
    Q = Batch(D, COUNTS, seed=0)
    Q.s_override = P.s_diag.copy()
    Q.s_override[int(P.off[k]) + 41] = 0.0
    g = _loo(B, Q, dtype, layout, "diagonal", st)
    assert g[4][k] == 42 and not np.any(g[4][others]) and g[3][k] == CANARY
    assert all(np.all(a[P.sl(k)] == CANARY) for a in g[:3])
    for b in others:
        assert all(np.array_equal(a[P.sl(b)], r[P.sl(b)]) for a, r in zip(g[:3], ref[1][:3]))


@pytest.mark.parametrize("D", [128, 16])
def test_degenerate_leverage_gives_nan_and_counts(B, D):
    dtype, layout = np.float64, "col"
    Q = Batch(D, [40, 70, 33], seed=11)
    Q.s_reg[:] = 1.0
    P1 = Batch(D, [40, 70, 33], seed=11)
    P1.s_reg[:] = 1.0
    st1 = P1.states("one", dtype)
    ref = _loo(B, P1, dtype, layout, "one", st1)
    k = 1
    Q.X[:, Q.sl(k)] = 0.0
    Q.X[0, Q.sl(k)] = 2.0  # squared norm 4, T = I, s = 1: 1 - h_n = -3
    T2 = st1[1].copy()
    T2[k] = np.eye(D)
    h = B._abi.default_handle()
    before = h.get_stat("loo_degenerate")
    g = _loo(B, Q, dtype, layout, "one", (st1[0], T2))
    assert h.get_stat("loo_degenerate") - before == 70
    assert not np.any(g[4]) and np.isnan(g[3][k])
    assert all(np.all(np.isnan(a[Q.sl(k)])) for a in g[:3])
    for b in (0, 2):
        assert all(np.array_equal(a[Q.sl(b)], r[Q.sl(b)]) for a, r in zip(g[:3], ref[:3])) and g[3][b] == ref[3][b]


# ---- a long regressor ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_large_n_in_one_regressor(B, dtype):
    D = 128
    P = _batch(D, seed=21, counts=[70000, 3])
    A = B._abi
    st = P.states("diagonal", dtype)
    m_o, v_o = _marg_reference(P, dtype, "diagonal", "factor")
    ref = [np.zeros(P.tot) for _ in range(3)]
    for b in range(P.nb):
        r = _loo_closed_form(P.X[:, P.sl(b)].astype(dtype).astype(np.float64), P.y[P.sl(b)].astype(dtype).astype(np.float64),
                             P.noise("diagonal", b).astype(dtype).astype(np.float64), st[0][b].astype(np.float64), st[1][b].astype(np.float64).T)
        for k in range(3):
            ref[k][P.sl(b)] = r[k]
    live = slice(LEAD, P.tot)
    res = []
    for item in (None, 4096):
        h = A.Handle()
        try:
            if item:
                h.set_option("RAGGED_ITEM", item)
            mg = _marg(B, P, dtype, "col", "diagonal", "factor", h=h)
            lg = _loo(B, P, dtype, "col", "diagonal", st, h=h)
        finally:
            h.close()
        res.append((mg, lg))
        rtol, atol = _tol(dtype, False)
        np.testing.assert_allclose(mg[0][live], m_o[live], rtol=rtol, atol=atol)
        np.testing.assert_allclose(mg[1][live], v_o[live], rtol=rtol, atol=atol)
        rtol, atol = _tol(dtype, True)
        np.testing.assert_allclose(lg[0][live], ref[0][live], rtol=rtol, atol=atol)
        np.testing.assert_allclose(lg[1][live], ref[1][live], rtol=rtol)
        np.testing.assert_allclose(lg[2][live], ref[2][live], rtol=rtol, atol=atol)
        _check_canaries(P, mg[:2] + lg[:3])
    for a, b in zip(res[0][0][:2] + res[0][1][:4], res[1][0][:2] + res[1][1][:4]):
        assert np.array_equal(a, b)
