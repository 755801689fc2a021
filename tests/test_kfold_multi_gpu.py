"""K-fold predictives of multi-output states (blr_kfold_multi_batched_*, kfold_columns, kfold_columns_map,
ResidentColumnsPosterior.kfold) on the GPU: brute-force refits with the CPU oracle on a toy problem, a lattice of
(D, N, F, S, layout) against the per-column closed form of tests/_kfold_multi_ref.py, the single-column and the leave-one-out
siblings, the bit promises of the header, fold and column locality, the NaN rule, the status and the Python surface.  All tests need
an MI355X."""
import functools
import math

import numpy as np
import pytest

from oracle import blr_oracle as O

from _kfold_ref import rng_of
from _kfold_multi_ref import brute_force_columns, closed_form_columns, columns_state, fp32_bounds_columns

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


@functools.lru_cache(maxsize=None)
def _problems64(nb, D, N, S, seed=0):
    out = []
    for b in range(nb):
        _, _, X, s, Y, M, T = columns_state(seed + 31 * b + D + N, D, N, S)
        out.append((X, Y, s, M, np.asfortranarray(T)))
    return tuple(np.stack([q[i] for q in out]) for i in range(5))


def _problems(nb, D, N, S, dtype=np.float64, seed=0):
    """nb multi-output states (M, T) that contain their N observations: X [nb, D, N], Y [nb, N, S], s [nb, N], M [nb, D, S],
    T [nb, D, D] of `dtype` (the state from the float64 oracle); fresh copies, the cached reference stays unchanged"""
    return [a.astype(dtype) for a in _problems64(nb, D, N, S, seed)]


def _cm(A, ld):
    """[nb, rows, cols] -> [nb, ld * cols]: column-major per regressor with leading dimension ld (the padding rows hold 77)"""
    nb, rows, cols = A.shape
    buf = np.full((nb, cols, ld), 77, dtype=A.dtype)
    buf[:, :, :rows] = A.transpose(0, 2, 1)
    return np.ascontiguousarray(buf.reshape(nb, cols * ld))


def _run(B, h, X, Y, s, M, T, F, layout="col", memspace="host", want=(True, True, True, True), fill=None, pad=0):
    """blr_kfold_multi_batched_* on stacked operands -> (mean [nb, N, S], var [nb, N], logpdf [nb, nfolds, S], total [nb, S], info);
    pad: ldY = N + pad, ldm = D + pad"""
    A, R = B._abi, B.regressor
    nb, D, N = X.shape
    S = Y.shape[2]
    dtype = X.dtype.type
    nf = -(-N // F)
    ldY, ldm = max(N, 1) + pad, D + pad
    if layout == "col":
        Xf, lay, ldx = X.transpose(0, 2, 1).reshape(nb, N * D), A.LAYOUT_COLVECS, D
    else:
        Xf, lay, ldx = X.reshape(nb, D * N), A.LAYOUT_ROWVECS, max(N, 1)
    Tf = T.transpose(0, 2, 1).reshape(nb, D * D)
    fv = np.nan if fill is None else fill
    outs = [np.full((nb, S * N), fv, dtype=dtype), np.full((nb, N), fv, dtype=dtype), np.full((nb, S * nf), fv), np.full((nb, S), fv)]
    info = np.full(nb, -7, dtype=np.int32)
    ins = [np.ascontiguousarray(a) for a in (Xf, _cm(Y, ldY), s, _cm(M, ldm), Tf)]
    strides = [a.shape[1] for a in ins]
    tail = (N, S * N, N, nf, S * nf, S)  # ld_km, stride_km, stride_kv, ld_kl, stride_kl, stride_kt
    if memspace == "host":
        o = [a if w else None for a, w in zip(outs, want)]
        h.kfold_multi_batched(dtype, A.MEM_HOST, lay, nb, D, N, S, F, ins[0], ldx, strides[0], ins[1], ldY, strides[1], A.NOISE_DIAGONAL,
                              ins[2], strides[2], ins[3], ldm, strides[3], ins[4], D, D * D, o[0], tail[0], tail[1], o[1], tail[2], o[2],
                              tail[3], tail[4], o[3], tail[5], info)
    else:
        bufs = [R._DeviceBuffer.of(h, a) for a in ins + outs + [info]]
        try:
            p = [b.ptr for b in bufs]
            o = [q if w else None for q, w in zip(p[5:9], want)]
            h.kfold_multi_batched(dtype, A.MEM_DEVICE, lay, nb, D, N, S, F, p[0], ldx, strides[0], p[1], ldY, strides[1], A.NOISE_DIAGONAL,
                                  p[2], strides[2], p[3], ldm, strides[3], p[4], D, D * D, o[0], tail[0], tail[1], o[1], tail[2], o[2],
                                  tail[3], tail[4], o[3], tail[5], p[9])
            for host, ptr in zip(outs + [info], p[5:]):
                h.memcpy_d2h(host, ptr)
        finally:
            for b in bufs:
                b.free()
    return (outs[0].reshape(nb, S, N).transpose(0, 2, 1), outs[1], outs[2].reshape(nb, S, nf).transpose(0, 2, 1), outs[3], info)


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


# ---- 1. brute force on a toy problem ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [1, 2, 5, 13, 64])
@pytest.mark.parametrize("prior", ["diagonal", "dense", "pdmat"])
@pytest.mark.parametrize("noise", ["isotropic", "diagonal"])
def test_brute_force_toy(B, prior, noise, F):
    rng = rng_of(1)
    N, D, S = 13, 7, 3
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
    Y = rng.standard_normal((N, S))
    Sy = B.Diagonal(s) if noise == "diagonal" else s
    r = B.kfold_columns(f(X, Sy), Y, F)
    nf = -(-N // F)
    assert isinstance(r, B.KFold) and r.logpdf.dtype == np.float64
    assert r.logpdf.shape == (nf, S) and r.mean.shape == (N, S) and r.var.shape == (N,) and r.total.shape == (S,)
    m_o, v_o, lp_o = brute_force_columns(mw, Lw_d, np.asarray(X), np.array(np.broadcast_to(s, (N,))), Y, F)
    print("toy", prior, noise, F, np.max(np.abs(r.mean - m_o)), np.max(np.abs(r.var / v_o[:, 0] - 1)), np.max(np.abs(r.logpdf / lp_o - 1)))
    np.testing.assert_allclose(r.mean, m_o, rtol=1e-9, atol=1e-12)
    for c in range(S):
        np.testing.assert_allclose(r.var, v_o[:, c], rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(r.logpdf, lp_o, rtol=1e-9, atol=1e-12)
    for c in range(S):
        assert r.total[c] == pytest.approx(math.fsum(r.logpdf[:, c]), rel=1e-12)


# ---- 2. the lattice against the closed form ---------------------------------------------------------------------------------
def _lattice():
    """A pairwise-covering subset of D x N x F x S x layout (every pair of values of two factors occurs): the 25 (D, N) pairs with F, S
    and the layout walking through their values at coprime steps, the cases of tests/test_kfold_gpu.py that the walk misses, then
    completed greedily."""
    Ds, Ns, Fs, Ss, Ls = [1, 16, 17, 100, 128], [1, 63, 64, 65, 200], [1, 3, 16, 17, 33, 64], [1, 3, 16, 17, 33], ["col", "row"]
    facs = [Ds, Ns, Fs, Ss, Ls]
    nf = len(facs)
    cases = set()
    for i, D in enumerate(Ds):
        for j, N in enumerate(Ns):
            cases.add((D, N, Fs[(i + j) % 6], Ss[(2 * i + j) % 5], Ls[(i + 2 * j) % 2]))
    # a partial last fold inside a partial last pack (N = 200, F = 3), a fold of 33 (31 rows idle), full packs with a partial last fold
    # (N = 65, F = 16), each with more than one pass of columns
    cases |= {(128, 200, 3, 17, "col"), (100, 200, 33, 33, "row"), (17, 65, 16, 17, "col"), (128, 200, 64, 33, "row"), (128, 200, 17, 16, "col")}

    def missing():
        return [(a, x, b, y) for a in range(nf) for b in range(a + 1, nf) for x in facs[a] for y in facs[b]
                if not any(c[a] == x and c[b] == y for c in cases)]

    k = 0
    while True:  # complete greedily: a case for the first missing pair, its other factors from the next missing pairs they fit
        miss = missing()
        if not miss:
            break
        a, x, b, y = miss[0]
        case = {a: x, b: y}
        for a2, x2, b2, y2 in miss[1:]:
            if all(case.get(f, v) == v for f, v in ((a2, x2), (b2, y2))):
                case.update({a2: x2, b2: y2})
        for f in range(nf):
            case.setdefault(f, facs[f][k % len(facs[f])])
        k += 1
        cases.add(tuple(case[f] for f in range(nf)))
    return sorted(cases)


LATTICE = _lattice()
assert len(LATTICE) <= 60


def test_lattice_is_pairwise_covering():
    cols = list(zip(*LATTICE))
    vals = [sorted(set(c), key=str) for c in cols]
    assert [len(v) for v in vals] == [5, 5, 6, 5, 2]
    for a in range(5):
        for b in range(a + 1, 5):
            assert {(x, y) for x in vals[a] for y in vals[b]} <= set(zip(cols[a], cols[b])), (a, b)
    assert any(N % F and (N % ((64 // F) * F)) for _, N, F, _, _ in LATTICE)


def _pad(D, N, S):
    return 3 if (D + N + S) % 2 else 0  # ldm > D and ldY > N in about half of the cases


@pytest.mark.parametrize("D,N,F,S,layout", LATTICE)
def test_lattice_fp64(B, h, D, N, F, S, layout):
    X, Y, s, M, T = _problems(2, D, N, S)
    m, v, lp, tot, info = _run(B, h, X, Y, s, M, T, F, layout=layout, pad=_pad(D, N, S))
    assert not info.any()
    assert not any(np.isnan(a).any() for a in (m, v, lp, tot))
    for b in range(2):
        m_o, v_o, lp_o, _ = closed_form_columns(M[b], T[b], X[b], s[b], Y[b], F)
        np.testing.assert_allclose(m[b], m_o, rtol=1e-9, atol=1e-12)
        np.testing.assert_allclose(v[b], v_o, rtol=1e-9, atol=1e-12)
        np.testing.assert_allclose(lp[b], lp_o, rtol=1e-9, atol=1e-12)
        for c in range(S):
            assert tot[b][c] == pytest.approx(math.fsum(lp[b][:, c]), rel=1e-12)


@pytest.mark.parametrize("D,N,F,S,layout", LATTICE)
def test_lattice_fp32(B, h, D, N, F, S, layout):
    """fp32 per column against the float64 closed form on the fp32-rounded inputs: 4 x the error of the same closed form in NumPy float32
    on them plus a floor of 8 eps32 of the output's scale (tests/_kfold_ref.py fp32_bounds)."""
    X, Y, s, M, T = _problems(1, D, N, S, dtype=np.float32)
    m, v, lp, tot, info = _run(B, h, X, Y, s, M, T, F, layout=layout, pad=_pad(D, N, S))
    assert not info.any() and m.dtype == np.float32 and v.dtype == np.float32 and lp.dtype == np.float64
    assert not any(np.isnan(a).any() for a in (m, v, lp, tot))
    worst = {}
    for c, (truth, bounds) in enumerate(fp32_bounds_columns(M[0], T[0], X[0], s[0], Y[0], F)):
        for got, t, bd, name in zip((m[0][:, c], v[0], lp[0][:, c]), truth, bounds, ("mean", "var", "logpdf")):
            err = float(np.max(np.abs(got.astype(np.float64) - t)))
            if err / bd >= worst.get(name, (0.0,))[0]:
                worst[name] = (err / bd, c, err, bd)
            assert err <= bd, (name, c, err, bd)
        assert tot[0][c] == pytest.approx(math.fsum(lp[0][:, c]), rel=1e-12)
    print("fp32", D, N, F, S, layout, worst)


# ---- 3. against the siblings -------------------------------------------------------------------------------------------------
def test_columns_match_the_single_column_call_and_loo_multi(B, h):
    D, N, F, S = 64, 150, 25, 5
    A = B._abi
    X, Y, s, M, T = _problems(1, D, N, S)
    m, v, lp, tot, info = _run(B, h, X, Y, s, M, T, F)
    assert not info.any()
    Xf, Tf = np.ascontiguousarray(X[0].reshape(-1, order="F")), np.ascontiguousarray(T[0].reshape(-1, order="F"))
    nf = -(-N // F)
    for c in range(S):
        km, kv, kl, kt, ki = np.empty(N), np.empty(N), np.empty(nf), np.empty(1), np.zeros(1, dtype=np.int32)
        h.kfold(np.float64, A.MEM_HOST, A.LAYOUT_COLVECS, 1, D, N, F, Xf, D, 0, np.ascontiguousarray(Y[0][:, c]), 0, A.NOISE_DIAGONAL, s[0], 0,
                np.ascontiguousarray(M[0][:, c]), 0, Tf, D, 0, km, N, kv, N, kl, nf, kt, ki)
        assert ki[0] == 0
        np.testing.assert_allclose(m[0][:, c], km, rtol=1e-9, atol=1e-12)
        np.testing.assert_allclose(v[0], kv, rtol=1e-9)
        np.testing.assert_allclose(lp[0][:, c], kl, rtol=1e-9)
        assert tot[0][c] == pytest.approx(kt[0], rel=1e-9)
    # F = 1: leave-one-out
    m1, v1, lp1, tot1, _ = _run(B, h, X, Y, s, M, T, 1)
    lm, lv, ll, lt, li = np.empty(S * N), np.empty(N), np.empty(S * N), np.empty(S), np.zeros(1, dtype=np.int32)
    h.loo_multi_batched(np.float64, A.MEM_HOST, A.LAYOUT_COLVECS, 1, D, N, S, Xf, D, 0, np.ascontiguousarray(Y[0].reshape(-1, order="F")), N, 0,
                        A.NOISE_DIAGONAL, s[0], 0, np.ascontiguousarray(M[0].reshape(-1, order="F")), D, 0, Tf, D, 0, lm, N, 0, lv, N, ll, N, 0,
                        lt, S, li)
    assert li[0] == 0
    np.testing.assert_allclose(m1[0], lm.reshape(S, N).T, rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(v1[0], lv, rtol=1e-9)
    np.testing.assert_allclose(lp1[0], ll.reshape(S, N).T, rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(tot1[0], lt, rtol=1e-9)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_variances_are_the_single_column_calls_bit_for_bit(B, h, dtype):
    """kf_var depends on the fold factor alone: kfold_cols_kernel and kfold_kernel form it by the same steps from the same rows of Z"""
    D, N, F, S = 20, 70, 5, 3
    A = B._abi
    X, Y, s, M, T = _problems(1, D, N, S, dtype=dtype)
    _, v, _, _, info = _run(B, h, X, Y, s, M, T, F)
    assert not info.any() and not np.isnan(v).any()
    Xf, Tf = np.ascontiguousarray(X[0].reshape(-1, order="F")), np.ascontiguousarray(T[0].reshape(-1, order="F"))
    kv, ki = np.empty(N, dtype=dtype), np.zeros(1, dtype=np.int32)
    h.kfold(dtype, A.MEM_HOST, A.LAYOUT_COLVECS, 1, D, N, F, Xf, D, 0, np.ascontiguousarray(Y[0][:, 0]), 0, A.NOISE_DIAGONAL, s[0], 0,
            np.ascontiguousarray(M[0][:, 0]), 0, Tf, D, 0, None, N, kv, N, None, -(-N // F), None, ki)
    assert ki[0] == 0
    assert np.array_equal(v[0], kv)


# ---- 4. bit promises -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_bits_do_not_depend_on_batch_chunks_memspace_outputs_or_the_other_columns(B, h, dtype):
    nb, D, N, F, S = 7, 33, 150, 8, 19
    X, Y, s, M, T = _problems(nb, D, N, S, dtype=dtype)
    h.set_option("MAX_CHUNK", None)
    ref = _run(B, h, X, Y, s, M, T, F)
    assert not ref[4].any() and not any(np.isnan(a).any() for a in ref[:4])
    assert h.get_stat("last_chunks") == 1
    again = _run(B, h, X, Y, s, M, T, F)
    assert all(_same(a, b) for a, b in zip(ref, again))                       # call to call
    for b in (0, 3, 6):                                                       # B = 7 against B = 1
        one = _run(B, h, *(a[b:b + 1] for a in (X, Y, s, M, T)), F)
        assert all(_same(a[b:b + 1], o) for a, o in zip(ref[:4], one[:4])), b
    perm = np.array([4, 0, 6, 2, 5, 1, 3])                                    # a permuted batch
    pr = _run(B, h, *(a[perm] for a in (X, Y, s, M, T)), F)
    assert all(_same(a[perm], o) for a, o in zip(ref[:4], pr[:4]))
    for cap, chunks in ((1, 7), (2, 4), (3, 3)):                              # chunk seams
        h.set_option("MAX_CHUNK", str(cap))
        try:
            got = _run(B, h, X, Y, s, M, T, F)
            assert h.get_stat("last_chunks") == chunks
            tot_only = _run(B, h, X, Y, s, M, T, F, want=(False, False, False, True))   # (the log densities through workspace)
        finally:
            h.set_option("MAX_CHUNK", None)
        assert all(_same(a, o) for a, o in zip(ref, got)), cap
        assert _same(tot_only[3], ref[3]), cap
    dev = _run(B, h, X, Y, s, M, T, F, memspace="device")                    # host against device memspace
    assert all(_same(a, o) for a, o in zip(ref, dev))
    padded = _run(B, h, X, Y, s, M, T, F, pad=5)                              # leading dimensions
    assert all(_same(a, o) for a, o in zip(ref, padded))
    for k in range(4):                                                        # each output alone
        want = tuple(i == k for i in range(4))
        alone = _run(B, h, X, Y, s, M, T, F, want=want)
        assert _same(alone[k], ref[k]), k
        assert all(np.isnan(alone[i]).all() for i in range(4) if i != k)      # the others are not touched
    for c in (0, 15, 16, 18):                                                 # column c alone against column c inside S = 19
        one = _run(B, h, X, Y[:, :, c:c + 1], s, M[:, :, c:c + 1], T, F)
        assert _same(one[0][:, :, 0], ref[0][:, :, c]) and _same(one[2][:, :, 0], ref[2][:, :, c]) and _same(one[3][:, 0], ref[3][:, c]), c
        assert _same(one[1], ref[1]), c                                       # kf_var at S = 1 against S = 19
    cp = np.random.Generator(np.random.PCG64(5)).permutation(S)               # permuted columns give permuted bits
    pc = _run(B, h, X, Y[:, :, cp], s, M[:, :, cp], T, F)
    assert _same(pc[0], ref[0][:, :, cp]) and _same(pc[2], ref[2][:, :, cp]) and _same(pc[3], ref[3][:, cp]) and _same(pc[1], ref[1])


# ---- 5. fold locality ------------------------------------------------------------------------------------------------------------
def test_a_fold_depends_on_its_own_data_only(B, h):
    """tests/test_kfold_gpu.py's test of that name with S = 5.  F = 8: eight folds share a workgroup.  New X, Y and s in fold 2 alone:
    every other fold keeps its bits; and a fold keeps its bits when N shrinks or when it lands elsewhere in a workgroup."""
    D, N, F, S = 33, 150, 8, 5
    X, Y, s, M, T = _problems(1, D, N, S)
    ref = _run(B, h, X, Y, s, M, T, F)
    X2, Y2, s2 = X.copy(), Y.copy(), s.copy()
    rng = rng_of(9)
    X2[0][:, 16:24] *= 0.5
    Y2[0][16:24, :] = rng.standard_normal((8, S))
    s2[0][16:24] *= 1.5
    got = _run(B, h, X2, Y2, s2, M, T, F)
    keep = np.r_[0:16, 24:N]
    assert _same(got[0][0][keep], ref[0][0][keep]) and _same(got[1][0][keep], ref[1][0][keep])
    assert _same(np.delete(got[2][0], 2, axis=0), np.delete(ref[2][0], 2, axis=0))
    assert not (got[2][0][2] == ref[2][0][2]).any() and not np.isnan(got[2]).any()
    # the first 5 folds alone (N = 40: one pack of five folds instead of eight)
    short = _run(B, h, X[:, :, :40], Y[:, :40], s[:, :40], M, T, F)
    assert _same(short[0][0], ref[0][0][:40]) and _same(short[1][0], ref[1][0][:40]) and _same(short[2][0], ref[2][0][:5])
    # folds 3 .. 9 as folds 0 .. 6: another place in the workgroup
    moved = _run(B, h, X[:, :, 24:80], Y[:, 24:80], s[:, 24:80], M, T, F)
    assert _same(moved[0][0], ref[0][0][24:80]) and _same(moved[1][0], ref[1][0][24:80]) and _same(moved[2][0], ref[2][0][3:10])


# ---- 6. column locality and the NaN rule -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_a_nan_target_stays_in_its_column_and_fold(B, h, dtype):
    nb, D, N, F, S = 2, 33, 150, 8, 5
    X, Y, s, M, T = _problems(nb, D, N, S, dtype=dtype)
    ref = _run(B, h, X, Y, s, M, T, F)
    Y2 = Y.copy()
    Y2[:, 20, 2] = np.nan
    before = h.get_stat("kfold_degenerate")
    got = _run(B, h, X, Y2, s, M, T, F)
    assert h.get_stat("kfold_degenerate") == before and not got[4].any()
    for b in range(nb):
        assert np.isnan(got[0][b][16:24, 2]).all() and np.isnan(got[2][b][2, 2]) and np.isnan(got[3][b][2])
        mean_r, lp_r, tot_r = ref[0][b].copy(), ref[2][b].copy(), ref[3][b].copy()
        mean_r[16:24, 2], lp_r[2, 2], tot_r[2] = np.nan, np.nan, np.nan
        assert _same(got[0][b], mean_r) and _same(got[2][b], lp_r) and _same(got[3][b], tot_r)   # every other number keeps its bits
        assert _same(got[1][b], ref[1][b])                                                        # all of kf_var


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_degenerate_fold_is_nan_in_every_column_and_counted_once(B, h, dtype):
    nb, D, N, F, S = 3, 33, 150, 8, 5
    X, Y, s, M, T = _problems(nb, D, N, S, dtype=dtype)
    ref = _run(B, h, X, Y, s, M, T, F)
    s2 = s.copy()
    s2[:, 24:32] *= dtype(1e-6)  # the state holds these observations with 1e6 times less weight: I - H~ is not positive definite
    before = h.get_stat("kfold_degenerate")
    got = _run(B, h, X, Y, s2, M, T, F)
    assert h.get_stat("kfold_degenerate") - before == nb   # once per fold, not once per column
    assert not got[4].any()
    keep = np.r_[0:24, 32:N]
    for b in range(nb):
        assert np.isnan(got[0][b][24:32]).all() and np.isnan(got[1][b][24:32]).all() and np.isnan(got[2][b][3]).all() and np.isnan(got[3][b]).all()
        assert _same(got[0][b][keep], ref[0][b][keep]) and _same(got[1][b][keep], ref[1][b][keep])
        rest = np.delete(got[2][b], 3, axis=0)
        assert _same(rest, np.delete(ref[2][b], 3, axis=0)) and not np.isnan(rest).any()


# ---- 7. status and no-ops ---------------------------------------------------------------------------------------------------------
def test_status_leaves_the_outputs_untouched_and_the_no_ops(B, h):
    nb, D, N, F, S = 3, 33, 70, 8, 5
    X, Y, s, M, T = _problems(nb, D, N, S)
    T[0][4, 4] = -1.0   # diagonal entry 5 of the first factor
    s[2][10] = 0.0      # variance 11 of the third regressor
    m, v, lp, tot, info = _run(B, h, X, Y, s, M, T, F, fill=-123.0)
    assert list(info) == [5, 0, 11]
    for b in (0, 2):
        assert (m[b] == -123.0).all() and (v[b] == -123.0).all() and (lp[b] == -123.0).all() and (tot[b] == -123.0).all()
    m_o, v_o, lp_o, _ = closed_form_columns(M[1], T[1], X[1], s[1], Y[1], F)
    np.testing.assert_allclose(m[1], m_o, rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(v[1], v_o, rtol=1e-9)
    np.testing.assert_allclose(lp[1], lp_o, rtol=1e-9)
    # N = 0: empty sums
    ok = [a[1:2].repeat(nb, 0) for a in (M, T)]
    z = _run(B, h, X[:, :, :0], Y[:, :0], s[:, :0], ok[0], ok[1], F)
    assert not z[4].any() and (z[3] == 0.0).all() and z[3].shape == (nb, S)
    # S = 0 and B = 0: nothing is touched, info included
    z = _run(B, h, X, Y[:, :, :0], s, M[:, :, :0], T, F, fill=-5.0)
    assert (z[1] == -5.0).all() and (z[4] == -7).all()
    z = _run(B, h, X[:0], Y[:0], s[:0], M[:0], T[:0], F)
    assert z[4].shape == (0,)


# ---- 8. the Python surface ---------------------------------------------------------------------------------------------------------
def _fx(B, seed, D, N, S):
    """-> (finite regressor, targets, (mw, U, X, s, Y, M, T) of tests/_kfold_multi_ref.py)"""
    st = columns_state(seed, D, N, S)
    mw, U, X, s, Y = st[:5]
    return B.BayesianLinearRegressor(mw, B.PDMat(U))(B.ColVecs(X), B.Diagonal(s)), Y, st


def test_kfold_columns_map_perm_and_mixed_shapes(B):
    D, N, F, S, nb = 16, 70, 16, 5, 3
    fxs, Ys, sts = zip(*[_fx(B, 40 + b, D, N, S) for b in range(nb)])
    many = B.kfold_columns_map(fxs, Ys, F)
    for r, fx, Y, st in zip(many, fxs, Ys, sts):
        one = B.kfold_columns(fx, Y, F)
        assert r.mean.shape == (N, S) and r.logpdf.shape == (5, S)
        assert _same(r.mean, one.mean) and _same(r.var, one.var) and _same(r.logpdf, one.logpdf) and _same(r.total, one.total)
        m_o, v_o, lp_o, _ = closed_form_columns(st[5], st[6], st[2], st[3], Y, F)
        np.testing.assert_allclose(r.mean, m_o, rtol=1e-8, atol=1e-10)
        np.testing.assert_allclose(r.var, v_o, rtol=1e-8)
        np.testing.assert_allclose(r.logpdf, lp_o, rtol=1e-8)
    # unequal shapes: one pair of calls per problem, the same numbers
    fx50, Y50, (mw, U, X, s, _, _, _) = _fx(B, 50, D, 50, S)
    mixed = B.kfold_columns_map([fxs[0], fx50, fxs[2]], [Ys[0], Y50, Ys[2]], F)
    assert mixed[1].logpdf.shape == (4, S) and _same(mixed[0].mean, many[0].mean) and _same(mixed[2].logpdf, many[2].logpdf)
    # random folds: the same as the gathered problem, scattered back
    perm = rng_of(11).permutation(50)
    rp = B.kfold_columns(fx50, Y50, F, perm=perm)
    g = B.kfold_columns(B.BayesianLinearRegressor(mw, B.PDMat(U))(B.ColVecs(np.asfortranarray(X[:, perm])), B.Diagonal(s[perm])), Y50[perm], F)
    assert _same(rp.mean[perm], g.mean) and _same(rp.var[perm], g.var) and _same(rp.logpdf, g.logpdf) and _same(rp.total, g.total)
    assert _same(mixed[1].logpdf, B.kfold_columns(fx50, Y50, F).logpdf)


def test_resident_kfold_matches_forget_predict_condition(B):
    D, N, F, S = 64, 150, 25, 3
    mw, U, X, s, Y, _, _ = columns_state(4, D, N, S)
    st = B.ResidentColumnsPosterior(B.BayesianLinearRegressor(mw, B.PDMat(U)), S=S)
    st.condition(B.ColVecs(X), B.Diagonal(s), Y)

    M0, T0 = st.state()
    r = st.kfold(B.ColVecs(X), B.Diagonal(s), Y, F)
    M1, T1 = st.state()
    assert np.array_equal(M0, M1) and np.array_equal(T0, T1)  # the state is not modified
    assert r.mean.shape == (N, S) and r.var.shape == (N,) and r.logpdf.shape == (6, S) and r.total.shape == (S,)
    f = 2  # one fold per column: forget it, predict at its inputs, put it back
    a, b = f * F, min((f + 1) * F, N)
    xf, sf, Yf = B.ColVecs(np.asfortranarray(X[:, a:b])), B.Diagonal(s[a:b]), np.asfortranarray(Y[a:b])
    lp_forget = st.forget(xf, sf, Yf)
    m, v = st.mean_and_var(xf, sf)
    st.condition(xf, sf, Yf)
    np.testing.assert_allclose(r.mean[a:b], m, rtol=1e-8, atol=1e-10)
    np.testing.assert_allclose(r.var[a:b], v, rtol=1e-8)
    np.testing.assert_allclose(r.logpdf[f], lp_forget, rtol=1e-8)
