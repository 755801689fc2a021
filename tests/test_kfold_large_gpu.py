"""Leave-fold-out predictives for large folds (blr_kfold_large_batched_*, kfold_large, kfold_large_map,
ResidentPosterior.kfold_large) on the GPU: brute-force refits with the CPU oracle on a toy problem, a lattice of
(D, N, F, layout) against the weight-space closed form of tests/_kfold_large_ref.py, a fold of several column blocks, agreement with
blr_kfold_batched_* at F <= 64, the bit promises of the header, the NaN rule, the status, the map and resident forms, and the
resources of the two new kernels.  All tests but the last need an MI355X."""
import functools
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from oracle import blr_oracle as O

from _kfold_ref import brute_force, posterior_state, rng_of, state
from _kfold_large_ref import closed_form_large, fp32_bounds_large

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
def _problems64(nb, D, N, seed=0):
    """nb states (mw', T) that contain their N observations, float64 arrays [nb, ...] (computed once per shape; read-only)"""
    out = []
    for b in range(nb):
        mw, U, X, s, y = state(rng_of(seed + 31 * b + D + N), D, N)
        mwp, T = posterior_state(mw, U, X, s, y)
        out.append((X, y, s, mwp, np.asfortranarray(T)))
    arrs = [np.stack([q[i] for q in out]) for i in range(5)]
    for a in arrs:
        a.setflags(write=False)
    return arrs


def _problems(nb, D, N, dtype=np.float64, seed=0):
    return [a.astype(dtype) for a in _problems64(nb, D, N, seed)]


@functools.lru_cache(maxsize=None)
def _reference64(nb, D, N, F):
    X, y, s, mw, T = _problems64(nb, D, N)
    return [closed_form_large(mw[b], T[b], X[b], s[b], y[b], F)[:3] for b in range(nb)]


@functools.lru_cache(maxsize=None)
def _yardstick32(D, N, F):
    X, y, s, mw, T = _problems(1, D, N, dtype=np.float32)
    return fp32_bounds_large(mw[0], T[0], X[0], s[0], y[0], F)


def _run(B, h, X, y, s, mw, T, F, layout="col", memspace="host", want=(True, True, True, True), fill=None, small=False):
    """blr_kfold_large_batched_* (small: blr_kfold_batched_*) on stacked operands X [nb, D, N], y, s [nb, N], mw [nb, D], T [nb, D, D]
    -> (mean, var, logpdf, total, info)"""
    A, R = B._abi, B.regressor
    nb, D, N = X.shape
    dtype = X.dtype.type
    nf = -(-N // F)
    fn = h.kfold if small else h.kfold_large
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
        fn(dtype, A.MEM_HOST, lay, nb, D, N, F, ins[0], ldx, D * N, ins[1], N, A.NOISE_DIAGONAL, ins[2], N, ins[3], D, ins[4], D, D * D,
           o[0], N, o[1], N, o[2], nf, o[3], info)
    else:
        bufs = [R._DeviceBuffer.of(h, a) for a in ins + outs + [info]]
        try:
            p = [b.ptr for b in bufs]
            o = [q if w else None for q, w in zip(p[5:9], want)]
            fn(dtype, A.MEM_DEVICE, lay, nb, D, N, F, p[0], ldx, D * N, p[1], N, A.NOISE_DIAGONAL, p[2], N, p[3], D, p[4], D, D * D,
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
@pytest.mark.parametrize("F", [5, 13, 64])
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
    r = B.kfold_large(f(X, Sy), y, F)
    nf = -(-N // F)
    assert isinstance(r, B.KFold) and r.logpdf.dtype == np.float64 and r.logpdf.shape == (nf,) and r.mean.shape == (N,) and r.var.shape == (N,)
    m_o, v_o, lp_o = brute_force(mw, Lw_d, np.asarray(X), np.array(np.broadcast_to(s, (N,))), y, F)
    print("toy", prior, noise, F, np.max(np.abs(r.mean - m_o)), np.max(np.abs(r.var / v_o - 1)), np.max(np.abs(r.logpdf / lp_o - 1)))
    np.testing.assert_allclose(r.mean, m_o, rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(r.var, v_o, rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(r.logpdf, lp_o, rtol=1e-9, atol=1e-12)
    assert r.total == pytest.approx(math.fsum(r.logpdf), rel=1e-12)


# ---- 2. the lattice against the closed form ---------------------------------------------------------------------------------
DS = [1, 16, 17, 100, 128]
# (N, F): (65, 65) one fold with a second tile of one row, (130, 65) two such folds, (200, 100) a partial second tile, (200, 128) a last
# fold of 72, (200, 200) one fold of everything, (130, 300) F > N, (1100, 220) five folds of four tiles
NFS = [(65, 65), (130, 65), (200, 100), (200, 128), (200, 200), (130, 300), (1100, 220)]
# every (D, (N, F)) pair once, the layout alternating along both: every pair of values of two factors occurs; plus a last fold of fewer
# than 64 rows ((150, 100): 50 rows) in both layouts
LATTICE = [(D, N, F, ("col", "row")[(i + j) % 2]) for i, D in enumerate(DS) for j, (N, F) in enumerate(NFS)]
LATTICE += [(17, 150, 100, "col"), (128, 150, 100, "row")]


def test_lattice_is_pairwise_covering():
    for D in DS:
        assert {c[3] for c in LATTICE if c[0] == D} == {"col", "row"}
        assert {(c[1], c[2]) for c in LATTICE if c[0] == D} >= set(NFS)
    for N, F in NFS:
        assert {c[3] for c in LATTICE if (c[1], c[2]) == (N, F)} == {"col", "row"}
    assert any(0 < N % F < 64 for _, N, F, _ in LATTICE)            # a last fold of fewer than 64 rows
    assert any(min(F, N) % 64 for _, N, F, _ in LATTICE)            # a fold whose last tile is partial


@pytest.mark.parametrize("D,N,F,layout", LATTICE)
def test_lattice_fp64(B, h, D, N, F, layout):
    X, y, s, mw, T = _problems(2, D, N)
    m, v, lp, tot, info = _run(B, h, X, y, s, mw, T, F, layout=layout)
    assert not info.any()
    for b, (m_o, v_o, lp_o) in enumerate(_reference64(2, D, N, F)):
        print("fp64", D, N, F, layout, np.max(np.abs(m[b] - m_o)), np.max(np.abs(v[b] / v_o - 1)), np.max(np.abs(lp[b] / lp_o - 1)))
        np.testing.assert_allclose(m[b], m_o, rtol=1e-9, atol=1e-12)
        np.testing.assert_allclose(v[b], v_o, rtol=1e-9, atol=1e-12)
        np.testing.assert_allclose(lp[b], lp_o, rtol=1e-9, atol=1e-12)
        assert tot[b] == pytest.approx(math.fsum(lp[b]), rel=1e-12)


def _check_fp32(B, h, D, N, F, layout):
    X, y, s, mw, T = _problems(1, D, N, dtype=np.float32)
    m, v, lp, tot, info = _run(B, h, X, y, s, mw, T, F, layout=layout)
    assert not info.any() and m.dtype == np.float32 and lp.dtype == np.float64
    truth, bounds = _yardstick32(D, N, F)
    for got, t, bd, name in zip((m[0], v[0], lp[0]), truth, bounds, ("mean", "var", "logpdf")):
        err = float(np.max(np.abs(got.astype(np.float64) - t)))
        print("fp32", D, N, F, layout, name, err, bd)
        assert err <= bd, (name, err, bd)
    assert tot[0] == pytest.approx(math.fsum(lp[0]), rel=1e-12)


@pytest.mark.parametrize("D,N,F,layout", LATTICE)
def test_lattice_fp32(B, h, D, N, F, layout):
    """fp32 against the float64 closed form on the fp32-rounded inputs: 4 x the error of the same closed form in NumPy float32 on them
    plus a floor of 8 eps32 of the output's scale (tests/_kfold_large_ref.py fp32_bounds_large).  The hard cases are D = 1 with one
    fold that holds all the data (cancellation of A - G_f 19 x and more): with G_f accumulated in fp32 they missed this bound by
    1.02 - 1.25 x, which is why the fp32 statistics are accumulated in double."""
    _check_fp32(B, h, D, N, F, layout)


# ---- 3. a fold of several column blocks: the reduce (kfl_splits cuts n_f = 2100 into two blocks; the last fold has 100 rows and one) --
@pytest.mark.parametrize("layout", ["col", "row"])
def test_column_blocks_fp64(B, h, layout):
    D, N, F = 32, 2200, 2100
    X, y, s, mw, T = _problems(1, D, N)
    m, v, lp, tot, info = _run(B, h, X, y, s, mw, T, F, layout=layout)
    assert not info.any()
    (m_o, v_o, lp_o), = _reference64(1, D, N, F)
    print("blocks fp64", layout, np.max(np.abs(m[0] - m_o)), np.max(np.abs(v[0] / v_o - 1)), np.max(np.abs(lp[0] / lp_o - 1)))
    np.testing.assert_allclose(m[0], m_o, rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(v[0], v_o, rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(lp[0], lp_o, rtol=1e-9, atol=1e-12)


@pytest.mark.parametrize("layout", ["col", "row"])
def test_column_blocks_fp32(B, h, layout):
    _check_fp32(B, h, 32, 2200, 2100, layout)


# ---- 4. agreement with blr_kfold_batched_* at F <= 64 -------------------------------------------------------------------------
@pytest.mark.parametrize("D,N,F", [(128, 200, 64), (100, 130, 16)])
def test_agrees_with_the_hat_matrix_entry_point(B, h, D, N, F):
    X, y, s, mw, T = _problems(2, D, N)
    big = _run(B, h, X, y, s, mw, T, F)
    small = _run(B, h, X, y, s, mw, T, F, small=True)
    assert not big[4].any() and not small[4].any()
    for a, b, name in zip(big[:4], small[:4], ("mean", "var", "logpdf", "total")):
        print("agree", D, N, F, name, np.max(np.abs(a - b)))
        np.testing.assert_allclose(a, b, rtol=1e-9, atol=1e-12, err_msg=name)


# ---- 5. bit promises -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_bits_do_not_depend_on_batch_chunks_memspace_or_outputs(B, h, dtype):
    nb, D, N, F = 5, 33, 260, 65
    X, y, s, mw, T = _problems(nb, D, N, dtype=dtype)
    h.set_option("MAX_CHUNK", None)
    ref = _run(B, h, X, y, s, mw, T, F)
    assert not ref[4].any() and not any(np.isnan(a).any() for a in ref[:4])
    assert h.get_stat("last_chunks") == 1
    again = _run(B, h, X, y, s, mw, T, F)
    assert all(_same(a, b) for a, b in zip(ref, again))                       # two identical calls
    for b in (0, 2, 4):                                                       # a regressor alone against inside the batch of 5
        one = _run(B, h, *(a[b:b + 1] for a in (X, y, s, mw, T)), F)
        assert all(_same(a[b:b + 1], o) for a, o in zip(ref[:4], one[:4])), b
    h.set_option("MAX_CHUNK", "2")                                            # chunk seams
    try:
        got = _run(B, h, X, y, s, mw, T, F)
        assert h.get_stat("last_chunks") == 3
    finally:
        h.set_option("MAX_CHUNK", None)
    assert all(_same(a, o) for a, o in zip(ref, got))
    dev = _run(B, h, X, y, s, mw, T, F, memspace="device")                    # host against device memspace
    assert all(_same(a, o) for a, o in zip(ref, dev))
    subsets = [tuple(i == k for i in range(4)) for k in range(4)] + [(True, False, False, True), (False, True, True, False)]
    for want in subsets:                                                      # any subset of the outputs
        part = _run(B, h, X, y, s, mw, T, F, want=want)
        for i in range(4):
            if want[i]:
                assert _same(part[i], ref[i]), (want, i)
            else:
                assert np.isnan(part[i]).all(), (want, i)                     # the others are not touched
    # folds 1 and 2 of (N = 260, F = 65) presented as the folds 0 and 1 of a call with N = 130
    mid = _run(B, h, X[:, :, 65:195], y[:, 65:195], s[:, 65:195], mw, T, F)
    assert _same(mid[0], ref[0][:, 65:195]) and _same(mid[1], ref[1][:, 65:195]) and _same(mid[2], ref[2][:, 1:3])


# ---- 6. a degenerate fold -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_fold_the_state_does_not_contain_is_nan_and_alone(B, h, dtype):
    """Regressor 1 of 3 is conditioned on the last 100 of its 300 observations only: A - G_0 of its fold [0, 200) is negative on the
    diagonal.  That fold is NaN everywhere and counted once; its fold [200, 300) has the bits of a call on those rows alone, and the
    other two regressors those of their own calls."""
    nb, D, N, F = 3, 17, 300, 200
    X, y, s, mw, T = _problems(nb, D, N)
    mw, T = mw.copy(), T.copy()
    pm, pU, pX, ps, py = state(rng_of(31 + D + N), D, N)  # regressor 1 as _problems64 makes it: the same data, less of it in the state
    assert np.array_equal(pX, X[1])
    mw[1], T[1] = posterior_state(pm, pU, pX[:, 200:], ps[200:], py[200:])
    A1 = T[1].T @ T[1] - (X[1][:, :200] / s[1][:200]) @ X[1][:, :200].T
    assert np.max(np.diag(A1)) < 0                         # (the premise)
    X, y, s, mw, T = (a.astype(dtype) for a in (X, y, s, mw, T))
    before = h.get_stat("kfold_degenerate")
    got = _run(B, h, X, y, s, mw, T, F)
    assert h.get_stat("kfold_degenerate") - before == 1
    assert not got[4].any()
    assert np.isnan(got[0][1][:200]).all() and np.isnan(got[1][1][:200]).all() and np.isnan(got[2][1][0]) and np.isnan(got[3][1])
    clean = _run(B, h, X[1:2, :, 200:], y[1:2, 200:], s[1:2, 200:], mw[1:2], T[1:2], F)
    assert not np.isnan(clean[0]).any() and not np.isnan(clean[2]).any()
    assert _same(got[0][1][200:], clean[0][0]) and _same(got[1][1][200:], clean[1][0]) and _same(got[2][1][1], clean[2][0][0])
    for b in (0, 2):
        one = _run(B, h, *(a[b:b + 1] for a in (X, y, s, mw, T)), F)
        assert all(_same(a[b:b + 1], o) for a, o in zip(got[:4], one[:4])) and not np.isnan(one[3]).any()


# ---- 7. status -----------------------------------------------------------------------------------------------------------------
def test_status_leaves_the_outputs_untouched(B, h):
    nb, D, N, F = 3, 33, 260, 100
    X, y, s, mw, T = _problems(nb, D, N)
    T[0][4, 4] = -1.0   # diagonal entry 5 of the first factor
    s[2][10] = 0.0      # variance 11 of the third regressor
    m, v, lp, tot, info = _run(B, h, X, y, s, mw, T, F, fill=-123.0)
    assert list(info) == [5, 0, 11]
    for b in (0, 2):
        assert (m[b] == -123.0).all() and (v[b] == -123.0).all() and (lp[b] == -123.0).all() and tot[b] == -123.0
    m_o, v_o, lp_o = closed_form_large(mw[1], T[1], X[1], s[1], y[1], F)[:3]
    np.testing.assert_allclose(m[1], m_o, rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(v[1], v_o, rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(lp[1], lp_o, rtol=1e-9, atol=1e-12)
    assert tot[1] == pytest.approx(math.fsum(lp[1]), rel=1e-12)
    # both at once: the factor comes first
    s[0][3] = -1.0
    assert list(_run(B, h, X, y, s, mw, T, F, fill=-123.0)[4]) == [5, 0, 11]
    # N = 0: an empty sum
    z = _run(B, h, X[:, :, :0], y[:, :0], s[:, :0], mw[1:2].repeat(nb, 0), T[1:2].repeat(nb, 0), F)
    assert not z[4].any() and (z[3] == 0.0).all()


# ---- 8. the map and resident forms ----------------------------------------------------------------------------------------------
def test_kfold_large_map_is_bit_identical_to_single_calls(B):
    rng = rng_of(11)
    D, N, F, nb = 16, 210, 100, 3
    fxs, ys, raw = [], [], []
    for _ in range(nb):
        mw, U, X, s, y = state(rng, D, N)
        fxs.append(B.BayesianLinearRegressor(mw, B.PDMat(U))(B.ColVecs(X), B.Diagonal(s)))
        ys.append(y)
        raw.append((mw, U, X, s))
    many = B.kfold_large_map(fxs, ys, F)
    assert len(many) == nb and all(r.logpdf.shape == (3,) for r in many)
    for r, fx, y in zip(many, fxs, ys):
        one = B.kfold_large(fx, y, F)
        assert _same(r.mean, one.mean) and _same(r.var, one.var) and _same(r.logpdf, one.logpdf) and r.total == one.total
    # random folds: the same as the gathered problem, scattered back; cross_validate picks this entry point at F = 105
    perm = rng.permutation(N)
    rp = B.cross_validate(fxs[0], ys[0], 2, perm=perm)
    mw, U, X, s = raw[0]
    g = B.kfold_large(B.BayesianLinearRegressor(mw, B.PDMat(U))(B.ColVecs(np.asfortranarray(X[:, perm])), B.Diagonal(s[perm])), ys[0][perm], 105)
    assert _same(rp.mean[perm], g.mean) and _same(rp.var[perm], g.var) and _same(rp.logpdf, g.logpdf)


def test_resident_kfold_large_after_a_condition(B):
    D, N, F = 64, 330, 150
    mw, U, X, s, y = state(rng_of(4), D, N)
    st = B.ResidentPosterior(B.BayesianLinearRegressor(mw, B.PDMat(U)))
    st.condition(B.ColVecs(X), B.Diagonal(s), y)
    m0, T0 = st.state()
    r = st.kfold_large(B.ColVecs(X), B.Diagonal(s), y, F)
    m1, T1 = st.state()
    assert np.array_equal(m0, m1) and np.array_equal(T0, T1)  # the state is not modified
    assert r.logpdf.shape == (3,) and r.total == pytest.approx(math.fsum(r.logpdf), rel=1e-12)
    m_o, v_o, lp_o = brute_force(mw, U.T @ U, X, s, y, F)
    np.testing.assert_allclose(r.mean, m_o, rtol=1e-8, atol=1e-10)
    np.testing.assert_allclose(r.var, v_o, rtol=1e-8)
    np.testing.assert_allclose(r.logpdf, lp_o, rtol=1e-8)


# ---- 9. resources of the two new kernels ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel,count", [("kfl_factor_kernel", 16), ("kfl_predict_kernel", 4)])  # 2 types x 8 block counts; x 2 layouts
def test_kfold_large_kernel_resources(tmp_path, kernel, count):
    """Registers and scratch of every kfl_factor_kernel and kfl_predict_kernel instantiation from the code object's notes: at most
    256 registers, no scratch and no spilled register (DESIGN.md K24 states this build's figures).  kfl_factor_kernel inlines
    phase_chol / phase_backsolve at its two call statements: as calls their frames cost it 8 - 12 B of scratch per lane."""
    from blr_amd import _abi

    objdump = "/opt/rocm/lib/llvm/bin/llvm-objdump"
    readelf = "/opt/rocm/lib/llvm/bin/llvm-readelf"
    if not (os.path.exists(objdump) and os.path.exists(readelf)):
        pytest.skip("ROCm LLVM tools not installed")
    so = shutil.copy(_abi.LIB_PATH, tmp_path / "lib.so")
    subprocess.run([objdump, "--offloading", str(so)], check=True, capture_output=True, cwd=tmp_path)
    cos = [p for p in os.listdir(tmp_path) if "gfx950" in p]
    assert cos, "no gfx950 code object in the library"
    notes = "".join(subprocess.run([readelf, "--notes", str(tmp_path / c)], check=True, capture_output=True, text=True).stdout for c in sorted(cos))
    props, name = {}, None
    for line in notes.splitlines():
        m = re.match(r"\s+(?:- )?\.(name|vgpr_count|vgpr_spill_count|private_segment_fixed_size):\s+(\S+)", line)
        if m and m.group(1) == "name":
            name = m.group(2)
        elif m and name is not None:
            props.setdefault(name, {})[m.group(1)] = int(m.group(2))
    kf = {k: v for k, v in props.items() if kernel in k}
    assert len(kf) == count, sorted(kf)
    for k, v in kf.items():
        print(k, v)
        assert v["vgpr_count"] <= 256, (k, v)
        assert v["vgpr_spill_count"] == 0, (k, v)
    for k, v in kf.items():
        assert v["private_segment_fixed_size"] == 0, (k, v)
