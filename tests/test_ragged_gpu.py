"""blr_posterior_ragged_* on the device: regressors with unequal observation counts in one call, through the C
ABI.  Every regressor is held to the oracle at the header's tolerances AND to the bits of blr_posterior_batched_* with B = 1 on
its slice (a handle with NO_I8_GRAM = 1, NO_WAVE_KERNEL = 1: the same phases on the same data)."""
import numpy as np
import pytest

import blr_amd as B
from _small_d_problems import COUNTS, _batch, _check_oracle, _outputs, _result, _same_bits, _single
from blr_amd import _abi
from oracle import blr_oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def h():
    hd = _abi.Handle()
    yield hd
    hd.close()


@pytest.fixture(scope="module")
def h1():
    """the equal-count entry point kept on the phases the ragged kernel runs"""
    hd = _abi.Handle()
    hd.set_option("NO_I8_GRAM", "1")
    hd.set_option("NO_WAVE_KERNEL", "1")
    yield hd
    hd.close()


def _ragged(hd, q, o, memspace=_abi.MEM_HOST, arrays=None):
    a = arrays or dict(X=q["X"], y=q["y"], s=q["s"], mw=q["mw"], Lw=q["Lw"], mw_post=o["mw_post"], T=o["T"], A=o["A"], lp=o["lp"],
                       info=o["info"])
    return hd.posterior_ragged(q["dtype"], memspace, q["layout"], q["nb"], q["D"], q["offsets"], a["X"], q["ldx"], a["y"], q["noise_kind"],
                               a["s"], q["strides"], q["prior_kind"], a["mw"], q["stridemw"], a["Lw"], q["ldl"], q["strideLw"],
                               a["mw_post"], o["stride_mwpost"], a["T"], o["ldt"], o["strideT"], a["A"], o["ldt"], o["strideT"], a["lp"],
                               a["info"])


# (data layout, noise, prior, shared prior): every value of every axis, five sets per (D, dtype)
VARIANTS = [("col16", "iso", "diag", False), ("colodd", "diag", "dense", True), ("row", "iso0", "factor", False),
            ("col16", "diag", "factor", True), ("row", "diag", "dense", False)]


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("D", [5, 16, 40, 56, 72, 90, 100, 128])
@pytest.mark.parametrize("variant", VARIANTS, ids=["-".join(map(str, v)) for v in VARIANTS])
def test_every_regressor_matches_the_oracle_and_the_single_call_bit_for_bit(h, h1, D, dtype, variant):
    q = _batch(D, dtype, *variant)
    o = _outputs(q["nb"], D, dtype)
    assert _ragged(h, q, o) == 0
    mode = 1 if variant[0] == "row" else (4 if variant[0] == "col16" and D % (16 // np.dtype(dtype).itemsize) == 0 else 0)
    assert h.last_route() == f"fused_ragged_kernel<{'double' if dtype == np.float64 else 'float'}, {(D + 15) // 16}, {mode}>"
    for b in range(q["nb"]):
        res = _result(q, o, b)
        _check_oracle(q, b, res)
        _same_bits(res, _single(h1, q, b), f"regressor {b}")


@pytest.mark.parametrize("D,dtype,variant", [(40, np.float64, VARIANTS[0]), (128, np.float64, VARIANTS[3]), (16, np.float32, VARIANTS[4])])
def test_bits_do_not_depend_on_the_order_of_the_batch_or_on_the_call(h, D, dtype, variant):
    q = _batch(D, dtype, *variant)
    o = _outputs(q["nb"], D, dtype)
    o2 = _outputs(q["nb"], D, dtype)
    assert _ragged(h, q, o) == 0 and _ragged(h, q, o2) == 0
    for k in ("mw_post", "T", "A", "lp", "info"):
        assert np.array_equal(o[k], o2[k], equal_nan=True), k
    # the same regressors in another order (a fixed permutation; reversed for the second case), packed again
    nb = q["nb"]
    perm = list(range(nb))[::-1] if D == 128 else [4, 0, 8, 2, 6, 1, 7, 3, 5]
    cnt = [COUNTS[i] for i in perm]
    off = q["offsets"]
    qp = dict(q, offsets=np.concatenate(([0], np.cumsum(cnt))).astype(np.int64))
    cols = np.concatenate([np.arange(off[i], off[i + 1]) for i in perm]).astype(np.int64)
    if q["layout"] == _abi.LAYOUT_ROWVECS:
        Xp = q["X"].copy(order="F")
        Xp[:cols.size, :] = q["X"][cols, :]
    else:
        Xp = np.asfortranarray(q["X"][:, cols])
    qp["X"], qp["y"] = Xp, q["y"][cols]
    qp["s"] = q["s"][cols] if q["noise_kind"] == _abi.NOISE_DIAGONAL else (q["s"][perm] if q["strides"] else q["s"])
    if q["stridemw"]:
        qp["mw"], qp["Lw"] = q["mw"][perm], q["Lw"][perm]
    op = _outputs(nb, D, dtype)
    assert _ragged(h, qp, op) == 0
    for pos, i in enumerate(perm):
        _same_bits(_result(q, o, i), _result(qp, op, pos), f"regressor {i} at position {pos}")


@pytest.mark.parametrize("xkind,D,dtype", [("colodd", 40, np.float64), ("colpad", 40, np.float64), ("row", 24, np.float32), ("col16", 126, np.float32)])
def test_padding_is_never_read_and_gaps_are_never_written(h, xkind, D, dtype):
    """NaN in the rows beyond D of a padded ldx (RowVecs: beyond offsets[B]) and in the gaps of strided outputs"""
    q = _batch(D, dtype, xkind, "diag", "dense", False, pad_value=np.nan)
    ref = _batch(D, dtype, xkind, "diag", "dense", False, pad_value=0.0)
    o, oref = _outputs(q["nb"], D, dtype, gaps=True), _outputs(q["nb"], D, dtype, gaps=False, fill=0.0)
    assert _ragged(h, q, o) == 0 and _ragged(h, ref, oref) == 0
    assert np.all(o["info"] == 0) and np.all(np.isfinite(o["lp"]))
    written_m = np.zeros(o["mw_post"].shape, dtype=bool)
    written_T = np.zeros(o["T"].shape, dtype=bool)
    for b in range(q["nb"]):
        _same_bits(_result(q, o, b), _result(ref, oref, b), f"regressor {b}")
        written_m[b * o["stride_mwpost"]:b * o["stride_mwpost"] + D] = True
        for c in range(D):
            written_T[b * o["strideT"] + c * o["ldt"]:b * o["strideT"] + c * o["ldt"] + D] = True
    for buf, wr in ((o["mw_post"], written_m), (o["T"], written_T), (o["A"], written_T)):
        assert np.all(np.isfinite(buf[wr])) and np.all(np.isnan(buf[~wr]))


def test_one_bad_regressor_leaves_the_others_alone(h):
    D, dtype = 24, np.float64
    good = _batch(D, dtype, "col16", "diag", "diag", False)
    bad = _batch(D, dtype, "col16", "diag", "diag", False)
    bad["Lw"][3, 6] = -1.0                       # prior of regressor 3: entry 7 of the diagonal precision
    bad["s"][int(bad["offsets"][6]) + 10] = 0.0  # noise of regressor 6: observation 11
    og, ob = _outputs(good["nb"], D, dtype), _outputs(bad["nb"], D, dtype, fill=-5.0)
    assert _ragged(h, good, og) == 0 and _ragged(h, bad, ob) == 0
    assert ob["info"][3] == 7 and ob["info"][6] == 11
    for b in range(good["nb"]):
        if b in (3, 6):
            assert np.isnan(ob["lp"][b])
            m, T, _, _, _ = _result(bad, ob, b)
            assert np.all(m == -5.0) and np.all(T == -5.0)
        else:
            _same_bits(_result(good, og, b), _result(bad, ob, b), f"regressor {b}")


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_in_place_update_of_a_factor_state(h, dtype):
    D = 40
    q = _batch(D, dtype, "col16", "iso", "factor", False)
    o = _outputs(q["nb"], D, dtype)
    assert _ragged(h, q, o) == 0
    mw, Lw = q["mw"].copy(), q["Lw"].copy()
    lp, info = np.zeros(q["nb"]), np.zeros(q["nb"], dtype=np.int32)
    rc = h.posterior_ragged(dtype, _abi.MEM_HOST, q["layout"], q["nb"], D, q["offsets"], q["X"], q["ldx"], q["y"], q["noise_kind"], q["s"],
                            q["strides"], q["prior_kind"], mw, D, Lw, D, D * D, mw, D, Lw, D, D * D, None, D, D * D, lp, info)
    assert rc == 0 and np.all(info == 0)
    assert np.array_equal(lp, o["lp"])
    assert np.array_equal(mw.reshape(-1), o["mw_post"])
    assert np.array_equal(Lw.reshape(-1), o["T"])


def test_more_regressors_than_one_round_of_workgroups(h):
    """B = 3000 at D = 8: more workgroups than are resident at once"""
    D, dtype, nb = 8, np.float64, 3000
    counts = np.random.Generator(np.random.PCG64(5)).integers(0, 41, size=nb).tolist()
    q = _batch(D, dtype, "col16", "diag", "diag", False, counts=counts)
    o = _outputs(nb, D, dtype)
    assert _ragged(h, q, o) == 0
    assert np.all(o["info"] == 0)
    off = q["offsets"]
    f64 = lambda a: np.asarray(a, dtype=np.float64)  # noqa: E731
    lp_o = np.array([O.logpdf_literal(f64(q["mw"][b]), f64(q["Lw"][b]), f64(q["Xd"][:, off[b]:off[b + 1]]), f64(q["s"][off[b]:off[b + 1]]),
                                      f64(q["y"][off[b]:off[b + 1]])) for b in range(nb)])
    assert np.all(np.abs(o["lp"] - lp_o) <= 1e-10 * np.maximum(1.0, np.abs(lp_o)))
    for b in range(0, nb, 97):
        _check_oracle(q, b, _result(q, o, b))


@pytest.mark.parametrize("use_async", [False, True], ids=["sync", "async"])
def test_device_memspace_gives_the_host_memspace_bits(h, use_async):
    D, dtype = 40, np.float64
    q = _batch(D, dtype, "col16", "diag", "dense", False)
    o = _outputs(q["nb"], D, dtype)
    assert _ragged(h, q, o) == 0
    od = _outputs(q["nb"], D, dtype)
    host = dict(X=q["X"], y=q["y"], s=q["s"], mw=q["mw"], Lw=q["Lw"], mw_post=od["mw_post"], T=od["T"], A=od["A"], lp=od["lp"], info=od["info"])
    dev = {k: h.device_alloc(v.nbytes) for k, v in host.items()}
    try:
        for k, v in host.items():
            h.memcpy_h2d(dev[k], v)
        h.set_async(use_async)
        assert _ragged(h, q, od, memspace=_abi.MEM_DEVICE, arrays=dev) == 0
        if use_async:
            h.synchronize()
        for k in ("mw_post", "T", "A", "lp", "info"):
            h.memcpy_d2h(host[k], dev[k])
    finally:
        h.set_async(False)
        for p in dev.values():
            h.device_free(p)
    for k in ("mw_post", "T", "A", "lp", "info"):
        assert np.array_equal(o[k], od[k], equal_nan=True), k


def test_large_d_runs_one_regressor_after_the_other(h, h1):
    D, dtype = 130, np.float64
    q = _batch(D, dtype, "col16", "diag", "diag", False, counts=[0, 7, 140])
    o = _outputs(q["nb"], D, dtype)
    assert _ragged(h, q, o) == 0
    for b in range(q["nb"]):
        res = _result(q, o, b)
        _check_oracle(q, b, res)
        one = _single(h1, q, b)
        assert res[4] == one[4] == 0
        assert abs(res[3] - one[3]) <= 1e-10 * max(1.0, abs(one[3]))
        np.testing.assert_allclose(res[0], one[0], rtol=1e-9, atol=1e-11)
        np.testing.assert_allclose(res[1], one[1], rtol=1e-9, atol=1e-11)


def test_maps_over_problems_of_different_lengths_are_one_ragged_call():
    D, Ns = 24, [3, 50, 77, 0, 130]
    rng = np.random.Generator(np.random.PCG64(77))
    fxs, ys = [], []
    for N in Ns:
        f = B.BayesianLinearRegressor(0.2 * rng.standard_normal(D), B.Diagonal(np.exp(0.3 * rng.standard_normal(D))))
        fxs.append(f(B.ColVecs(np.asfortranarray(rng.standard_normal((D, N)))), np.exp(0.2 * rng.standard_normal(N))))
        ys.append(rng.standard_normal(N))
    lps = B.logpdf_map(fxs, ys)
    assert "fused_ragged_kernel<double, 2, 4>" == _abi.default_handle().last_route()
    posts = B.posterior_map(fxs, ys)
    assert "fused_ragged_kernel" in _abi.default_handle().last_route()
    for fx, y, lp, fp in zip(fxs, ys, lps, posts):
        assert lp == pytest.approx(B.logpdf(fx, y), rel=1e-12, abs=1e-12)
        one = B.posterior(fx, y)
        np.testing.assert_allclose(fp.mw, one.mw, rtol=1e-10, atol=1e-12)
        assert type(fp.Lw) is type(one.Lw)
        np.testing.assert_allclose(fp.Lw.toarray(), one.Lw.toarray(), rtol=1e-10, atol=1e-10)
    # the packed form gives the same numbers
    off = np.concatenate(([0], np.cumsum(Ns)))
    Xp = np.asfortranarray(np.concatenate([fx.x.X for fx in fxs], axis=1))
    lp_packed = B.logpdf_ragged([fx.f for fx in fxs], B.ColVecs(Xp), off, B.Diagonal(np.concatenate([fx.Sy for fx in fxs])), np.concatenate(ys))
    assert np.array_equal(lp_packed, np.array(lps))
    pp = B.posterior_ragged([fx.f for fx in fxs], B.ColVecs(Xp), off, B.Diagonal(np.concatenate([fx.Sy for fx in fxs])), np.concatenate(ys))
    assert all(np.array_equal(a.mw, b_.mw) for a, b_ in zip(pp, posts))
    # the first problem that is not positive definite raises, and says which one it was
    s_bad = np.ones(Ns[2])
    s_bad[4] = -1.0
    broken = list(fxs)
    broken[2] = fxs[2].f(fxs[2].x, s_bad)
    with pytest.raises(B.PosDefException) as ei:
        B.logpdf_map(broken, ys)
    assert ei.value.info == 5 and ei.value.index == 2
