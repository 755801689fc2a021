"""blr_loo_batched_x16 (loo_x16_kernel) on the GPU: 16-bit inputs against numpy float64 on the exactly widened values over a
lattice of formats, loaders, column-block counts and tile seams; to the last place on integers; status, NaN rule, chunk seams, N = 0
and both memspaces; argument errors; the Python front."""
import numpy as np
import pytest

import blr_amd as R
from blr_amd import _abi
from oracle import blr_oracle as O
from _x16_problems import EPS32, EXACT_LIMIT, XKINDS, _problem, _rel, declared_mode, features_as_integers, marg_exact_problem

pytestmark = pytest.mark.gpu
NB = 5
OUTS = ("mean", "var", "ll")
LOO_DS, LOO_NS = (8, 24, 33, 64, 88, 97, 113, 120, 127, 128), (1, 15, 16, 17, 293)


@pytest.fixture(scope="module")
def hd():
    h = _abi.Handle(0)
    yield h
    h.close()


def _lattice():
    """Every (fmt, D, layout kind) cell at one N, the noise kind alternating with the cell and the N; then N = 293 (19 tiles: a wave
    hands over a second tile) in every (fmt, layout kind) with both noise kinds."""
    rows, c = [], 0
    for f, fmt in enumerate(("bf16", "f16")):
        for D in LOO_DS:
            for xkind in XKINDS:
                rows.append((fmt, xkind, D, LOO_NS[c % 5], (c // 5 + c) % 2 == 1))
                c += 1
        rows += [(fmt, xkind, 120 if k % 2 == 0 else 127, 293, dn) for k, xkind in enumerate(XKINDS) for dn in (False, True)]
    return list(dict.fromkeys(rows))


def formula(mw, T, X, y, s, dtype):
    """include/blr_mi355x.h, blr_loo_batched_*: (loo_mean, loo_var, loo_logpdf, sigma2) of one regressor evaluated in `dtype`"""
    X, y, s = np.asfortranarray(X, dtype=dtype), y.astype(dtype), np.broadcast_to(s, y.shape).astype(dtype)
    m, sig2 = O.marginals_direct(mw.astype(dtype), T.astype(dtype), X, np.zeros(len(y), dtype))
    omh, r = (s - sig2) / s, y - m
    with np.errstate(invalid="ignore", divide="ignore"):
        out = y - r / omh, s / omh, -dtype(0.5) * (dtype(np.log(2 * np.pi)) + np.log(s) - np.log(omh) + r * r / (s * omh))
    bad = ~((omh > 0) & np.isfinite(omh))
    return tuple(np.where(bad, np.nan, o) for o in out) + (sig2,)


def fitted_problem(fmt, xkind, D, N, diag_noise):
    """_problem's features and targets; s = 2 max_n x_n'Lw^-1 x_n (times 1 .. 2 per input under diagonal noise), so that every leverage is
    at most 0.5; the state is the float64 fit on the exactly widened features, rounded to fp32."""
    q = _problem(fmt, xkind, D, N, "diag", nb=NB)
    rng = np.random.Generator(np.random.PCG64(13 * D + N))
    Xw = q["Xw"].astype(np.float64)
    s = 2.0 * np.max(np.einsum("bdn,bd->bn", Xw * Xw, 1.0 / q["Lw"].astype(np.float64)), axis=1)
    q["s"] = (s[:, None] * (1.0 + rng.random((NB, N))) if diag_noise else s).astype(np.float32)
    fits = [O.posterior_logpdf_direct(q["mw"][b].astype(np.float64), q["Lw"][b].astype(np.float64), np.asfortranarray(Xw[b]),
                                      q["s"][b].astype(np.float64), q["y"][b].astype(np.float64)) for b in range(NB)]
    q.update(noise_kind=_abi.NOISE_DIAGONAL if diag_noise else _abi.NOISE_ISOTROPIC, strides=N if diag_noise else 1,
             mw=np.stack([m for m, *_ in fits]).astype(np.float32), T=np.stack([np.triu(T).reshape(-1, order="F") for _, T, *_ in fits]).astype(np.float32),
             route=f"marg_image_kernel<float> + loo_x16_kernel<{fmt}, {declared_mode(xkind, D)}>")
    return q


def _out(N, nb=NB):
    return dict(mean=np.full((nb, N + 3), np.nan, np.float32), var=np.full((nb, N + 5), np.nan, np.float32), ll=np.full((nb, N + 1), np.nan),
                tot=np.full(nb, np.nan), info=np.full(nb, 7, np.int32))


def _call(hd, q, o, ll=True, memspace=_abi.MEM_HOST, **over):
    a = dict(q, **over)
    p = (lambda x: x.data_ptr()) if memspace == _abi.MEM_DEVICE else (lambda x: x)
    return hd.loo_batched_x16(a["xfmt"], memspace, a["layout"], a["nb"], a["D"], a["N"], p(a["X"]), a["ldx"], a["strideX"], p(a["y"]), a["y"].shape[1],
                              a["noise_kind"], p(a["s"]), a["strides"], p(a["mw"]), a["D"], p(a["T"]), a["D"], a["D"] ** 2, p(o["mean"]),
                              o["mean"].shape[1], p(o["var"]), o["var"].shape[1], p(o["ll"]) if ll else None, o["ll"].shape[1], p(o["tot"]), p(o["info"]))


def reference(q, b, dtype=np.float64):
    D, N = q["D"], q["N"]
    return formula(q["mw"][b], q["T"][b].reshape((D, D), order="F"), q["Xw"][b], q["y"][b, :N], q["s"][b], dtype)


@pytest.mark.parametrize("fmt,xkind,D,N,diag_noise", _lattice(), ids=lambda v: str(v))
def test_x16_loo_lattice_against_float64(hd, fmt, xkind, D, N, diag_noise):
    """Each output within 4 x the error numpy float32 makes on the same formula against float64, plus 4 eps32 of the output's scale (the
    rule of _x16_problems._assert_within_oracle); leverages <= 0.5.  The yardstick is non-zero and finite in every case (run on the CPU
    while this was written: 6.6e-11 .. 2.7e-5).  The sharpest case is f16-col_al-8-1-False, regressor 4, loo_mean: with
    N = 1 the scale is one value, loo_mean = -0.0770 at y = -1.897, r = -1.214, condition 11.8 against sigma2: one fp32 ulp of sigma2 is
    8.3e-7 there, above the bound of 6.3e-7 -- the kernel hands sigma2 to the epilogue unrounded and measures 3.5e-7."""
    q = fitted_problem(fmt, xkind, D, N, diag_noise)
    o = _out(N)
    _call(hd, q, o)
    assert hd.last_route() == q["route"] and np.all(o["info"] == 0)
    for b in range(NB):
        ref, f32 = reference(q, b), reference(q, b, np.float32)
        assert np.max(ref[3] / np.broadcast_to(q["s"][b], (N,))) <= 0.5
        for k, name in enumerate(OUTS):
            yard, err = _rel(f32[k], ref[k]), _rel(o[name][b, :N], ref[k])
            print(f"{q['route']} D={D} N={N} regressor {b} {name}: error {err:.3g}, float32 {yard:.3g}")
            assert f32[k].dtype == np.float32 and 0 < yard < np.inf and err <= 4 * yard + 4 * EPS32, (b, name, err, yard)
        assert abs(o["tot"][b] - np.sum(o["ll"][b, :N])) <= 1e-12 * np.sum(np.abs(o["ll"][b, :N]))
    assert all(np.all(np.isnan(o[k][:, N:])) for k in OUTS)  # nothing written behind the N outputs


def exact_problem(fmt, xkind, D, N, diag_noise):
    """marg_exact_problem (integer features and mw, T = I + a strictly upper integer matrix whose inverse is integer too: m_n and sigma2_n
    are exact integers), integer y, s a power of two above 2 max sigma2 (times 1, 2, 4 in turn per input under diagonal noise)."""
    q, _, var, big = marg_exact_problem(fmt, xkind, D, N, diag_noise, nb=NB)
    sig2 = var.astype(np.int64) - q["s"].astype(np.int64).reshape(NB, -1)
    s0 = 2.0 ** np.ceil(np.log2(2 * sig2.max() + 1))
    assert 4 * s0 < EXACT_LIMIT and big < EXACT_LIMIT and np.abs(features_as_integers(q)).max() <= 8
    q["s"] = (s0 * 2.0 ** (np.arange(NB * N).reshape(NB, N) % 3) if diag_noise else np.full(NB, s0)).astype(np.float32)
    q.update(T=q["Lw"], strides=N if diag_noise else 1)
    return q


def _ulp_close(got, ref):
    return np.all(np.abs(got.astype(np.float64) - ref) <= np.spacing(np.abs(ref).astype(np.float32)))


@pytest.mark.parametrize("diag_noise", [False, True], ids=["iso", "diagnoise"])
@pytest.mark.parametrize("D,xkind", [(97, "col_odd"), (113, "row_al"), (127, "row_odd"), (120, "col_al")])
@pytest.mark.parametrize("fmt", ["bf16", "f16"])
def test_x16_loo_exact_on_integers(hd, fmt, xkind, D, diag_noise):
    """m_n and sigma2_n are exact, so only the double epilogue rounds: loo_mean / loo_var within one fp32 ulp of numpy float64, loo_logpdf and
    the total to rtol 1e-12 (the bound tests/test_loo_gpu.py uses between its double routes); the total has the same bits without
    loo_logpdf, on a second call and at another batch position."""
    N = 293
    q = exact_problem(fmt, xkind, D, N, diag_noise)
    o, again, no_ll, rolled = (_out(N) for _ in range(4))
    _call(hd, q, o)
    _call(hd, q, again)
    _call(hd, q, no_ll, ll=False)
    roll = lambda x: np.roll(x, 1, axis=0)
    _call(hd, dict(q, X=roll(q["X"][:NB * q["strideX"]].reshape(NB, -1)).reshape(-1), **{k: roll(q[k]) for k in ("y", "s", "mw", "T")}), rolled)
    assert np.all(o["info"] == 0)
    for b in range(NB):
        ref = reference(q, b)
        assert _ulp_close(o["mean"][b, :N], ref[0]) and _ulp_close(o["var"][b, :N], ref[1]), b
        np.testing.assert_allclose(o["ll"][b, :N], ref[2], rtol=1e-12, atol=0)
    np.testing.assert_allclose(o["tot"], np.sum(o["ll"][:, :N], axis=1), rtol=1e-12, atol=0)
    assert np.all(np.isnan(no_ll["ll"]))
    for other in (again["tot"], no_ll["tot"], np.roll(rolled["tot"], -1)):
        assert np.array_equal(o["tot"].view(np.int64), other.view(np.int64))


@pytest.mark.parametrize("fmt,xkind,diag_noise", [("bf16", "col_al", True), ("f16", "row_odd", False), ("bf16", "row_al", False), ("f16", "col_odd", True)])
def test_x16_loo_status_nan_and_chunk_seams(hd, fmt, xkind, diag_noise):
    import torch
    D, N = 97, 37
    q = exact_problem(fmt, xkind, D, N, diag_noise)
    q["T"] = q["T"].copy()
    q["T"][4].reshape((D, D), order="F")[4, 4] = 0.0  # the last chunk: info = 5
    sig2 = reference(q, 1)[3]
    if diag_noise:
        q["s"][3, 6], q["s"][1, 10] = -1.0, sig2[10] / 2  # info = 7; one degenerate observation
    else:
        q["s"][3], q["s"][1] = 0.0, np.max(sig2)          # info = 1; 1 - h_n = 0 where sigma2_n is largest
    deg = np.flatnonzero(~(np.broadcast_to(q["s"][1], (N,)) - sig2 > 0))
    o, empty = _out(N), _out(0)
    before = hd.get_stat("loo_degenerate")
    hd.set_option("MAX_CHUNK", "2")
    try:
        _call(hd, q, o)
        assert hd.get_stat("last_chunks") == 3
    finally:
        hd.set_option("MAX_CHUNK", None)
    assert hd.get_stat("loo_degenerate") - before == len(deg) >= 1
    assert list(o["info"]) == [0, 0, 0, 7 if diag_noise else 1, 5]
    for b in (3, 4):  # a failed regressor keeps its sentinels
        assert all(np.all(np.isnan(o[k][b])) for k in OUTS + ("tot",))
    for k in OUTS:
        assert np.all(np.isnan(o[k][1, deg])) and not np.any(np.isnan(np.delete(o[k][1, :N], deg))) and not np.any(np.isnan(o[k][(0, 2), :N]))
    assert np.isnan(o["tot"][1]) and np.all(np.isfinite(o["tot"][[0, 2]]))
    _call(hd, q, empty, N=0)
    assert np.array_equal(empty["tot"][:3], np.zeros(3)) and list(empty["info"]) == [0, 0, 0, 0, 5]
    dev = lambda x: torch.from_numpy(x.view(np.int16) if x.dtype == np.uint16 else x).to("cuda:0")
    qd, od = dict(q, **{k: dev(q[k]) for k in ("X", "y", "s", "mw", "T")}), {k: dev(v) for k, v in _out(N).items()}
    torch.cuda.synchronize()
    _call(hd, qd, od, memspace=_abi.MEM_DEVICE)
    torch.cuda.synchronize()
    for k in OUTS + ("tot", "info"):
        assert np.array_equal(od[k].cpu().numpy(), o[k], equal_nan=True), k


@pytest.mark.parametrize("what,code", [("D129", -6), ("xfmt", -4), ("dense_noise", -13)])
def test_x16_loo_argument_errors(hd, what, code):
    q = _problem("bf16", "col_al", 129 if what == "D129" else 16, 29, "diag", nb=NB)
    q.update(T=np.tile(np.eye(q["D"], dtype=np.float32).reshape(-1), (NB, 1)), noise_kind=_abi.NOISE_ISOTROPIC, strides=1)
    o = _out(29)
    with pytest.raises(_abi.BLRError) as e:
        _call(hd, q, o, **{"dense_noise": dict(noise_kind=_abi.NOISE_DENSE), "xfmt": dict(xfmt=2)}.get(what, {}))
    assert e.value.code == code and len(str(e.value).split(":", 2)[2].strip()) > 0
    assert all(np.all(np.isnan(o[k])) for k in OUTS + ("tot",)) and np.all(o["info"] == 7)


@pytest.mark.parametrize("col", [True, False], ids=["ColVecs16", "RowVecs16"])
def test_x16_loo_python_front(col):
    """loo_map on three equally shaped problems = loo per problem, bit for bit; on a toy, loo = refitting without observation n in numpy
    float64 at the fp32 tolerances of tests/test_loo_gpu.py::test_c2_fp32."""
    rng = np.random.Generator(np.random.PCG64(5))
    D, N, s = 3, 9, 0.5
    fxs, ys, raw = [], [], []
    for fmt in ("bf16", "f16", "bf16", "bf16"):
        Xf = (rng.integers(-8, 9, size=(D, N)) / 4.0).astype(np.float32)  # exact in both formats
        X16 = R.bf16_bits(Xf) if fmt == "bf16" else Xf.astype(np.float16)
        x = R.ColVecs16(np.asfortranarray(X16), fmt) if col else R.RowVecs16(np.ascontiguousarray(X16.T), fmt)
        mw, d, y = (0.2 * rng.standard_normal(D)).astype(np.float32), np.exp(0.3 * rng.standard_normal(D)).astype(np.float32), rng.standard_normal(N).astype(np.float32)
        fxs.append(R.BayesianLinearRegressor(mw, R.Diagonal(d))(x, np.float32(s)))
        ys.append(y)
        raw.append((mw.astype(float), d.astype(float), Xf.astype(float), y.astype(float)))
    singles = [R.loo(fx, y) for fx, y in zip(fxs, ys)]
    for (mw, d, X, y), got in zip(raw[:2], singles):
        assert got.mean.dtype == got.var.dtype == np.float32 and got.logpdf.dtype == np.float64
        for n in range(N):
            keep = np.arange(N) != n
            m, T, _, _ = O.posterior_logpdf_direct(mw, d, np.asfortranarray(X[:, keep]), s, y[keep])
            pm, pv = O.marginals_direct(m, T, np.asfortranarray(X[:, n:n + 1]), s)
            lp = -0.5 * (np.log(2 * np.pi * pv[0]) + (y[n] - pm[0]) ** 2 / pv[0])
            np.testing.assert_allclose([got.mean[n], got.var[n], got.logpdf[n]], [pm[0], pv[0], lp], rtol=1e-3, atol=1e-3)
        np.testing.assert_allclose(got.total, np.sum(got.logpdf), rtol=1e-12)
    for got, k in zip(R.loo_map([fxs[0], fxs[2], fxs[3]], [ys[0], ys[2], ys[3]]), (0, 2, 3)):
        assert all(np.array_equal(a, b) for a, b in zip(got[:3], singles[k][:3])) and got.total == singles[k].total
