"""The four routes through the tall-matrix panel sweep (TallSweep<T>, blr_abi.hip; kernels in blr_tall.hpp) at the smallest shapes
where the shared launcher can go wrong, against oracle/blr_oracle.py.

D = 130: two column blocks, one trailing launch each way.  D = 300: three column blocks, trailing widths 2 then 1 forward and
2 then 1 from the other end backward.  N = 70 / 131: one / two row blocks, both ragged.  S = 5 columns.  ColVecs everywhere,
RowVecs at D = 300.  Tolerances are those of the existing test of each route in test_gpu_parity.py (named at each use).
Every output is allocated with NaN beyond the extent the library may write; the NaN must survive."""
import numpy as np
import pytest

import _tall_sweep_calls as C
from oracle import blr_oracle as O

pytestmark = pytest.mark.gpu

SHAPES = [(130, 70), (130, 131), (300, 70), (300, 131)]
DTYPES = [np.float64, np.float32]


COLVECS, ROWVECS = 0, 1  # BLR_LAYOUT_* of the C ABI (asserted against the binding in the abi fixture)


def _cases():
    out = []
    for dtype in DTYPES:
        for D, N in SHAPES:
            for layout in ([COLVECS, ROWVECS] if D == 300 else [COLVECS]):
                out.append(pytest.param(dtype, D, N, layout, id=f"{np.dtype(dtype).name}-D{D}-N{N}-{'row' if layout else 'col'}"))
    return out


@pytest.fixture(scope="module")
def abi():
    from blr_amd import _abi

    assert (_abi.LAYOUT_COLVECS, _abi.LAYOUT_ROWVECS) == (COLVECS, ROWVECS)
    _abi.default_handle()  # raises if the extension or the GPU is missing: no silent fallback
    return _abi


_PROBLEMS, _REFS = {}, {}


def _problems(dtype, D, N):
    key = (np.dtype(dtype).name, D, N)
    if key not in _PROBLEMS:
        _PROBLEMS[key] = [C.problem(dtype, D, N, 1000 * g + D + N) for g in range(3)]
    return _PROBLEMS[key]


def _ref(dtype, D, N, g):
    """the oracle's answers for regressor g of a shape, computed once in fp64 from the rounded inputs and never changed"""
    key = (np.dtype(dtype).name, D, N, g)
    if key not in _REFS:
        P = _problems(dtype, D, N)[g]
        mw, Lw, X, s = C.f64(P["mw"]), C.f64(P["Lw"]), C.f64(P["X"]), C.f64(P["s"])
        r = dict(mean=O.mean(mw, X), var=O.var(mw, Lw, X, s), grad=O.logpdf_grad(mw, Lw, X, s, C.f64(P["y"])))
        if g == 0:
            r["cov"] = O.cov(mw, Lw, X, s)
            r["lps"] = np.array([O.logpdf_literal(mw, Lw, X, s, C.f64(P["Y"][:, j])) for j in range(C.S_COLS)])
            r["means"] = np.stack([O.posterior_literal(mw, Lw, X, s, C.f64(P["Y"][:, j]))[0] for j in range(C.S_COLS)], axis=1)
        for v in r.values():
            for a in (v[1].values() if isinstance(v, tuple) else [v]):
                a.setflags(write=False)
        _REFS[key] = r
    return _REFS[key]


def _only_nan(a):
    return bool(np.all(np.isnan(a)))


@pytest.mark.parametrize("dtype,D,N", [(dt, D, N) for dt in DTYPES for D, N in SHAPES])
def test_inputs_and_oracle_are_finite(dtype, D, N):
    # checked without the library: the oracle alone gives finite values with the seeds the GPU cases use
    for g in range(3):
        P = _problems(dtype, D, N)[g]
        assert all(np.all(np.isfinite(P[k])) for k in ("X", "mw", "Lw", "U", "s", "Y"))
        assert np.all(np.diag(P["U"]) > 0)
        r = _ref(dtype, D, N, g)
        assert np.all(np.isfinite(r["mean"])) and np.all(np.isfinite(r["var"])) and np.all(r["var"] > 0)
        assert np.isfinite(r["grad"][0]) and all(np.all(np.isfinite(a)) for a in r["grad"][1].values())
        if g == 0:
            assert all(np.all(np.isfinite(r[k])) for k in ("cov", "lps", "means"))


@pytest.mark.parametrize("prior", ["dense", "factor"])
@pytest.mark.parametrize("dtype,D,N,layout", _cases())
def test_variance_marginals(abi, dtype, D, N, layout, prior):
    P, r = _problems(dtype, D, N)[0], _ref(dtype, D, N, 0)
    out = C.run_marginals(abi.default_handle(), abi, dtype, layout, P, prior)
    assert out["info"].tolist() == [0, -77]
    rt = 1e-10 if dtype == np.float64 else 3e-4  # test_large_d_marginals
    np.testing.assert_allclose(out["mean"][:N], r["mean"], rtol=rt, atol=rt * 10)
    np.testing.assert_allclose(out["var"][:N], r["var"], rtol=rt)
    assert _only_nan(out["mean"][N:]) and _only_nan(out["var"][N:])


@pytest.mark.parametrize("dtype,D,N,layout", _cases())
def test_mean_and_cov_dense_prior(abi, dtype, D, N, layout):
    P, r = _problems(dtype, D, N)[0], _ref(dtype, D, N, 0)
    out = C.run_cov(abi.default_handle(), abi, dtype, layout, P, "dense")
    assert out["info"].tolist() == [0, -77]
    Cv = out["cov"][:, :N].T
    if dtype == np.float64:
        np.testing.assert_allclose(Cv, r["cov"], rtol=1e-9, atol=1e-10)  # test_finitegp_interface_cov
        np.testing.assert_allclose(out["mean"][:N], r["mean"], rtol=1e-10, atol=1e-12)
    else:
        # no fp32 covariance test exists.  C_ij = alpha_i'alpha_j + s_i [i = j] is the marginal variance's sum with two different
        # columns, so its error is the variance's bound (3e-4 relative, test_large_d_marginals) on |alpha_i||alpha_j| <= sqrt(C_ii C_jj)
        bound = 3e-4 * np.sqrt(np.outer(np.diag(r["cov"]), np.diag(r["cov"])))
        assert np.all(np.abs(Cv - r["cov"]) <= bound)
        np.testing.assert_allclose(out["mean"][:N], r["mean"], rtol=3e-4, atol=3e-3)  # test_large_d_marginals
    assert _only_nan(out["cov"][:, N:]) and _only_nan(out["mean"][N:])


@pytest.mark.parametrize("G", [1, 3])
@pytest.mark.parametrize("with_ainv", [False, True])
@pytest.mark.parametrize("dtype,D,N,layout", _cases())
def test_logpdf_and_gradient(abi, dtype, D, N, layout, with_ainv, G):
    Ps = _problems(dtype, D, N)[:G]
    out = C.run_grad(abi.default_handle(), abi, dtype, layout, Ps, "dense", with_ainv)
    assert out["info"].tolist() == [0] * G + [-77]
    rt = 1e-8 if dtype == np.float64 else 3e-3  # test_large_d_logpdf_gradient: rtol = rt, atol = rt max|ref|, logpdf 1e-10 / 3e-4
    for g in range(G):
        lp_o, g_o = _ref(dtype, D, N, g)["grad"]
        assert out["lp"][g] == pytest.approx(lp_o, rel=1e-10 if dtype == np.float64 else 3e-4)
        dX = out["dX"][g]
        if layout == abi.LAYOUT_COLVECS:
            gX = dX[:N, :D].T
            assert _only_nan(dX[N:]) and _only_nan(dX[:, D:])
        else:
            gX = dX[:D, :N]
            assert _only_nan(dX[D:]) and _only_nan(dX[:, N:])
        pairs = [(gX, g_o["X"]), (out["dy"][g, :N], g_o["y"]), (out["ds"][g, :N], g_o["s"]), (out["dmw"][g, :D], g_o["mw"]),
                 (out["mw_post"][g, :D], g_o["mw_post"])]
        if with_ainv:
            Ai = out["Ainv"][g]
            pairs.append((Ai[:D, :D].T, g_o["Ainv"]))  # (the Lw gradient of that test is this matrix and mw_post, combined on the host)
            assert _only_nan(Ai[D:]) and _only_nan(Ai[:, D:])
        for got, ref in pairs:
            np.testing.assert_allclose(got, ref, rtol=rt, atol=rt * np.abs(ref).max())
        assert _only_nan(out["dy"][g, N:]) and _only_nan(out["ds"][g, N:]) and _only_nan(out["dmw"][g, D:]) and _only_nan(out["mw_post"][g, D:])
    assert np.isnan(out["lp"][G])


@pytest.mark.parametrize("dtype,D,N,layout", _cases())
def test_logpdf_columns_with_means(abi, dtype, D, N, layout):
    P, r = _problems(dtype, D, N)[0], _ref(dtype, D, N, 0)
    out = C.run_multi(abi.default_handle(), abi, dtype, layout, P, "dense")
    assert out["info"].tolist() == [0, -77]
    S = C.S_COLS
    rt = 1e-10 if dtype == np.float64 else 3e-4  # the multi-output test of test_gpu_parity.py: logpdf rt, means 100 rt
    np.testing.assert_allclose(out["lp"][:S], r["lps"], rtol=rt)
    np.testing.assert_allclose(out["means"][:S, :D].T, r["means"], rtol=rt * 100, atol=rt * 100)
    assert _only_nan(out["lp"][S:]) and _only_nan(out["means"][S:]) and _only_nan(out["means"][:, D:])
