"""Random-Fourier features (RandomFourierFeatures, blr_rff_features_*, blr_posterior_rff_*) on every route, against plain
high-precision references.  The routes of blr_posterior_rff_*:

  fused, chunk-staged    fp32, D > 128, D_in <= 8                 planes_kernel<*, true>, the chunk's inputs staged once (xs_chunk)
  fused, k-block staged  fp32, D > 128, 8 < D_in <= 832           planes_kernel<*, true>, a [D_in][16] LDS tile per k-block
  materialised           fp64; fp32 at D <= 128 or D_in > 832;    rff_features_kernel (16-wide D_in tiles), then the plain path
                         NO_PLANES / NO_BF16X3
  prior-mean term        fused route with mw != 0                  colstats_kernel's basis branch

fp32 inference is judged on the device's OWN features (blr_rff_features_f32: the same kernel the materialised route runs and
the same arithmetic as the planes pass), so the error of the feature map stays out of the inference check; the feature map
has its own elementwise bound.  All tests need an MI355X."""
import numpy as np
import pytest

from _yardsticks import _assert_fp32_within_lapack
from oracle import blr_oracle as O

pytestmark = pytest.mark.gpu

FUSED_MAX_DIN = 832  # kRffFusedMaxDin (csrc/blr_abi.hip): the largest D_in evaluated inside the planes pass
FUSED_LABEL = " (basis in planes pass)"


@pytest.fixture(scope="module")
def B():
    import blr_amd

    blr_amd._abi.default_handle()  # raises if the extension or the GPU is missing: no silent fallback
    return blr_amd


@pytest.fixture(scope="module")
def A(B):
    return B._abi


@pytest.fixture
def opt(B):
    """Run-time switches of the process-wide handle, restored to their defaults after the test."""
    h = B._abi.default_handle()
    touched = []

    def set_(key, value):
        h.set_option(key, value)
        touched.append(key)

    yield set_
    for key in touched:
        h.set_option(key, None)


def _rng(i=0):
    return np.random.Generator(np.random.PCG64(424242 + i))


def _padded(M, ld):
    """M (rows x cols) stored column-major with leading dimension ld >= rows; the padding rows hold NaN (a kernel that reads
    them poisons its result)."""
    P = np.full((ld, M.shape[1]), np.nan, dtype=M.dtype, order="F")
    P[: M.shape[0]] = M
    return P


# ---- the basis and its fp64 / extended-precision reference ---------------------------------------------------------
def _basis(rng, dtype, Din, D, N, omega_sd=None):
    Xin = np.asfortranarray(rng.standard_normal((Din, N)).astype(dtype))
    sd = 1.0 / np.sqrt(Din) if omega_sd is None else omega_sd  # (default: arguments of order one at any D_in)
    Om = np.asfortranarray((sd * rng.standard_normal((Din, D))).astype(dtype))
    beta = (2 * np.pi * rng.random(D)).astype(dtype)
    return Xin, Om, beta


def _phi_ref(Xin, Om, beta, scale):
    """scale cos(Omega' x + beta) from the given (rounded) inputs, in extended precision (x87 long double: u = 2^-64), and the
    magnitude |beta_f| + sum_k |omega_kf x_kn| of the argument."""
    L = np.longdouble
    arg = Om.astype(L).T @ Xin.astype(L) + beta.astype(L)[:, None]
    mag = np.abs(beta.astype(np.float64))[:, None] + np.abs(Om.astype(np.float64)).T @ np.abs(Xin.astype(np.float64))
    return L(scale) * np.cos(arg), mag


def _features(A, dtype, Xin, Om, beta, scale, ldxin=None, ldo=None):
    """blr_rff_features_* through the ABI, host memory, any leading dimensions of the inputs."""
    Din, N = Xin.shape
    D = Om.shape[1]
    Xa = Xin if ldxin is None else _padded(Xin, ldxin)
    Oa = Om if ldo is None else _padded(Om, ldo)
    Phi = np.full((D, N), np.nan, dtype=dtype, order="F")
    A.default_handle().rff_features(dtype, A.MEM_HOST, Din, D, N, Xa, Xa.shape[0], Oa, Oa.shape[0], beta, scale, Phi, D)
    return Phi


# ---- 1a. the feature map, elementwise ------------------------------------------------------------------------------
# |phi_dev - phi| <= |scale| ((D_in + 3) u (|beta_f| + sum_k |omega_kf x_kn|) + eps_cos): D_in roundings of the multiply-add
# chain, two of the reduction to revolutions (x / 2 pi and the rounded constant), one spare; eps_cos the absolute error of
# the cosine.  fp64: eps_cos = 2^-52 (cos to an ulp, the product by scale, the reference's own rounding to fp64 -- the
# reference itself is computed in long double).  fp32: eps_cos = 2^-20 is an ASSUMPTION -- the absolute error of the
# hardware cosine behind rff_cos (v_cos_f32 on the reduced revolution) is not documented to a bound; the tests print the
# largest error / bound ratio of every case, marked when it comes close to 1 (then the assumption, not the kernel, needs a look).
_U = {np.float32: 2.0 ** -24, np.float64: 2.0 ** -53}
_EPS_COS = {np.float32: 2.0 ** -20, np.float64: 2.0 ** -52}


def _close(r):
    return "  <-- close to 1: check the assumed cosine error" if r > 0.8 else ""


def _check_features(dtype, Phi, Xin, Om, beta, scale, what):
    scale_t = float(dtype(scale))  # the library rounds scale to the element type
    ref, mag = _phi_ref(Xin, Om, beta, scale_t)
    err = np.abs(Phi.astype(np.longdouble) - ref).astype(np.float64)
    Din = Xin.shape[0]
    bound = abs(scale_t) * ((Din + 3) * _U[dtype] * mag + _EPS_COS[dtype])
    assert np.all(np.isfinite(Phi)), what
    ratio = float(np.max(err / bound)) if err.size else 0.0
    i = np.unravel_index(np.argmax(err / bound), err.shape)
    assert ratio <= 1.0, (what, "largest error / bound", ratio, "at", i, err[i], bound[i])
    return ratio


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("Din", [1, 7, 8, 9, 16, 17, 33, 100, 512, 1024, 3000])
def test_feature_map_elementwise(A, dtype, Din):
    # rff_features_kernel: 32 columns per workgroup (N = 31, 32, 33), 16-wide D_in tiles in LDS (D_in = 16, 17, 33, ...),
    # 256 features per workgroup (D = 129: a ragged feature block; 256: exactly one)
    rng = _rng(100 + Din + (0 if dtype == np.float32 else 5000))
    worst = 0.0
    for D in (64, 129, 256):
        for N in (1, 31, 32, 33):
            Xin, Om, beta = _basis(rng, dtype, Din, D, N)
            scale = -np.sqrt(2.0 / D) if D == 129 else np.sqrt(2.0 / D)  # (a negative scale at one width)
            Phi = _features(A, dtype, Xin, Om, beta, scale)
            worst = max(worst, _check_features(dtype, Phi, Xin, Om, beta, scale, f"{np.dtype(dtype).name} Din={Din} D={D} N={N}"))
    print(f"feature map {np.dtype(dtype).name} D_in = {Din}: largest error / bound {worst:.3g}{_close(worst)}")


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("Din", [1, 8, 100])
def test_feature_map_short_lengthscale(A, dtype, Din):
    # Omega ~ N(0, 30^2): arguments in the hundreds, so rff_cos's reduction rev - rint(rev) does real work
    rng = _rng(200 + Din + (0 if dtype == np.float32 else 5000))
    D, N = 256, 300
    Xin, Om, beta = _basis(rng, dtype, Din, D, N, omega_sd=30.0)
    scale = np.sqrt(2.0 / D)
    Phi = _features(A, dtype, Xin, Om, beta, scale)
    arg = np.abs(Om.astype(float).T @ Xin.astype(float) + beta.astype(float)[:, None])
    assert arg.max() > 100.0
    r = _check_features(dtype, Phi, Xin, Om, beta, scale, f"short lengthscale {np.dtype(dtype).name} Din={Din}")
    print(f"feature map, short lengthscale, {np.dtype(dtype).name} D_in = {Din}: largest |argument| {arg.max():.0f}, "
          f"largest error / bound {r:.3g}{_close(r)}")


# ---- 1b. inference on every route, against the oracle --------------------------------------------------------------
def _dyadic_factor(rng, D, band):
    """Upper-banded U = 2 I + multiples of 1/16 above the diagonal: U'U is exact in fp32, so a PDMat prior U and the dense
    prior precision the oracle takes are the SAME problem in either type."""
    U = 2.0 * np.eye(D)
    for k in range(1, band + 1):
        U += np.diag(rng.integers(-4, 5, D - k) / 16.0, k)
    return U


def _problem(rng, dtype, Din, D, N, prior, noise, mean, scale_sign=1, omega_sd=None):
    Xin, Om, beta = _basis(rng, dtype, Din, D, N, omega_sd)
    scale = scale_sign * np.sqrt(2.0 / D)
    Phi64 = float(dtype(scale)) * np.cos(Om.astype(float).T @ Xin.astype(float) + beta.astype(float)[:, None])
    if noise == "iso":
        s = np.array([0.3], dtype=dtype)
    else:  # variances spanning 1e-3 .. 1e3
        s = (10.0 ** rng.uniform(-3.0, 3.0, N)).astype(dtype)
        s[0] = dtype(1e-3)
        if N > 1:
            s[-1] = dtype(1e3)
    sn = s[0] if noise == "iso" else s
    y = (Phi64.T @ rng.standard_normal(D) + np.sqrt(sn.astype(float)) * rng.standard_normal(N)).astype(dtype)
    mw = (0.1 * rng.standard_normal(D)).astype(dtype) if mean == "nonzero" else np.zeros(D, dtype=dtype)
    if prior == "diag":
        Lw_dev = np.exp(0.2 * rng.standard_normal(D)).astype(dtype)
        Lw_ref = Lw_dev
    elif prior == "dense":
        U = _dyadic_factor(rng, D, 4)
        Lw_ref = np.asfortranarray((U.T @ U).astype(dtype))
        Lw_dev = Lw_ref
    else:  # PDMat: the upper factor itself
        U = _dyadic_factor(rng, D, 3)
        Lw_dev = np.asfortranarray(U.astype(dtype))
        Lw_ref = np.asfortranarray((U.T @ U).astype(dtype))
    return dict(Xin=Xin, Om=Om, beta=beta, scale=scale, Phi64=Phi64, s=s, noise=noise, y=y, mw=mw, prior=prior,
                Lw_dev=Lw_dev, Lw_ref=Lw_ref)


def _posterior_rff(A, dtype, p, want_post, ldxin=None, ldo=None, ldt=None):
    """blr_posterior_rff_* through the ABI, host memory -> (logpdf, mw', T, Lw' or None)."""
    h = A.default_handle()
    Xin, Om = p["Xin"], p["Om"]
    Din, N = Xin.shape
    D = Om.shape[1]
    Xa = Xin if ldxin is None else _padded(Xin, ldxin)
    Oa = Om if ldo is None else _padded(Om, ldo)
    prior_kind = {"diag": A.PRIOR_DIAGONAL, "dense": A.PRIOR_DENSE, "pdmat": A.PRIOR_UPPER_FACTOR}[p["prior"]]
    ldl = 1 if p["prior"] == "diag" else D
    noise_kind = A.NOISE_ISOTROPIC if p["noise"] == "iso" else A.NOISE_DIAGONAL
    ldt = D if ldt is None else ldt
    lp = np.zeros(1, dtype=np.float64)
    info = np.full(1, -77, dtype=np.int32)
    mwp = T = Lp = None
    if want_post:
        mwp = np.full(D, np.nan, dtype=dtype)
        T = np.full((ldt, D), np.nan, dtype=dtype, order="F")
        Lp = np.full((ldt, D), np.nan, dtype=dtype, order="F") if p["prior"] != "pdmat" else None
    h.posterior_rff(dtype, A.MEM_HOST, Din, D, N, Xa, Xa.shape[0], Oa, Oa.shape[0], p["beta"], p["scale"], p["y"], noise_kind,
                    p["s"], prior_kind, p["mw"], p["Lw_dev"], ldl, mwp, T, ldt, Lp, ldt, lp, info)
    assert info[0] == 0, info
    if want_post:
        T = T[:D]
        Lp = Lp[:D] if Lp is not None else None
    return float(lp[0]), mwp, T, Lp


def _check_inference(A, dtype, p, lp, mwp, T, Lp, what, lp_only=None):
    """fp32: within 4x fp32 LAPACK on the device's own features (+ the helper's floors); fp64: the oracle at rel 1e-10."""
    D = p["Om"].shape[1]
    Apost = Lp if Lp is not None else (T.astype(np.float64).T @ T.astype(np.float64))
    if dtype == np.float32:
        Phi = np.asfortranarray(_features(A, dtype, p["Xin"], p["Om"], p["beta"], p["scale"]))
        s32 = p["s"][0] if p["noise"] == "iso" else p["s"]
        e, yard = _assert_fp32_within_lapack(p["mw"], p["Lw_ref"], Phi, s32, p["y"], mwp, Apost, lp, got_T=T, what=what)
        print(f"{what}: rel err (mw', A, logpdf) GPU {tuple(f'{x:.2e}' for x in e)}  fp32 LAPACK {tuple(f'{x:.2e}' for x in yard)}")
        if lp_only is not None:  # the evidence-only launch (no posterior outputs) against the same bound
            _assert_fp32_within_lapack(p["mw"], p["Lw_ref"], Phi, s32, p["y"], mwp, Apost, lp_only, what=what + " (logpdf only)")
        return e
    s64 = float(p["s"][0]) if p["noise"] == "iso" else p["s"].astype(float)
    mw_o, T_o, A_o, lp_o = O.posterior_logpdf_direct(p["mw"].astype(float), p["Lw_ref"].astype(float), p["Phi64"], s64,
                                                     p["y"].astype(float))
    assert lp == pytest.approx(lp_o, rel=1e-10), what
    if lp_only is not None:
        assert lp_only == pytest.approx(lp_o, rel=1e-10), what
    np.testing.assert_allclose(mwp, mw_o, rtol=1e-8, atol=1e-9 * np.abs(mw_o).max(), err_msg=what)
    np.testing.assert_allclose(Apost, A_o, rtol=1e-9, atol=1e-9 * np.abs(A_o).max(), err_msg=what)
    np.testing.assert_allclose(T.T @ T, A_o, rtol=1e-9, atol=1e-9 * np.abs(A_o).max(), err_msg=what)
    assert np.all(np.tril(T, -1) == 0)
    print(f"{what}: fp64 logpdf rel err {abs(lp - lp_o) / abs(lp_o):.2e}")
    return None


# id: dtype, D_in, D, N, prior, noise, prior mean, option, outputs, sign of scale
#   fused chunk-staged (fp32, D > 128, D_in <= 8): every D, N, prior, noise, mean, option, output set and sign of scale at least once
#   fused k-block staged (fp32, D > 128, 8 < D_in <= 832): the same
#   materialised: fp64 (D <= 128 and D > 128), fp32 D <= 128, NO_PLANES, NO_BF16X3 -- at D_in > 16
F32, F64 = np.float32, np.float64
CASES = [
    ("chunk-1", F32, 1, 129, 1, "diag", "iso", "zero", None, "logpdf", 1),
    ("chunk-2", F32, 8, 256, 15, "dense", "diag", "nonzero", "NO_FP16_PLANES", "full", -1),
    ("chunk-3", F32, 1, 1024, 1000, "pdmat", "iso", "nonzero", "PLANES8", "full", 1),
    ("chunk-4", F32, 8, 129, 17, "diag", "diag", "zero", None, "full", -1),
    ("chunk-5", F32, 1, 256, 16, "dense", "iso", "zero", "PLANES8", "logpdf", -1),
    ("chunk-6", F32, 8, 1024, 4127, "pdmat", "diag", "nonzero", "NO_FP16_PLANES", "logpdf", 1),
    ("chunk-7", F32, 8, 256, 4127, "diag", "diag", "nonzero", None, "full", 1),
    ("kblock-1", F32, 9, 129, 1, "pdmat", "diag", "nonzero", "PLANES8", "full", -1),
    ("kblock-2", F32, 17, 256, 15, "diag", "iso", "zero", None, "full", 1),
    ("kblock-3", F32, 100, 1024, 16, "dense", "diag", "nonzero", "NO_FP16_PLANES", "logpdf", -1),
    ("kblock-4", F32, 512, 129, 17, "dense", "iso", "nonzero", None, "full", 1),
    ("kblock-5", F32, 9, 256, 1000, "pdmat", "iso", "zero", "NO_FP16_PLANES", "full", 1),
    ("kblock-6", F32, 17, 1024, 4127, "diag", "diag", "zero", "PLANES8", "logpdf", -1),
    ("kblock-7", F32, 100, 256, 4127, "diag", "diag", "nonzero", None, "full", -1),
    ("kblock-8", F32, 512, 256, 1000, "pdmat", "diag", "nonzero", None, "logpdf", 1),
    ("mat-f64-small", F64, 17, 96, 300, "diag", "diag", "nonzero", None, "full", 1),
    ("mat-f64-dense", F64, 100, 200, 500, "dense", "iso", "zero", None, "logpdf", -1),
    ("mat-f64-pdmat", F64, 3000, 129, 64, "pdmat", "diag", "nonzero", None, "full", 1),
    ("mat-f64-512", F64, 512, 256, 1000, "diag", "iso", "nonzero", None, "full", -1),
    ("mat-f32-small", F32, 33, 128, 500, "diag", "iso", "nonzero", None, "full", 1),
    ("mat-f32-small-pdmat", F32, 17, 64, 1, "pdmat", "diag", "zero", None, "full", -1),
    ("mat-f32-no-planes", F32, 100, 256, 1000, "pdmat", "diag", "nonzero", "NO_PLANES", "full", 1),
    ("mat-f32-no-bf16x3", F32, 17, 129, 17, "dense", "iso", "zero", "NO_BF16X3", "logpdf", -1),
]


def _route_kind(dtype, Din, D, option):
    if dtype == np.float32 and D > 128 and Din <= FUSED_MAX_DIN and option not in ("NO_PLANES", "NO_BF16X3"):
        return "fused"
    return "materialised"


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_inference_routes(A, opt, case):
    name, dtype, Din, D, N, prior, noise, mean, option, outputs, sign = case
    if option:
        opt(option, "1")
    rng = _rng(300 + sum(map(ord, name)))
    p = _problem(rng, dtype, Din, D, N, prior, noise, mean, sign)
    lp_only = None
    if outputs == "logpdf":
        lp_only, _, _, _ = _posterior_rff(A, dtype, p, want_post=False)
    lp, mwp, T, Lp = _posterior_rff(A, dtype, p, want_post=True)
    route = A.default_handle().last_route()
    kind = _route_kind(dtype, Din, D, option)
    assert (FUSED_LABEL in route) == (kind == "fused"), (name, route)
    if kind == "fused":  # (the option reached the Gram launch)
        want = {"NO_FP16_PLANES": "gram_planes_kernel<3>", "PLANES8": "gram_planes_kernel<2>"}.get(option, "gram_planes4_kernel")
        assert route == want + FUSED_LABEL, (name, route)
    _check_inference(A, dtype, p, lp, mwp, T, Lp, f"{name} [{route}]", lp_only)


@pytest.mark.timeout(900)
def test_inference_chunk_filling(A):
    # D = 1024, N = 65531: every planes workgroup gets the full 64 k-blocks (the most LDS the chunk-staged branch uses), the
    # last k-block holds 11 columns
    rng = _rng(400)
    p = _problem(rng, F32, 8, 1024, 65531, "diag", "diag", "nonzero")
    lp, mwp, T, Lp = _posterior_rff(A, F32, p, want_post=True)
    route = A.default_handle().last_route()
    assert route == "gram_planes4_kernel" + FUSED_LABEL, route
    _check_inference(A, F32, p, lp, mwp, T, Lp, f"chunk filling [{route}]")


# ---- 1c. bit identities ----------------------------------------------------------------------------------------------
# (dtype, D_in, D, option): both fused branches, the fp64 and fp32 materialised routes, NO_PLANES
BIT_ROUTES = [(F32, 5, 256, None), (F32, 40, 256, None), (F32, 40, 256, "NO_FP16_PLANES"), (F64, 40, 256, None),
              (F32, 40, 100, None), (F64, 20, 100, None), (F32, 40, 256, "NO_PLANES"), (F32, 1000, 256, None)]


@pytest.mark.parametrize("dtype,Din,D,option", BIT_ROUTES, ids=[f"{np.dtype(r[0]).name}-Din{r[1]}-D{r[2]}-{r[3]}" for r in BIT_ROUTES])
def test_padded_and_repeated_calls_bit_identical(A, opt, dtype, Din, D, option):
    # ldxin = D_in + 3, ldo = D_in + 5 (padding rows hold NaN) give the unpadded call's bits, and so does the same call again
    if option:
        opt(option, "1")
    rng = _rng(500 + Din + D)
    p = _problem(rng, dtype, Din, D, 700, "diag", "diag", "nonzero")
    base = _posterior_rff(A, dtype, p, want_post=True)
    again = _posterior_rff(A, dtype, p, want_post=True)
    padded = _posterior_rff(A, dtype, p, want_post=True, ldxin=Din + 3, ldo=Din + 5, ldt=D + 2)
    for other, what in ((again, "repeated"), (padded, "padded")):
        assert other[0] == base[0], (what, other[0], base[0])
        for x, y in zip(base[1:], other[1:]):
            if x is not None:
                np.testing.assert_array_equal(x, y, err_msg=what)
    Phi = _features(A, dtype, p["Xin"], p["Om"], p["beta"], p["scale"])
    np.testing.assert_array_equal(_features(A, dtype, p["Xin"], p["Om"], p["beta"], p["scale"]), Phi)
    np.testing.assert_array_equal(_features(A, dtype, p["Xin"], p["Om"], p["beta"], p["scale"], ldxin=Din + 3, ldo=Din + 5), Phi)


@pytest.mark.parametrize("dtype,Din,D,option", BIT_ROUTES[:4] + BIT_ROUTES[-1:],
                         ids=[f"{np.dtype(r[0]).name}-Din{r[1]}-D{r[2]}-{r[3]}" for r in BIT_ROUTES[:4] + BIT_ROUTES[-1:]])
def test_host_and_device_memspace_bit_identical(A, opt, dtype, Din, D, option):
    import torch

    if option:
        opt(option, "1")
    h = A.default_handle()
    dev = torch.device("cuda:0")
    rng = _rng(600 + Din + D)
    N = 700
    p = _problem(rng, dtype, Din, D, N, "dense", "iso", "nonzero")
    lp_h, mw_h, T_h, L_h = _posterior_rff(A, dtype, p, want_post=True)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a).T if np.ndim(a) == 2 else a)).to(dev)  # column-major
    Xd, Od, bd, yd, sd, mwd, Lwd = (t(p[k]) for k in ("Xin", "Om", "beta", "y", "s", "mw", "Lw_dev"))
    tdt = torch.float64 if dtype == np.float64 else torch.float32
    mwp = torch.full((D,), float("nan"), dtype=tdt, device=dev)
    Tp = torch.full((D, D), float("nan"), dtype=tdt, device=dev)
    Lp = torch.full((D, D), float("nan"), dtype=tdt, device=dev)
    lp = torch.zeros((1,), dtype=torch.float64, device=dev)
    info = torch.full((1,), -77, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()  # (the fills above run on torch's stream, the library on its own non-blocking one)
    h.posterior_rff(dtype, A.MEM_DEVICE, Din, D, N, Xd.data_ptr(), Din, Od.data_ptr(), Din, bd.data_ptr(), p["scale"],
                    yd.data_ptr(), A.NOISE_ISOTROPIC, sd.data_ptr(), A.PRIOR_DENSE, mwd.data_ptr(), Lwd.data_ptr(), D,
                    mwp.data_ptr(), Tp.data_ptr(), D, Lp.data_ptr(), D, lp.data_ptr(), info.data_ptr())
    h.synchronize()
    assert int(info.cpu()[0]) == 0
    assert float(lp.cpu()[0]) == lp_h
    np.testing.assert_array_equal(mwp.cpu().numpy(), mw_h)
    np.testing.assert_array_equal(Tp.cpu().numpy().T, T_h)
    np.testing.assert_array_equal(Lp.cpu().numpy().T, L_h)
    Phi = torch.full((N, D), float("nan"), dtype=tdt, device=dev)
    torch.cuda.synchronize()
    h.rff_features(dtype, A.MEM_DEVICE, Din, D, N, Xd.data_ptr(), Din, Od.data_ptr(), Din, bd.data_ptr(), p["scale"],
                   Phi.data_ptr(), D)
    h.synchronize()
    np.testing.assert_array_equal(Phi.cpu().numpy().T, _features(A, dtype, p["Xin"], p["Om"], p["beta"], p["scale"]))


@pytest.mark.parametrize("mean", ["zero", "nonzero"])
@pytest.mark.parametrize("Din", [8, 9, 17, 100, 512])
def test_fused_equals_blr_on_device_features(B, Din, mean):
    # test_rff_basis_config5_family's BFR == BLR o phi at its fp32 shape (D = 512, N = 2048), on both fused branches: the planes
    # pass evaluates the features with rff_features_kernel's arithmetic and picks the same power-of-two row scales, so the
    # posterior mean and precision are the same bits.  The evidence is too with a zero prior mean.  With a non-zero one the
    # two routes take different branches of colstats_kernel (the basis branch: one column per wave; the materialised features:
    # two per wave), which group the fp64 partial sums of q = sum_n delta_n^2 / s_n and of sum_n log s_n differently over the
    # workgroup's threads -- the evidence may then differ by the rounding of those two sums (one ulp at D_in = 9 and 17).
    rng = _rng(700 + Din)
    D, N = 512, 2048
    Xin, Om, beta = _basis(rng, np.float32, Din, D, N)
    rff = B.RandomFourierFeatures(Om, beta)
    Phi = rff(B.ColVecs(Xin)).X
    s = np.exp(0.3 * rng.standard_normal(N)).astype(np.float32)
    y = (Phi.astype(float).T @ rng.standard_normal(D) + np.sqrt(s) * rng.standard_normal(N)).astype(np.float32)
    mw = (0.1 * rng.standard_normal(D)).astype(np.float32) if mean == "nonzero" else np.zeros(D, dtype=np.float32)
    blr = B.BayesianLinearRegressor(mw, B.Diagonal(np.ones(D, dtype=np.float32)))
    fx = B.BasisFunctionRegressor(blr, rff)(B.ColVecs(Xin), s)
    gx = blr(B.ColVecs(np.asfortranarray(Phi)), s)
    lp = B.logpdf(fx, y)
    assert FUSED_LABEL in B._abi.default_handle().last_route()
    lp_phi = B.logpdf(gx, y)
    p_f, p_m = B.posterior(fx, y), B.posterior(gx, y)
    np.testing.assert_array_equal(p_f.blr.mw, p_m.mw)
    np.testing.assert_array_equal(p_f.blr.Lw.toarray(), p_m.Lw.toarray())
    if mean == "zero":
        assert lp == lp_phi, (lp, lp_phi)
    else:
        # two groupings of the same fp64 terms: each sum is within (N - 1) u64 sum |terms| of the exact one
        delta = y.astype(float) - Phi.astype(float).T @ mw.astype(float)
        terms = float(np.sum(delta * delta / s.astype(float)) + np.sum(np.abs(np.log(s.astype(float)))))
        bound = (N - 1) * 2.0 ** -53 * terms
        print(f"BFR vs BLR o phi, D_in = {Din}: evidence differs by {abs(lp - lp_phi):.2e} (bound of the regrouped sums {bound:.2e})")
        assert abs(lp - lp_phi) <= bound, (lp, lp_phi, bound)


# ---- 1d. D_in straddling the fused limit -----------------------------------------------------------------------------
@pytest.mark.parametrize("Din", [FUSED_MAX_DIN, FUSED_MAX_DIN + 1, 1024, 3000])
def test_straddle_fused_limit(A, Din):
    # up to kRffFusedMaxDin the planes pass evaluates the basis ([D_in][16] floats of LDS per k-block beside 12 KiB); above it
    # the features are materialised.  A launch beyond the kernel's LDS limit must never come back as a posterior.
    rng = _rng(800 + Din)
    p = _problem(rng, F32, Din, 256, 500, "diag", "diag", "nonzero")
    lp, mwp, T, Lp = _posterior_rff(A, F32, p, want_post=True)
    route = A.default_handle().last_route()
    if Din <= FUSED_MAX_DIN:
        assert route == "gram_planes4_kernel" + FUSED_LABEL, route
    else:
        assert route == "gram_planes4_kernel", route  # the planes Gram on materialised features
    _check_inference(A, F32, p, lp, mwp, T, Lp, f"straddle Din={Din} [{route}]")


# ---- 1e. resident state --------------------------------------------------------------------------------------------------
def test_resident_basis_condition_loo_forget(B, A):
    rng = _rng(900)
    Din, D, N, k = 100, 256, 600, 100
    Xin, Om, beta = _basis(rng, np.float32, Din, D, N)
    rff = B.RandomFourierFeatures(Om, beta)
    Phi = np.asfortranarray(rff(B.ColVecs(Xin)).X)  # the device's own features
    s = np.float32(0.3)
    y = (Phi.astype(float).T @ rng.standard_normal(D) + np.sqrt(0.3) * rng.standard_normal(N)).astype(np.float32)
    mw = (0.1 * rng.standard_normal(D)).astype(np.float32)
    dvec = np.exp(0.2 * rng.standard_normal(D)).astype(np.float32)
    bfr = B.BasisFunctionRegressor(B.BayesianLinearRegressor(mw, B.Diagonal(dvec)), rff)
    st = B.ResidentPosterior(bfr)
    lp = st.condition(B.ColVecs(Xin), s, y)

    def state():
        r = st.regressor()
        r = r.blr if isinstance(r, B.BasisFunctionRegressor) else r
        T = np.asarray(r.Lw.U)
        return r.mw, T, T.astype(float).T @ T.astype(float)

    mwp, T, Ap = state()
    _assert_fp32_within_lapack(mw, dvec, Phi, s, y, mwp, Ap, lp, got_T=T, what="resident condition")
    # the same data through the fused posterior: both inside the yardstick
    post = B.posterior(bfr(B.ColVecs(Xin), s), y)
    lp_f = B.logpdf(bfr(B.ColVecs(Xin), s), y)
    _assert_fp32_within_lapack(mw, dvec, Phi, s, y, post.blr.mw, post.blr.Lw.toarray(), lp_f, what="resident: posterior")

    # leave-one-out: against the fp64 N x N formula on the same features; bound 4x the same formula in fp32 LAPACK
    r = st.loo(B.ColVecs(Xin), s, y)
    K = lambda dt: (Phi.astype(dt).T @ (Phi.astype(dt) / dvec.astype(dt)[:, None]) + dt(s) * np.eye(N, dtype=dt))

    def loo_lp(dt):
        Ki = np.linalg.inv(K(dt))
        d = np.diag(Ki)
        a = Ki @ (y.astype(dt) - Phi.astype(dt).T @ mw.astype(dt))
        var, res = 1 / d, a / d
        return -0.5 * (np.log(2 * np.pi) + np.log(var.astype(float)) + res.astype(float) ** 2 / var.astype(float))

    lo64, lo32 = loo_lp(np.float64), loo_lp(np.float32)
    e_dev, e_32 = np.max(np.abs(np.asarray(r.logpdf) - lo64)), np.max(np.abs(lo32 - lo64))
    floor = 4 * np.finfo(np.float32).eps * np.max(np.abs(lo64))
    print(f"resident loo: max abs err of the LOO log densities GPU {e_dev:.2e}  fp32 LAPACK {e_32:.2e}")
    assert e_dev <= 4 * e_32 + floor, (e_dev, e_32, floor)

    # forget the last k observations: the state is the posterior of the first N - k, and the returned density is
    # log p(y_removed | y_kept) = logpdf(all) - logpdf(kept)
    lp_rm = st.forget(B.ColVecs(np.asfortranarray(Xin[:, N - k:])), s, y[N - k:])
    mwp, T, Ap = state()
    Pk = np.asfortranarray(Phi[:, : N - k])
    _assert_fp32_within_lapack(mw, dvec, Pk, s, y[: N - k], mwp, Ap, lp - lp_rm, got_T=T, what="resident forget")
    f64 = lambda a: np.asarray(a, dtype=np.float64)
    lp_all32 = O.logpdf_literal(mw, dvec, Phi, s, y)
    lp_kept32 = O.logpdf_literal(mw, dvec, Pk, s, y[: N - k])
    s64 = float(s)
    lp_all = O.logpdf_literal(f64(mw), f64(dvec), f64(Phi), s64, f64(y))
    lp_kept = O.logpdf_literal(f64(mw), f64(dvec), f64(Pk), s64, f64(y[: N - k]))
    e_rm = abs(lp_rm - (lp_all - lp_kept))
    yard = abs(lp_all32 - lp_all) + abs(lp_kept32 - lp_kept)
    floor = 4 * np.finfo(np.float32).eps * (abs(lp_all) + abs(lp_kept))
    print(f"resident forget: log p(y_removed | y_kept) abs err GPU {e_rm:.2e}  fp32 LAPACK {yard:.2e}")
    assert e_rm <= 4 * yard + floor, (e_rm, yard, floor)
