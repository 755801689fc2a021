"""fused_i8_kernel reads y (and 1 / sqrt(s_n) under diagonal noise) of a wave's column octet with scalar loads into SGPRs
(blr_fused_i8.hpp, I8SliceSteps).  Here y and s are views into larger device buffers -- batch stride N + 3 doubles, first element at
offset 1 -- so the 64-byte scalar loads straddle cache lines and are only 8-byte aligned, and the gaps hold NaN: a load that reaches
beyond its regressor's values and into a result shows up as NaN.  N = 512 (the route's smallest), 543 (a partial last block), 544
(nk = 17, odd), 1056 (nk = 33).  Every case: the int8 route with no hand-back, info 0, and mw', T, logpdf against the same call on the
fp64 kernel (NO_I8_GRAM) within the bounds of test_i8_gram_path_vs_oracle_and_fp64_kernel (tests/test_gpu_parity.py)."""
import numpy as np
import pytest

from blr_amd import _abi

pytestmark = pytest.mark.gpu

D, NB = 128, 3


@pytest.fixture(scope="module")
def hd():
    h = _abi.Handle()
    yield h
    h.close()


def _padded(torch, vals, dev):
    """[NB, N] values as a view into a NaN-filled buffer: batch stride N + 3, first element at offset 1"""
    nb, N = vals.shape
    buf = torch.full((nb * (N + 3) + 8,), float("nan"), dtype=torch.float64, device=dev)
    view = buf[1:1 + nb * (N + 3)].view(nb, N + 3)[:, :N]
    view.copy_(torch.tensor(vals, dtype=torch.float64))
    return buf, view


@pytest.mark.parametrize("prior_mean", [False, True], ids=["mw0", "mw"])
@pytest.mark.parametrize("layout", ["col", "row"])
@pytest.mark.parametrize("noise", ["iso", "diag"])
@pytest.mark.parametrize("N", [512, 543, 544, 1056])
def test_scalar_y_on_unaligned_nan_padded_views(hd, N, noise, layout, prior_mean):
    import torch

    h, a = hd, _abi
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(7100 + N)
    X = rng.standard_normal((NB, N, D))  # [b, n, d]: D x N ColVecs per regressor
    w = rng.standard_normal((NB, D))
    y = np.einsum("bnd,bd->bn", X, w) + np.sqrt(0.1) * rng.standard_normal((NB, N))
    mw = rng.standard_normal((NB, D)) if prior_mean else np.zeros((NB, D))
    lam = np.exp(0.3 * rng.standard_normal((NB, D)))
    ybuf, yv = _padded(torch, y, dev)
    if noise == "diag":
        s = np.exp(rng.standard_normal((NB, N)))
        sbuf, sv = _padded(torch, s, dev)
        nk, sptr, ss = a.NOISE_DIAGONAL, sv.data_ptr(), N + 3
    else:
        s = np.full((NB, N), 0.1)
        sbuf = torch.tensor([0.1], dtype=torch.float64, device=dev)
        nk, sptr, ss = a.NOISE_ISOTROPIC, sbuf.data_ptr(), 0
    assert yv.data_ptr() % 64 == 8 and yv.stride(0) == N + 3
    if layout == "col":
        Xd = torch.tensor(X, dtype=torch.float64, device=dev)
        lay, ldx, sx = a.LAYOUT_COLVECS, D, N * D
    else:
        ld = N + (N & 1)
        Xr = np.zeros((NB, D, ld))
        Xr[:, :, :N] = X.transpose(0, 2, 1)
        Xd = torch.tensor(Xr, dtype=torch.float64, device=dev)
        lay, ldx, sx = a.LAYOUT_ROWVECS, ld, D * ld
    mwd = torch.tensor(mw, dtype=torch.float64, device=dev)
    lamd = torch.tensor(lam, dtype=torch.float64, device=dev)

    def run():
        mp = torch.full((NB, D), 7.0, dtype=torch.float64, device=dev)
        Tp = torch.full((NB, D, D), 7.0, dtype=torch.float64, device=dev)
        Ap = torch.full((NB, D, D), 7.0, dtype=torch.float64, device=dev)
        lp = torch.zeros(NB, dtype=torch.float64, device=dev)
        info = torch.full((NB,), 9, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        h.posterior_batched(np.float64, a.MEM_DEVICE, lay, NB, D, N, Xd.data_ptr(), ldx, sx, yv.data_ptr(), N + 3, nk, sptr, ss,
                            a.PRIOR_DIAGONAL, mwd.data_ptr(), D, lamd.data_ptr(), 1, D, mp.data_ptr(), D, Tp.data_ptr(), D, D * D,
                            Ap.data_ptr(), D, D * D, lp.data_ptr(), info.data_ptr())
        torch.cuda.synchronize()
        return mp.cpu().numpy(), Tp.cpu().numpy(), lp.cpu().numpy(), info.cpu().numpy()

    h.set_option("NO_I8_GRAM", None)
    try:
        h.reset_stats()
        fast = run()
        assert h.last_route() == "fused_i8_kernel"
        assert h.get_stat("i8_regressors") == NB and h.get_stat("i8_handed_back") == 0
        h.set_option("NO_I8_GRAM", "1")
        slow = run()
        assert h.last_route().startswith("fused_small_kernel<double, 8,")
    finally:
        h.set_option("NO_I8_GRAM", None)
    assert fast[3].tolist() == [0] * NB and slow[3].tolist() == [0] * NB
    for b in range(NB):
        for out in fast[:3]:
            assert np.all(np.isfinite(out[b]))
        Ts = np.triu(slow[1][b].T)  # (column-major upper factor)
        Tf = np.triu(fast[1][b].T)
        A_s = Ts.T @ Ts
        dA = np.sqrt(np.diag(A_s))
        dlt = y[b] - X[b] @ mw[b]
        lp_tol = 1e-11 * abs(slow[2][b]) + 1e-14 * float(np.sum(dlt * dlt / s[b]))
        dlp = abs(fast[2][b] - slow[2][b])
        dmw = np.abs((fast[0][b] - slow[0][b]) * dA).max()
        dT = (np.abs(Tf.T @ Tf - A_s) / np.outer(dA, dA)).max()
        print(f"N {N} {noise} {layout} mw {prior_mean} regressor {b}: |dlogpdf| {dlp:.3e} (bound {lp_tol:.3e}), |dmw| {dmw:.3e} "
              f"(bound {1e-10 * np.abs(slow[0][b] * dA).max():.3e}), T'T {dT:.3e} (bound 1e-10)")
        assert dlp <= lp_tol
        assert dmw <= 1e-10 * np.abs(slow[0][b] * dA).max()
        assert dT <= 1e-10
