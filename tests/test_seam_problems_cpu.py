"""tests/_seam_problems.py's vectorised fp64 references against oracle/ on the first 16 regressors of the batch shape the
grid.y seam tests use (D = 3, N = 5): the GPU tests compare 65537 regressors with the restatement, this file ties it to the oracle."""
import numpy as np

import _seam_problems as SP
from oracle import blr_oracle as O

NB, D, N, S = 16, 3, 5, 2


def _batch():
    return SP.batch(NB, D, N, S, seed=65537)


def test_marginals_restatement_matches_the_oracle():
    p = _batch()
    mean, var = SP.marginals_ref(p["X"], p["M"], p["U"], p["s"])
    dprec = 0.5 + np.abs(p["mw"])
    mean_d, var_d = SP.diag_marginals_ref(p["X"], p["M"], dprec, p["s"])
    for b in range(NB):
        Xb, Ub = p["X"][b].T, SP.upper(p)[b]
        for c in range(S):
            m_o, v_o = O.marginals_direct(p["M"][b, c], Ub, Xb, p["s"][b])
            np.testing.assert_allclose(mean[b, c], m_o, rtol=1e-13, atol=1e-14)
            np.testing.assert_allclose(var[b], v_o, rtol=1e-13)
        np.testing.assert_allclose(var[b], O.var(p["mw"][b], Ub.T @ Ub, Xb, p["s"][b]), rtol=1e-12)
        np.testing.assert_allclose(var_d[b], O.var(p["mw"][b], dprec[b], Xb, p["s"][b]), rtol=1e-13)
        np.testing.assert_allclose(mean_d[b, 0], O.mean(p["M"][b, 0], Xb), rtol=1e-13, atol=1e-14)


def test_conditioned_states_and_loo_restatement_match_the_oracle():
    p = _batch()
    Mpost, T = SP.condition(p, p["Y"])
    mean, var, lp, tot = SP.loo_ref(p["X"], Mpost, T, p["s"], p["Y"])
    for b in range(NB):
        Xb, Ub = p["X"][b].T, SP.upper(p)[b]
        Lw = Ub.T @ Ub
        K = Xb.T @ np.linalg.solve(Lw, Xb) + np.diag(p["s"][b])
        Ki = np.linalg.inv((K + K.T) / 2)
        for c in range(S):
            m_o, T_o, _, _ = O.posterior_logpdf_direct(p["M"][b, c], None, Xb, p["s"][b], p["Y"][b, c], prior_factor=Ub)
            np.testing.assert_allclose(Mpost[b, c], m_o, rtol=1e-11, atol=1e-12)
            np.testing.assert_allclose(T[b].T, T_o, rtol=1e-11, atol=1e-13)
            # R&W eq. 5.12 on the N x N system: [K^-1]_nn and [K^-1 (y - X'mw)]_n
            a = Ki @ (p["Y"][b, c] - Xb.T @ p["M"][b, c])
            v_o = 1.0 / np.diag(Ki)
            m_loo = p["Y"][b, c] - a * v_o
            l_o = -0.5 * (SP.LOG2PI + np.log(v_o) + (p["Y"][b, c] - m_loo) ** 2 / v_o)
            np.testing.assert_allclose(var[b], v_o, rtol=1e-10)
            np.testing.assert_allclose(mean[b, c], m_loo, rtol=1e-9, atol=1e-10)
            np.testing.assert_allclose(lp[b, c], l_o, rtol=1e-9, atol=1e-10)
            np.testing.assert_allclose(tot[b, c], l_o.sum(), rtol=1e-9)


def test_gradient_restatement_matches_the_oracle():
    p = _batch()
    lp, dX, dy, ds, dmw, mwp = SP.grad_ref(p["X"], p["y"], p["s"], p["mw"], p["U"])
    for b in range(NB):
        Xb, Ub = p["X"][b].T, SP.upper(p)[b]
        lp_o, g = O.logpdf_grad(p["mw"][b], Ub.T @ Ub, Xb, p["s"][b], p["y"][b])
        assert abs(lp[b] - lp_o) <= 1e-12 * max(1.0, abs(lp_o))
        for got, ref in ((dX[b].T, g["X"]), (dy[b], g["y"]), (ds[b], g["s"]), (dmw[b], g["mw"]), (mwp[b], g["mw_post"])):
            np.testing.assert_allclose(got, ref, rtol=1e-10, atol=1e-12 * max(1.0, np.abs(ref).max()))


def test_out_keeps_payload_and_gaps_apart():
    o = SP.Out(np.float64, 4, cols=3, nb=2)
    assert o.ld == 7 and o.stride == 2 * 7 + 4 + 3 and o.gaps_kept(o.a)
    a = o.a.copy()
    a[o.idx.ravel()] = 1.0
    assert o.gaps_kept(a) and o.payload(a).shape == (2, 3, 4) and o.per_regressor(a).shape == (2, 3, 4)
    a[4] = 0.0
    assert not o.gaps_kept(a)
