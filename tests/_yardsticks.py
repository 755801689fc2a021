"""Yardsticks of the GPU tests: fp32 results are judged against the fp64 oracle run on the same fp32-rounded inputs, with a bound
of 4x the error fp32 LAPACK makes on them (tests/test_gpu_parity.py, tests/test_rff_gpu.py).  A plain module, not a conftest."""
import numpy as np

from oracle import blr_oracle as O


def _rel_errs(mw, A, lp, mw_o, A_o, lp_o):
    """(posterior mean: relative 2-norm; posterior precision: max abs over max abs; log evidence: relative)"""
    return (float(np.linalg.norm(np.asarray(mw, float) - mw_o) / np.linalg.norm(mw_o)),
            float(np.max(np.abs(np.asarray(A, float) - A_o)) / np.max(np.abs(A_o))),
            abs(float(lp) - lp_o) / abs(lp_o))


def _fp32_lapack_yardstick(mw32, d32, X32, s32, y32, mw_o, A_o, lp_o):
    """errors of fp32 LAPACK on the same inputs: max over the literal sequence and the direct form"""
    m_d, T_d, A_d, lp_d = O.posterior_logpdf_direct(mw32, d32, X32, s32, y32)  # dtype follows X: sgemm / spotrf / strtrs
    e_direct = _rel_errs(m_d, A_d, lp_d, mw_o, A_o, lp_o)
    m_l, T_l, A_l = O.posterior_literal(mw32, d32, X32, s32, y32)
    lp_l = O.logpdf_literal(mw32, d32, X32, s32, y32)
    e_lit = _rel_errs(m_l, A_l, lp_l, mw_o, A_o, lp_o)
    assert m_d.dtype == np.float32 and A_l.dtype == np.float32
    return tuple(max(a, b) for a, b in zip(e_direct, e_lit)), e_direct, e_lit


def _assert_fp32_within_lapack(mw32, Lw32, X32, s32, y32, got_mw, got_A, got_lp, got_T=None, floor=(2e-6, 5e-7, 2e-7),
                               what=""):
    """fp32 results against the fp64 oracle run on the SAME fp32-rounded inputs; bound = 4x the error fp32 LAPACK makes on
    them with the reference's own op sequence (:72-89) -- nothing hand-picked but the floor of a few fp32 ulps that covers
    problems LAPACK happens to solve exactly (N = 0, N = 1).  Lw32: diagonal (1-D) or dense (2-D) prior precision; s32:
    scalar / vector / dense matrix, as the oracle takes them.  Returns (gpu errors, yardstick)."""
    f64 = lambda a: np.asarray(a, dtype=np.float64)
    for a32 in (mw32, Lw32, X32, y32):
        assert np.asarray(a32).dtype == np.float32
    mw_o, T_o, A_o = O.posterior_literal(f64(mw32), f64(Lw32), f64(X32), f64(s32), f64(y32))
    lp_o = O.logpdf_literal(f64(mw32), f64(Lw32), f64(X32), f64(s32), f64(y32))
    m_l, _, A_l = O.posterior_literal(mw32, Lw32, X32, np.asarray(s32, dtype=np.float32), y32)
    lp_l = O.logpdf_literal(mw32, Lw32, X32, np.asarray(s32, dtype=np.float32), y32)
    assert m_l.dtype == np.float32 and A_l.dtype == np.float32
    lp_ref = lp_o if abs(lp_o) >= 1.0 else float(np.copysign(1.0, lp_o))  # an evidence near 0 (no data) is judged absolutely
    errs = lambda m, A, lp: _rel_errs(m, A, lp_ref + (float(lp) - lp_o), mw_o, A_o, lp_ref)
    yard = errs(m_l, A_l, lp_l)
    if np.ndim(s32) < 2:  # the one-pass Gram form in fp32 LAPACK as well (diagonal / isotropic noise only)
        m_d, _, A_d, lp_d = O.posterior_logpdf_direct(mw32, Lw32, X32, np.asarray(s32, dtype=np.float32), y32)
        yard = tuple(max(a, b) for a, b in zip(yard, errs(m_d, A_d, lp_d)))
    e = errs(got_mw, got_A, got_lp)
    # The evidence is a DIFFERENCE of large terms (reference :57-58: the quadratic form delta' Sy^-1 delta against |v|^2): fp32
    # cannot deliver it to better than a few ulps of the largest term, whatever the algorithm, and where fp32 LAPACK happens
    # to land inside one ulp of that term its error is luck, not a yardstick -- so the evidence bound never drops below
    # 4 eps32 x (quadratic form + N log 2pi + |logdet A| + |logdet Lw|), relative to the evidence.
    dy = f64(y32) - f64(X32).T @ f64(mw32)
    if np.ndim(s32) < 2:
        quad = float(np.sum(dy * dy / np.broadcast_to(f64(s32), dy.shape))) if dy.size else 0.0
    else:
        quad = float(dy @ np.linalg.solve(f64(s32), dy))
    Lw64 = f64(Lw32)
    ld_prior = float(np.sum(np.log(Lw64))) if Lw64.ndim == 1 else float(np.linalg.slogdet(Lw64)[1])
    ld_post = float(np.linalg.slogdet(A_o)[1])  # the other two large terms of the sum: logdet of the posterior / prior precision
    cancel = 4 * float(np.finfo(np.float32).eps) * (quad + dy.size * np.log(2 * np.pi) + abs(ld_prior) + abs(ld_post)) / abs(lp_ref)
    floor = (floor[0], floor[1], max(floor[2], cancel))
    for i, name in enumerate(("posterior mean", "posterior precision", "log evidence")):
        assert e[i] <= 4 * yard[i] + floor[i], (what, name, e, yard, floor)
    if got_T is not None:
        Tn = np.triu(np.asarray(got_T, dtype=np.float64))
        eT = float(np.max(np.abs(Tn.T @ Tn - A_o)) / np.max(np.abs(A_o)))
        assert eT <= 4 * yard[1] + floor[1], (what, "T'T", eT, yard)
        assert np.all(np.tril(np.asarray(got_T), -1) == 0)
    return e, yard
