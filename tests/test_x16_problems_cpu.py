"""The lattices and exact cases of tests/_x16_problems.py (no GPU): what they cover, stated on the data with a mirror of the host
formulas; the declared routes against the restated dispatch; the yardsticks of the GPU assertions, so that no GPU case can fail for
the reference's sake; the exactness bounds of the integer cases; the bytes a case stages."""
import numpy as np
import pytest

import _x16_problems as P
from _small_d_problems import _outputs
from _yardsticks import _assert_fp32_within_lapack
from blr_amd import _abi
from oracle import blr_oracle as O

FMTS = ("bf16", "f16")
CUS = (256, 64)  # the properties of the launch arithmetic hold for both


def _post_coverage(lattice):
    ids = [c.id for c in lattice]
    assert len(set(ids)) == len(ids) and 180 <= len(ids) <= 230
    reach = {(f, nb, P.declared_mode(k, D)) for f in FMTS for nb, Ds in P.POST_DS.items() for D in Ds for k in P.XKINDS}
    assert len(reach) == 32  # every instantiation of fused_x16_kernel
    for key in reach:
        Ns = {c.N for c in lattice if (c.fmt, c.NB, c.mode) == key}
        assert Ns & {160, 161} and Ns & {293, 320}, key  # a DMA stage into a used slot; two ring revolutions
    for mode in range(4):
        assert {c.N for c in lattice if c.mode == mode} == set(P.POST_NS), mode
    for f in FMTS:
        for col in (True, False):
            assert {c.D for c in lattice if c.fmt == f and c.xkind.startswith("col") == col} == {D for Ds in P.POST_DS.values() for D in Ds}
    assert {c.prior for c in lattice if c.NB == 8 and c.D < 128} == set(P.PRIORS)
    # the seams, derived: (nst, nfull) of the DMA modes as the issue tabulates them, none on the register modes
    table = {0: (0, 0), 1: (1, 0), 31: (1, 0), 32: (1, 1), 33: (2, 1), 96: (3, 3), 97: (4, 3), 128: (4, 4), 160: (5, 5), 161: (6, 5),
             293: (10, 9), 320: (10, 10)}
    for c in lattice:
        assert c.NB == 2 * ((c.D + 31) // 32) and c.D in P.POST_DS[c.NB]
        assert P.post_stages(c.N, 2) == table[c.N] and P.post_stages(c.N, c.mode)[1] == (table[c.N][1] if c.mode >= 2 else 0)
    dma = [P.post_stages(c.N, c.mode) for c in lattice if c.mode >= 2]
    assert any(nfull >= 5 for _, nfull in dma) and any(nfull >= 9 for _, nfull in dma)           # slot reuse by a DMA stage, twice round
    assert any(nst == nfull and nst > 3 for nst, nfull in dma) and (3, 3) in dma and (4, 3) in dma  # ends on a DMA stage; nst == LA, LA + 1
    nb8 = {(c.D, c.mode) for c in lattice if c.NB == 8}
    assert {D for D, _ in nb8} >= {97, 100, 104, 120, 127} and (104, 2) in nb8 and (120, 2) in nb8  # pad rows on the static-wave path


def _marg_coverage(lattice):
    ids = [c.id for c in lattice]
    assert len(set(ids)) == len(ids) and 100 <= len(ids) <= 160
    table = {8: (1, 1), 24: (2, 1), 33: (3, 2), 64: (4, 2), 88: (6, 3), 97: (7, 4), 104: (7, 4), 113: (8, 4), 120: (8, 4), 127: (8, 4)}
    assert {D: P.marg_blocks(D) for D in P.MARG_DS} == table
    reach = {(P.marg_blocks(D)[0], f, P.declared_mode(k, D)) for f in FMTS for D in P.MARG_DS for k in P.XKINDS}
    assert {c[0] for c in reach} == {1, 2, 3, 4, 6, 7, 8}
    assert reach == {(c.nJ, c.fmt, c.mode) for c in lattice}
    assert {c.N for c in lattice} == set(P.MARG_NS) and {c.D for c in lattice} == set(P.MARG_DS)
    for f in FMTS:
        for mode in range(4):
            assert any(c.N == 293 and c.prior != "diag" for c in lattice if (c.fmt, c.mode) == (f, mode)), (f, mode)
            assert {c.nJ for c in lattice if (c.fmt, c.mode) == (f, mode)} >= {1, 2, 4, 6, 7, 8}
    for D in (113, 97):
        assert {(c.prior, c.diag_noise) for c in lattice if c.D == D} == {(p, dn) for p in P.PRIORS for dn in (False, True)}, D
    assert {c.mode for c in lattice if c.D in (8, 24, 104, 120) and c.xkind == "col_al"} == {2}  # ColVecs 16-byte loads
    for cus in CUS:
        nb = P.MARG_LATTICE_NB
        assert P.marg_walk(293, nb, cus, image=True)[0] == 2   # gridDim.x > 1 on the image path
        assert P.marg_walk(128, nb, cus, image=True) == (1, 2) and P.marg_walk(17, nb, cus, image=True) == (1, 1)
        assert P.marg_walk(293, 2, cus, image=True)[0] == 2    # ... and in a chunk of two (MAX_CHUNK = 2)


def test_posterior_lattice_covers_what_it_claims():
    _post_coverage(P.POST_LATTICE)


def test_marginals_lattice_covers_what_it_claims():
    _marg_coverage(P.MARG_LATTICE)


def test_coverage_statements_notice_a_missing_row():
    """the statements are about the rows: without the only N = 0 row of a loader, or the rows of D = 113, they fail"""
    c0 = next(c for c in P.POST_LATTICE if c.N == 0 and c.mode == 2)
    with pytest.raises(AssertionError):
        _post_coverage(tuple(c for c in P.POST_LATTICE if not (c.N == 0 and c.mode == c0.mode)))
    with pytest.raises(AssertionError):
        _post_coverage(tuple(c for c in P.POST_LATTICE if not (c.N in (293, 320) and (c.fmt, c.NB, c.mode) == ("f16", 6, 2))))
    with pytest.raises(AssertionError):
        _marg_coverage(tuple(c for c in P.MARG_LATTICE if not (c.D == 113 and c.prior == "dense" and c.diag_noise)))
    with pytest.raises(AssertionError):
        _marg_coverage(tuple(c for c in P.MARG_LATTICE if not (c.N == 293 and (c.fmt, c.mode) == ("bf16", 1))))


@pytest.mark.parametrize("cus", CUS)
def test_pure_stream_walks_at_least_two_tiles_per_wave(cus):
    """B = 8 CUs + 1 regressors at N = 131: one workgroup per regressor, nine tiles on four waves"""
    B = 8 * cus + 1
    assert P.marg_walk(P.PURE_N, B, cus, image=False) == (1, 3) and P.marg_least_walk(P.PURE_N, B, cus, image=False) == 2
    # ... where the lattice's pure-stream cases (five regressors) never take a second tile below N = 293
    assert P.marg_walk(128, 5, cus, image=False)[1] == 1 and P.marg_walk(131, 5, cus, image=False)[1] == 1


def test_expected_route_restates_the_dispatch():
    r = P.expected_route
    assert r("posterior", "bf16", "col", 128, 128, 128 * 50) == "fused_x16_kernel<bf16, 8, 2>"
    assert r("posterior", "bf16", "col", 128, 128, 128 * 50, options=("NO_LDSDMA",)) == "fused_x16_kernel<bf16, 8, 0>"
    assert r("posterior", "f16", "col", 100, 104, 104 * 50) == "fused_x16_kernel<f16, 8, 0>"      # D % 8
    assert r("posterior", "f16", "row", 100, 56, 5600) == "fused_x16_kernel<f16, 8, 3>"
    assert r("posterior", "f16", "row", 33, 56, 5601) == "fused_x16_kernel<f16, 4, 1>"            # strideX % 8, B > 1
    assert r("posterior", "f16", "row", 33, 56, 5601, B=1) == "fused_x16_kernel<f16, 4, 3>"       # ... is not asked of one regressor
    assert r("posterior", "f16", "row", 1, 56, 56, base_offset_bytes=8) == "fused_x16_kernel<f16, 2, 1>"
    assert r("marginals", "bf16", "col", 24, 24, 0, options=("NO_LDSDMA",)) == "marginals_x16_kernel<bf16, 2>"
    assert r("marginals", "bf16", "col", 24, 25, 0) == "marginals_x16_kernel<bf16, 0>"
    assert r("marginals", "f16", "row", 5, 136, 0, base_offset_bytes=2) == "marginals_x16_kernel<f16, 1>"


@pytest.mark.parametrize("case", P.POST_LATTICE, ids=lambda c: c.id)
def test_posterior_case(case):
    """the declared route is the dispatch's; fp32 LAPACK's own result passes the GPU assertion (N = 0 and N = 1 on the floors)"""
    q = P.post_lattice_problem(case)
    col = "col" if q["layout"] == _abi.LAYOUT_COLVECS else "row"
    assert q["route"] == case.route == P.expected_route("posterior", case.fmt, col, case.D, q["ldx"], q["strideX"], 0, q["nb"])
    assert (q["ldx"] % 8 == 0) == case.xkind.endswith("_al") and q["X"].size >= q["nb"] * q["strideX"]
    assert P.staged_bytes(q, _outputs(q["nb"], case.D, np.float32, gaps=True)) <= 32 << 20
    for b in range(q["nb"]):
        X = np.asfortranarray(q["Xw"][b])
        m, T, A, lp = O.posterior_logpdf_direct(q["mw"][b], q["dense"][b], X, q["s"][b], q["y"][b])
        assert m.dtype == np.float32 and A.dtype == np.float32
        _assert_fp32_within_lapack(q["mw"][b], q["dense"][b], X, q["s"][b], q["y"][b], m, A, lp, got_T=T, what=case.id)


@pytest.mark.parametrize("case", P.MARG_LATTICE, ids=lambda c: c.id)
def test_marginals_case(case):
    """the declared route is the dispatch's; the yardstick of _assert_within_oracle is non-zero and finite for every regressor"""
    q = P.marg_lattice_problem(case)
    col = "col" if q["layout"] == _abi.LAYOUT_COLVECS else "row"
    assert q["route"] == case.route == P.expected_route("marginals", case.fmt, col, case.D, q["ldx"], q["strideX"], 0, q["nb"])
    assert P.staged_bytes(q, P._out(case.N, q["nb"])) <= 32 << 20
    for b in range(q["nb"]):
        ref, f32, yards = P.oracle_yardsticks(q, b)
        assert all(0 < y < np.inf for y in yards), (case.id, b, yards)
        assert np.all(np.isfinite(ref[0])) and np.all(ref[1] > 0)


@pytest.mark.parametrize("fmt,scale", [("bf16", 1.0), ("f16", 1.0), ("f16", P.SUBNORMAL)])  # (the subnormal cases are fp16's)
def test_exact_cases_stay_below_2_24(fmt, scale):
    """Every sum of |terms| of the int64 references stays below 2^24 (so does every partial sum, in any order), every scaled value is
    held by the format (features_as_integers and marg_exact_problem assert it) and every scaled result is an fp32 value."""
    tiny = np.float64(np.finfo(np.float32).tiny)
    for xkind in ("col_al", "row_odd"):
        for D in P.GRAM_EXACT_DS + (40,):
            for N in P.GRAM_EXACT_NS + (131,):
                q, ref, big = P.gram_exact_problem(fmt, xkind, D, N, scale)
                assert big < P.EXACT_LIMIT and scale * scale >= tiny and np.all(q["Lw"].astype(np.float64) == scale * scale)
                assert P.staged_bytes(q, _outputs(q["nb"], D, np.float32)) <= 32 << 20
        for D in P.MARG_EXACT_DS + (40,):
            for N in P.MARG_EXACT_NS + (131,):
                for dn in (False, True):
                    q, mean, var, big = P.marg_exact_problem(fmt, xkind, D, N, dn, scale)
                    assert big < P.EXACT_LIMIT and np.all(var >= 1) and np.all(mean == np.rint(mean))
                    U = q["Lw"][0].reshape((D, D), order="F").astype(np.float64) / scale
                    assert np.array_equal(U, np.rint(U)) and np.array_equal(np.tril(U, -1), np.zeros((D, D)))
                    # the reference is the marginal of this problem: fp64 on the very inputs agrees to rounding
                    m64, v64 = O.marginals_direct(q["mw"][0].astype(float), q["Lw"][0].reshape((D, D), order="F").astype(float),
                                                  q["Xw"][0].astype(float), (q["s"][0] if dn else q["s"][0:1].repeat(N)).astype(float))
                    assert np.allclose(m64, mean[0], rtol=1e-12, atol=1e-9) and np.allclose(v64, var[0], rtol=1e-12)
        if scale == 1.0:
            for D in P.PURE_DS:
                for cus in CUS:
                    q, mean, var, big = P.pure_stream_problem(fmt, xkind, D, 8 * cus + 1)
                    assert big < P.EXACT_LIMIT and q["strideX"] == 0 and q["mw"].shape == (8 * cus + 1, D)
                    assert P.staged_bytes(q, P._out(P.PURE_N, q["nb"])) <= 32 << 20
                    b = 8 * cus  # the last regressor, against the oracle in fp64
                    v64 = O.var(q["mw"][b].astype(float), q["Lw"][b].astype(float), q["Xw"][0].astype(float), q["s"][b].astype(float))
                    assert np.allclose(v64, var[b], rtol=1e-12) and np.array_equal(q["Xw"][0].T.astype(float) @ q["mw"][b], mean[b])
