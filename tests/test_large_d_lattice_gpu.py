"""Every Gram route of the large-D update (D > 128, plan_large: gram_tile_kernel<double>, gram_planes4_kernel, gram_planes_kernel<2>,
gram_planes_kernel<3>, gram_tile_kernel<float, true>, gram_tile_kernel<float>) on the device, off the clean shape: ragged last row
blocks, N either side of a k-block and of a stage, a short / empty last column chunk of the planes pass, the four loaders, both
noise kinds, three priors, a zero and a non-zero prior mean, groups of regressors (tests/_large_d_problems.py LARGE_LATTICE), through
the C ABI in device memspace on handles of this module (per-handle options only).  Each call is held to the route it must take, to
the oracle (fp32: 4 x fp32 LAPACK, tests/_yardsticks.py; fp64: test_large_d_posterior_logpdf_f64's tolerances), to the gaps of its
output buffers, to the bits of a second call, to row scales that must not depend on the rows' magnitude, and to the failure it
must report in the last row of the ragged block."""
import numpy as np
import pytest

from _large_d_problems import (LARGE_LATTICE, OPTION_SETS, ROUTES, _outputs, _result, _same_bits, _written, check_oracle, expected_route,
                               fp32_bound_used, large_problem, pack_image, ragged_rows, run_on_device)
from blr_amd import _abi

pytestmark = pytest.mark.gpu

# the option set that reaches each route with aligned ColVecs
ROUTE_OPTSET = {"gram_tile_kernel<double>": "default", "gram_planes4_kernel": "default", "gram_planes_kernel<2>": "planes8",
                "gram_planes_kernel<3>": "nofp16", "gram_tile_kernel<float, true>": "noplanes", "gram_tile_kernel<float>": "nobf16x3"}
FP32_ROUTES = ROUTES[1:]
WORST = {}  # route -> largest error / bound over the lattice (printed at teardown: LOG.md's head-room figures)


@pytest.fixture(scope="module")
def handles():
    """{option set: handle}; the default handle and the environment stay as they are"""
    hs = {}
    for name, options in OPTION_SETS.items():
        hs[name] = _abi.Handle()
        for key, value in options.items():
            hs[name].set_option(key, value)
    yield hs
    for hd in hs.values():
        hd.close()
    if WORST:
        print("\nlarge-D lattice, worst error / (4 x fp32 LAPACK + default floor) per route as (mean | precision, evidence): "
              + "; ".join(f"{k} ({v[0]:.3f}, {v[1]:.3f})" for k, v in sorted(WORST.items())))


def _row(route, **over):
    """a lattice-style row on the route's own option set: D = 200, N = 33, aligned ColVecs, diagonal noise"""
    optset = ROUTE_OPTSET[route]
    row = dict(id=route, dtype=np.float64 if route == ROUTES[0] else np.float32, D=200, N=33, xkind="col16", noise="diag", prior="diag",
               prior_mean="zero", nb=1, optset=optset, options=OPTION_SETS[optset], seed=4242, route=route)
    row.update(over)
    assert expected_route(row["dtype"], row["D"], row["N"], row["xkind"], row["options"]) == route
    return row


def _call(hd, row, q, gaps=True, fill=np.nan):
    o = _outputs(q["nb"], row["D"], row["dtype"], gaps=gaps, fill=fill)
    assert run_on_device(hd, q, o) == 0
    assert hd.last_route() == row["route"]
    return o


@pytest.mark.parametrize("row", LARGE_LATTICE, ids=[r["id"] for r in LARGE_LATTICE])
def test_every_route_matches_the_oracle(handles, row):
    """What this table found: with three plane products only (h h, h l, l h), planes4_nospec-D129-N16-col16-iso-diag-zero-nb1 missed
    the evidence bound -- errors (mean, precision, evidence) = (1.96e-5, 1.22e-7, 1.94e-6), fp32 LAPACK (2.81e-5, 4.19e-7, 8.0e-8),
    evidence bound 4 x 8.0e-8 + 1.41e-6 (the yardstick's cancellation floor) = 1.73e-6.  sum_n l_n l_n' is positive semi-definite with
    directions outside the span of N = 16 observations, where A is the weak prior alone: dropping it moved logdet A by -1.4e-4.  The
    NP = 2 Gram kernels now keep the fourth product where N < 2 DP (GramPlanesArgs::ll, blr_planes.hpp)."""
    hd = handles[row["optset"]]
    q = large_problem(row)
    o = _outputs(q["nb"], row["D"], row["dtype"], gaps=True)
    assert run_on_device(hd, q, o) == 0
    assert hd.last_route() == row["route"] == expected_route(row["dtype"], row["D"], row["N"], row["xkind"], row["options"])
    assert np.all(o["info"] == 0) and np.all(np.isfinite(o["lp"]))
    for b in range(q["nb"]):
        used = check_oracle(q, b, _result(q, o, b), what=row["id"])
        if used is not None:
            WORST[row["route"]] = tuple(max(a, b) for a, b in zip(WORST.get(row["route"], (0.0, 0.0)), fp32_bound_used(*used)))
    written_m, written_T = _written(q["nb"], row["D"], o)
    for buf, wr in ((o["mw_post"], written_m), (o["T"], written_T), (o["A"], written_T)):
        assert np.all(np.isfinite(buf[wr])) and np.all(np.isnan(buf[~wr]))


@pytest.mark.parametrize("row", ragged_rows(), ids=lambda r: r["id"])
def test_a_second_call_gives_the_same_bits(handles, row):
    """the split-K reduction and the b partials are summed in a fixed order on every route and option set"""
    hd = handles[row["optset"]]
    q = large_problem(row)
    o1, o2 = _call(hd, row, q), _call(hd, row, q)
    assert np.all(o1["info"] == 0)
    for k in ("mw_post", "T", "A", "lp", "info"):
        assert np.array_equal(o1[k], o2[k], equal_nan=True), k


@pytest.mark.parametrize("optset", ["default", "nospec", "planes8", "nofp16", "noplanes", "nobf16x3"])
def test_padding_rows_and_tail_columns_do_not_leak(handles, optset):
    """D = 200 (56 zero rows in the planes), N = 33 (k-block 2 holds one real column, the stage padding of NP = 2 a whole zero
    k-block), diagonal noise, a zero prior mean: X 2^k and the prior 2^2k scale every quantity of the problem by a power of two
    -- exactly, in the fp64 oracle and in fp32 LAPACK alike, so the yardstick of the scaled problem is the unscaled one's -- and the
    kernels' errors must not care either: the sampled row scales and the fp16 planes under per-row power-of-two scales see rows
    of 2^40 and of 2^-40 as they see rows of 1 (all inside the fp32 range: |x| < 8, the precision's entries < 2^87).  Then row 199, the
    last real row, 2^12 larger than the others in every column: the sample sees it, no second planes pass is asked for."""
    hd = handles[optset]
    base = _row("gram_planes4_kernel")
    row = dict(base, optset=optset, options=OPTION_SETS[optset], route=expected_route(np.float32, 200, 33, "col16", OPTION_SETS[optset]))

    def run(scale_log2, big_row):
        q = large_problem(row)
        q["Xd"][199, :] *= np.float32(2.0 ** big_row)
        q["Xd"] *= np.float32(2.0 ** scale_log2)
        q["Lw"] *= np.float32(2.0 ** (2 * scale_log2))
        assert np.all(np.isfinite(q["Xd"])) and np.all(np.isfinite(q["Lw"])) and np.all(q["mw"] == 0)
        pack_image(q)
        hd.reset_stats()
        o = _call(hd, row, q)
        assert o["info"][0] == 0
        e, yard = check_oracle(q, 0, _result(q, o, 0), what=f"{optset} 2^{scale_log2} row 199 x 2^{big_row}")
        assert hd.get_stat("planes_redone") == 0
        return e, yard

    (e0, y0), (eu, yu), (ed, yd) = run(0, 0), run(40, 0), run(-40, 0)
    # the yardstick itself is scale-free (the premise of the comparison): fp32 LAPACK's errors on the scaled problems are the unscaled ones'
    assert np.allclose(yu[:2], y0[:2], rtol=1e-3, atol=0) and np.allclose(yd[:2], y0[:2], rtol=1e-3, atol=0), (y0, yu, yd)
    run(0, 12)
    run(40, 12)


@pytest.mark.parametrize("route", ROUTES)
def test_a_bad_pivot_in_the_ragged_last_block_is_named_on_every_route(handles, route):
    """D = 200, dense prior, three regressors in one group; regressor 1's prior has its leading minor of order 200 -- the last row
    of the ragged second block -- as the first that is not positive definite (built as test_large_d_factorisation_names_the_first_bad_pivot
    builds it): info = [0, 200, 0], its evidence NaN, and regressors 0 and 2 keep the bits of the same call with a good regressor 1."""
    hd = handles[ROUTE_OPTSET[route]]
    row = _row(route, prior="dense", nb=3, prior_mean="nonzero", N=33)
    D = row["D"]
    good, bad = large_problem(row), large_problem(row)
    Lc = np.linalg.cholesky(good["dense_of"](1).astype(np.float64))
    Lc[D - 1, D - 1] = 0.0
    Lw_bad = Lc @ Lc.T
    Lw_bad[D - 1, D - 1] -= 1.0
    bad["Lw"][1] = Lw_bad.astype(row["dtype"]).reshape(-1, order="F")
    og, ob = _call(hd, row, good, gaps=False), _call(hd, row, bad, gaps=False, fill=-5.0)
    assert np.all(og["info"] == 0)
    assert list(ob["info"]) == [0, D, 0]
    assert np.isnan(ob["lp"][1])
    for b in (0, 2):
        _same_bits(_result(good, og, b), _result(bad, ob, b), f"regressor {b}")
        check_oracle(good, b, _result(good, og, b), what=route)
