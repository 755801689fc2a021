"""The lattice of fused small-D kernel instantiations (tests/_small_d_problems.py) is complete, and every problem the GPU tests
draw for it is one the references solve: checked here, without a GPU, before any GPU time is spent."""
import re
from collections import defaultdict

import numpy as np
import pytest

from _small_d_problems import (ALL_ROUTES, LATTICE, LATTICE_B, LATTICE_NS, LATTICE_OPTIONS, LATTICE_OPTIONS_MODE3, VEC, _check_oracle,
                               _oracle_inputs, expected_route, lattice_batch, lattice_widths)
from oracle import blr_oracle as O


def test_the_table_names_all_64_instantiations_and_nothing_else():
    assert len(ALL_ROUTES) == 64
    assert {r["route"] for r in LATTICE} == ALL_ROUTES
    assert len({r["id"] for r in LATTICE}) == len(LATTICE) == 480  # 160 cells x 3 N


def test_every_instantiation_is_reached_at_two_widths_or_more():
    widths = defaultdict(set)
    for r in LATTICE:
        widths[r["route"]].add(r["D"])
    for route in ALL_ROUTES:
        mode = int(re.fullmatch(r"fused_small_kernel<\w+, \d, (\d)>", route).group(1))
        # modes 3 and 4 need whole 16-byte vectors: D_mid and D_hi; modes 0 and 1 take the odd D_lo as well
        assert len(widths[route]) == (3 if mode in (0, 1) else 2), (route, widths[route])


def test_every_instantiation_is_run_at_every_width_it_reaches_with_every_n():
    """below one stage, one 64-column or two 32-column stages, several stages and a tail: each for every kernel at every width"""
    ns = defaultdict(set)
    for r in LATTICE:
        ns[r["route"], r["D"]].add(r["N"])
    assert len(ns) == 2 * 8 * 10 and all(v == set(LATTICE_NS) for v in ns.values())


def test_widths_blocks_and_rotations():
    for dtype in (np.float64, np.float32):
        for NB in range(1, 9):
            lo, mid, hi = lattice_widths(dtype, NB)
            assert (lo, mid, hi) == (16 * NB - 15, 16 * NB - VEC[dtype], 16 * NB) and lo % 2 == 1
            rows = [r for r in LATTICE if r["dtype"] == dtype and r["NB"] == NB]
            assert all((r["D"] + 15) // 16 == NB for r in rows) and {r["D"] for r in rows} == {lo, mid, hi}
            # every (noise, prior) pair for every NB in each type, every N, shared and own priors
            assert {(r["noise"], r["prior"]) for r in rows} == {(n, p) for n in ("iso", "iso0", "diag") for p in ("diag", "dense", "factor")}
            assert {r["shared_prior"] for r in rows} == {False, True}
            # D_lo reaches modes 0 and 1 only, the other two widths all four
            modes = lambda D: sorted({int(r["route"][-2]) for r in rows if r["D"] == D})  # noqa: E731
            assert modes(lo) == [0, 1] and modes(mid) == [0, 1, 3, 4] and modes(hi) == [0, 1, 3, 4]


def test_expected_route_restates_the_dispatch_rules():
    opt, opt3 = LATTICE_OPTIONS, LATTICE_OPTIONS_MODE3
    assert expected_route(np.float64, 72, "row", opt) == "fused_small_kernel<double, 5, 1>"
    assert expected_route(np.float64, 72, "row", opt3) == "fused_small_kernel<double, 5, 1>"
    assert expected_route(np.float64, 72, "col16", opt) == "fused_small_kernel<double, 5, 4>"
    assert expected_route(np.float64, 72, "colpad", opt3) == "fused_small_kernel<double, 5, 3>"
    assert expected_route(np.float64, 72, "colodd", opt) == "fused_small_kernel<double, 5, 0>"
    assert expected_route(np.float64, 73, "col16", opt) == "fused_small_kernel<double, 5, 0>"
    assert expected_route(np.float32, 90, "col16", opt) == "fused_small_kernel<float, 6, 0>"   # 90 is no multiple of 4 ...
    assert expected_route(np.float64, 90, "col16", opt) == "fused_small_kernel<double, 6, 4>"  # ... but of 2
    assert expected_route(np.float32, 1, "col16", opt3) == "fused_small_kernel<float, 1, 0>"
    assert expected_route(np.float32, 128, "col16", opt3) == "fused_small_kernel<float, 8, 3>"
    for bad in ({}, {"NO_I8_GRAM": "1"}, {"NO_WAVE_KERNEL": "1"}):
        with pytest.raises(ValueError):
            expected_route(np.float64, 64, "col16", bad)
    with pytest.raises(ValueError):
        expected_route(np.float64, 129, "col16", opt)


@pytest.mark.parametrize("row", LATTICE, ids=[r["id"] for r in LATTICE])
def test_the_references_solve_every_generated_problem(row):
    """fp64: posterior_literal / logpdf_literal return finite values.  fp32: the fp32 LAPACK yardstick of
    _assert_fp32_within_lapack evaluates to finite errors (the helper is run on the oracle's own results)."""
    q = lattice_batch(row)
    assert q["nb"] == LATTICE_B and q["N"] == row["N"] and q["X"].dtype == row["dtype"]
    per16 = 16 // np.dtype(row["dtype"]).itemsize
    if row["xkind"] == "col16":  # what expected_route assumes of the layout kinds
        assert q["ldx"] % per16 == 0 and q["strideX"] % per16 == 0
    elif row["xkind"] == "colodd":
        assert q["ldx"] % 2 == 1 and q["ldx"] > row["D"]
    f64 = lambda a: np.asarray(a, dtype=np.float64)  # noqa: E731
    for b in range(q["nb"]):
        mw, Lw, Xb, sb, yb = (f64(a) for a in _oracle_inputs(q, b))
        mw_o, T_o, A_o = O.posterior_literal(mw, Lw, Xb, sb, yb)
        lp_o = O.logpdf_literal(mw, Lw, Xb, sb, yb)
        assert np.all(np.isfinite(mw_o)) and np.all(np.isfinite(T_o)) and np.all(np.isfinite(A_o)) and np.isfinite(lp_o)
        dt = row["dtype"]
        errs = _check_oracle(q, b, (mw_o.astype(dt), T_o.astype(dt), A_o.astype(dt), lp_o, 0))
        if dt == np.float32:
            e, yard = errs
            assert np.all(np.isfinite(e)) and np.all(np.isfinite(yard)) and all(v > 0 for v in yard), (b, e, yard)
        else:
            assert errs == (0.0, 0.0, 0.0, 0.0)
