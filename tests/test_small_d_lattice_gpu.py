"""Every fused_small_kernel<T, NB, MODE> instantiation on the device: 2 types x NB 1..8 x the four loaders, each at two or three
widths (tests/_small_d_problems.py LATTICE), through the C ABI on handles of this module (NO_I8_GRAM = 1, NO_WAVE_KERNEL = 1; a
second one with NO_LDSDMA = 1 for the mode-3 rows).  Each call is held to the route it must take, to the oracle at the header's
tolerances (fp32: 4 x fp32 LAPACK, tests/_yardsticks.py), to the gaps of its output buffers, to the bits of the same regressor
run alone, to the failure it must report in the last row of a partly filled block, and to an evidence of 0 without observations."""
import numpy as np
import pytest

from _small_d_problems import (LATTICE, LATTICE_OPTIONS, LATTICE_OPTIONS_MODE3, _batch, _batched, _check_oracle, _equal_batch, _outputs, _result,
                               _same_bits, _single, _written, expected_route, lattice_batch, lattice_widths)
from blr_amd import _abi

pytestmark = pytest.mark.gpu


def _handle(options):
    hd = _abi.Handle()
    for key, value in options.items():
        hd.set_option(key, value)
    return hd


@pytest.fixture(scope="module")
def handles():
    """{mode-3 row?: handle}; the default handle and the environment stay as they are"""
    hs = {False: _handle(LATTICE_OPTIONS), True: _handle(LATTICE_OPTIONS_MODE3)}
    yield hs
    for hd in hs.values():
        hd.close()


@pytest.mark.parametrize("row", LATTICE, ids=[r["id"] for r in LATTICE])
def test_every_instantiation_matches_the_oracle(handles, row):
    hd = handles[row["mode3"]]
    q = lattice_batch(row)
    o = _outputs(q["nb"], row["D"], row["dtype"], gaps=True)
    assert _batched(hd, q, o) == 0
    assert hd.last_route() == row["route"] == expected_route(row["dtype"], row["D"], row["xkind"], row["options"])
    assert np.all(o["info"] == 0) and np.all(np.isfinite(o["lp"]))
    for b in range(q["nb"]):
        _check_oracle(q, b, _result(q, o, b))
    written_m, written_T = _written(q["nb"], row["D"], o)
    for buf, wr in ((o["mw_post"], written_m), (o["T"], written_T), (o["A"], written_T)):
        assert np.all(np.isfinite(buf[wr])) and np.all(np.isnan(buf[~wr]))


def _d_mid_rows():
    """the D_mid rows of every (type, NB, mode), one per N: a last block that is short by one vector"""
    rows = [r for r in LATTICE if r["D"] == lattice_widths(r["dtype"], r["NB"])[1]]
    assert len({r["route"] for r in rows}) == 64 and len(rows) == 3 * 64
    return rows


@pytest.mark.parametrize("row", _d_mid_rows(), ids=lambda r: r["id"])
def test_a_regressor_of_a_batch_has_the_bits_of_the_same_regressor_alone(handles, row):
    hd = handles[row["mode3"]]
    q = lattice_batch(row)
    o = _outputs(q["nb"], row["D"], row["dtype"])
    assert _batched(hd, q, o) == 0
    assert hd.last_route() == row["route"]
    in_batch = _result(q, o, 3)
    assert in_batch[4] == 0
    alone = _single(hd, q, 3)
    assert hd.last_route() == row["route"]  # B = 1 on the same ldx and alignment class: the same instantiation
    _same_bits(in_batch, alone, "regressor 3")


@pytest.mark.parametrize("NB", range(1, 9))
def test_failures_in_the_last_row_of_a_partly_filled_block_stay_local(handles, NB):
    """a negative diagonal-prior entry in row D = D_lo (the one row of the last block) and a zero noise variance: each is reported
    with its 1-based index, leaves its regressor's outputs alone and the other regressors' bits as they were"""
    hd = handles[False]
    D, dtype, N = lattice_widths(np.float64, NB)[0], np.float64, 64
    good = _equal_batch(D, dtype, N, "col16", "diag", "diag", False, nb=4)
    bad = _equal_batch(D, dtype, N, "col16", "diag", "diag", False, nb=4)
    bad["Lw"][1, D - 1] = -1.0   # prior of regressor 1: the last entry of the diagonal precision
    bad["s"][2 * N + 4] = 0.0    # noise of regressor 2: observation 5
    og, ob = _outputs(4, D, dtype), _outputs(4, D, dtype, fill=-5.0)
    assert _batched(hd, good, og) == 0
    assert hd.last_route() == expected_route(dtype, D, "col16", LATTICE_OPTIONS) == f"fused_small_kernel<double, {NB}, 0>"
    assert _batched(hd, bad, ob) == 0
    assert hd.last_route() == f"fused_small_kernel<double, {NB}, 0>"
    assert np.all(og["info"] == 0)
    assert ob["info"][1] == D and ob["info"][2] == 5
    for b in range(4):
        if b in (1, 2):
            assert np.isnan(ob["lp"][b])
            m, T, _, _, _ = _result(bad, ob, b)
            assert np.all(m == -5.0) and np.all(T == -5.0)  # (Lw' may already hold A: include/blr_mi355x.h)
        else:
            _same_bits(_result(good, og, b), _result(bad, ob, b), f"regressor {b}")


@pytest.mark.parametrize("NB", range(1, 9))
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_no_observations_under_a_diagonal_prior_give_zero_evidence(handles, dtype, NB):
    """N = 0: A = Lw, and the kernel takes logdet Lw from the diagonal of chol(diag(d)) as it rounds it, so the evidence
    (logdet Lw - logdet A) / 2 is the difference of two double sums of the SAME D terms 2 log L_ii added in different orders: at most
    D eps64 sum |log d_i| (L_ii = sqrt(d_i) to a few ulps of the type), in fp32 as in fp64 -- not the few fp32 ulps per row that
    sum log d_i against 2 sum log L_ii leaves.  The oracle returns 0."""
    hd = handles[False]
    for D in lattice_widths(dtype, NB)[::2]:
        for xkind in ("col16", "row"):
            q = _batch(D, dtype, xkind, "iso", "diag", False, counts=[0, 3])
            mw_p, T, A, lp, info = _single(hd, q, 0)
            assert info == 0 and hd.last_route() == expected_route(dtype, D, xkind, LATTICE_OPTIONS)
            d = q["Lw"][0].astype(np.float64)
            assert abs(lp) <= D * np.finfo(np.float64).eps * np.sum(np.abs(np.log(d))), (D, xkind, lp)
            _check_oracle(q, 0, (mw_p, T, A, lp, info))
