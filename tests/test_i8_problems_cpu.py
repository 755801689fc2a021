"""The fixtures and the host model of tests/test_i8_edges_gpu.py, checked without a GPU: every fixture is exact (assert_exact_fixture), the
model's block marks and hand-backs are the ones written down here by hand, the interval rule in Python ints agrees with the slicing
emulated in IEEE doubles, the digit extraction agrees with tools/i8_digits_emul.py, and the kept Gram is the plain one whenever no
digit pair with s + t >= NG occurs."""
import importlib.util
import pathlib

import numpy as np
import pytest

import _i8_problems as P

PLANS = [("iso", 6), ("iso", 7), ("diag", 7), ("diag", 6)]
PLAN_IDS = [f"{n}-{g}" for n, g in PLANS]

# marked blocks per regressor, by hand from the plants (the same under every plan: plants are placed in capacities of the plan)
MARKED = {
    "values512": [[5, 9], [3, 5, 9], [5, 9], [5, 9], [3, 5, 9], [3], [3], [3]],
    "values543": [[5, 9], [3, 5, 9], [5, 9], [5, 9], [3, 5, 9], [3], [3], [3]],
    "far543": [[15], [15], [5, 9], [3, 5, 9], [5, 9], [5, 9, 15]],   # column 95 raises the capacity; 96 marks; the partial block never marks
    "positions512": [[3], [15], [3], [15], [3], [15], [15], [3]],
    "ends512": [[5, 9], [5, 9], [3, 5, 9], [5, 9, 15], [3], [15]],   # the two inner ends fit, the two outer ones mark
    "words2112": [[63], [64], [65], [3, 63, 64, 65], [3, 10, 63, 64, 65], [63, 64]],
    "multi512": [[4], [6], [7], [3, 15], [4, 6], [4, 6, 8], [4, 8]],
    "multi1536": [[4], [6], [7], [3, 47], [4, 6, 8], [4, 6, 8, 10], [4, 8]],
    "lattice512": [[]] * 6,
    "extreme512": [[], [], [], [7], [], []],
    "prior_mean543": [[], [4], [], [6], [], [8]],
}
# handed back: more marked blocks than max(2, nk / 16) (2 at N = 512 / 543, 3 at 1536, 4 at 2112), or a row beyond 2^400
HANDED_BACK = {
    "values512": [0, 1, 0, 0, 1, 0, 0, 0], "values543": [0, 1, 0, 0, 1, 0, 0, 0], "far543": [0, 0, 0, 1, 0, 1], "ends512": [0, 0, 1, 1, 0, 0], "positions512": [0] * 8,
    "words2112": [0, 0, 0, 0, 1, 0], "multi512": [0, 0, 0, 0, 0, 1, 0], "multi1536": [0, 0, 0, 0, 0, 1, 0], "lattice512": [0] * 6,
    "extreme512": [0, 0, 0, 0, 0, 1], "prior_mean543": [0] * 6,
}


def test_the_tables_cover_every_batch():
    assert set(MARKED) == set(HANDED_BACK) == set(P.BATCHES)


@pytest.mark.parametrize("noise,NG", PLANS, ids=PLAN_IDS)
@pytest.mark.parametrize("name", sorted(P.BATCHES))
def test_every_fixture_is_exact_and_marks_what_was_planted(name, noise, NG):
    ps = P.batch(name, noise, NG)
    assert 6 <= len(ps) <= 8 and len(ps) == len(MARKED[name])
    for b, p in enumerate(ps):
        m = p["model"]
        assert m.marked == MARKED[name][b], (b, m.marked)
        assert m.handed_back == bool(HANDED_BACK[name][b]), b
        assert P.marked_blocks(p["X"], NG, p["svec"]) == m.marked and P.handed_back(p["X"], NG, p["svec"]) == m.handed_back
        assert np.array_equal(m.fit, m.fit_emulated)  # the interval rule == the high-word test on x + magic
        A = P.expected_A(p)  # raises unless exact everywhere but on p["allow"]
        assert np.array_equal(A, A.T) and np.all(np.isfinite(A))
        assert len(p["allow"]) == (1 if name == "far543" and b < 2 else 0)
        assert np.array_equal(m.e, P.capacity_exponent(p["X"], NG, 4.0 if noise == "diag" else 1.0, diag=noise == "diag"))
        if name != "extreme512":
            assert np.array_equal(m.e, p["e"])  # the capacities the plants were measured in
        # the plain Gram is the kept one whenever no digit pair with s + t >= NG occurs (balanced digits of what the stream sliced)
        dg = P.balanced_digits(m.cint)
        top = [max((s for s in range(6) if np.any(dg[s][r])), default=0) for r in range(P.D)]
        all_kept = all(top[i] + top[j] < NG for i in range(P.D) for j in range(P.D))
        if all_kept:
            assert np.all(m.kept == m.plain)
        if name == "lattice512":
            assert not all_kept and not np.all(m.kept == m.plain)
            i, j = 5, 11  # two rows of digit 5: everything but the anchors' product is dropped
            assert m.kept[i, j] == 1 << (2 * ((46 if noise == "diag" else 47) - P.cap_of(NG)))  # (column 0 has 1 / sqrt(s_0) = 2 of the largest 4)


def test_planted_values_against_the_interval_rule_in_python_ints():
    for e in (-398, -12, 0, 9, 404):
        got = {k: P.fits(np.ldexp(v, e), e) for k, v in P.VALUES.items()}
        assert got == {"fit+": True, "out+": False, "fit-1": True, "fit-": True, "out-": False, "wrap+": False, "wrap-": False, "far+": False,
                       "far-": False}
        # the ends themselves: Q + 0x8080808080 in [-2^47, 2^47)
        g = np.ldexp(1.0, e - 47)
        assert P.fits(((1 << 47) - P.BAL - 1) * g, e) and not P.fits(((1 << 47) - P.BAL) * g, e)
        assert P.fits((-(1 << 47) - P.BAL) * g, e) and not P.fits((-(1 << 47) - P.BAL - 1) * g, e)
        xs = np.array([[((1 << 47) - P.BAL - 1) * g, ((1 << 47) - P.BAL) * g, (-(1 << 47) - P.BAL) * g, (-(1 << 47) - P.BAL - 1) * g, np.inf, np.nan]])
        eb = np.array([e + 1023])
        assert P.fits_array(xs, np.array([e])).tolist() == [[True, False, True, False, False, False]]
        assert P.slice_emulated(xs, eb)[0].tolist() == [[True, False, True, False, False, False]]
    assert not P.fits(np.inf, 0) and not P.fits(np.nan, 0)


def test_digit_extraction_agrees_with_the_emulation_tool():
    spec = importlib.util.spec_from_file_location("i8_digits_emul", pathlib.Path(__file__).resolve().parents[1] / "tools" / "i8_digits_emul.py")
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    rng = np.random.Generator(np.random.PCG64(4711))
    Q = rng.integers(-(1 << 47) - P.BAL, (1 << 47) - P.BAL, size=10 ** 4)
    edge = [int(round(v * 2 ** 47)) for k, v in P.VALUES.items() if k.startswith("fit")] + [(1 << 47) - P.BAL - 1, -(1 << 47) - P.BAL, 0, 1, -1]
    Q = np.concatenate([Q, np.array(edge, dtype=np.int64)])
    mine, theirs = P.balanced_digits(Q), tool.digits(Q, balanced=True)
    for s in range(6):
        assert np.array_equal(mine[s], theirs[s])
        assert mine[s].min() >= -128 and mine[s].max() <= 127
    assert np.array_equal(sum(mine[s] << (8 * (5 - s)) for s in range(6)), Q)
    # and through the doubles: x + magic leaves Q + 0x8080808080 in the low mantissa bits
    ok, c = P.slice_emulated(Q[None, :].astype(np.float64) * 2.0 ** (9 - 47), np.array([9 + 1023]))
    assert ok.all() and np.array_equal(c[0], Q)
    # a wrapped entry stands for x - 2^(e + 1): 1.5 capacities -> -0.5
    ok, c = P.slice_emulated(np.array([[1.5, -1.5]]), np.array([1023]))
    assert not ok.any() and c[0].tolist() == [-(1 << 46), 1 << 46]
