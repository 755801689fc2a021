"""The draw lattice (tests/_draw_problems.py) checked without a GPU: the route every case declares against a mirror of the host's
predicates, the coverage of every route bit and every reason for the scalar projection per dtype, the references against
np.longdouble, the conditioning of the priors, and the sizes."""
import numpy as np
import pytest

import _draw_problems as DP
from oracle import blr_oracle as O

IDS = [c.id for c in DP.LATTICE]


def test_ids_are_unique_and_the_lattice_is_what_it_says():
    assert len(set(IDS)) == len(IDS)
    for e in ("sample_weights", "apply_weights", "rand", "rand_batched"):
        assert {c.dtype for c in DP.BY_ENTRY[e]} == {"f32", "f64"}
    w = [c for c in DP.BY_ENTRY["sample_weights"] if c.D <= 128]
    for dt in ("f32", "f64"):
        assert {(c.D, c.prior) for c in w if c.dtype == dt} >= {(D, p) for D in (1, 15, 16, 17, 33, 112, 113, 127, 128)
                                                                 for p in ("diag", "dense", "factor")}
        assert {c.S for c in w if c.dtype == dt} >= {1, 63, 64, 65, 129, 512 * 64 + 65}
        assert any(c.D * c.S > 1024 * 256 and c.prior == "diag" for c in w if c.dtype == dt)
        wl = {(c.D, c.S, c.prior) for c in DP.BY_ENTRY["sample_weights"] if c.D > 128 and c.dtype == dt}
        assert wl == {(D, S, p) for D in (129, 144, 256, 257) for S in (1, 5) for p in ("diag", "dense", "factor")} | \
            {(129, 1025, p) for p in ("diag", "dense", "factor")}
        # the matrix-core projection: every N and every S with every parity of nchunks, nchunks 1..5 with and without a partial chunk
        m = [c for c in DP.BY_ENTRY["apply_weights"] if c.dtype == dt and c.route == DP.P_MFMA]
        kc = DP.KC[dt]
        assert {(-(-c.D // kc), c.D % kc == 0) for c in m} >= {(1, True), (2, False), (2, True), (3, False), (3, True), (4, True),
                                                              (5, False), (5, True)}
        for par in (0, 1):
            assert {c.N for c in m if -(-c.D // kc) % 2 == par} == {1, 127, 128, 129, 257}
            assert {c.S for c in m if -(-c.D // kc) % 2 == par} == {1, 15, 16, 17, 63, 64, 65}
        twins = {c.seed_key for c in DP.BY_ENTRY["apply_weights"] if c.dtype == dt and dict(c.options).get("NO_MFMA_PROJECT")}
        assert twins == {c.seed_key for c in m}
        b = [c for c in DP.BY_ENTRY["rand_batched"] if c.dtype == dt]
        assert {c.B for c in b} >= {1, 3, 37} and {c.S for c in b} >= {1, 4, 5, 7}
        fused = [c for c in b if c.route & DP.P_FUSED]
        assert {-(-c.N // 64) for c in fused} >= {2, 8} and any(c.N * c.S == 512 for c in fused)
        assert any(c.N * c.S == 513 for c in b)


@pytest.mark.parametrize("c", DP.LATTICE, ids=IDS)
def test_declared_route_is_what_the_host_picks(c):
    assert DP.expected_route(c) == c.route, (bin(DP.expected_route(c)), bin(c.route))
    g = DP.operands(c)
    for name, geo in g.items():  # the call's own argument checks
        assert geo.ld >= geo.rows and geo.off >= 0
        if geo.out and geo.count > 1:
            assert geo.stride >= geo.ld * geo.cols
    if c.route & DP.P_SCALAR and c.entry == "apply_weights":
        assert DP.scalar_reasons(c)


def test_every_route_bit_and_every_scalar_reason_is_reached_per_dtype():
    for dt in ("f32", "f64"):
        cases = [c for c in DP.LATTICE if c.dtype == dt]
        for name, bit in DP.ROUTE_BITS.items():
            assert any(c.route & bit for c in cases), (dt, name)
        assert any(c.entry != "sample_weights" and c.N > 0 and not c.route & (DP.P_FUSED | DP.P_SCALAR | DP.P_MFMA) for c in cases) or \
            any(c.entry == "rand_batched" and c.N == 0 for c in cases)  # projection: none
        assert any(c.route == DP.W_MFMA for c in cases) and any(c.route == DP.W_MFMA | DP.W_UVEC for c in cases)
        for entry in ("apply_weights", "rand_batched"):
            alone = {tuple(DP.scalar_reasons(c)) for c in cases if c.entry == entry and c.route & DP.P_SCALAR}
            for reason in DP.SCALAR_REASONS:  # each reason on its own, not only next to another
                assert (reason,) in alone, (dt, entry, reason)


def _rel(a, b):
    scale = float(np.max(np.abs(b))) if b.size else 1.0
    return float(np.max(np.abs(a - b))) / scale if b.size else 0.0


@pytest.mark.parametrize("c", DP.LATTICE, ids=IDS)
def test_fp64_reference_against_longdouble(c):
    """the fp64 numpy reference is not the noise floor of the fp64 bounds: 1e-13 relative to np.longdouble on every case"""
    assert np.finfo(np.longdouble).eps < 1e-18
    p = DP.problem(c)
    regs = [b for b in range(c.B) if not (c.bad and c.bad[0] == b)][:3]  # (a batch repeats one construction: three regressors of it)
    for b in regs:
        if c.entry == "apply_weights":
            W64, Wld = p["W"][0], p["W"][0].astype(np.longdouble)
        else:
            Wld = DP.ref_weights(c, p, b, "ld")
            W64 = DP.ref_weights(c, p, b, "f64")
            prec = p["L"][b] if c.prior != "factor" else p["L"][b].T @ p["L"][b]
            W_o = O.sample_weights(p["mw"][b], prec, p["Z1"][b])
            assert _rel(W64, Wld) <= 1e-13 and _rel(W_o, Wld) <= 1e-13
        if c.entry == "sample_weights" or c.N == 0:
            continue
        X = DP.x_of(c, p, b)
        Yld = X.astype(np.longdouble).T @ Wld + DP.noise_term(c, p, b).astype(np.longdouble)
        Y64 = X.T @ W64 + DP.noise_term(c, p, b)
        assert _rel(Y64, Yld) <= 1e-13
        if c.noise is not None:
            s = p["s"][b] if c.noise == "diag" else float(p["s"][b][0])
            assert _rel(O.rand(p["mw"][b], prec, X, s, p["Z1"][b], p["Z2"][b]), Yld) <= 1e-13


def test_prior_condition_numbers_are_capped():
    worst = 0.0
    for c in DP.LATTICE:
        if c.entry == "apply_weights" or c.prior == "diag":
            continue
        p = DP.problem(c)
        for b in range(min(c.B, 3)):
            if c.bad and c.bad[0] == b:
                continue
            L = p["L"][b]
            k = np.linalg.cond(L, 2)
            worst = max(worst, float(k) if c.prior == "factor" else float(np.sqrt(k)))
    print("largest cond_2(U):", worst)
    assert worst <= DP.COND_CAP_U


def test_padding_is_nan_and_outputs_are_sentinel():
    for c in (DP.LATTICE[0], DP.BY_ENTRY["rand_batched"][3], DP.BY_ENTRY["apply_weights"][-1], DP.BY_ENTRY["rand"][1]):
        p = DP.problem(c)
        bufs = DP.buffers(c, p)
        for name, g in DP.operands(c).items():
            m = DP.logical_mask(g)
            assert bufs[name].dtype == c.np_dtype and bufs[name].size == g.size
            if g.out:
                assert np.all(bufs[name] == DP.SENTINEL)
            else:
                assert np.all(np.isnan(bufs[name][~m])) and not np.any(np.isnan(bufs[name][m]))
                assert (~m).sum() >= DP.TAIL + g.off


def test_largest_case_moves_less_than_64_mib():
    big = max(DP.LATTICE, key=DP.moved_bytes)
    print(big.id, DP.moved_bytes(big) / 2 ** 20, "MiB")
    assert DP.moved_bytes(big) < 64 << 20
