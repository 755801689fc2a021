"""fused_i8_kernel (blr_fused_i8.hpp) at the edges of its capacity test, in its repair and over its digit plan, held to
the BITS of an exact-integer host model (tests/_i8_problems.py) instead of a tolerance: the fixtures live on the rows' dyadic grids, so
every partial sum the kernel forms on its way to A is a float64, and A must equal diag(lam) + G_kept / s exactly -- in all eight
instantiations the dispatcher reaches (ColVecs / RowVecs x isotropic / diagonal noise x 6 / 7 digit groups).  The fp64 kernel
(NO_I8_GRAM) is held to the same bits wherever the plain Gram is the kept one.  The hand-back counter at the threshold max(2, nk / 16)
turns a missed or a spurious block mark into a wrong count.

One entry per fixture is excused from exactness and held to 2^-50 of itself instead: the diagonal entry of a row with an entry planted
beyond 16 capacities.  Its repair term 2 d c + d d has 94 significant bits (d = 2^53 + ..., c the wrapped value), so the kernel's
four roundings there (2 d c, d d, their sum, the addition to A_rr; each <= 2^-53 of a magnitude <= 1.01 A_rr) cannot be avoided by any
choice of value beyond 16 capacities (tests/_i8_problems.py assert_exact_fixture names exactly these entries on the CPU)."""
import numpy as np
import pytest

import _i8_problems as P
from blr_amd import _abi
from oracle import blr_oracle as O

pytestmark = pytest.mark.gpu

D = P.D
CONFIGS = [(layout, noise, NG) for layout in ("col", "row") for noise in ("iso", "diag") for NG in (6, 7)]
CONFIG_IDS = [f"{l}-{n}-{g}" for l, n, g in CONFIGS]


@pytest.fixture(scope="module")
def hd():
    h = _abi.Handle()
    yield h
    h.close()


def _route(noise, NG):
    default = 6 if noise == "iso" else 7
    return "fused_i8_kernel" if NG == default else f"fused_i8_kernel ({NG} digit groups)"


def _run(h, ps, layout, wide=False):
    nb, N = len(ps), ps[0]["N"]
    X = np.ascontiguousarray(np.stack([p["X"].T for p in ps]))  # [nb, N, D] in C order: D x N ColVecs (np.stack alone keeps the views' layout)
    y = np.stack([p["y"] for p in ps])
    mw = np.stack([p["mw"] for p in ps])
    lam = np.stack([p["lam"] for p in ps])
    if ps[0]["svec"] is None:
        nk, s, ss = _abi.NOISE_ISOTROPIC, np.array([P.S_ISO]), 0
    else:
        nk, s, ss = _abi.NOISE_DIAGONAL, np.stack([p["svec"] for p in ps]), N
    if layout == "col":
        lay, Xin, ldx, sx = _abi.LAYOUT_COLVECS, X, D, N * D
    else:
        ld = N + (N & 1) + (2 if wide else 0)
        Xin = np.full((nb, D, ld), 3.0e5)  # (the padding behind row N must never be read: it would break every capacity)
        Xin[:, :, :N] = X.transpose(0, 2, 1)
        assert Xin.flags.c_contiguous
        lay, ldx, sx = _abi.LAYOUT_ROWVECS, ld, D * ld
    mp = np.full((nb, D), 7.0); Tp = np.full((nb, D, D), 7.0); Ap = np.full((nb, D, D), 7.0); lp = np.zeros(nb); info = np.full(nb, 9, dtype=np.int32)
    h.posterior_batched(np.float64, _abi.MEM_HOST, lay, nb, D, N, Xin, ldx, sx, y, N, nk, s, ss, _abi.PRIOR_DIAGONAL, mw, D, lam, 1, D,
                        mp, D, Tp, D, D * D, Ap, D, D * D, lp, info)
    return mp, Tp, Ap, lp, info


def _oracle(p):
    if "oracle" not in p:
        p["oracle"] = O.posterior_logpdf_direct(p["mw"], p["lam"], p["X"], P.S_ISO if p["svec"] is None else p["svec"], p["y"])
    return p["oracle"]


def _check_oracle(p, mp, Tp, Ap, lp):
    """the tolerances of test_i8_gram_path_vs_oracle_and_fp64_kernel"""
    mw_o, T_o, A_o, lp_o = _oracle(p)
    sv = P.S_ISO if p["svec"] is None else p["svec"]
    dlt = p["y"] - p["X"].T @ p["mw"]
    assert abs(lp - lp_o) <= 1e-11 * abs(lp_o) + 1e-14 * float(np.sum(dlt * dlt / sv))
    dA = np.sqrt(np.diag(A_o))
    np.testing.assert_allclose(mp * dA, mw_o * dA, rtol=1e-8, atol=1e-9 * np.abs(mw_o * dA).max())
    assert (np.abs(Ap - A_o) / np.outer(dA, dA)).max() <= 1e-12
    Tn = np.triu(Tp.T)
    assert (np.abs(Tn.T @ Tn - A_o) / np.outer(dA, dA)).max() <= 1e-10


def _check_batch(h, name, layout, noise, NG, wide=False):
    ps = P.batch(name, noise, NG)
    nb = len(ps)
    h.set_option("NO_I8_GRAM", None)
    h.set_option("I8_GROUPS", str(NG))
    try:
        h.reset_stats()
        fast = _run(h, ps, layout, wide)
        assert h.last_route() == _route(noise, NG)
        sent, back = h.get_stat("i8_regressors"), h.get_stat("i8_handed_back")
        again = _run(h, ps, layout, wide)
        h.set_option("NO_I8_GRAM", "1")
        slow = _run(h, ps, layout, wide)
        assert h.last_route().startswith("fused_small_kernel<double, 8,")
    finally:
        h.set_option("NO_I8_GRAM", None)
        h.set_option("I8_GROUPS", None)
    for u, v in zip(fast, again):
        np.testing.assert_array_equal(u, v)
    want_back = [bool(p["model"].handed_back) for p in ps]
    print(f"{name} {layout}-{noise}-{NG}: sent {sent}, handed back {back} (model {sum(want_back)})")
    assert sent == nb
    assert back == sum(want_back)
    for b, p in enumerate(ps):
        exp = P.expected_A(p)
        excused = np.zeros((D, D), bool)
        for i, j in p["allow"]:
            excused[i, j] = True
        dev_fast = np.abs(fast[2][b] - exp)
        dev_slow = np.abs(slow[2][b] - exp)
        pm = P.plain_mask(p)
        print(f"  regressor {b}: marked {p['model'].marked}, max |A_i8 - A_exact| = {dev_fast[~excused].max():.3e}, excused {dev_fast[excused].max() if excused.any() else 0.0:.3e}, "
              f"max |A_fp64 - A_exact| where the plain Gram is the kept one = {dev_slow[pm].max():.3e}, info {fast[4][b]} / {slow[4][b]}")
        if want_back[b]:  # the fp64 kernel's bits in every output
            for u, v in zip(fast, slow):
                np.testing.assert_array_equal(u[b], v[b])
        else:
            assert np.array_equal(fast[2][b][~excused], exp[~excused]), f"regressor {b}: {int((dev_fast[~excused] != 0).sum())} entries differ, first at {np.argwhere((dev_fast != 0) & ~excused)[:4].tolist()}"
            assert np.all(dev_fast[excused] <= 2.0 ** -50 * np.abs(exp[excused]))
        assert np.array_equal(slow[2][b][pm], exp[pm]), f"regressor {b} (fp64 kernel): first at {np.argwhere((dev_slow != 0) & pm)[:4].tolist()}"
        if not p.get("singular"):
            assert fast[4][b] == 0 and slow[4][b] == 0
            for mp, Tp, Ap, lp, _ in (fast, slow):
                _check_oracle(p, mp[b], Tp[b], Ap[b], lp[b])


@pytest.mark.parametrize("layout,noise,NG", CONFIGS, ids=CONFIG_IDS)
@pytest.mark.parametrize("N", [512, 543])
def test_capacity_interval_ends_as_third_marked_block(hd, layout, noise, NG, N):
    """family (b), values: +-2^e (1 -+ 2^-7 / 2^-9), -2^e as the third marked block of a regressor (handed back iff they mark), wrapped ones alone"""
    _check_batch(hd, f"values{N}", layout, noise, NG, wide=(N == 543))


@pytest.mark.parametrize("layout,noise,NG", CONFIGS, ids=CONFIG_IDS)
@pytest.mark.parametrize("name", ["far543", "ends512", "positions512", "words2112"])
def test_planted_entries_by_position(hd, layout, noise, NG, name):
    """family (b): beyond 16 capacities, columns 95 / 96, the last partial block; the first and last integer the capacity test accepts; every 32-row tile, column octet and column in the octet;
    blocks 63 / 64 / 65 and the limit of four marked blocks at N = 2112"""
    _check_batch(hd, name, layout, noise, NG)


@pytest.mark.parametrize("layout,noise,NG", CONFIGS, ids=CONFIG_IDS)
@pytest.mark.parametrize("N", [512, 1536])
def test_several_wrapped_entries_and_the_hand_back_threshold(hd, layout, noise, NG, N):
    """family (c)"""
    _check_batch(hd, f"multi{N}", layout, noise, NG)


@pytest.mark.parametrize("layout,noise,NG", CONFIGS, ids=CONFIG_IDS)
def test_digit_lattice(hd, layout, noise, NG):
    """family (d): every digit pair in every tile pair; dropped pairs leave exactly the anchors' product, (3, 3) comes through TD"""
    _check_batch(hd, "lattice512", layout, noise, NG)


@pytest.mark.parametrize("layout,noise,NG", CONFIGS, ids=CONFIG_IDS)
@pytest.mark.parametrize("name", ["extreme512", "prior_mean543"])
def test_extreme_scales_and_a_dyadic_prior_mean(hd, layout, noise, NG, name):
    """family (e), and the one case with mw != 0"""
    _check_batch(hd, name, layout, noise, NG)
