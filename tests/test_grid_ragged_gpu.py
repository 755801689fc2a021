"""The evidence grid for regressors with unequal observation counts (blr_logpdf_grid_ragged_*, logpdf_grid_ragged,
posterior_best_ragged, logpdf_grid_map): bit equality with blr_logpdf_grid_* at B = 1 on every regressor's slice -- the entry point's
specification --, against the CPU oracle, and against itself (permutations, added regressors, determinism, local failures).  All
tests need an MI355X."""
import numpy as np
import pytest

from oracle import blr_oracle as O

import _grid_ragged_data as R

pytestmark = pytest.mark.gpu

# fp64 bounds of tests/test_grid_gpu.py: the project's own (header of blr_posterior_batched_*)
TOL_LP, TOL_MW, TOL_A = 1e-10, 1e-9, 1e-9


@pytest.fixture(scope="module")
def B():
    import blr_amd

    blr_amd._abi.default_handle()  # raises if the extension or the GPU is missing: no silent fallback
    return blr_amd


# (D, loader, noise, prior, dtype, shared grid): D = 5, 33, 64, 128 (NB = 1, 3, 4, 8: the classes of SmallCfg that differ in code)
# times the three loaders; noise kinds, prior kinds, element types and shared / per-regressor grids rotate over them
CASES = [
    (5, "col", "shared", "diag", np.float64, True),
    (5, "colpad", "iso", "dense", np.float32, False),
    (5, "row", "diag", "diag", np.float64, False),
    (33, "col", "iso", "dense", np.float32, True),
    (33, "colpad", "diag", "diag", np.float64, True),
    (33, "row", "shared", "dense", np.float32, False),
    (64, "col", "diag", "dense", np.float64, False),
    (64, "colpad", "shared", "diag", np.float32, True),
    (64, "row", "iso", "dense", np.float64, True),
    (128, "col", "diag", "diag", np.float32, False),
    (128, "col", "iso", "dense", np.float64, True),
    (128, "colpad", "diag", "dense", np.float64, False),
    (128, "row", "shared", "diag", np.float32, True),
    (128, "row", "diag", "dense", np.float64, False),
]
_IDS = ["-".join(str(getattr(v, "__name__", v)) for v in c) for c in CASES]


def _mode(B, D, xkind, dtype):
    vec = 2 if dtype == np.float64 else 4
    return 1 if xkind == "row" else (4 if xkind == "col" and D % vec == 0 else 0)


@pytest.mark.parametrize("case", CASES, ids=_IDS)
def test_every_regressor_has_the_bits_of_the_single_call(B, case):
    """counts at every seam of grid_splits and of the 64-column stages in one batch: every output of every regressor equals
    blr_logpdf_grid_* with B = 1 on its slice; two calls give the same bits; the route names the statistics kernel"""
    D, xkind, noise, prior, dtype, shared = case
    probs = R.draw(7000 + D, D, R.COUNTS, noise, prior)
    pk = R.pack(B._abi, probs, xkind, noise, dtype)
    alpha, tau = R.grids(pk["nb"], shared)
    h = B._abi.default_handle()
    got = R.call_ragged(B, pk, alpha, tau, shared)
    route = h.last_route()
    assert h.get_stat("last_chunks") == 1
    tname = "double" if dtype == np.float64 else "float"
    assert route == f"ragged_evidence_stats_kernel<{tname}, {(D + 15) // 16}, {_mode(B, D, xkind, dtype)}>", route
    ref = R.call_singles(B, pk, alpha, tau, shared)
    assert np.all(ref["info"] == 0) and np.all(np.isfinite(ref["lp"])) and np.all(ref["best"] >= 0)
    R.same_bits(got, ref)
    R.same_bits(R.call_ragged(B, pk, alpha, tau, shared), got)


@pytest.mark.parametrize("case", [CASES[10], CASES[5], CASES[4]], ids=[_IDS[10], _IDS[5], _IDS[4]])
def test_host_and_device_memspace_same_bits(B, case):
    D, xkind, noise, prior, dtype, shared = case
    pk = R.pack(B._abi, R.draw(7100 + D, D, R.COUNTS, noise, prior), xkind, noise, dtype)
    alpha, tau = R.grids(pk["nb"], shared)
    R.same_bits(R.call_ragged(B, pk, alpha, tau, shared, device=True), R.call_ragged(B, pk, alpha, tau, shared))


@pytest.mark.parametrize("D,xkind,noise,dtype", [(64, "col", "diag", np.float64), (33, "row", "iso", np.float32)])
def test_permuting_or_growing_the_batch_changes_no_bits(B, D, xkind, noise, dtype):
    probs = R.draw(7200 + D, D, R.COUNTS, noise, "dense")
    alpha, tau = R.grids(len(probs), False)
    base = R.call_ragged(B, R.pack(B._abi, probs, xkind, noise, dtype), alpha, tau, False)
    perm = np.random.Generator(np.random.PCG64(3)).permutation(len(probs))
    moved = R.call_ragged(B, R.pack(B._abi, [probs[i] for i in perm], xkind, noise, dtype), alpha[perm], tau[perm], False)
    R.same_bits(moved, base, rows2=perm)
    extra = R.draw(7300, D, (3000,), noise, "dense")
    a9, t9 = R.grids(1, True)
    for at in (0, 4, len(probs)):  # in front, in the middle, behind
        grown = probs[:at] + extra + probs[at:]
        keep = [i for i in range(len(grown)) if i != at]
        r = R.call_ragged(B, R.pack(B._abi, grown, xkind, noise, dtype), np.insert(alpha, at, a9[0], axis=0), np.insert(tau, at, t9[0], axis=0), False)
        R.same_bits(r, base, rows1=keep)
    one = R.call_ragged(B, R.pack(B._abi, probs[3:4], xkind, noise, dtype), alpha[3:4], tau[3:4], False)
    R.same_bits(one, base, rows2=[3])  # the 9000-observation regressor alone (B = 1)
    g = 5
    alone = R.call_ragged(B, R.pack(B._abi, probs, xkind, noise, dtype), alpha[:, g:g + 1], tau[:, g:g + 1], False, want_post=False, want_best=False)
    assert np.array_equal(alone["lp"][:, 0], base["lp"][:, g]) and np.array_equal(alone["info"][:, 0], base["info"][:, g])


def _conditioned(p, a, t):
    """tests/test_grid_gpu.py's precondition, on the CPU: the oracle's two formulations agree to a tenth of the bounds"""
    X, y, s0, mw, L0 = p
    lp = O.logpdf_literal(mw, a * L0, X, t * s0, y)
    m, _, A = O.posterior_literal(mw, a * L0, X, t * s0, y)
    md, _, Ad, lpd = O.posterior_logpdf_direct(mw, a * L0, X, t * s0 if np.ndim(s0) else np.float64(t * s0), y)
    ok = (abs(lpd - lp) <= 0.1 * TOL_LP * abs(lp) and np.linalg.norm(md - m) <= 0.1 * TOL_MW * np.linalg.norm(m)
          and np.max(np.abs(Ad - A)) <= 0.1 * TOL_A * np.max(np.abs(A)))
    return ok, lp, m, A


# the counts of the bit tests without 0: with no observation the evidence is 0 up to rounding and a relative bound says nothing
# (that regressor is covered by the bit equality with blr_logpdf_grid_* at N = 0)
ORACLE_COUNTS = tuple(n for n in R.COUNTS if n > 0)


@pytest.mark.parametrize("D,xkind,noise,prior", [(33, "colpad", "diag", "dense"), (64, "row", "iso", "diag"), (128, "col", "diag", "dense")])
def test_against_the_oracle_f64(B, D, xkind, noise, prior):
    """every setting of every regressor against logpdf_literal (1e-10), the winner's posterior against posterior_literal (1e-9,
    1e-9), after the CPU conditioning check; a regressor that fails the check is re-drawn, never loosened"""
    probs = []
    for i, n in enumerate(ORACLE_COUNTS):
        for attempt in range(8):
            p = R.draw(7400 + 100 * D + 10 * i + 1000 * attempt, D, (n,), noise, prior)[0]
            refs = [_conditioned(p, a, t) for a, t in zip(R.ALPHA, R.TAU)]
            if all(r[0] for r in refs):
                break
        else:
            raise AssertionError(("no well-conditioned draw", D, n))
        probs.append((p, refs))
    pk = R.pack(B._abi, [p for p, _ in probs], xkind, noise, np.float64)
    alpha, tau = R.grids(pk["nb"], True)
    got = R.call_ragged(B, pk, alpha, tau, True)
    assert np.all(got["info"] == 0)
    for b, (p, refs) in enumerate(probs):
        for g, (_, lp_o, _, _) in enumerate(refs):
            e = abs(got["lp"][b, g] - lp_o) / abs(lp_o)
            print("evidence", D, pk["counts"][b], g, e)
            assert e <= TOL_LP, (b, g, got["lp"][b, g], lp_o)
        k = int(got["best"][b])
        assert k == int(np.argmax(got["lp"][b]))
        _, _, m_o, A_o = refs[k]
        T = got["T_best"][b].reshape(D, D).T  # column-major D x D
        assert np.all(np.tril(T, -1) == 0)
        e_m = np.linalg.norm(got["mw_best"][b] - m_o) / np.linalg.norm(m_o)
        e_A = np.max(np.abs(T.T @ T - A_o)) / np.max(np.abs(A_o))
        print("posterior", D, pk["counts"][b], k, e_m, e_A)
        assert e_m <= TOL_MW and e_A <= TOL_A, (b, k, e_m, e_A)


@pytest.mark.parametrize("D,xkind", [(33, "row"), (128, "col")])
def test_failures_stay_local(B, D, xkind):
    counts = (2049, 70, 0, 1500, 9)
    probs = R.draw(7500 + D, D, counts, "diag", "dense")
    alpha, tau = R.grids(len(probs), True)
    good = R.call_ragged(B, R.pack(B._abi, probs, xkind, "diag", np.float64), alpha, tau, True)
    assert np.all(good["info"] == 0)
    # a bad setting: status 1 for that setting only, the others keep their bits
    a_bad, t_bad = alpha.copy(), tau.copy()
    a_bad[:, 2], t_bad[:, 4], t_bad[:, 7] = 0.0, -1.0, np.nan
    keep = [g for g in range(9) if g not in (2, 4, 7)]
    bad = R.call_ragged(B, R.pack(B._abi, probs, xkind, "diag", np.float64), a_bad, t_bad, True)
    for g in (2, 4, 7):
        assert np.all(bad["info"][:, g] == 1) and np.all(np.isnan(bad["lp"][:, g]))
    assert np.array_equal(bad["lp"][:, keep], good["lp"][:, keep]) and np.all(bad["info"][:, keep] == 0)
    # a non-positive base noise entry: its 1-based index within the regressor's OWN slice, all G settings of that regressor only
    # (regressor 3, observation 1101: behind the first column block and behind the regressors packed in front of it)
    X, y, s0, mw, L0 = probs[3]
    s_bad = s0.copy()
    s_bad[1100], s_bad[1300] = -0.5, 0.0
    broken = list(probs)
    broken[3] = (X, y, s_bad, mw, L0)
    # ... and a base prior with a negative eigenvalue: its failing minor for all G settings of regressor 1 only
    X1, y1, s1, mw1, L1 = probs[1]
    w, V = np.linalg.eigh(L1)
    w[0] = -0.5
    L1b = (V * w) @ V.T
    broken[1] = (X1, y1, s1, mw1, L1b)
    minor = next(k for k in range(1, D + 1) if np.linalg.eigvalsh(L1b[:k, :k])[0] <= 0)
    pk = R.pack(B._abi, broken, xkind, "diag", np.float64)
    r = R.call_ragged(B, pk, alpha, tau, True, sentinel=-3.25)
    assert np.all(r["info"][3] == 1101) and np.all(np.isnan(r["lp"][3])) and r["best"][3] == -1
    assert np.all(r["info"][1] == minor) and np.all(np.isnan(r["lp"][1])) and r["best"][1] == -1
    for b in (1, 3):  # no winner: the sentinels stay
        assert np.all(r["mw_best"][b] == -3.25) and np.all(r["T_best"][b] == -3.25)
    R.same_bits(r, good, rows1=[0, 2, 4], rows2=[0, 2, 4])
    R.same_bits(r, R.call_singles(B, pk, alpha, tau, True, sentinel=-3.25))


def test_optional_arguments(B):
    """alpha = NULL, tau = NULL (all ones, G = 1), best = NULL, no refit outputs"""
    probs = R.draw(7600, 40, (5, 0, 1300, 64), "iso", "diag")
    pk = R.pack(B._abi, probs, "col", "iso", np.float64)
    ones = np.ones((4, 1))
    full = R.call_ragged(B, pk, ones, ones, True)
    for a, t in ((None, None), (None, ones), (ones, None)):
        r = R.call_ragged(B, pk, a, t, True, want_best=False, want_post=False)
        assert np.array_equal(r["lp"], full["lp"]) and np.array_equal(r["info"], full["info"])
    assert np.all(full["best"] == 0)
    # the refit with one of its two outputs NULL
    only_mw = R.call_ragged(B, pk, ones, ones, True, want_post="mw")
    only_T = R.call_ragged(B, pk, ones, ones, True, want_best=False, want_post="T")
    assert only_mw["T_best"] is None and np.array_equal(only_mw["mw_best"], full["mw_best"]) and np.array_equal(only_mw["best"], full["best"])
    assert only_T["mw_best"] is None and np.array_equal(only_T["T_best"], full["T_best"]) and np.array_equal(only_T["lp"], full["lp"])


def test_d144_goes_one_by_one_with_the_single_calls_bits(B):
    for noise, prior, xkind in (("diag", "dense", "col"), ("iso", "diag", "row")):
        pk = R.pack(B._abi, R.draw(7700, 144, (0, 7, 200), noise, prior), xkind, noise, np.float64)
        alpha, tau = R.grids(3, False)
        R.same_bits(R.call_ragged(B, pk, alpha, tau, False), R.call_singles(B, pk, alpha, tau, False))


# ---- the Python front ------------------------------------------------------------------------------------------------------------------
def _same_grid(g1, g2):
    assert np.array_equal(g1.logpdf, g2.logpdf, equal_nan=True) and g1.best == g2.best
    assert np.array_equal(g1.alpha, g2.alpha) and np.array_equal(g1.tau, g2.tau)


@pytest.mark.parametrize("prior", ["diag", "dense", "pdmat"])
def test_python_packed_front_equals_the_list(B, prior):
    D, counts = 24, (300, 0, 17, 1100)
    rng = np.random.Generator(np.random.PCG64(7800))
    offsets = np.concatenate(([0], np.cumsum(counts)))
    X = rng.standard_normal((D, offsets[-1]))
    y = rng.standard_normal(offsets[-1])
    s = np.exp(0.3 * rng.standard_normal(offsets[-1]))
    Bm = rng.standard_normal((D, D))
    Lw = {"diag": B.Diagonal(np.exp(0.3 * rng.standard_normal(D))), "dense": Bm @ Bm.T / D + np.eye(D),
          "pdmat": B.PDMat(np.linalg.cholesky(Bm @ Bm.T / D + np.eye(D)).T)}[prior]
    f = B.BayesianLinearRegressor(0.3 * rng.standard_normal(D), Lw)
    ps, ns = [0.1, 1.0, 10.0], [0.5, 2.0]
    grids = B.logpdf_grid_ragged(f, B.ColVecs(X), offsets, B.Diagonal(s), y, ps, ns)
    posts, grids2 = B.posterior_best_ragged(f, B.ColVecs(X), offsets, B.Diagonal(s), y, ps, ns)
    assert len(grids) == len(posts) == len(grids2) == len(counts)
    for b in range(len(counts)):
        sl = slice(offsets[b], offsets[b + 1])
        fx = f(B.ColVecs(np.asfortranarray(X[:, sl])), B.Diagonal(s[sl]))
        _same_grid(grids[b], B.logpdf_grid(fx, y[sl], ps, ns))
        _same_grid(grids2[b], grids[b])
        post, g1 = B.posterior_best(fx, y[sl], ps, ns)
        _same_grid(g1, grids[b])
        assert type(posts[b].Lw) is type(post.Lw) and np.array_equal(posts[b].mw, post.mw)
        assert np.array_equal(posts[b].Lw.toarray(), post.Lw.toarray())
    assert B.logpdf_grid_ragged(f, B.ColVecs(X[:, :0]), [0], 0.5, y[:0]) == []


def test_posterior_best_ragged_raises_with_the_index_of_the_first_failure(B):
    D = 6
    rng = np.random.Generator(np.random.PCG64(7900))
    offsets = np.array([0, 10, 30, 45])
    X, y = rng.standard_normal((D, 45)), rng.standard_normal(45)
    s = np.ones(45)
    s[12] = -1.0  # observation 3 of regressor 1
    with pytest.raises(B._abi.PosDefException) as e:
        B.posterior_best_ragged(B.BayesianLinearRegressor(np.zeros(D), B.Diagonal(np.ones(D))), B.ColVecs(X), offsets, B.Diagonal(s), y, [1.0, 2.0])
    assert e.value.index == 1 and e.value.info == 3


# how the problems of logpdf_grid_map are handed over -> (container, the library's layout): each of the four (container, memory order)
# pairs, so that both branches of the packing run
_CONTAINERS = {
    "ColVecs-F": (lambda B, X: B.ColVecs(np.asfortranarray(X)), "col"),         # D x N column-major
    "RowVecs-C": (lambda B, X: B.RowVecs(np.ascontiguousarray(X.T)), "col"),    # N x D row-major: the same memory
    "RowVecs-F": (lambda B, X: B.RowVecs(np.asfortranarray(X.T)), "row"),       # N x D column-major
    "ColVecs-C": (lambda B, X: B.ColVecs(np.ascontiguousarray(X)), "row"),      # D x N row-major: the same memory
}


@pytest.mark.parametrize("kind", list(_CONTAINERS))
def test_grid_map_packs_problems_that_differ_only_in_n(B, kind):
    """problems that differ only in N -- one of them empty, whose layout is ambiguous -- go out in ONE call of
    blr_logpdf_grid_ragged_*: the handle's route, set to another kernel's by an ordinary update just before, names the new
    statistics kernel with the loader of the batch's layout afterwards; every result equals the per-problem call's"""
    from blr_amd import regressor as Rg

    wrap, lay = _CONTAINERS[kind]
    D = 20
    rng = np.random.Generator(np.random.PCG64(8000))
    f = B.BayesianLinearRegressor(0.1 * rng.standard_normal(D), B.Diagonal(np.exp(0.2 * rng.standard_normal(D))))
    h = B._abi.default_handle()
    ps, ns = [0.1, 1.0, 10.0], [0.1, 1.0, 10.0]
    fxs, ys = [], []
    for n in (40, 1500, 0, 7):
        fxs.append(f(wrap(B, rng.standard_normal((D, n))), 0.3 + 0.1 * len(fxs)))
        ys.append(rng.standard_normal(n))
    want = B._abi.LAYOUT_COLVECS if lay == "col" else B._abi.LAYOUT_ROWVECS
    assert all(Rg._x_layout(fx.x, np.float64)[1] == want for fx in fxs if len(fx.x) > 0)  # the case is what its name says
    B.logpdf(fxs[0], ys[0])
    assert "ragged_evidence" not in h.last_route()
    many = B.logpdf_grid_map(fxs, ys, ps, ns)
    assert h.last_route() == f"ragged_evidence_stats_kernel<double, 2, {4 if lay == 'col' else 1}>", h.last_route()
    for fx, y, g in zip(fxs, ys, many):
        _same_grid(g, B.logpdf_grid(fx, y, ps, ns))
    # a problem of another D, noise kind or prior kind: one call per problem, as before
    B.logpdf(fxs[0], ys[0])
    other = B.BayesianLinearRegressor(np.zeros(D + 1), B.Diagonal(np.ones(D + 1)))(wrap(B, rng.standard_normal((D + 1, 5))), 0.5)
    mixed = B.logpdf_grid_map(fxs[:2] + [other], ys[:2] + [rng.standard_normal(5)], ps, ns)
    assert "ragged_evidence" not in h.last_route()
    _same_grid(mixed[0], many[0])
    _same_grid(mixed[1], many[1])
