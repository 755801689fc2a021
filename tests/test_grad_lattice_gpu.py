"""blr_logpdf_grad_batched_* for D <= 128 on both device routes -- logpdf_grad_kernel (sweeps) and marg_image_kernel +
grad_gemm_kernel (products), each followed by grad_reduce_kernel -- against truth, through the C ABI (_abi.Handle): block counts,
tile walks, the gate between the routes, optional outputs and a failed regressor.  Problems, truth, yardstick, the bound and the
host restatement of which walk a case takes: tests/_grad_problems.py (checked without a GPU by tests/test_grad_problems_cpu.py).

Every judged output obeys  err_gpu <= 4 err_yardstick + FLOOR eps,  err = max |got - truth| / max |truth| per regressor.

Measured on the MI355X over every case of this file (worst over cases and regressors; "ratio" = err_gpu / err_yardstick where the
yardstick's error is not 0, "floor needed" = max (err_gpu - 4 err_yardstick) / eps, "floor" = _grad_problems.FLOOR):

    output    dtype   worst ratio   floor needed   floor
    logpdf    f64         64.02           2.55        4
    dX        f64         21.02           2.93        4
    dy        f64          5.12           0.39        0.5
    ds        f64          5.32           1.69        2
    dmw       f64          6.81           1.53        2
    mw_post   f64          5.72           2.34        4
    Ainv      f64          7.79           4.13        8
    logpdf    f32         33.85           1.67        2
    dX        f32          6.81           5.65        8
    dy        f32         28.73           0.81        1
    ds        f32          6.48           1.74        2
    dmw       f32          2.55           0.00        0
    mw_post   f32         10.23           5.31        8
    Ainv      f32         99.81           7.82        8
(the large ratios belong to N = 1 and D = 1 problems NumPy solves nearly exactly; the bound's floor is what covers them)

dmw is what grad_reduce_kernel's refinement step buys: the plain sum X W r at the rounded fp32 posterior mean missed the bound at
D = 1, N = 65 (RowVecs, diagonal prior and noise) by 53 eps -- the sum cancels 16 - 32 fold there and carried the mean's 7.7 eps
with that factor -- and needed floors of 8 (fp32) and 8 (fp64) elsewhere.
"""
import numpy as np
import pytest

import _grad_problems as GP

pytestmark = pytest.mark.gpu

F64, F32 = GP.F64, GP.F32
ids = lambda cases: [c["id"] for c in cases]  # noqa: E731


@pytest.fixture(scope="module")
def B():
    import blr_amd

    blr_amd._abi.default_handle()  # raises if the extension or the GPU is missing: no silent fallback
    return blr_amd


@pytest.fixture
def opt(B):
    """Run-time switches of the process-wide handle (blr_set_option), restored to their defaults after the test."""
    h = B._abi.default_handle()
    touched = []

    def set_(key, value):
        h.set_option(key, value)
        touched.append(key)

    yield set_
    for key in touched:
        h.set_option(key, None)


def run(B, opt, c, null=(), no_gemm=None):
    """one call of the case on the process-wide handle -> (outs, the filled flat arrays)"""
    h = B._abi.default_handle()
    opt("NO_GRAD_GEMM", "1" if (c["no_gemm"] if no_gemm is None else no_gemm) else None)
    ins, outs = GP.pack(c)
    return outs, GP.call(h, c, ins, outs, null=null)


def check(c, outs, got, regs=None):
    """padding kept, status, and every returned output of the regressors `regs` (default: all) within the bound"""
    for k, a in got.items():
        assert outs[k].gaps_kept(a), f"{k}: padding overwritten"
    info = outs["info"].payload(got["info"])[0]
    good = [b for b in range(c["B"]) if b != c["bad"]] if regs is None else regs
    assert not info[good].any(), info
    return GP.judge(GP.case_problem(c), GP.payloads(c, outs, got), regs=good, what=c["id"])


def same_bits(outs, got1, got2, keys=None, regs=None):
    for k in (keys if keys is not None else got1):
        a, b = outs[k].per_regressor(got1[k]), outs[k].per_regressor(got2[k])
        if regs is not None:
            a, b = a[regs], b[regs]
        assert np.array_equal(a, b, equal_nan=True), f"{k}: the bits differ"


# ---- the sweep route: block counts x tile counts x dtype x layout x noise x prior --------------------------------------------------
@pytest.mark.parametrize("c", GP.SWEEP_BLOCKS, ids=ids(GP.SWEEP_BLOCKS))
def test_sweep_blocks(B, opt, c):
    outs, got = run(B, opt, c)
    check(c, outs, got)


@pytest.mark.parametrize("dt", [F64, F32], ids=["f64", "f32"])
def test_no_observations_are_refused(B, opt, dt):
    # include/blr_mi355x.h takes the arguments of blr_posterior_batched_* but this entry point documents no N = 0: the call is an
    # argument error (N is argument 6) and touches no output
    c = GP.case(dt, "col", 3, 17, 1, "diag", "diag")
    ins, outs = GP.pack(c)
    h = B._abi.default_handle()
    v = {k: o.a.copy() for k, o in outs.items()}
    with pytest.raises(B._abi.BLRError, match="N out of range"):
        h.logpdf_grad_batched(dt, B._abi.MEM_HOST, B._abi.LAYOUT_COLVECS, 3, 17, 0, ins["X"], c["ldx"], c["strideX"], ins["y"], 1, B._abi.NOISE_DIAGONAL,
                              ins["s"], 1, B._abi.PRIOR_DIAGONAL, ins["mw"], 17, ins["Lw"], 1, 17, v["logpdf"], v["dX"], outs["dX"].ld, outs["dX"].stride,
                              v["dy"], outs["dy"].stride, v["ds"], outs["ds"].stride, v["dmw"], outs["dmw"].stride, v["mw_post"],
                              outs["mw_post"].stride, v["Ainv"], outs["Ainv"].ld, outs["Ainv"].stride, v["info"])
    for k, o in outs.items():
        assert np.array_equal(v[k].view(np.uint8), o.a.view(np.uint8)), k


# ---- the sweep route: workgroups that walk several tiles ------------------------------------------------------------------------------
@pytest.mark.parametrize("c", GP.SWEEP_WALKS, ids=ids(GP.SWEEP_WALKS))
def test_sweep_walks(B, opt, c):
    outs, got = run(B, opt, c)
    check(c, outs, got)


# ---- the product route -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", GP.PRODUCTS, ids=ids(GP.PRODUCTS))
def test_products(B, opt, c):
    outs, got = run(B, opt, c)
    check(c, outs, got)


@pytest.mark.parametrize("dt", [F64, F32], ids=["f64", "f32"])
def test_a_failed_regressor_on_both_routes(B, opt, dt):
    # include/blr_mi355x.h: info names the regressor, its logpdf is NaN, its dmw is zeros and its other outputs are left untouched,
    # on either route; every other regressor stays within the bound
    prod, sweep = [c for c in GP.BROKEN if c["dt"] == dt]
    assert GP.takes_products(prod) and not GP.takes_products(sweep) and prod["bad"] == sweep["bad"] == 2
    res = []
    for c in (prod, sweep):
        outs, got = run(B, opt, c)
        check(c, outs, got)
        info = outs["info"].payload(got["info"])[0]
        assert info[c["bad"]] > 0 and np.count_nonzero(info) == 1, info
        assert np.isnan(outs["logpdf"].payload(got["logpdf"])[0][c["bad"]])
        assert np.all(outs["dmw"].per_regressor(got["dmw"])[c["bad"]] == 0)
        for k in ("dX", "dy", "ds", "mw_post", "Ainv"):
            assert np.array_equal(outs[k].per_regressor(got[k])[c["bad"]].view(np.uint8), outs[k].per_regressor(outs[k].a)[c["bad"]].view(np.uint8)), k
        res.append((outs, got))
    same_bits(res[0][0], res[0][1], res[1][1], keys=("info", "logpdf", "mw_post"))  # the posterior kernel is shared
    same_bits(res[0][0], res[0][1], res[1][1], regs=[2])                             # the failed regressor: the same on both routes


# ---- the gate between the routes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c,same", GP.GATES, ids=ids([g for g, _ in GP.GATES]))
def test_gate(B, opt, c, same):
    # A case that fails the gate is already on the sweep route, whose reductions have a fixed order: NO_GRAD_GEMM changes no bit.
    # A case that passes it must change at least one bit of dX -- the switch really switches.
    outs, got = run(B, opt, c, no_gemm=False)
    check(c, outs, got)
    outs2, forced = run(B, opt, c, no_gemm=True)
    check(c, outs2, forced)
    if same:
        same_bits(outs, got, forced)
    else:
        assert not np.array_equal(outs["dX"].payload(got["dX"]), outs["dX"].payload(forced["dX"])), "the product route gave the sweep route's bits"


# ---- optional outputs ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", GP.OPTIONALS, ids=ids(GP.OPTIONALS))
def test_optional_outputs(B, opt, c):
    outs, full = run(B, opt, c)
    check(c, outs, full)
    for null in [(k,) for k in GP.OPTIONAL] + [GP.OPTIONAL]:
        _, got = run(B, opt, c, null=null)
        assert set(got) == set(outs) - set(null)
        for k, a in got.items():
            assert outs[k].gaps_kept(a), f"{k}: padding overwritten without {null}"
        keys = set(got)
        if "Ainv" in null and not GP.takes_products(c):
            # without A^-1 the sweep route has no pseudo tiles: fewer workgroups per regressor, another partition of dmw's sum --
            # held to the truth bound, not to the bits
            keys.discard("dmw")
        same_bits(outs, full, got, keys=keys)
        GP.judge(GP.case_problem(c), GP.payloads(c, outs, got), what=f"{c['id']} without {','.join(null)}")
