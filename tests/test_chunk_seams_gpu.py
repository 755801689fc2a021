"""Every batched entry point across its regressor-chunk seams (csrc/blr_abi.hip cuts a batch into several launches beyond grid.y =
65535, the 256 MiB of triangular-inverse images, or a workspace bound, and re-derives every operand's pointer per chunk).

Capped seams: B = 7 with option MAX_CHUNK = 3 -- chunks of 3, 3, 1: a partial last chunk, two non-zero chunk origins -- on the code
an over-bound batch walks.  Every regressor has its own X, targets, noise, mean and factor; regressor 4 (second chunk) is broken
where the entry point reports it; every output sits in a sentinel-filled array with padded strides.  Each call is compared (a) with
the fp64 oracle per regressor, at the tolerance the entry point's own GPU test file uses (cited at TOL), (b) with the same call on the
same handle without the cap (rtol / atol 1e-12 in fp64 as tests/test_loo_gpu.py:189 and tests/test_loo_multi_gpu.py:195 hold between
two routes; fp32: the 1e-5 of tests/test_gpu_parity.py:1258 -- not bits: per_reg depends on the chunk's size), (c) info exactly,
(d) blr_get_stat "last_chunks" == 3.

Real bounds, no option: grid.y at B = 65537 (D = 3, N = 5; where images are needed they cut the batch first and only the status
loop crosses 65535 -- the test names say which) against the vectorised restatement of tests/_seam_problems.py (pinned to
the oracle by tests/test_seam_problems_cpu.py), and the image bound at B = kMaxChunk + 2 (D = 128, N = 64, shared X).

Crossing kLooWorkspace / per, kDowndateWorkspace / per and the 32768 of the state-columns route for real takes 2 - 4 GB of state:
those seams are covered by capped cases only."""
import math

import numpy as np
import pytest

import _seam_problems as SP

pytestmark = pytest.mark.gpu

B7, CAP, BAD = 7, 3, 4
F64, F32 = np.float64, np.float32

# (rtol on variances and logpdfs, rtol = atol on means) against the oracle, by entry point and dtype:
TOL = {
    # tests/test_gpu_parity.py:897-905 and :988-997 (marginals, every route: mean rtol = rt, atol = 10 rt; var rtol = rt)
    ("marginals", "float64"): 1e-10, ("marginals", "float32"): 3e-4,
    # tests/test_gpu_parity.py:1260 (the D = 128 product stream)
    ("marginals128", "float64"): 1e-9, ("marginals128", "float32"): 5e-4,
    # tests/test_marg_multi_gpu.py:142 / :344
    ("marginals_multi", "float64"): 1e-10, ("marginals_multi", "float32"): 2e-4,
    # tests/test_loo_gpu.py:139-141 (fp64: rtol = atol = 1e-9) and :150-152 (fp32: 1e-3); tests/test_loo_multi_gpu.py:171-173
    ("loo", "float64"): 1e-9, ("loo", "float32"): 1e-3,
}


@pytest.fixture(scope="module")
def handle():
    from blr_amd import _abi
    h = _abi.Handle(0)
    yield h
    h.set_option("MAX_CHUNK", None)
    h.close()


def run(h, memspace, ins, outs, call):
    """-> {output name: the filled flat array}"""
    from blr_amd import _abi
    if memspace == _abi.MEM_HOST:
        got = {k: o.a.copy() for k, o in outs.items()}
        call(h, memspace, {**ins, **got})
        return got
    ptrs = {}
    try:
        for k, a in ins.items():
            ptrs[k] = None if a is None else h.device_alloc(a.nbytes)
            if a is not None:
                h.memcpy_h2d(ptrs[k], a)
        for k, o in outs.items():
            ptrs[k] = h.device_alloc(o.a.nbytes)
            h.memcpy_h2d(ptrs[k], o.a)
        call(h, memspace, ptrs)
        h.synchronize()
        got = {k: np.empty_like(o.a) for k, o in outs.items()}
        for k in outs:
            h.memcpy_d2h(got[k], ptrs[k])
    finally:
        for q in ptrs.values():
            if q:
                h.device_free(q)
    return got


def flat(a, dt):
    return None if a is None else np.ascontiguousarray(a, dtype=dt).ravel()


class Case:
    """ins / outs / call; the oracle's payloads `ref` {name: (array, rtol, atol[, fn])} (fn maps one regressor's payload to what is
    compared); `bad`: the regressors whose status must be non-zero; `pair` {name: (rtol, atol)}: capped against uncapped where the
    default of check_capped does not apply"""

    def __init__(self, ins, outs, call, ref, breaks, B=B7, bad=(BAD,), pair=None):
        self.ins, self.outs, self.call, self.ref, self.B = ins, outs, call, ref, B
        self.bad = tuple(b % B for b in bad) if breaks else ()
        self.pair = pair or {}


def pair_tol(dt, name):
    """capped against uncapped: fp64 rtol = atol = 1e-12 (tests/test_loo_gpu.py:189, tests/test_loo_multi_gpu.py:195-197); fp32 as two
    routes of one product in tests/test_gpu_parity.py:1257-1258: means rtol = atol = 1e-5, everything else rtol 1e-6"""
    if dt == F64:
        return 1e-12, 1e-12
    return (1e-5, 1e-5) if name in ("mean", "lm") else (1e-6, 0.0)


def check_capped(h, case, dt, host=False, chunks=3):
    from blr_amd import _abi
    h.set_option("MAX_CHUNK", None)
    base = run(h, _abi.MEM_DEVICE, case.ins, case.outs, case.call)
    assert h.get_stat("last_chunks") == 1
    h.set_option("MAX_CHUNK", str(CAP))
    try:
        runs = [run(h, _abi.MEM_DEVICE, case.ins, case.outs, case.call)]
        assert h.get_stat("last_chunks") == chunks                                      # (d)
        if host:
            runs.append(run(h, _abi.MEM_HOST, case.ins, case.outs, case.call))
            assert h.get_stat("last_chunks") == chunks
    finally:
        h.set_option("MAX_CHUNK", None)
    good = [b for b in range(case.B) if b not in case.bad]
    for got in runs:
        info = case.outs["info"].payload(got["info"])[0]
        print("info", info.tolist())
        assert np.array_equal(info, case.outs["info"].payload(base["info"])[0])          # (c)
        assert all(info[b] != 0 for b in case.bad) and not info[good].any(), info
        for k, o in case.outs.items():
            assert o.gaps_kept(got[k]), f"{k}: padding overwritten"
            if k == "info":
                continue
            pay, pay0 = o.per_regressor(got[k]).astype(F64), o.per_regressor(base[k]).astype(F64)
            print(k, "capped vs uncapped: max abs diff", np.abs(pay[good] - pay0[good]).max())
            prt, pat = case.pair.get(k, pair_tol(dt, k))
            np.testing.assert_allclose(pay[good], pay0[good], rtol=prt, atol=pat, err_msg=f"{k}: capped vs uncapped")   # (b)
            for b in case.bad:
                assert np.array_equal(pay[b], pay0[b], equal_nan=True), f"{k}: the broken regressor's output differs"
            ref, rtol, atol = case.ref[k][:3]
            fn = case.ref[k][3] if len(case.ref[k]) > 3 else (lambda v: v)
            for b in good:
                v = fn(pay[b])
                print(k, b, "vs oracle: max abs err", np.abs(v - ref[b]).max())
                np.testing.assert_allclose(v, ref[b], rtol=rtol, atol=atol, err_msg=f"{k}: regressor {b} against the oracle")   # (a)


def x_arg(p, layout, dt):
    """-> (X flat, ldx, strideX) of a batch's inputs in the layout (RowVecs: N x D column-major)"""
    from blr_amd import _abi
    X = p["X"]
    sx = 0 if X.shape[0] == 1 and p["B"] > 1 else p["N"] * p["D"]
    if layout == _abi.LAYOUT_COLVECS:
        return flat(X, dt), p["D"], sx
    return flat(np.swapaxes(X, 1, 2), dt), p["N"], sx


def rounded(p, dt):
    """the batch as the device sees it: every operand rounded to dt, then back in fp64 for the oracle"""
    q = dict(p)
    for k in ("X", "y", "Y", "s", "mw", "M", "U"):
        q[k] = p[k].astype(dt).astype(F64)
    return q


# ---- blr_marginals_batched_* ----------------------------------------------------------------------------------------------------
def marginals_case(dt, D, N, layout, prior, mean_only=False, B=B7, seed=1, shared_x=False, bad=(BAD,)):
    from blr_amd import _abi
    lay = _abi.LAYOUT_COLVECS if layout == "col" else _abi.LAYOUT_ROWVECS
    p = rounded(SP.batch(B, D, N, 1, seed=seed + D + N, shared_x=shared_x), dt)
    breaks = False
    Mw = p["mw"][:, None, :]
    if prior == "diag":
        dprec = (0.5 + np.abs(p["mw"][:, ::-1])).astype(dt).astype(F64)
        Lw, kind, ldl, sl = dprec, _abi.PRIOR_DIAGONAL, D, D
        mean_o, var_o = SP.diag_marginals_ref(p["X"], Mw, dprec, p["s"])
    elif prior == "factor":
        Lw, kind, ldl, sl = p["U"].copy(), _abi.PRIOR_UPPER_FACTOR, D, D * D
        mean_o, var_o = SP.marginals_ref(p["X"], Mw, p["U"], p["s"])
        if D > 128 and not mean_only:  # (D <= 128 takes a factor as it is: nothing reports there)
            Lw[list(bad), 2, 2] = -1.0
            breaks = True
    else:  # dense precision U'U, formed in fp64 and rounded: the oracle factors what the device gets
        Uu = SP.upper(p)
        Lw = (np.swapaxes(Uu, 1, 2) @ Uu).astype(dt).astype(F64)
        kind, ldl, sl = _abi.PRIOR_DENSE, D, D * D
        Ucm = np.linalg.cholesky(Lw)  # lower L = U' row-major == U column-major
        mean_o, var_o = SP.marginals_ref(p["X"], Mw, Ucm, p["s"])
        if not mean_only:
            Lw[list(bad), 2, 2] = -50.0
            breaks = True
    X, ldx, sx = x_arg(p, lay, dt)
    ins = {"X": X, "s": flat(p["s"], dt), "mw": flat(p["mw"], dt), "Lw": flat(Lw, dt)}
    outs = {"mean": SP.Out(dt, N, nb=B), "info": SP.Out(np.int32, B)}
    if not mean_only:
        outs["var"] = SP.Out(dt, N, nb=B)
    sm = outs["mean"].stride

    def call(h, m, v):
        h.marginals_batched(dt, m, lay, B, D, N, v["X"], ldx, sx, _abi.NOISE_DIAGONAL, v["s"], N, kind, v["mw"], D, v["Lw"], ldl, sl, v["mean"], sm,
                            v.get("var"), sm, v["info"])

    rt = TOL[("marginals128" if D == 128 and prior == "factor" and not mean_only else "marginals", np.dtype(dt).name)]
    ref = {"mean": (mean_o[:, 0, :], rt, 10 * rt), "var": (var_o, rt, 0.0)}
    return Case(ins, outs, call, ref, breaks, B, bad)


MARG = [(5, 40, "col", "diag", False), (5, 40, "col", "factor", False), (5, 40, "col", "dense", False), (5, 40, "col", "factor", True),
        (128, 64, "col", "factor", False), (128, 64, "row", "factor", False), (144, 40, "col", "factor", False), (144, 40, "col", "dense", False)]


@pytest.mark.parametrize("dt", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("D,N,layout,prior,mean_only", MARG, ids=[f"D{d}-N{n}-{l}-{p}{'-meanonly' if m else ''}" for d, n, l, p, m in MARG])
def test_marginals_capped(handle, dt, D, N, layout, prior, mean_only):
    check_capped(handle, marginals_case(dt, D, N, layout, prior, mean_only), dt, host=(D == 5 and prior == "factor" and not mean_only))


# ---- blr_loo_batched_* ------------------------------------------------------------------------------------------------------------
def loo_case(dt, D, N, mode, B=B7, seed=2, shared_x=False, bad=(BAD,)):
    """mode: "full" (all outputs), "total" (loo_total alone: the log densities live in the chunk's workspace), "empty" (N = 0)"""
    from blr_amd import _abi
    lay = _abi.LAYOUT_COLVECS
    p = rounded(SP.batch(B, D, N, 1, seed=seed + D + N, shared_x=shared_x), dt)
    Mpost, T = SP.condition(p)
    Mpost, T = Mpost.astype(dt).astype(F64), T.astype(dt).astype(F64)
    mean_o, var_o, lp_o, tot_o = SP.loo_ref(p["X"], Mpost, T, p["s"], p["y"][:, None, :])
    Tin = T.copy()
    Tin[[b % B for b in bad], 2, 2] = -1.0
    X, ldx, sx = x_arg(p, lay, dt)
    n = 0 if mode == "empty" else N
    ins = {"X": X, "y": flat(p["y"], dt), "s": flat(p["s"], dt), "mw": flat(Mpost, dt), "T": flat(Tin, dt)}
    outs = {"total": SP.Out(F64, B), "info": SP.Out(np.int32, B)}
    if mode == "full":
        outs.update(lm=SP.Out(dt, N, nb=B), lv=SP.Out(dt, N, nb=B), ll=SP.Out(F64, N, nb=B))
    st = N + 3

    def call(h, m, v):
        h.loo(dt, m, lay, B, D, n, v["X"], ldx, sx, v["y"], N, _abi.NOISE_DIAGONAL, v["s"], N, v["mw"], D, v["T"], D, D * D, v.get("lm"), st,
              v.get("lv"), st, v.get("ll"), st, v["total"], v["info"])

    rt = TOL[("loo", np.dtype(dt).name)]
    # total = a sum of N log densities, each within rt (relative and absolute) of the oracle's: rt on the sum, N rt absolute
    tot_ref = np.zeros((B, 1)) if mode == "empty" else tot_o
    ref = {"lm": (mean_o[:, 0, :], rt, rt), "lv": (var_o, rt, 0.0), "ll": (lp_o[:, 0, :], rt, rt), "total": (tot_ref, rt, N * rt)}
    return Case(ins, outs, call, ref, True, B, bad)


@pytest.mark.parametrize("dt", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("mode", ["full", "total"])
@pytest.mark.parametrize("D,N", [(128, 64), (5, 40), (144, 40)], ids=["fused-D128", "composed-D5", "composed-D144"])
def test_loo_capped(handle, dt, D, N, mode):
    check_capped(handle, loo_case(dt, D, N, mode), dt, host=(D == 5 and mode == "full"))


@pytest.mark.parametrize("dt", [F64, F32], ids=["f64", "f32"])
def test_loo_empty_totals_capped(handle, dt):
    check_capped(handle, loo_case(dt, 5, 40, "empty"), dt)


# ---- blr_loo_multi_batched_* / blr_marginals_multi_batched_* ------------------------------------------------------------------------
def loo_multi_case(dt, D, N, S, layout, mode, B=B7, seed=3, shared_x=False, bad=(BAD,)):
    from blr_amd import _abi
    lay = _abi.LAYOUT_COLVECS if layout == "col" else _abi.LAYOUT_ROWVECS
    p = rounded(SP.batch(B, D, N, S, seed=seed + D + N, shared_x=shared_x), dt)
    Mpost, T = SP.condition(p, p["Y"])
    Mpost, T = Mpost.astype(dt).astype(F64), T.astype(dt).astype(F64)
    mean_o, var_o, lp_o, tot_o = SP.loo_ref(p["X"], Mpost, T, p["s"], p["Y"])
    Tin = T.copy()
    Tin[[b % B for b in bad], 2, 2] = -1.0
    X, ldx, sx = x_arg(p, lay, dt)
    ins = {"X": X, "Y": flat(p["Y"], dt), "s": flat(p["s"], dt), "M": flat(Mpost, dt), "T": flat(Tin, dt)}
    outs = {"total": SP.Out(F64, S, nb=B), "info": SP.Out(np.int32, B)}
    if mode == "full":
        outs.update(lm=SP.Out(dt, N, cols=S, nb=B), lv=SP.Out(dt, N, nb=B), ll=SP.Out(F64, N, cols=S, nb=B))
    ld, stm, stv, stt = N + 3, (S - 1) * (N + 3) + N + 3, N + 3, outs["total"].stride

    def call(h, m, v):
        h.loo_multi_batched(dt, m, lay, B, D, N, S, v["X"], ldx, sx, v["Y"], N, N * S, _abi.NOISE_DIAGONAL, v["s"], N, v["M"], D, D * S, v["T"], D,
                            D * D, v.get("lm"), ld, stm, v.get("lv"), stv, v.get("ll"), ld, stm, v["total"], stt, v["info"])

    rt = TOL[("loo", np.dtype(dt).name)]
    ref = {"lm": (mean_o, rt, rt), "lv": (var_o, rt, 0.0), "ll": (lp_o, rt, rt), "total": (tot_o, rt, N * rt)}
    return Case(ins, outs, call, ref, True, B, bad)


MULTI = [(20, 70, "col"), (128, 64, "col"), (128, 64, "row"), (144, 40, "col")]


@pytest.mark.parametrize("dt", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("mode", ["full", "total"])
@pytest.mark.parametrize("D,N,layout", MULTI, ids=[f"D{d}-N{n}-{l}" for d, n, l in MULTI])
def test_loo_multi_capped(handle, dt, D, N, layout, mode):
    check_capped(handle, loo_multi_case(dt, D, N, 3, layout, mode), dt, host=(D == 20 and mode == "full"))


def marg_multi_case(dt, D, N, S, layout, prior, mean_only=False, B=B7, seed=4, shared_x=False, bad=(BAD,)):
    from blr_amd import _abi
    lay = _abi.LAYOUT_COLVECS if layout == "col" else _abi.LAYOUT_ROWVECS
    p = rounded(SP.batch(B, D, N, S, seed=seed + D + N, shared_x=shared_x), dt)
    breaks = False
    if prior == "diag":
        dprec = (0.5 + np.abs(p["mw"][:, ::-1])).astype(dt).astype(F64)
        Lw, kind, ldl, sl = dprec, _abi.PRIOR_DIAGONAL, D, D
        mean_o, var_o = SP.diag_marginals_ref(p["X"], p["M"], dprec, p["s"])
    elif prior == "dense":  # (the only prior D <= 128 reports: its Cholesky's status, then read by the image kernel)
        Uu = SP.upper(p)
        Lw = (np.swapaxes(Uu, 1, 2) @ Uu).astype(dt).astype(F64)
        kind, ldl, sl = _abi.PRIOR_DENSE, D, D * D
        mean_o, var_o = SP.marginals_ref(p["X"], p["M"], np.linalg.cholesky(Lw), p["s"])
        Lw[list(bad), 2, 2] = -50.0
        breaks = True
    else:
        Lw, kind, ldl, sl = p["U"].copy(), _abi.PRIOR_UPPER_FACTOR, D, D * D
        mean_o, var_o = SP.marginals_ref(p["X"], p["M"], p["U"], p["s"])
        if D > 128 and not mean_only:  # (as blr_marginals_batched_*: D <= 128 takes a factor as it is)
            Lw[list(bad), 2, 2] = -1.0
            breaks = True
    X, ldx, sx = x_arg(p, lay, dt)
    ins = {"X": X, "s": flat(p["s"], dt), "M": flat(p["M"], dt), "Lw": flat(Lw, dt)}
    outs = {"mean": SP.Out(dt, N, cols=S, nb=B), "info": SP.Out(np.int32, B)}
    if not mean_only:
        outs["var"] = SP.Out(dt, N, nb=B)
    ld, stm, stv = N + 3, outs["mean"].stride, N + 3

    def call(h, m, v):
        h.marginals_multi_batched(dt, m, lay, B, D, N, S, v["X"], ldx, sx, _abi.NOISE_DIAGONAL, v["s"], N, kind, v["M"], D, D * S, v["Lw"], ldl, sl,
                                  v["mean"], ld, stm, v.get("var"), stv, v["info"])

    rt = TOL[("marginals_multi", np.dtype(dt).name)]
    ref = {"mean": (mean_o, rt, 10 * rt), "var": (var_o, rt, 0.0)}
    return Case(ins, outs, call, ref, breaks, B, bad)


# (D = 144 with a diagonal prior or without variances: one regressor at a time through the tall-matrix route -- no chunk, no seam)
MARG_MULTI = [(d, n, l, pr, mo) for d, n, l in MULTI for pr, mo in (("factor", False), ("diag", False), ("factor", True))
              if d <= 128 or (pr == "factor" and not mo)]


@pytest.mark.parametrize("dt", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("D,N,layout,prior,mean_only", MARG_MULTI,
                         ids=[f"D{d}-N{n}-{l}-{p}{'-meanonly' if m else ''}" for d, n, l, p, m in MARG_MULTI])
def test_marginals_multi_capped(handle, dt, D, N, layout, prior, mean_only):
    check_capped(handle, marg_multi_case(dt, D, N, 3, layout, prior, mean_only), dt, host=(D == 20 and prior == "factor" and not mean_only))


# ---- a second broken regressor, at index 0 of the FIRST chunk --------------------------------------------------------------------
# The image kernel reads the status to skip a broken factor.  With regressor 4 alone broken, a status pointer that lost its `+ b0`
# makes the second chunk read info[0..2] -- all zero -- and nothing changes.  With regressor 0 broken as well, that read skips the
# image of the GOOD regressor 3 (chunk-local 0 of the second chunk), whose variance then comes from a stale image.
BOTH = (0, BAD)


@pytest.mark.parametrize("dt", [F64, F32], ids=["f64", "f32"])
def test_two_broken_loo_fused(handle, dt):
    check_capped(handle, loo_case(dt, 128, 64, "full", bad=BOTH), dt)


@pytest.mark.parametrize("dt", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("D,N,layout", MULTI[:3], ids=[f"D{d}-N{n}-{l}" for d, n, l in MULTI[:3]])
def test_two_broken_loo_multi(handle, dt, D, N, layout):
    check_capped(handle, loo_multi_case(dt, D, N, 3, layout, "full", bad=BOTH), dt)


@pytest.mark.parametrize("dt", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("D,N,layout", MULTI[:3], ids=[f"D{d}-N{n}-{l}" for d, n, l in MULTI[:3]])
def test_two_broken_marginals_multi_dense(handle, dt, D, N, layout):
    check_capped(handle, marg_multi_case(dt, D, N, 3, layout, "dense", bad=BOTH), dt)


@pytest.mark.parametrize("dt", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("D,N", [(128, 64), (144, 40)], ids=["product-D128", "group-D144"])
def test_two_broken_marginals_dense(handle, dt, D, N):
    check_capped(handle, marginals_case(dt, D, N, "col", "dense", bad=BOTH), dt)


# ---- blr_logpdf_grad_batched_*: the sweep route ------------------------------------------------------------------------------------
def grad_case(dt, D, N, B=B7, seed=5, bad=(BAD,)):
    """dense prior (its Cholesky reports the broken regressor); every output but A^-1"""
    from blr_amd import _abi
    p = rounded(SP.batch(B, D, N, 1, seed=seed + D + N), dt)
    Uu = SP.upper(p)
    Lw = (np.swapaxes(Uu, 1, 2) @ Uu).astype(dt).astype(F64)
    lp, dX, dy, ds, dmw, mwp = SP.grad_ref(p["X"], p["y"], p["s"], p["mw"], np.linalg.cholesky(Lw))
    Lw[[b % B for b in bad]] *= -1.0
    ins = {"X": flat(p["X"], dt), "y": flat(p["y"], dt), "s": flat(p["s"], dt), "mw": flat(p["mw"], dt), "Lw": flat(Lw, dt)}
    outs = {"logpdf": SP.Out(F64, B), "dX": SP.Out(dt, D, cols=N, nb=B), "dy": SP.Out(dt, N, nb=B), "ds": SP.Out(dt, N, nb=B),
            "dmw": SP.Out(dt, D, nb=B), "mw_post": SP.Out(dt, D, nb=B), "info": SP.Out(np.int32, B)}
    o = outs

    def call(h, m, v):
        h.logpdf_grad_batched(dt, m, _abi.LAYOUT_COLVECS, B, D, N, v["X"], D, D * N, v["y"], N, _abi.NOISE_DIAGONAL, v["s"], N, _abi.PRIOR_DENSE,
                              v["mw"], D, v["Lw"], D, D * D, v["logpdf"], v["dX"], o["dX"].ld, o["dX"].stride, v["dy"], o["dy"].stride, v["ds"],
                              o["ds"].stride, v["dmw"], o["dmw"].stride, v["mw_post"], o["mw_post"].stride, None, D, D * D, v["info"])

    f64 = dt == F64
    # tests/test_gpu_parity.py:1218 (logpdf: rel 1e-10 / 3e-4) and :1213, :1221 (rt = 1e-8 / 3e-3, atol = rt max |ref|)
    rl, rt = (1e-10, 1e-8) if f64 else (3e-4, 3e-3)
    ref = {"logpdf": (lp[:, None], rl, 0.0)}
    for k, v in (("dX", dX), ("dy", dy), ("ds", ds), ("dmw", dmw), ("mw_post", mwp)):
        ref[k] = (v, rt, rt * np.abs(v).max())
    # two routes of the gradient: tests/test_gpu_parity.py:1208-1210 (eq = 1e-9 / 2e-3, atol = eq max |.|)
    eq = 1e-9 if f64 else 2e-3
    pair = {k: (eq, eq * np.abs(r[0]).max()) for k, r in ref.items()}
    return Case(ins, outs, call, ref, True, B, bad, pair)


@pytest.mark.parametrize("dt", [F64, F32], ids=["f64", "f32"])
def test_logpdf_grad_capped(handle, dt):
    check_capped(handle, grad_case(dt, 5, 40), dt, host=True)


def test_grid_y_logpdf_grad_f64(handle):
    check_real(handle, grad_case(F64, 3, 5, B=GRID_B, seed=65537), 2)


# ---- blr_downdate_factor_*, blr_update_multi_factor_* / blr_downdate_multi_factor_*: the global routes (D = 144) ---------------------
RTOL_STATE = 1e-9  # tests/test_downdate_gpu.py:10 and _assert_state there (:50-54); tests/test_state_cols_gpu.py:11


def _ata(pay):
    """T'T from the payload of a factor (cols x rows = T' row-major)"""
    L = np.tril(pay)
    return L @ L.T


def state_case(entry, D, k, S, N=12, B=B7, seed=6):
    """entry: "downdate_factor" (S = 1), "update_multi_factor", "downdate_multi_factor".  The states hold N observations (all) or the
    N - k last ones (rest); an update goes rest -> all, a downdate all -> rest; logpdf = the evidence of the k under `rest`."""
    from blr_amd import _abi
    dt = F64
    p = SP.batch(B, D, N, S, seed=seed + D + k + S)
    multi = entry != "downdate_factor"
    Y = p["Y"] if multi else p["y"][:, None, :]
    if not multi:
        p["M"] = p["mw"][:, None, :]
    rest = dict(p, X=p["X"][:, k:], s=p["s"][:, k:], N=N - k)
    M_all, T_all = SP.condition(p, Y)
    M_rest, T_rest = SP.condition(rest, Y[:, :, k:])
    A_all, A_rest = T_all @ np.swapaxes(T_all, 1, 2), T_rest @ np.swapaxes(T_rest, 1, 2)  # (T column-major = L row-major: A = L L')
    from oracle import blr_oracle as O
    lp = np.array([[O.posterior_logpdf_direct(M_rest[b, c], None, p["X"][b, :k].T, p["s"][b, :k], Y[b, c, :k], prior_factor=T_rest[b].T)[3]
                    for c in range(Y.shape[1])] for b in range(B)])
    down = entry.startswith("downdate")
    M0, T0, M1, A1 = (M_all, T_all, M_rest, A_rest) if down else (M_rest, T_rest, M_all, A_all)
    T0 = T0.copy()
    T0[BAD, 2, 2] = -1.0
    Sc = Y.shape[1]
    ins = {"X": flat(p["X"][:, :k], dt), "Y": flat(Y[:, :, :k], dt), "s": flat(p["s"][:, :k], dt)}
    outs = {"M": SP.Out(dt, D, cols=Sc, nb=B, init=M0) if multi else SP.Out(dt, D, nb=B, init=M0),
            "T": SP.Out(dt, D, cols=D, nb=B, init=T0), "logpdf": SP.Out(F64, Sc, nb=B) if multi else SP.Out(F64, B),
            "info": SP.Out(np.int32, B)}
    o = outs

    def call(h, m, v):
        if multi:
            getattr(h, entry)(dt, m, _abi.LAYOUT_COLVECS, B, D, k, Sc, v["X"], D, D * k, v["Y"], k, k * Sc, _abi.NOISE_DIAGONAL, v["s"], k, v["M"],
                              o["M"].ld, o["M"].stride, v["T"], o["T"].ld, o["T"].stride, v["logpdf"], o["logpdf"].stride, v["info"])
        else:
            h.downdate_factor(dt, m, _abi.LAYOUT_COLVECS, B, D, k, v["X"], D, D * k, v["Y"], k, _abi.NOISE_DIAGONAL, v["s"], k, v["M"],
                              o["M"].stride, v["T"], o["T"].ld, o["T"].stride, v["logpdf"], v["info"])

    r = RTOL_STATE
    ref = {"M": (M1 if multi else M1[:, 0, :], 50 * r, r * np.abs(M1).max()), "T": (A1, r, r * np.abs(A1).max(), _ata),
           "logpdf": (lp if multi else lp[:, :1], r, 1e-10)}  # (tests/test_downdate_gpu.py:76: rel 1e-9, abs 1e-10)
    return Case(ins, outs, call, ref, True, B)


@pytest.mark.parametrize("entry,k,S", [("downdate_factor", 2, 1), ("update_multi_factor", 1, 3), ("downdate_multi_factor", 1, 3)])
def test_state_global_route_capped(handle, entry, k, S):
    check_capped(handle, state_case(entry, 144, k, S), F64, host=True)


# ---- blr_rand_batched_*: given normals -----------------------------------------------------------------------------------------------
def rand_case(D, N, S, B=B7, seed=7):
    from blr_amd import _abi
    from oracle import blr_oracle as O
    dt = F64
    p = SP.batch(B, D, N, S, seed=seed + D + N)
    rng = np.random.Generator(np.random.PCG64(seed + 1000))
    Z1, Z2 = rng.standard_normal((B, S, D)), rng.standard_normal((B, S, N))
    Uu = SP.upper(p)
    Lw = np.swapaxes(Uu, 1, 2) @ Uu
    W_o = np.stack([O.sample_weights(p["mw"][b], Lw[b], Z1[b].T).T for b in range(B)])                      # [B, S, D]
    Y_o = np.stack([O.rand(p["mw"][b], Lw[b], p["X"][b].T, p["s"][b], Z1[b].T, Z2[b].T).T for b in range(B)])  # [B, S, N]
    Lw[BAD, 2, 2] = -50.0
    ins = {"X": flat(p["X"], dt), "s": flat(p["s"], dt), "mw": flat(p["mw"], dt), "Lw": flat(Lw, dt), "Z1": flat(Z1, dt), "Z2": flat(Z2, dt)}
    outs = {"W": SP.Out(dt, D, cols=S, nb=B), "Y": SP.Out(dt, N, cols=S, nb=B), "info": SP.Out(np.int32, B)}
    o = outs

    def call(h, m, v):
        h.rand_batched(dt, m, _abi.LAYOUT_COLVECS, B, D, N, S, v["X"], D, D * N, _abi.NOISE_DIAGONAL, v["s"], N, _abi.PRIOR_DENSE, v["mw"], D,
                       v["Lw"], D, D * D, v["Z1"], D, D * S, v["Z2"], N, N * S, v["W"], o["W"].ld, o["W"].stride, v["Y"], o["Y"].ld, o["Y"].stride,
                       v["info"])

    ref = {"W": (W_o, 1e-10, 1e-11), "Y": (Y_o, 1e-10, 1e-11)}  # tests/test_rand_batched_gpu.py:10 (RTOL64, ATOL64), :135-137
    return Case(ins, outs, call, ref, True, B)


def test_rand_batched_projection_capped(handle):
    """N S > 512: the projection is a launch of its own, `per_launch` regressors at a time"""
    check_capped(handle, rand_case(5, 200, 3), F64, host=True)


def test_rand_batched_fused_has_no_chunks(handle):
    """D = 5, N = 17, S = 3: N S <= 512 projects inside the solve kernel -- one launch whatever the cap, and the same numbers"""
    check_capped(handle, rand_case(5, 17, 3), F64, chunks=1)


# ---- blr_posterior_batched_f64 on the int8 route: slices ----------------------------------------------------------------------------
def i8_case(noise, B=B7, seed=8):
    from blr_amd import _abi
    from oracle import blr_oracle as O
    dt, D, N = F64, 128, 512
    rng = np.random.Generator(np.random.PCG64(seed))
    X = rng.standard_normal((B, N, D))
    y = rng.standard_normal((B, N))
    mw = 0.3 * rng.standard_normal((B, D))
    dpr = np.exp(0.3 * rng.standard_normal((B, D)))
    s = np.exp(0.3 * rng.standard_normal((B, N))) if noise == "diag" else 0.3 + rng.random((B, 1))
    res = [O.posterior_logpdf_direct(mw[b], dpr[b], X[b].T, s[b] if noise == "diag" else float(s[b, 0]), y[b]) for b in range(B)]
    s_in = s.copy()
    s_in[BAD, 0] = -1.0
    ins = {"X": flat(X, dt), "y": flat(y, dt), "s": flat(s_in, dt), "mw": flat(mw, dt), "Lw": flat(dpr, dt)}
    outs = {"mw_post": SP.Out(dt, D, nb=B), "T": SP.Out(dt, D, cols=D, nb=B), "logpdf": SP.Out(F64, B), "info": SP.Out(np.int32, B)}
    o = outs
    nk, ss = (_abi.NOISE_DIAGONAL, N) if noise == "diag" else (_abi.NOISE_ISOTROPIC, 1)

    def call(h, m, v):
        h.posterior_batched(dt, m, _abi.LAYOUT_COLVECS, B, D, N, v["X"], D, N * D, v["y"], N, nk, v["s"], ss, _abi.PRIOR_DIAGONAL, v["mw"], D, v["Lw"],
                            1, D, v["mw_post"], o["mw_post"].stride, v["T"], o["T"].ld, o["T"].stride, None, D, D * D, v["logpdf"], v["info"])
        assert h.last_route() == "fused_i8_kernel"

    A = np.stack([r[2] for r in res])
    # tests/test_gpu_parity.py:2871-2873 (int8 route: logpdf rel 1e-10, mean rtol 1e-7 / atol 1e-9); the precision T'T at the mean's
    # rtol, absolute part scaled as tests/test_downdate_gpu.py:53 scales it
    ref = {"mw_post": (np.stack([r[0] for r in res]), 1e-7, 1e-9), "T": (A, 1e-7, 1e-7 * np.abs(A).max(), _ata),
           "logpdf": (np.array([[r[3]] for r in res]), 1e-10, 0.0)}
    # a slice after one that handed a regressor back may leave its own to the fp64 kernel: the two kernels agree as each agrees with
    # the oracle, not to 1e-12
    pair = {"mw_post": (1e-7, 1e-9), "T": (1e-7, 1e-9), "logpdf": (1e-10, 0.0)}
    return Case(ins, outs, call, ref, True, B, pair=pair)


@pytest.mark.parametrize("noise", ["iso", "diag"])
def test_i8_posterior_slices_capped(handle, noise):
    check_capped(handle, i8_case(noise), F64, host=(noise == "iso"))


# ---- real bounds, no option ---------------------------------------------------------------------------------------------------------
def check_real(h, case, chunks):
    from blr_amd import _abi
    h.set_option("MAX_CHUNK", None)
    got = run(h, _abi.MEM_DEVICE, case.ins, case.outs, case.call)
    assert h.get_stat("last_chunks") == chunks
    info = case.outs["info"].payload(got["info"])[0]
    good = np.ones(case.B, dtype=bool)
    for b in case.bad:
        good[b] = False
        assert info[b] != 0
    assert not info[good].any(), np.flatnonzero(info)[:10]
    for k, o in case.outs.items():
        assert o.gaps_kept(got[k]), f"{k}: padding overwritten"
        if k == "info":
            continue
        ref, rtol, atol = case.ref[k][:3]
        pay = o.per_regressor(got[k]).astype(F64)
        err = np.abs(pay[good] - ref[good])
        print(k, "max abs err", err.max(), "worst regressor", int(np.flatnonzero(good)[err.reshape(err.shape[0], -1).max(axis=1).argmax()]))
        np.testing.assert_allclose(pay[good], ref[good], rtol=rtol, atol=atol, err_msg=k)


GRID_B = 65537


def test_grid_y_marginals_f64(handle):
    check_real(handle, marginals_case(F64, 3, 5, "col", "factor", B=GRID_B, seed=65537), 2)


def test_grid_y_loo_f64(handle):
    check_real(handle, loo_case(F64, 3, 5, "total", B=GRID_B, seed=65537), 2)


def test_grid_y_loo_empty_f64(handle):
    check_real(handle, loo_case(F64, 3, 5, "empty", B=GRID_B, seed=65537), 2)


def test_grid_y_check_loop_loo_multi_f64(handle):
    # (only loo_check_kernel's loop crosses 65535 here: at D <= 128 the images cut the column kernel's chunks long before grid.y)
    check_real(handle, loo_multi_case(F64, 3, 5, 2, "col", "full", B=GRID_B, seed=65537), math.ceil(GRID_B / image_bound(F64)))


def test_many_image_chunks_marginals_multi_f32(handle):
    # (the images cut the batch into ten chunks; grid.y itself: test_grid_y_marginals_multi_column_kernel_f32)
    check_real(handle, marg_multi_case(F32, 3, 5, 2, "col", "factor", B=GRID_B, seed=65537), math.ceil(GRID_B / image_bound(F32)))


def image_bound(dt):
    return (256 << 20) // (9216 * np.dtype(dt).itemsize)


def test_image_bound_marginals_f64(handle):
    B = image_bound(F64) + 2
    assert B == 3642
    check_real(handle, marginals_case(F64, 128, 64, "col", "factor", B=B, seed=3642, shared_x=True), 2)


def test_image_bound_loo_multi_f64(handle):
    B = image_bound(F64) + 2
    check_real(handle, loo_multi_case(F64, 128, 64, 2, "col", "full", B=B, seed=3642, shared_x=True), 2)


def test_image_bound_loo_fused_f32(handle):
    B = image_bound(F32) + 2
    assert B == 7283
    check_real(handle, loo_case(F32, 128, 64, "full", B=B, seed=7283, shared_x=True), 2)


def test_image_bound_marginals_multi_f32(handle):
    B = image_bound(F32) + 2
    check_real(handle, marg_multi_case(F32, 128, 64, 2, "col", "factor", B=B, seed=7283, shared_x=True), 2)


# ---- marginals_large_group (D = 144, N = 40): the images of NC = 2 blocks per regressor, and chol_large's group of 128 ---------------
def test_large_group_image_bound_f32_factor(handle):
    B = (256 << 20) // (2 * 9216 * 4) + 2
    assert B == 3642
    check_real(handle, marginals_case(F32, 144, 40, "col", "factor", B=B, seed=144, shared_x=True), 2)


def test_large_group_chain_bound_f64_dense(handle):
    check_real(handle, marginals_case(F64, 144, 40, "col", "dense", B=130, seed=130, shared_x=True), 2)


def test_grid_y_marginals_multi_column_kernel_f32(handle):
    """mean-only: no images, so the column kernel's own grid.y = 65535 is what cuts the batch"""
    check_real(handle, marg_multi_case(F32, 3, 5, 2, "col", "factor", mean_only=True, B=GRID_B, seed=65537), 2)
