"""blr_posterior_multi_batched_x16 (fused_x16_kernel + multi_cols_x16_kernel) on the GPU: every column against the
fp64 oracle on the exactly widened features at the fp32 route's tolerance; the bits of a column against its slot, its pass, the batch,
the chunking and the other columns; edge calls, a failed regressor, device memspace, argument errors and the Python column fronts."""
import numpy as np
import pytest

import blr_amd as R
from _x16_problems import PRIORS, XKINDS, _problem
from _yardsticks import _assert_fp32_within_lapack
from blr_amd import _abi

pytestmark = pytest.mark.gpu
NB = 2


@pytest.fixture(scope="module")
def hd():
    h = _abi.Handle(0)
    yield h
    h.close()


def _targets(q, S, offset=0.0):
    """(nb, N, S) float32: column 0 is the problem's y, the others are y plus unit noise of their own"""
    rng = np.random.Generator(np.random.PCG64(17 * q["D"] + q["N"] + S))
    Y = (q["y"][:, :, None] + rng.standard_normal((q["nb"], q["N"], S))).astype(np.float32)
    Y[:, :, 0] = q["y"]
    return Y + np.float32(offset)


def _out(q, S, nb=None):
    D, nb = q["D"], nb or q["nb"]
    return dict(ldmp=D + 1, st_m=(D + 1) * S + 2, ldt=D + 2, st_T=(D + 2) * D + 5, st_lp=S + 1, M=np.full(nb * ((D + 1) * S + 2), np.nan, np.float32),
                T=np.full(nb * ((D + 2) * D + 5), np.nan, np.float32), A=np.full(nb * ((D + 2) * D + 5), np.nan, np.float32),
                lp=np.full(nb * (S + 1), 123.0), info=np.full(nb, -7, np.int32))


def _multi(hd, q, Y, o, memspace=_abi.MEM_HOST, T=True, **over):
    a = dict(q, noise_kind=_abi.NOISE_ISOTROPIC, nb=Y.shape[0])
    a.update(over)
    N, S = Y.shape[1], Y.shape[2]
    ldY, stY = N + 1, (N + 1) * S + 3
    Yb = np.full(max(Y.shape[0] * stY, 1), np.nan, np.float32)
    for b in range(Y.shape[0]):
        Yb[b * stY:b * stY + ldY * S].reshape((ldY, S), order="F")[:N] = Y[b]
    arr = dict(X=a["X"], Y=Yb, s=a["s"], mw=a["mw"], Lw=a["Lw"], M=o["M"], T=o["T"] if T else None, A=o["A"], lp=o["lp"], info=o["info"])
    if memspace == _abi.MEM_DEVICE:
        import torch
        dev = {k: None if v is None else torch.from_numpy(v.view(np.int16) if v.dtype.itemsize == 2 else v).cuda() for k, v in arr.items()}
        p = {k: None if v is None else v.data_ptr() for k, v in dev.items()}
    else:
        dev, p = None, arr
    hd.posterior_multi_batched_x16(a["xfmt"], memspace, a["layout"], a["nb"], a["D"], N, S, p["X"], a["ldx"], a["strideX"], p["Y"], ldY, stY,
                                   a["noise_kind"], p["s"], 1, a["prior_kind"], p["mw"], a["D"], p["Lw"], a["ldl"], a["Lw"].shape[1], p["M"],
                                   o["ldmp"], o["st_m"], p["T"], o["ldt"], o["st_T"], p["A"], o["ldt"], o["st_T"], p["lp"], o["st_lp"], p["info"])
    if dev is not None:
        hd.synchronize()
        for k in ("M", "T", "A", "lp", "info"):
            if dev[k] is not None:
                arr[k][...] = dev[k].cpu().numpy()


def _col(q, o, b, s):
    D = q["D"]
    return o["M"][b * o["st_m"] + s * o["ldmp"]:][:D], o["lp"][b * o["st_lp"] + s]


def _mat(q, o, b, key):
    return o[key][b * o["st_T"]:b * o["st_T"] + o["ldt"] * q["D"]].reshape((o["ldt"], q["D"]), order="F")[:q["D"]]


def _against_oracle(q, Y, o, what):
    for b in range(Y.shape[0]):
        assert o["info"][b] == 0
        for s in range(Y.shape[2]):
            m, lp = _col(q, o, b, s)
            _assert_fp32_within_lapack(q["mw"][b], q["dense"][b], np.asfortranarray(q["Xw"][b]), q["s"][b], np.ascontiguousarray(Y[b, :, s]), m,
                                       _mat(q, o, b, "A"), lp, got_T=_mat(q, o, b, "T"), what=f"{what} regressor {b} column {s}")


def _route(q):
    return q["route"] + " + " + q["route"].replace("fused_x16_kernel", "multi_cols_x16_kernel")


@pytest.mark.parametrize("S", [2, 17])
@pytest.mark.parametrize("N", [1, 31, 33, 131])
@pytest.mark.parametrize("D", [5, 40, 72, 128])
@pytest.mark.parametrize("xkind", XKINDS)
@pytest.mark.parametrize("fmt", ["bf16", "f16"])
def test_columns_against_oracle(hd, fmt, xkind, D, N, S):
    """Every loader, block count, stage seam and a second column tile: each column at 4 x the error of fp32 LAPACK, nothing added."""
    q = _problem(fmt, xkind, D, N, PRIORS[(D // 8 + N + XKINDS.index(xkind)) % 3], nb=NB)
    Y, o = _targets(q, S), _out(q, S)
    _multi(hd, q, Y, o)
    assert hd.last_route() == _route(q)
    _against_oracle(q, Y, o, hd.last_route())


@pytest.mark.parametrize("fmt", ["bf16", "f16"])
def test_targets_with_a_large_common_offset(hd, fmt):
    """Y = 1000 + unit noise against a zero prior mean: the residuals are 1000 + O(1), their low bf16 piece carries the noise."""
    q = _problem(fmt, "col_al", 72, 131, "diag", nb=NB)
    q["mw"] = np.zeros_like(q["mw"])
    Y = (_targets(q, 3) * 0 + 1000 + np.random.Generator(np.random.PCG64(5)).standard_normal((NB, 131, 3))).astype(np.float32)
    o = _out(q, 3)
    _multi(hd, q, Y, o)
    _against_oracle(q, Y, o, "offset")


@pytest.mark.parametrize("xkind,D", [("col_al", 128), ("row_odd", 40)])
def test_column_zero_is_the_single_column_call(hd, xkind, D):
    q = _problem("bf16", xkind, D, 131, "dense", nb=NB)
    Y, o = _targets(q, 5), _out(q, 5)
    _multi(hd, q, Y, o)
    one = dict(m=np.full(NB * D, np.nan, np.float32), T=np.full_like(o["T"], np.nan), A=np.full_like(o["A"], np.nan), lp=np.zeros(NB),
               info=np.full(NB, -7, np.int32))
    hd.posterior_batched_x16(q["xfmt"], _abi.MEM_HOST, q["layout"], NB, D, 131, q["X"], q["ldx"], q["strideX"], q["y"], 131, _abi.NOISE_ISOTROPIC,
                             q["s"], 1, q["prior_kind"], q["mw"], D, q["Lw"], q["ldl"], q["Lw"].shape[1], one["m"], D, one["T"], o["ldt"], o["st_T"],
                             one["A"], o["ldt"], o["st_T"], one["lp"], one["info"])
    for b in range(NB):
        assert np.array_equal(_col(q, o, b, 0)[0], one["m"][b * D:(b + 1) * D]) and _col(q, o, b, 0)[1] == one["lp"][b]
    for k in ("T", "A", "info"):
        assert np.array_equal(o[k], one[k], equal_nan=True), k
    # S = 1 is that call as well
    o1 = _out(q, 1)
    _multi(hd, q, Y[:, :, :1], o1)
    assert hd.last_route() == _route(q)
    for b in range(NB):
        assert np.array_equal(_col(q, o1, b, 0)[0], one["m"][b * D:(b + 1) * D]) and _col(q, o1, b, 0)[1] == one["lp"][b]
    assert np.array_equal(o1["T"], one["T"], equal_nan=True)


@pytest.mark.parametrize("fmt,xkind,D", [("bf16", "col_al", 128), ("f16", "row_al", 72), ("bf16", "col_odd", 5)])
def test_a_column_keeps_its_bits(hd, fmt, xkind, D):
    """... in slot 1 against slot 40, in pass 1 against pass 2 (S = 65, 130), with the other columns NaN, in a batch of one, under
    MAX_CHUNK = 2 and with a shared X"""
    q = _problem(fmt, xkind, D, 131, "factor", nb=3)
    Y = _targets(q, 130)
    ref = _out(q, 130)
    _multi(hd, q, Y, ref)
    want = lambda b, s: (_col(q, ref, b, s)[0].copy(), _col(q, ref, b, s)[1])
    same = lambda got, exp, what: (np.array_equal(got[0], exp[0]) and got[1] == exp[1]) or pytest.fail(what)

    def run(Yc, regs=(0, 1, 2), **over):
        sub = dict(q, X=q["X"][regs[0] * q["strideX"]:] if len(regs) == 1 else q["X"], y=q["y"][list(regs)], s=q["s"][list(regs)],
                   mw=q["mw"][list(regs)], Lw=q["Lw"][list(regs)])
        o = _out(q, Yc.shape[2], nb=len(regs))
        _multi(hd, sub, Yc, o, **over)
        return o

    for order, at in (([0, 1, 2], 1), ([0] + list(range(2, 41)) + [1], 40), ([0] + list(range(2, 65)) + [1], 64), ([0] + list(range(2, 129)) + [1], 128)):
        o = run(Y[:, :, order])  # column 1 of Y in slot 1, slot 40, slot 1 of pass 2 (S = 65), slot 2 of pass 3 (S = 129)
        for b in range(3):
            same(_col(q, o, b, at), want(b, 1), f"column 1 at {at}")
    Yn = Y[:, :, :20].copy()
    Yn[:, :, 2:] = np.nan
    Yn[:, :, 17] = Y[:, :, 17]
    o = run(Yn)
    for b in range(3):
        same(_col(q, o, b, 1), want(b, 1), "NaN neighbours, column 1")
        same(_col(q, o, b, 17), want(b, 17), "NaN neighbours, column 17")
    o = run(Y[1:2, :, :70], regs=(1,))
    same(_col(q, o, 0, 69), want(1, 69), "B = 1")
    hd.set_option("MAX_CHUNK", "2")
    try:
        o = run(Y)
        assert hd.get_stat("last_chunks") == 2
    finally:
        hd.set_option("MAX_CHUNK", None)
    for k in ("M", "T", "A", "lp", "info"):
        assert np.array_equal(o[k], ref[k], equal_nan=True), ("MAX_CHUNK", k)
    # three regressors on regressor 0's X: strideX = 0 against copies
    qs = dict(q, X=q["X"][:q["strideX"]].copy())
    shared, copies = _out(q, 70), _out(q, 70)
    _multi(hd, qs, Y[:, :, :70], shared, strideX=0)
    _multi(hd, dict(q, X=np.tile(qs["X"], 3)), Y[:, :, :70], copies)
    for k in ("M", "T", "A", "lp", "info"):
        assert np.array_equal(shared[k], copies[k], equal_nan=True), ("strideX = 0", k)


def test_edge_calls(hd):
    q = _problem("bf16", "col_al", 40, 0, "diag", nb=NB)
    o = _out(q, 3)
    _multi(hd, q, np.zeros((NB, 0, 3), np.float32), o)
    for b in range(NB):
        for s in range(3):
            assert np.array_equal(_col(q, o, b, s)[0], q["mw"][b]) and _col(q, o, b, s)[1] == 0.0
    q = _problem("f16", "row_al", 72, 33, "dense", nb=NB)
    Y, full, lean = _targets(q, 4), _out(q, 4), _out(q, 4)
    _multi(hd, q, Y, full)
    hd.release_workspace()
    before = hd.get_stat("workspace_bytes")
    _multi(hd, q, Y, lean, T=False)
    assert hd.get_stat("workspace_bytes") - before >= NB * 72 * 72 * 4
    assert np.array_equal(lean["M"], full["M"], equal_nan=True) and np.array_equal(lean["lp"], full["lp"]) and np.all(np.isnan(lean["T"]))


def test_a_failed_regressor_in_the_second_chunk(hd):
    q = _problem("bf16", "col_al", 40, 33, "dense", nb=4)
    Y, good = _targets(q, 3), _out(q, 3)
    _multi(hd, q, Y, good)
    bad = dict(q, Lw=q["Lw"].copy())
    bad["Lw"][2, 0] = -1.0  # regressor 2: the leading minor of its prior is negative
    o = _out(q, 3)
    hd.set_option("MAX_CHUNK", "2")
    try:
        _multi(hd, bad, Y, o)
    finally:
        hd.set_option("MAX_CHUNK", None)
    assert o["info"][2] > 0 and np.all(np.isnan(o["lp"][2 * o["st_lp"]:2 * o["st_lp"] + 3]))
    assert np.all(np.isnan(o["M"][2 * o["st_m"]:3 * o["st_m"]]))
    for b in (0, 1, 3):
        assert o["info"][b] == 0
        for s in range(3):
            assert np.array_equal(_col(q, o, b, s)[0], _col(q, good, b, s)[0]) and _col(q, o, b, s)[1] == _col(q, good, b, s)[1]


@pytest.mark.parametrize("asynchronous", [False, True])
def test_device_memspace_gives_the_host_bits(hd, asynchronous):
    q = _problem("f16", "col_al", 128, 131, "factor", nb=NB)
    Y, host, dev = _targets(q, 17), _out(q, 17), _out(q, 17)
    _multi(hd, q, Y, host)
    hd.set_async(asynchronous)
    try:
        _multi(hd, q, Y, dev, memspace=_abi.MEM_DEVICE)
    finally:
        hd.set_async(False)
    for k in ("M", "T", "A", "lp", "info"):
        assert np.array_equal(host[k], dev[k], equal_nan=True), k


@pytest.mark.parametrize("what,code", [("D129", -6), ("diag_noise", -15), ("dense_noise", -15), ("xfmt", -4)])
def test_argument_errors(hd, what, code):
    q = _problem("bf16", "col_al", 129 if what == "D129" else 16, 29, "diag", nb=NB)
    Y, o = _targets(q, 3), _out(q, 3)
    over = {"diag_noise": dict(noise_kind=_abi.NOISE_DIAGONAL), "dense_noise": dict(noise_kind=_abi.NOISE_DENSE), "xfmt": dict(xfmt=2)}.get(what, {})
    with pytest.raises(_abi.BLRError) as e:
        _multi(hd, q, Y, o, **over)
    assert e.value.code == code
    assert np.all(np.isnan(o["M"])) and np.all(np.isnan(o["T"])) and np.all(o["lp"] == 123.0) and np.all(o["info"] == -7)


@pytest.mark.parametrize("vecs", ["ColVecs16", "RowVecs16"])
@pytest.mark.parametrize("fmt", ["bf16", "f16"])
def test_python_column_fronts(fmt, vecs):
    q = _problem(fmt, "col_al", 40, 131, "diag", nb=NB)
    Y = _targets(q, 5)
    X16 = [R.bf16_bits(q["Xw"][b]) if fmt == "bf16" else q["Xw"][b].astype(np.float16) for b in range(NB)]
    xs = [R.ColVecs16(np.asfortranarray(x), fmt) if vecs == "ColVecs16" else R.RowVecs16(np.ascontiguousarray(x.T), fmt) for x in X16]
    fxs = [R.BayesianLinearRegressor(q["mw"][b], R.Diagonal(q["Lw"][b]))(xs[b], float(q["s"][b])) for b in range(NB)]
    lps = R.logpdf_columns_map(fxs, list(Y))
    posts = R.posterior_columns_map(fxs, list(Y))
    assert lps.shape == (NB, 5)
    for b in range(NB):
        assert np.array_equal(R.logpdf_columns(fxs[b], Y[b]), lps[b])
        assert all(p.Lw is posts[b][0].Lw for p in posts[b])
        A = np.asarray(posts[b][0].Lw.toarray() if hasattr(posts[b][0].Lw, "toarray") else posts[b][0].Lw, np.float32)
        # the loop of single-column calls: column 0 is that call bit for bit, every column and the loop are held to the yardstick
        assert lps[b, 0] == R.logpdf(fxs[b], Y[b, :, 0]) and np.array_equal(posts[b][0].mw, R.posterior(fxs[b], Y[b, :, 0]).mw)
        for s in range(5):
            one = R.posterior(fxs[b], Y[b, :, s])
            _assert_fp32_within_lapack(q["mw"][b], q["dense"][b], np.asfortranarray(q["Xw"][b]), q["s"][b], np.ascontiguousarray(Y[b, :, s]),
                                       np.asarray(one.mw, np.float32), A, R.logpdf(fxs[b], Y[b, :, s]), what=f"loop {vecs} {fmt} {b} {s}")
            _assert_fp32_within_lapack(q["mw"][b], q["dense"][b], np.asfortranarray(q["Xw"][b]), q["s"][b], np.ascontiguousarray(Y[b, :, s]),
                                       np.asarray(posts[b][s].mw, np.float32), A, lps[b, s], what=f"{vecs} {fmt} {b} {s}")
