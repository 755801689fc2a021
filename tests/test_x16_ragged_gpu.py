"""blr_posterior_ragged_x16 (ragged_x16_kernel, ragged_x16_part_kernel + ragged_x16_finish_kernel) on the GPU: one
packed batch whose counts sit on the stage and item seams, RAGGED_ITEM = 64 (131 observations: 3 items, 200: 4, the last ones
partial; the others stay whole).  Whole regressors bit for bit against blr_posterior_batched_x16 at B = 1 on their slice, every
regressor against the fp64 oracle at the fp32 route's tolerance, the Gram matrix exactly on integer features, the cut regressors'
bits across B / chunking / history, argument errors, a failed regressor, the Python front."""
import numpy as np
import pytest

import blr_amd as R
from _small_d_problems import _outputs, _result
from _x16_problems import PRIORS, XKINDS, _problem, x_layout
from _yardsticks import _assert_fp32_within_lapack
from blr_amd import _abi

pytestmark = pytest.mark.gpu

# offsets 0, 64, 64, 264, 265, 396, 425, 457, 490: the RowVecs slices of 64, 0, 200 and 1 start on 16-byte boundaries, the others do not
COUNTS = (64, 0, 200, 1, 131, 29, 32, 33)
OFFSETS = np.concatenate([[0], np.cumsum(COUNTS)]).astype(np.int64)
NB, W, CUT = len(COUNTS), 64, (2, 4)


@pytest.fixture(scope="module")
def hd():
    h = _abi.Handle(0)
    h.set_option("RAGGED_ITEM", W)
    yield h
    h.close()


def _packed(fmt, xkind, D, prior, ints=False):
    """_problem's regressors, the first COUNTS[b] observations of each packed side by side in the layout of `xkind` (gaps hold NaN)"""
    q = _problem(fmt, xkind, D, max(COUNTS), prior, ints=ints, nb=NB)
    total = int(OFFSETS[-1])
    col, _, rows, cols, ldx, _ = x_layout(xkind, D, total)
    X16 = R.bf16_bits(q["Xw"]) if fmt == "bf16" else q["Xw"].astype(np.float16)
    buf = np.full(ldx * cols, 0x7FC0 if fmt == "bf16" else np.nan, dtype=X16.dtype)
    M = np.concatenate([X16[b][:, :n] for b, n in enumerate(COUNTS)], axis=1)
    buf.reshape((ldx, cols), order="F")[:rows, :] = M if col else M.T
    q.update(X=buf, ldx=ldx, yp=np.concatenate([q["y"][b, :n] for b, n in enumerate(COUNTS)]), strides=1,
             noise_kind=_abi.NOISE_ISOTROPIC, offsets=OFFSETS)
    return q


def _ragged(hd, q, o, regs=range(NB), **over):
    """the packed call on the regressors `regs` (a run of neighbours) into their part of the outputs"""
    a = dict(q, **over)
    b0, nb = regs[0], len(regs)
    part = lambda v, st: v[b0 * st:]
    return hd.posterior_ragged_x16(a["xfmt"], _abi.MEM_HOST, a["layout"], nb, a["D"], a["offsets"][b0:b0 + nb + 1], a["X"], a["ldx"], a["yp"],
                                   a["noise_kind"], a["s"][b0:], a["strides"], a["prior_kind"], a["mw"][b0:], a["D"], a["Lw"][b0:], a["ldl"],
                                   a["Lw"].shape[1], part(o["mw_post"], o["stride_mwpost"]), o["stride_mwpost"], part(o["T"], o["strideT"]),
                                   o["ldt"], o["strideT"], part(o["A"], o["strideT"]), o["ldt"], o["strideT"], o["lp"][b0:], o["info"][b0:])


def _single(hd, q, o, b):
    """blr_posterior_batched_x16 with B = 1 on the slice of regressor b, into slot b of the outputs"""
    off = int(OFFSETS[b]) * (q["ldx"] if q["layout"] == _abi.LAYOUT_COLVECS else 1)
    st_m, st_T = o["stride_mwpost"], o["strideT"]
    hd.posterior_batched_x16(q["xfmt"], _abi.MEM_HOST, q["layout"], 1, q["D"], COUNTS[b], q["X"][off:], q["ldx"], 0, q["yp"][OFFSETS[b]:], 0,
                             _abi.NOISE_ISOTROPIC, q["s"][b:], 1, q["prior_kind"], q["mw"][b], q["D"], q["Lw"][b], q["ldl"], 0,
                             o["mw_post"][b * st_m:], st_m, o["T"][b * st_T:], o["ldt"], st_T, o["A"][b * st_T:], o["ldt"], st_T, o["lp"][b:],
                             o["info"][b:])


def _same(o, p, regs):
    return all(np.array_equal(o[k][b * st:(b + 1) * st], p[k][b * st:(b + 1) * st], equal_nan=True) for b in regs
               for k, st in (("mw_post", o["stride_mwpost"]), ("T", o["strideT"]), ("A", o["strideT"]), ("lp", 1), ("info", 1)))


def _inst(q, D):
    return f"<{q['fmt']}, {2 * ((D + 31) // 32)}, {'col' if q['layout'] == _abi.LAYOUT_COLVECS else 'row'}>"


@pytest.mark.parametrize("D", [5, 40, 128])
@pytest.mark.parametrize("xkind", XKINDS)
@pytest.mark.parametrize("fmt", ["bf16", "f16"])
def test_x16_ragged_against_single_calls_and_oracle(hd, fmt, xkind, D):
    """Whole regressors: the bits of the B = 1 call on the slice.  Every regressor, cut ones included: 4 x the error of fp32 LAPACK on
    the widened features, nothing added.  The route names the three kernels."""
    q = _packed(fmt, xkind, D, PRIORS[(D // 8 + XKINDS.index(xkind)) % 3])
    o, p = _outputs(NB, D, np.float32, gaps=True), _outputs(NB, D, np.float32, gaps=True)
    _ragged(hd, q, o)
    inst = _inst(q, D)
    assert hd.last_route() == f"ragged_x16_kernel{inst} + ragged_x16_part_kernel{inst} + ragged_x16_finish_kernel<{inst.split(', ')[1]}>"
    whole = [b for b in range(NB) if b not in CUT]
    for b in whole:
        _single(hd, q, p, b)
    assert _same(o, p, whole)
    for b, n in enumerate(COUNTS):
        mw_p, T, A, lp, info = _result(q, o, b)
        assert info == 0
        _assert_fp32_within_lapack(q["mw"][b], q["dense"][b], np.asfortranarray(q["Xw"][b][:, :n]), q["s"][b], q["y"][b, :n], mw_p, A, lp,
                                   got_T=T, what=f"{hd.last_route()} regressor {b} ({n} observations)")


@pytest.mark.parametrize("D", [40, 128])
@pytest.mark.parametrize("xkind", XKINDS)
@pytest.mark.parametrize("fmt", ["bf16", "f16"])
def test_x16_ragged_gram_is_exact_on_integers(hd, fmt, xkind, D):
    """Integer features in [-8, 8], unit prior and noise: Lw' = I + X X' bit for bit, for the cut regressors too (every partial sum is
    below 2^24) -- a dropped, doubled or mis-seamed column at an item boundary would show."""
    q = _packed(fmt, xkind, D, "diag", ints=True)
    o = _outputs(NB, D, np.float32)
    _ragged(hd, q, o)
    for b, n in enumerate(COUNTS):
        Xi = q["Xw"][b][:, :n].astype(np.int64)
        assert np.array_equal(_result(q, o, b)[2].astype(np.float64), np.eye(D) + Xi @ Xi.T), (hd.last_route(), b)


@pytest.mark.parametrize("xkind", ["col_al", "row_odd"])
def test_x16_ragged_cut_bits_do_not_depend_on_the_call(hd, xkind):
    """A cut regressor alone in a call, among the others, under MAX_CHUNK = 2 and in a second call on the same handle: the same bits."""
    q = _packed("bf16", xkind, 40, "dense")
    among = _outputs(NB, 40, np.float32)
    _ragged(hd, q, among)
    for b in CUT:
        alone = _outputs(NB, 40, np.float32)
        _ragged(hd, q, alone, regs=range(b, b + 1))
        assert hd.last_route() == f"ragged_x16_part_kernel{_inst(q, 40)} + ragged_x16_finish_kernel<4>"
        assert _same(alone, among, [b])
    hd.set_option("MAX_CHUNK", 2)
    try:
        chunked, again = _outputs(NB, 40, np.float32), _outputs(NB, 40, np.float32)
        _ragged(hd, q, chunked)
        assert hd.get_stat("last_chunks") == 4
    finally:
        hd.set_option("MAX_CHUNK", None)
    _ragged(hd, q, again)
    assert _same(chunked, among, range(NB)) and _same(again, among, range(NB))


@pytest.mark.parametrize("what,code", [("D129", -6), ("diag_noise", -11), ("dense_noise", -11), ("xfmt", -4), ("offsets", -7)])
def test_x16_ragged_argument_errors(hd, what, code):
    D = 129 if what == "D129" else 16
    q = _packed("bf16", "col_al", D, "diag")
    o = _outputs(NB, D, np.float32)
    before = {k: np.copy(v) for k, v in o.items() if isinstance(v, np.ndarray)}
    over = {"diag_noise": dict(noise_kind=_abi.NOISE_DIAGONAL, s=np.ones(int(OFFSETS[-1]), np.float32)), "dense_noise": dict(noise_kind=_abi.NOISE_DENSE),
            "xfmt": dict(xfmt=2), "offsets": dict(offsets=OFFSETS[::-1].copy())}.get(what, {})
    with pytest.raises(_abi.BLRError) as e:
        _ragged(hd, q, o, **over)
    assert e.value.code == code and len(str(e.value).split(":", 2)[2].strip()) > 0
    for k, v in before.items():
        assert np.array_equal(o[k], v, equal_nan=True), k


@pytest.mark.parametrize("bad", [5, 4])  # a whole regressor, a cut one
def test_x16_ragged_failed_regressor_stands_alone(hd, bad):
    """A non-positive variance: info, a NaN evidence, outputs kept; the neighbours (whole and cut) bit for bit what they were."""
    q = _packed("f16", "row_al", 40, "factor")
    good, o = _outputs(NB, 40, np.float32), _outputs(NB, 40, np.float32)
    _ragged(hd, q, good)
    s = q["s"].copy()
    s[bad] = -1.0
    _ragged(hd, q, o, s=s)
    mw_p, T, A, lp, info = _result(q, o, bad)
    assert info == 1 and np.isnan(lp) and np.all(np.isnan(mw_p)) and np.all(np.isnan(T)) and np.all(np.isnan(A))
    assert _same(o, good, [b for b in range(NB) if b != bad])


@pytest.mark.parametrize("cls", [R.ColVecs16, R.RowVecs16])
def test_x16_ragged_python_front(cls):
    """posterior_ragged / logpdf_ragged on 16-bit containers: the yardstick of the C ABI test, and one evidence from both."""
    q = _packed("bf16", "col_al" if cls is R.ColVecs16 else "row_al", 24, "diag")
    M = R.bf16_bits(np.concatenate([q["Xw"][b][:, :n] for b, n in enumerate(COUNTS)], axis=1))  # D x total
    f = [R.BayesianLinearRegressor(q["mw"][b], R.Diagonal(q["Lw"][b])) for b in range(NB)]
    x = cls(np.asfortranarray(M if cls is R.ColVecs16 else M.T), "bf16")  # (the layout of q: the C ABI call below gives the same bits)
    handle = _abi.default_handle()
    handle.set_option("RAGGED_ITEM", W)
    try:
        post = R.posterior_ragged(f, x, OFFSETS, q["s"], q["yp"])
        assert "ragged_x16_part_kernel<bf16, 2, " in handle.last_route()
        lp = R.logpdf_ragged(f, x, OFFSETS, q["s"], q["yp"])
    finally:
        handle.set_option("RAGGED_ITEM", None)
    o = _outputs(NB, 24, np.float32)
    hd = _abi.Handle(0)
    hd.set_option("RAGGED_ITEM", W)
    _ragged(hd, q, o)
    hd.close()
    assert np.array_equal(lp, o["lp"])
    for b, n in enumerate(COUNTS):
        _assert_fp32_within_lapack(q["mw"][b], q["dense"][b], np.asfortranarray(q["Xw"][b][:, :n]), q["s"][b], q["y"][b, :n], post[b].mw,
                                   post[b].Lw.toarray(), lp[b], what=f"{cls.__name__} regressor {b}")
