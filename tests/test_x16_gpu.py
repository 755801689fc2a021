"""blr_posterior_batched_x16 (fused_x16_kernel) on the GPU: 16-bit features against the fp64 oracle on the exactly
widened values at the fp32 route's tolerance, the Gram matrix bit for bit on integer features, argument errors, chunk seams, and
the Python front (ColVecs16 / RowVecs16)."""
import numpy as np
import pytest

import blr_amd as R
from _small_d_problems import _outputs, _result, _same_bits
from _x16_problems import NB, PRIORS, XKINDS, _problem
from _yardsticks import _assert_fp32_within_lapack
from blr_amd import _abi

pytestmark = pytest.mark.gpu

@pytest.fixture(scope="module")
def hd():
    h = _abi.Handle(0)
    yield h
    h.close()


def _call(hd, q, o, **over):
    a = dict(q, noise_kind=_abi.NOISE_ISOTROPIC, strides=1)
    a.update(over)
    return hd.posterior_batched_x16(a["xfmt"], _abi.MEM_HOST, a["layout"], a["nb"], a["D"], a["N"], a["X"], a["ldx"], a["strideX"], a["y"], a["N"],
                                    a["noise_kind"], a["s"], a["strides"], a["prior_kind"], a["mw"], a["D"], a["Lw"], a["ldl"], a["Lw"].shape[1],
                                    o["mw_post"], o["stride_mwpost"], o["T"], o["ldt"], o["strideT"], o["A"], o["ldt"], o["strideT"], o["lp"], o["info"])


@pytest.mark.parametrize("N", [29, 64, 131])
@pytest.mark.parametrize("D", [5, 16, 40, 72, 128])
@pytest.mark.parametrize("xkind", XKINDS)
@pytest.mark.parametrize("fmt", ["bf16", "f16"])
def test_x16_against_oracle(hd, fmt, xkind, D, N):
    """Every loader, block count and stage seam: 4 x the error of fp32 LAPACK on the widened features, nothing added."""
    q = _problem(fmt, xkind, D, N, PRIORS[(D // 8 + N + XKINDS.index(xkind)) % 3])
    o = _outputs(NB, D, np.float32, gaps=True)
    _call(hd, q, o)
    assert hd.last_route() == q["route"]
    for b in range(NB):
        mw_p, T, A, lp, info = _result(q, o, b)
        assert info == 0
        _assert_fp32_within_lapack(q["mw"][b], q["dense"][b], np.asfortranarray(q["Xw"][b]), q["s"][b], q["y"][b], mw_p, A, lp, got_T=T,
                                   what=f"{q['route']} regressor {b}")


@pytest.mark.parametrize("D", [40, 128])
@pytest.mark.parametrize("xkind", XKINDS)
@pytest.mark.parametrize("fmt", ["bf16", "f16"])
def test_x16_gram_is_exact_on_integers(hd, fmt, xkind, D):
    """Integer features in [-8, 8], unit prior and noise: Lw' = I + X X' bit for bit (every partial sum is below 2^24) -- a dropped or
    doubled tail column, a pad row that is not zero or operand maps that disagree would show."""
    q = _problem(fmt, xkind, D, 131, "diag", ints=True)
    o = _outputs(NB, D, np.float32)
    _call(hd, q, o)
    for b in range(NB):
        Xi = q["Xw"][b].astype(np.int64)
        assert np.array_equal(_result(q, o, b)[2].astype(np.int64), np.eye(D, dtype=np.int64) + Xi @ Xi.T), (q["route"], b)
        assert np.all(_result(q, o, b)[2] == np.rint(_result(q, o, b)[2]))


@pytest.mark.parametrize("what,code", [("D129", -6), ("diag_noise", -13), ("dense_noise", -13), ("xfmt", -4)])
def test_x16_argument_errors(hd, what, code):
    D = 129 if what == "D129" else 16
    q = _problem("bf16", "col_al", D, 29, "diag")
    o = _outputs(NB, D, np.float32)
    before = {k: np.copy(v) for k, v in o.items() if isinstance(v, np.ndarray)}
    over = {"diag_noise": dict(noise_kind=_abi.NOISE_DIAGONAL, s=np.ones(NB * 29, np.float32), strides=29),
            "dense_noise": dict(noise_kind=_abi.NOISE_DENSE), "xfmt": dict(xfmt=2)}.get(what, {})
    with pytest.raises(_abi.BLRError) as e:
        _call(hd, q, o, **over)
    assert e.value.code == code and len(str(e.value).split(":", 2)[2].strip()) > 0
    for k, v in before.items():
        assert np.array_equal(o[k], v, equal_nan=True), k


def test_x16_chunk_seams_and_shared_x(hd):
    q = _problem("f16", "row_al", 72, 64, "factor")
    whole, parts, shared, copies = (_outputs(NB, 72, np.float32) for _ in range(4))
    _call(hd, q, whole)
    hd.set_option("MAX_CHUNK", "2")
    try:
        _call(hd, q, parts)
        assert hd.get_stat("last_chunks") == 3
    finally:
        hd.set_option("MAX_CHUNK", None)
    # strideX = 0: every regressor reads the first one's features
    _call(hd, q, shared, strideX=0)
    rep = dict(q, X=np.tile(q["X"][:q["strideX"]], NB))
    _call(hd, rep, copies)
    for b in range(NB):
        _same_bits(_result(q, whole, b), _result(q, parts, b), f"MAX_CHUNK regressor {b}")
        _same_bits(_result(q, shared, b), _result(q, copies, b), f"strideX = 0 regressor {b}")


@pytest.mark.parametrize("fmt,col", [("bf16", True), ("f16", False)])
def test_x16_python_front(fmt, col):
    D, N = 40, 131
    rng = np.random.Generator(np.random.PCG64(7))
    fxs, ys, raw = [], [], []
    for b in range(3):
        Xf = rng.standard_normal((D, N)).astype(np.float32)
        X16 = R.bf16_bits(Xf) if fmt == "bf16" else Xf.astype(np.float16)
        mw, d = (0.2 * rng.standard_normal(D)).astype(np.float32), np.exp(0.3 * rng.standard_normal(D)).astype(np.float32)
        y = (R.widen16(X16, fmt).T.astype(float) @ (rng.standard_normal(D) / np.sqrt(D)) + rng.standard_normal(N)).astype(np.float32)
        x = R.ColVecs16(np.asfortranarray(X16), fmt) if col else R.RowVecs16(np.ascontiguousarray(X16.T), fmt)
        fxs.append(R.BayesianLinearRegressor(mw, R.Diagonal(d))(x, np.float32(0.6)))
        ys.append(y)
        raw.append((mw, d, np.asfortranarray(R.widen16(X16, fmt)), np.float32(0.6), y))
    posts, lps = R.posterior_map(fxs, ys), R.logpdf_map(fxs, ys)
    for (mw, d, Xw, s, y), post, lp in zip(raw, posts, lps):
        _assert_fp32_within_lapack(mw, d, Xw, s, y, post.mw, post.Lw.toarray(), lp)
    assert R.logpdf(fxs[0], ys[0]) == lps[0]
    short = R.BayesianLinearRegressor(raw[0][0], R.Diagonal(raw[0][1]))(R.ColVecs16(np.asfortranarray(fxs[0].x.X[:, :100] if col else fxs[0].x.X[:100].T), fmt), 0.6)
    with pytest.raises(ValueError, match="unequal N"):
        R.logpdf_map([fxs[0], short], [ys[0], ys[0][:100]])
