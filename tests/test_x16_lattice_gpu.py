"""The 16-bit feature routes at their ring, tile and padding seams (fused_x16_kernel; marg_planes_x16_kernel and
marginals_x16_kernel, K32): the two lattices of tests/_x16_problems.py against the oracle at the existing bounds, the integer cases bit
for bit against int64, both loaders against each other, device memspace at three base alignments, failed and non-finite regressors,
the pure stream over several tiles per wave, fp16 subnormal features.  What each lattice covers: tests/test_x16_problems_cpu.py."""
import numpy as np
import pytest

import _x16_problems as P
from _small_d_problems import _outputs, _result, _same_bits, _written
from _yardsticks import _assert_fp32_within_lapack
from blr_amd import _abi

pytestmark = pytest.mark.gpu

FMTS = ("bf16", "f16")
_id = lambda c: c.id  # noqa: E731


@pytest.fixture(scope="module")
def hd():
    h = _abi.Handle(0)
    yield h
    h.close()


def _gaps_keep_their_fill(q, o):
    wm, wT = _written(q["nb"], q["D"], o)
    assert np.all(np.isnan(o["mw_post"][~wm])) and np.all(np.isnan(o["T"][~wT])) and np.all(np.isnan(o["A"][~wT]))


def _dev(x):
    import torch
    return torch.from_numpy(x.view(np.int16) if x.dtype in (np.uint16, np.float16) else x).to("cuda:0")


def _outputs_equal(o1, o2, what=""):
    for k in ("mw_post", "T", "A", "lp", "info"):
        assert np.array_equal(o1[k], o2[k], equal_nan=True), (what, k)


# ---- a. the posterior lattice against the oracle ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", P.POST_LATTICE, ids=_id)
def test_posterior_lattice_against_oracle(hd, case):
    """4 x the error of fp32 LAPACK on the exactly widened features plus its floors (the rule of test_x16_gpu.py), per regressor"""
    q = P.post_lattice_problem(case)
    o = _outputs(q["nb"], case.D, np.float32, gaps=True)
    P.post_call(hd, q, o)
    assert hd.last_route() == case.route
    for b in range(q["nb"]):
        mw_p, T, A, lp, info = _result(q, o, b)
        assert info == 0
        _assert_fp32_within_lapack(q["mw"][b], q["dense"][b], np.asfortranarray(q["Xw"][b]), q["s"][b], q["y"][b], mw_p, A, lp, got_T=T,
                                   what=f"{case.id} regressor {b}")
    _gaps_keep_their_fill(q, o)


# ---- b. the Gram matrix on integers, both loaders ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", P.GRAM_EXACT_DS)
@pytest.mark.parametrize("xkind", P.XKINDS)
@pytest.mark.parametrize("fmt", FMTS)
def test_posterior_gram_exact_and_loaders_agree(hd, fmt, xkind, D):
    """Lw' = I + X X' bit for bit where a DMA stage lands in a used ring slot (N = 160), after two revolutions (293, 320) and where the
    call ends on a DMA stage (128, 160, 320); with NO_LDSDMA the register loaders build the same LDS image, so every output is the
    same bits."""
    for N in P.GRAM_EXACT_NS:
        q, ref, _ = P.gram_exact_problem(fmt, xkind, D, N)
        dma, regs = (_outputs(q["nb"], D, np.float32) for _ in range(2))
        P.post_call(hd, q, dma)
        assert hd.last_route() == q["route"]
        hd.set_option("NO_LDSDMA", "1")
        try:
            P.post_call(hd, q, regs)
            assert hd.last_route() == P.expected_route("posterior", fmt, xkind[:3], D, q["ldx"], q["strideX"], 0, q["nb"], ("NO_LDSDMA",))
            assert hd.last_route()[-2] in "01"
        finally:
            hd.set_option("NO_LDSDMA", None)
        for b in range(q["nb"]):
            A = _result(q, dma, b)[2]
            assert np.all(_result(q, dma, b)[4] == 0)
            assert np.array_equal(A.astype(np.float64), ref[b].astype(np.float64)), (q["route"], N, b)
        _outputs_equal(dma, regs, (q["route"], N))


# ---- c. device memspace at three base alignments ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("xkind", ["col_al", "row_al"])
@pytest.mark.parametrize("D", [40, 128])
def test_posterior_device_memspace_and_base_alignment(hd, D, xkind):
    import torch
    fmt = "bf16" if D == 40 else "f16"
    q = P._problem(fmt, xkind, D, 161, "factor", nb=P.LATTICE_NB)
    assert q["ldx"] % 8 == 0 and q["strideX"] % 8 == 0
    host = _outputs(q["nb"], D, np.float32, gaps=True)
    P.post_call(hd, q, host)
    assert hd.last_route() == q["route"] and q["route"][-2] in "23"
    qd = dict(q, **{k: _dev(q[k]) for k in ("y", "s", "mw", "Lw")})
    room = torch.zeros(q["X"].size + 8, dtype=torch.int16, device="cuda:0")
    assert room.data_ptr() % 16 == 0
    for off in (0, 2, 8):
        qd["X"] = room[off // 2:off // 2 + q["X"].size]
        qd["X"].copy_(_dev(q["X"]))
        od = {k: (_dev(v) if isinstance(v, np.ndarray) else v) for k, v in _outputs(q["nb"], D, np.float32, gaps=True).items()}
        torch.cuda.synchronize()
        P.post_call(hd, qd, od, memspace=_abi.MEM_DEVICE)
        torch.cuda.synchronize()
        assert hd.last_route() == P.expected_route("posterior", fmt, xkind[:3], D, q["ldx"], q["strideX"], off, q["nb"])
        assert (hd.last_route()[-2] in "23") == (off == 0)
        _outputs_equal({k: (v.cpu().numpy() if k in ("mw_post", "T", "A", "lp", "info") else v) for k, v in od.items()}, host, (xkind, D, off))
    # one regressor: an odd strideX is never applied, the aligned base decides
    one = _outputs(1, D, np.float32)
    P.post_call(hd, q, one, nb=1, strideX=q["strideX"] + 1)
    assert hd.last_route() == q["route"]
    _same_bits(_result(q, one, 0), _result(q, host, 0), "B = 1")


# ---- d. failed and non-finite regressors of the posterior ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["s0", "not_pd", "nan_feature"])
def test_posterior_failed_regressor_in_a_later_chunk(hd, what):
    D, N, nb, bad = 40, 161, 5, 3
    q = P._problem("bf16", "col_al", D, N, "dense", nb=nb)
    clean, got = (_outputs(nb, D, np.float32, gaps=True) for _ in range(2))
    P.post_call(hd, q, clean)
    if what == "s0":
        q["s"][bad] = 0.0
    elif what == "not_pd":
        q["Lw"][bad].reshape((D, D), order="F")[7, 7] = -1.0
    else:
        X = q["X"][bad * q["strideX"]:].reshape(-1)
        X[9 * q["ldx"] + 11] = 0x7FC0  # feature 11 of observation 9
    hd.set_option("MAX_CHUNK", "2")
    try:
        P.post_call(hd, q, got)
        assert hd.get_stat("last_chunks") == 3
    finally:
        hd.set_option("MAX_CHUNK", None)
    for b in range(nb):
        if b != bad:
            _same_bits(_result(q, got, b), _result(q, clean, b), f"{what}: regressor {b}")
    _gaps_keep_their_fill(q, got)
    if what == "nan_feature":
        return
    # what blr_posterior_batched_f32 says of the widened copy of the same regressor
    f = _outputs(1, D, np.float32)
    hd.posterior_batched(np.float32, _abi.MEM_HOST, _abi.LAYOUT_COLVECS, 1, D, N, np.asfortranarray(q["Xw"][bad]), D, 0, q["y"][bad], N,
                         _abi.NOISE_ISOTROPIC, q["s"][bad:bad + 1], 1, q["prior_kind"], q["mw"][bad], D, q["Lw"][bad], q["ldl"], D * D,
                         f["mw_post"], f["stride_mwpost"], f["T"], f["ldt"], f["strideT"], f["A"], f["ldt"], f["strideT"], f["lp"], f["info"])
    mw_p, T, _, _, info = _result(q, got, bad)
    assert info == int(f["info"][0]) and info != 0
    assert np.all(np.isnan(mw_p)) and np.all(np.isnan(T))


# ---- e. the marginals lattice against the oracle ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", P.MARG_LATTICE, ids=_id)
def test_marginals_lattice_against_oracle(hd, case):
    """4 x the float32 oracle's own error + 4 eps32 per regressor (the rule of test_x16_marg_gpu.py); NaN behind the N outputs"""
    q = P.marg_lattice_problem(case)
    o = P._out(case.N, q["nb"])
    P.marg_call(hd, q, o)
    assert hd.last_route() == case.route and np.all(o["info"] == 0)
    P._assert_within_oracle(q, o)


# ---- f. marginals on integers ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("diag_noise", [False, True], ids=["iso", "diagnoise"])
@pytest.mark.parametrize("D", P.MARG_EXACT_DS)
@pytest.mark.parametrize("xkind", P.XKINDS)
@pytest.mark.parametrize("fmt", FMTS)
def test_marginals_exact_on_integers(hd, fmt, xkind, D, diag_noise):
    """the construction of test_x16_marginals_exact_on_integers at nJ = 7 and 8 with pad rows in the last column block, with no partial
    tile (N = 128) and with two workgroups per regressor (N = 293); integer noise, per input too"""
    for N in P.MARG_EXACT_NS:
        q, mean, var, _ = P.marg_exact_problem(fmt, xkind, D, N, diag_noise)
        o = P._out(N, q["nb"])
        P.marg_call(hd, q, o)
        assert hd.last_route() == q["route"] and np.all(o["info"] == 0)
        assert np.array_equal(o["mean"][:, :N], mean) and np.array_equal(o["var"][:, :N], var), (q["route"], N)
        assert np.all(np.isnan(o["mean"][:, N:])) and np.all(np.isnan(o["var"][:, N:]))


# ---- g. the pure stream over several tiles per wave -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", P.PURE_DS)
@pytest.mark.parametrize("xkind", P.XKINDS)
@pytest.mark.parametrize("fmt", FMTS)
def test_pure_stream_over_several_tiles_per_wave(hd, fmt, xkind, D):
    """8 CUs + 1 regressors: one workgroup each, every wave prefetches and hands over at least one tile (features AND noise); then the
    same as a mean-only call without noise and prior"""
    import torch
    B = 8 * torch.cuda.get_device_properties(0).multi_processor_count + 1
    q, mean, var, _ = P.pure_stream_problem(fmt, xkind, D, B)
    o, m_only = P._out(P.PURE_N, B), P._out(P.PURE_N, B)
    P.marg_call(hd, q, o)
    assert hd.last_route() == q["route"] and np.all(o["info"] == 0)
    assert np.array_equal(o["mean"][:, :P.PURE_N], mean) and np.array_equal(o["var"][:, :P.PURE_N], var)
    assert np.all(np.isnan(o["mean"][:, P.PURE_N:])) and np.all(np.isnan(o["var"][:, P.PURE_N:]))
    P.marg_call(hd, dict(q, s=None, Lw=None), m_only, var=False)
    assert np.all(m_only["info"] == 0) and np.all(np.isnan(m_only["var"]))
    assert np.array_equal(m_only["mean"], o["mean"], equal_nan=True)


# ---- h. failed and non-finite inputs of the marginals ------------------------------------------------------------------------------------------------
def test_marginals_failed_regressor_in_a_later_chunk(hd):
    q = P._marg_problem("f16", "row_al", 88, 293, "dense", diag_noise=True)
    q["Lw"][3].reshape((88, 88), order="F")[7, 7] = -1.0  # not positive definite from the eighth leading minor on
    o = P._out(293)
    hd.set_option("MAX_CHUNK", "2")
    try:
        P.marg_call(hd, q, o)
        assert hd.get_stat("last_chunks") == 3
    finally:
        hd.set_option("MAX_CHUNK", None)
    assert o["info"][3] > 0 and np.all(np.delete(o["info"], 3) == 0)
    assert np.all(np.isnan(o["mean"][3])) and np.all(np.isnan(o["var"][3]))
    P._assert_within_oracle(q, o, regs=(0, 1, 2, 4))


@pytest.mark.parametrize("bad", ["inf", "nan"])
@pytest.mark.parametrize("prior", ["factor", "diag"])
@pytest.mark.parametrize("xkind", ["col_al", "row_odd"])
@pytest.mark.parametrize("fmt", FMTS)
def test_marginals_non_finite_feature_stays_in_its_input(hd, fmt, xkind, prior, bad):
    """include/blr_mi355x.h, Numerics of blr_marginals_batched_x16: with a factor prior var_n of THAT input is NaN; mean_n and the var_n
    of a diagonal prior follow fp32 arithmetic on the widened values; other inputs of the call are not affected"""
    D, N, reg, n, d = 40, 45, 2, 20, 11
    q = P._marg_problem(fmt, xkind, D, N, prior, diag_noise=(fmt == "f16"))
    clean, got = P._out(N), P._out(N)
    P.marg_call(hd, q, clean)
    bits = {("bf16", "inf"): 0xFF80, ("bf16", "nan"): 0x7FC0, ("f16", "inf"): 0xFC00, ("f16", "nan"): 0x7E00}[fmt, bad]
    at = reg * q["strideX"] + (n * q["ldx"] + d if xkind.startswith("col") else d * q["ldx"] + n)
    q["X"].view(np.uint16)[at] = bits
    x = q["Xw"][reg, :, n].copy()
    x[d] = -np.inf if bad == "inf" else np.nan
    P.marg_call(hd, q, got)
    assert np.all(got["info"] == 0)
    keep = np.ones((P.NB, N), bool)
    keep[reg, n] = False
    for k in ("mean", "var"):
        assert np.array_equal(got[k][:, :N][keep], clean[k][:, :N][keep]), k
        assert np.all(np.isnan(got[k][:, N:]))
    with np.errstate(all="ignore"):
        want_mean = np.sum(x * q["mw"][reg], dtype=np.float32)
        s_n = q["s"][reg, n] if fmt == "f16" else q["s"][reg]
        want_var = np.float32(np.nan) if prior == "factor" else np.sum(x * x / q["Lw"][reg], dtype=np.float32) + s_n
    same_class = lambda a, b: (np.isnan(a) and np.isnan(b)) or (np.isinf(a) and a == b)  # noqa: E731
    assert not np.isfinite(want_mean) and not np.isfinite(want_var)
    assert same_class(got["mean"][reg, n], want_mean), (got["mean"][reg, n], want_mean)
    assert same_class(got["var"][reg, n], want_var), (got["var"][reg, n], want_var)


# ---- i. fp16 subnormal features ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [40, 128])
@pytest.mark.parametrize("xkind", P.XKINDS)
def test_posterior_keeps_fp16_subnormals(hd, xkind, D):
    """features k 2^-24 (fp16 subnormals), prior 2^-48 I, unit noise: Lw' = 2^-48 (I + K K') bit for bit -- the matrix instruction
    flushes no subnormal operand, or the Gram matrix would be the prior"""
    q, ref, _ = P.gram_exact_problem("f16", xkind, D, 131, scale=P.SUBNORMAL)
    assert np.all(np.abs(q["Xw"]) < np.finfo(np.float16).tiny)
    o = _outputs(q["nb"], D, np.float32)
    P.post_call(hd, q, o)
    assert hd.last_route() == q["route"]
    for b in range(q["nb"]):
        _, _, A, _, info = _result(q, o, b)
        assert info == 0
        assert np.array_equal(A.astype(np.float64) * 2.0 ** 48, ref[b].astype(np.float64)), (q["route"], b)


@pytest.mark.parametrize("diag_noise", [False, True], ids=["iso", "diagnoise"])
@pytest.mark.parametrize("D", [40, 113])
@pytest.mark.parametrize("xkind", P.XKINDS)
def test_marginals_keep_fp16_subnormals(hd, xkind, D, diag_noise):
    """features k 2^-24, U = 2^-24 (I + N0), mw = 2^24 integers: the integer result of test_marginals_exact_on_integers bit for bit --
    the widening in registers flushes no subnormal (the matrix instruction sees their bf16 pieces, which are normal)"""
    q, mean, var, _ = P.marg_exact_problem("f16", xkind, D, 131, diag_noise, scale=P.SUBNORMAL)
    o = P._out(131, q["nb"])
    P.marg_call(hd, q, o)
    assert hd.last_route() == q["route"] and np.all(o["info"] == 0)
    assert np.array_equal(o["mean"][:, :131], mean) and np.array_equal(o["var"][:, :131], var), q["route"]
