"""blr_marginals_batched_x16 (marginals_x16_kernel) on the GPU: 16-bit inputs against the fp64 oracle on the exactly
widened values, bit for bit on integers, NULL outputs, chunk seams, shared X, both memspaces, a failed regressor, argument errors and
the Python front."""
import numpy as np
import pytest

import blr_amd as R
from blr_amd import _abi
from oracle import blr_oracle as O
from _x16_problems import EPS32, NB, PRIORS, XKINDS, _assert_within_oracle, _marg_problem, _out, _rel

pytestmark = pytest.mark.gpu

@pytest.fixture(scope="module")
def hd():
    h = _abi.Handle(0)
    yield h
    h.close()


def _call(hd, q, o, mean=True, var=True, memspace=_abi.MEM_HOST, **over):
    a = dict(q, **over)
    ptr = (lambda x: x.data_ptr()) if memspace == _abi.MEM_DEVICE else (lambda x: x)
    return hd.marginals_batched_x16(a["xfmt"], memspace, a["layout"], a["nb"], a["D"], a["N"], ptr(a["X"]), a["ldx"], a["strideX"],
                                    a["noise_kind"], ptr(a["s"]), a["strides"], a["prior_kind"], ptr(a["mw"]), a["D"], ptr(a["Lw"]), a["ldl"],
                                    a["Lw"].shape[1], ptr(o["mean"]) if mean else None, o["mean"].shape[1], ptr(o["var"]) if var else None,
                                    o["var"].shape[1], ptr(o["info"]))


@pytest.mark.parametrize("N", [1, 29, 131])
@pytest.mark.parametrize("D", [5, 16, 40, 72, 128])
@pytest.mark.parametrize("xkind", XKINDS)
@pytest.mark.parametrize("fmt", ["bf16", "f16"])
def test_x16_marginals_against_oracle(hd, fmt, xkind, D, N):
    """Every loader, column-block count and tile seam.  (prior, noise) = the six pairs in turn: at a fixed D the index below runs over
    all of 0 .. 5 (N contributes 0, 4, 2; xkind 0 .. 3; fmt 0, 3), so every pair occurs at D = 128 and at D = 40."""
    i = [1, 29, 131].index(N) * 4 + XKINDS.index(xkind) + 3 * (fmt == "f16") + D // 8
    q = _marg_problem(fmt, xkind, D, N, PRIORS[i % 3], diag_noise=(i % 6) >= 3)
    o = _out(N)
    _call(hd, q, o)
    assert hd.last_route() == q["route"] and np.all(o["info"] == 0)
    _assert_within_oracle(q, o)


@pytest.mark.parametrize("D", [40, 128])
@pytest.mark.parametrize("xkind", XKINDS)
@pytest.mark.parametrize("fmt", ["bf16", "f16"])
def test_x16_marginals_exact_on_integers(hd, fmt, xkind, D):
    """Integer features in [-8, 8]; U = I + N0 with N0 in rows < D / 2 and columns >= D / 2 (at most three entries of +-1 per column), so
    U^-1 = I - N0 exactly; integer mw, s = 1: every z entry is an integer of magnitude <= 32 and every partial sum is below 2^24, so
    mean and var are the int64 computation bit for bit -- a wrong operand map, a dropped k-step of the triangle, a pad row that is not
    zero or pieces added twice would show."""
    q = _marg_problem(fmt, xkind, D, 131, "factor", diag_noise=False, ints=True)
    rng = np.random.Generator(np.random.PCG64(D))
    N0 = np.zeros((NB, D, D), np.int64)
    for b in range(NB):
        for c in range(D // 2, D):
            N0[b, rng.choice(D // 2, size=3, replace=False), c] = rng.choice([-1, 1], size=3)
    q["Lw"] = np.stack([(np.eye(D, dtype=np.int64) + N0[b]).astype(np.float32).reshape(-1, order="F") for b in range(NB)])
    q["mw"] = rng.integers(-3, 4, size=(NB, D)).astype(np.float32)
    o = _out(131)
    _call(hd, q, o)
    assert np.all(o["info"] == 0)
    for b in range(NB):
        Xi = q["Xw"][b].astype(np.int64)
        z = (np.eye(D, dtype=np.int64) - N0[b]).T @ Xi  # U^-T x
        assert np.max(np.abs(z)) <= 32
        assert np.array_equal(o["mean"][b, :131], (Xi.T @ q["mw"][b].astype(np.int64)).astype(np.float32)), (q["route"], b)
        assert np.array_equal(o["var"][b, :131], (np.sum(z * z, axis=0) + 1).astype(np.float32)), (q["route"], b)


def test_x16_marginals_null_outputs_chunks_and_shared_x(hd):
    q = _marg_problem("f16", "row_al", 72, 131, "factor", diag_noise=True)
    both, m_only, v_only, parts, shared, copies = (_out(131) for _ in range(6))
    _call(hd, q, both)
    _call(hd, q, m_only, var=False)
    _call(hd, q, v_only, mean=False)
    assert np.all(np.isnan(m_only["var"])) and np.all(np.isnan(v_only["mean"]))
    assert np.array_equal(m_only["mean"], both["mean"], equal_nan=True) and np.array_equal(v_only["var"], both["var"], equal_nan=True)
    hd.set_option("MAX_CHUNK", "2")
    try:
        _call(hd, q, parts)
        assert hd.get_stat("last_chunks") == 3
    finally:
        hd.set_option("MAX_CHUNK", None)
    _call(hd, q, shared, strideX=0)  # every regressor reads the first one's inputs
    _call(hd, dict(q, X=np.tile(q["X"][:q["strideX"]], NB)), copies)
    for k in ("mean", "var"):
        assert np.array_equal(parts[k], both[k], equal_nan=True), k
        assert np.array_equal(shared[k], copies[k], equal_nan=True) and not np.array_equal(shared[k], both[k], equal_nan=True), k


def test_x16_marginals_device_memspace(hd):
    import torch
    q = _marg_problem("bf16", "col_al", 128, 131, "dense", diag_noise=False)
    host = _out(131)
    _call(hd, q, host)
    dev = lambda x: torch.from_numpy(x.view(np.int16) if x.dtype == np.uint16 else x).to("cuda:0")
    qd = dict(q, **{k: dev(q[k]) for k in ("X", "s", "mw", "Lw")})
    od = {k: dev(v) for k, v in _out(131).items()}
    torch.cuda.synchronize()
    _call(hd, qd, od, memspace=_abi.MEM_DEVICE)
    torch.cuda.synchronize()
    for k in ("mean", "var", "info"):
        assert np.array_equal(od[k].cpu().numpy(), host[k], equal_nan=True), k


def test_x16_marginals_failed_regressor(hd):
    q = _marg_problem("bf16", "col_odd", 40, 29, "dense", diag_noise=False)
    q["Lw"][2].reshape((40, 40), order="F")[7, 7] = -1.0  # not positive definite from the eighth leading minor on
    o = _out(29)
    _call(hd, q, o)
    assert o["info"][2] > 0 and np.all(np.delete(o["info"], 2) == 0)
    assert np.all(np.isnan(o["mean"][2])) and np.all(np.isnan(o["var"][2]))
    _assert_within_oracle(q, o, regs=(0, 1, 3, 4))


@pytest.mark.parametrize("what,code", [("D129", -6), ("dense_noise", -11), ("xfmt", -4)])
def test_x16_marginals_argument_errors(hd, what, code):
    D = 129 if what == "D129" else 16
    q = _marg_problem("bf16", "col_al", D, 29, "diag", diag_noise=False)
    o = _out(29)
    with pytest.raises(_abi.BLRError) as e:
        _call(hd, q, o, **{"dense_noise": dict(noise_kind=_abi.NOISE_DENSE), "xfmt": dict(xfmt=2)}.get(what, {}))
    assert e.value.code == code and len(str(e.value).split(":", 2)[2].strip()) > 0
    assert np.all(np.isnan(o["mean"])) and np.all(np.isnan(o["var"])) and np.all(o["info"] == 7)


def test_x16_marginals_python_front():
    D, N = 40, 131
    rng = np.random.Generator(np.random.PCG64(11))
    fxs, raw = [], []
    for fmt, col in (("bf16", True), ("f16", False), ("bf16", True), ("bf16", True)):
        X16 = R.bf16_bits(rng.standard_normal((D, N)).astype(np.float32)) if fmt == "bf16" else rng.standard_normal((D, N)).astype(np.float16)
        mw, d = (0.2 * rng.standard_normal(D)).astype(np.float32), np.exp(0.3 * rng.standard_normal(D)).astype(np.float32)
        x = R.ColVecs16(np.asfortranarray(X16), fmt) if col else R.RowVecs16(np.ascontiguousarray(X16.T), fmt)
        fxs.append(R.BayesianLinearRegressor(mw, R.Diagonal(d))(x, np.float32(0.6)))
        raw.append((mw, d, np.asfortranarray(R.widen16(X16, fmt)), np.full(N, 0.6, np.float32)))
    singles = [R.mean_and_var(fx) for fx in fxs]
    for p, got in zip(raw[:2], singles):  # a ColVecs16 (bf16) and a RowVecs16 (fp16) problem, at the bound of the oracle test
        for k, (r64, r32) in enumerate(zip(*([O.mean(a[0], a[2]), O.var(*a)] for a in ([x.astype(float) for x in p], p)))):
            assert got[k].dtype == np.float32 and _rel(got[k], r64) <= 4 * _rel(r32, r64) + 4 * EPS32, (k, _rel(got[k], r64))
    same = [fxs[0], fxs[2], fxs[3]]
    h = _abi.default_handle()
    h.set_option("MAX_CHUNK", "2")
    try:
        mapped = R.mean_and_var_map(same)
        assert h.get_stat("last_chunks") == 2  # ONE call for the three problems
    finally:
        h.set_option("MAX_CHUNK", None)
    for (m, v), k in zip(mapped, (0, 2, 3)):
        assert np.array_equal(m, singles[k][0]) and np.array_equal(v, singles[k][1])
    assert np.array_equal(R.mean(fxs[1]), singles[1][0]) and np.array_equal(R.var(fxs[1]), singles[1][1])
    big = R.BayesianLinearRegressor(np.zeros(129, np.float32), R.Diagonal(np.ones(129, np.float32)))
    with pytest.raises(ValueError, match="widen"):
        R.mean_and_var(big(R.RowVecs16(np.zeros((4, 129), np.float16)), 0.5))
