"""CPU-side checks of the leave-fold-out predictives for large folds (blr_kfold_large_batched_*, kfold_large, kfold_large_map,
cross_validate, ResidentPosterior.kfold_large): the symbols are declared, exported and bound, the header's contract
words, the Julia shim's arity, the argument checks that need no device (they come before the handle check), the routing of the Python
functions with the handle replaced by a recorder, and the weight-space closed form of tests/_kfold_large_ref.py (the yardstick of
tests/test_kfold_large_gpu.py) against brute-force refits with the oracle."""
import os
import re

import numpy as np
import pytest

import blr_amd
from blr_amd import _abi
from blr_amd import regressor as R

from _kfold_ref import brute_force, closed_form, posterior_state, rng_of, state
from _kfold_large_ref import SHAPES, closed_form_large, fp32_bounds_large
from _recorder import Recorder as _Recorder

SYMS = ("blr_kfold_large_batched_f64", "blr_kfold_large_batched_f32")
ARITY = 28


def _header(repo_root):
    return open(os.path.join(repo_root, "include", "blr_mi355x.h")).read()


def _arity(text, name):
    m = re.search(rf"\bint\s+{name}\s*\(([^;]*?)\)\s*;", text, flags=re.S)
    assert m, name
    return len([p for p in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",") if p.strip()])


def test_symbols_declared_exported_and_bound(repo_root):
    header = _header(repo_root)
    lib = _abi.load_library()
    for name in SYMS:
        assert re.search(rf"\bint\s+{name}\s*\(", header), name
        assert hasattr(lib, name), name
        assert name in _abi.EXPORTED_SYMBOLS
        assert _arity(header, name) == len(_abi._SIGS[name][0]) == ARITY
        assert _abi._SIGS[name] == _abi._SIGS[name.replace("_large", "")]  # the argument list of blr_kfold_batched_*
    assert hasattr(_abi.Handle, "kfold_large")
    block = header[header.index("predictives for LARGE folds"):header.index("int blr_kfold_large_batched_f64")]
    for word in ("1 <= D <= 128", "ceil(N / F) <= 1024", "F > N is allowed", "2^30", "kfold_degenerate", "bit-reproducible", "No float atomics",
                 "NOT promised", "Cancellation", "float32 shows it first", "65535", "256 MiB", "MAX_CHUNK", "last_chunks",
                 "stride of 0 shares", "blr_downdate_factor_*", "blr_posterior_batched_*", "src/bayesian_linear_regression.jl:55-58",
                 "read twice", "only enqueues", "left untouched", "Every other fold"):
        assert word in block, word
    assert "blr_kfold_large_batched_*" in header[header.index("Counters of the handle"):header.index("int blr_get_stat")]
    assert "blr_kfold_large_batched_*" in _abi.Handle.get_stat.__doc__


def test_python_surface():
    for name in ("kfold_large", "kfold_large_map", "cross_validate"):
        assert getattr(blr_amd, name) is getattr(R, name)
        assert name in blr_amd.__all__ and name in R.__all__
    assert callable(blr_amd.ResidentPosterior.kfold_large)


def test_julia_shim_calls_both_symbols_with_the_header_arity(repo_root):
    jl = open(os.path.join(repo_root, "julia", "BLRMI355X.jl")).read()
    header = _header(repo_root)
    assert "function kfold_large!(" in jl
    for name in SYMS:
        m = re.search(rf"ccall\(\(:{name}, LIB\), Cint,\s*\(([^)]*)\)", jl)
        assert m, name
        types = [t for t in m.group(1).split(",") if t.strip()]
        assert len(types) == _arity(header, name) == ARITY, name


def _call(name, **kw):
    """blr_kfold_large_batched_* with a NULL handle and valid arguments except those in kw."""
    lib = _abi.load_library()
    D, N, B, F = 4, 5, 2, 2
    a = dict(memspace=_abi.MEM_HOST, layout=_abi.LAYOUT_COLVECS, B=B, D=D, N=N, F=F, X=np.zeros((D, N * B)), ldx=D, strideX=D * N,
             y=np.zeros(N * B), stridey=N, noise_kind=_abi.NOISE_DIAGONAL, s=np.ones(N * B), strides=N, mw=np.zeros(D * B), stridemw=D,
             T=np.eye(D), ldt=D, strideT=0, km=np.zeros(N * B), stride_km=N, kv=np.zeros(N * B), stride_kv=N, kl=np.zeros(3 * B),
             stride_kl=3, tot=np.zeros(B), info=np.zeros(B, dtype=np.int32))
    a.update(kw)
    p = _abi._ptr
    return getattr(lib, name)(None, a["memspace"], a["layout"], a["B"], a["D"], a["N"], a["F"], p(a["X"]), a["ldx"], a["strideX"], p(a["y"]),
                              a["stridey"], a["noise_kind"], p(a["s"]), a["strides"], p(a["mw"]), a["stridemw"], p(a["T"]), a["ldt"],
                              a["strideT"], p(a["km"]), a["stride_km"], p(a["kv"]), a["stride_kv"], p(a["kl"]), a["stride_kl"], p(a["tot"]),
                              p(a["info"]))


@pytest.mark.parametrize("name", SYMS)
def test_argument_errors_without_a_device(name):
    # (the checks read no element of the data: the float64 buffers only provide non-NULL pointers for the f32 entry point too)
    assert _call(name, memspace=7) == -2
    assert _call(name, layout=2) == -3
    assert _call(name, B=-1) == -4
    assert _call(name, D=0) == -5
    assert _call(name, D=129, ldx=129, ldt=129) == -5                 # D > 128 is out of this entry point's range
    assert _call(name, N=-1) == -6
    assert _call(name, N=(1 << 30) + 1) == -6
    assert _call(name, F=0) == -7
    assert _call(name, F=-3) == -7
    assert _call(name, N=1025, F=1, B=1, X=np.zeros(1), y=np.zeros(1), s=np.zeros(1)) == -7       # ceil(N / F) = 1025
    assert _call(name, N=2049, F=2, B=1, X=np.zeros(1), y=np.zeros(1), s=np.zeros(1)) == -7       # ceil(2049 / 2) = 1025
    assert _call(name, X=None) == -8
    assert _call(name, ldx=3) == -9
    assert _call(name, layout=_abi.LAYOUT_ROWVECS, ldx=4) == -9
    assert _call(name, strideX=-1) == -10
    assert _call(name, y=None) == -11
    assert _call(name, stridey=-1) == -12
    assert _call(name, noise_kind=_abi.NOISE_DENSE) == -13            # dense noise couples the folds
    assert _call(name, noise_kind=7) == -13
    assert _call(name, s=None) == -14
    assert _call(name, strides=-1) == -15
    assert _call(name, mw=None) == -16
    assert _call(name, stridemw=-1) == -17
    assert _call(name, T=None) == -18
    assert _call(name, ldt=3) == -19
    assert _call(name, strideT=-1) == -20
    assert _call(name, stride_km=4) == -22                            # overlapping outputs for B = 2
    assert _call(name, stride_kv=4) == -24
    assert _call(name, stride_kl=2) == -26                            # nfolds = ceil(5 / 2) = 3
    assert _call(name, info=None) == -28
    # the ranges come first, in the order of the arguments
    assert _call(name, memspace=7, layout=2, F=0) == -2
    assert _call(name, F=0, ldx=0) == -7
    # valid arguments and a NULL handle: -1
    assert _call(name) == -1
    assert _call(name, strideX=0, stridey=0, strides=0, stridemw=0, strideT=0) == -1   # shared inputs
    assert _call(name, km=None, kv=None, kl=None, tot=None, stride_km=0, stride_kv=0, stride_kl=0) == -1   # any output may be NULL
    assert _call(name, B=1, stride_km=0, stride_kv=0, stride_kl=0) == -1                # a single regressor: any output stride
    assert _call(name, noise_kind=_abi.NOISE_ISOTROPIC, strides=1) == -1
    assert _call(name, F=65, stride_kl=1) == -1                                         # beyond blr_kfold_batched_*'s 64, and F > N: one fold
    assert _call(name, F=1 << 40, stride_kl=1) == -1
    assert _call(name, F=1, stride_kl=5, kl=np.zeros(10)) == -1
    assert _call(name, layout=_abi.LAYOUT_ROWVECS, ldx=5) == -1
    assert _call(name, N=0, X=None, y=None, s=None) == -1                               # the no-ops pass the checks
    assert _call(name, B=0) == -1
    assert _call(name, D=128, ldx=128, ldt=128, T=np.zeros(1), X=np.zeros(1), mw=np.zeros(1), B=1) == -1
    assert _call(name, N=1 << 30, F=1 << 20, X=np.zeros(1), B=1) == -1                  # 1024 folds of 2^20
    assert _call(name, N=1024, F=1, B=1, X=np.zeros(1), y=np.zeros(1), s=np.zeros(1)) == -1


def _problem(rng, D, N, x=None):
    f = R.BayesianLinearRegressor(rng.standard_normal(D), R.Diagonal(np.exp(0.1 * rng.standard_normal(D))))
    x = R.ColVecs(np.asfortranarray(rng.standard_normal((D, N)))) if x is None else x
    return f(x, R.Diagonal(np.exp(rng.standard_normal(N))))


def _buf(rec, ptr, dtype, count):
    return rec.bufs[ptr][:count * np.dtype(dtype).itemsize].view(dtype)


def test_equal_shapes_make_one_batched_call(monkeypatch):
    rec = _Recorder()
    monkeypatch.setattr(R, "_handle", lambda: rec)
    rng = np.random.default_rng(5)
    D, N, nb, F = 6, 211, 4, 100
    fxs = [_problem(rng, D, N) for _ in range(nb)]
    ys = [rng.standard_normal(N) for _ in range(nb)]
    out = R.kfold_large_map(fxs, ys, F)
    assert [k for k, _ in rec.calls] == ["posterior", "kfold_large"] and len(out) == nb
    assert all(isinstance(r, R.KFold) and r.mean.shape == (N,) and r.var.shape == (N,) and r.logpdf.shape == (3,) for r in out)
    a = rec.calls[1][1]
    assert a[:7] == (np.float64, _abi.MEM_DEVICE, _abi.LAYOUT_COLVECS, nb, D, N, F)
    assert a[8:10] == (D, D * N) and a[11] == N and a[12] == _abi.NOISE_DIAGONAL and a[14] == N
    assert a[16] == D and a[18:20] == (D, D * D)
    assert (a[21], a[23], a[25]) == (N, N, 3)
    # the state the posterior call wrote is what the K-fold call reads, and the data are staged once
    p = rec.calls[0][1]
    assert p[6] == a[7] and p[9] == a[10] and p[12] == a[13] and a[15] == p[20] and a[17] == p[22]


def test_mixed_shapes_fall_back_to_one_call_per_problem(monkeypatch):
    rec = _Recorder()
    monkeypatch.setattr(R, "_handle", lambda: rec)
    rng = np.random.default_rng(7)
    D = 6
    fxs = [_problem(rng, D, n) for n in (150, 140, 150)]
    out = R.kfold_large_map(fxs, [rng.standard_normal(n) for n in (150, 140, 150)], 70)
    assert [k for k, _ in rec.calls] == ["posterior", "kfold_large"] * 3
    assert [r.logpdf.shape for r in out] == [(3,), (2,), (3,)]
    assert all(c[1][3] == 1 for c in rec.calls)
    rec.calls.clear()
    assert R.kfold_large_map([], [], 70) == [] and rec.calls == []
    with pytest.raises(ValueError):
        R.kfold_large_map(fxs, [np.zeros(150)], 70)
    for bad in (0, -1, 2.5):
        with pytest.raises(ValueError):
            R.kfold_large(fxs[0], np.zeros(150), bad)
    with pytest.raises(ValueError, match="1024"):          # 1500 observations in folds of 1: 1500 folds
        R.kfold_large(_problem(rng, 2, 1500), np.zeros(1500), 1)
    with pytest.raises(NotImplementedError, match="128"):  # the limit is named
        R.kfold_large(_problem(rng, 129, 10), np.zeros(10), 5)
    with pytest.raises(NotImplementedError, match="128"):
        R.kfold_large_map([_problem(rng, 129, 10)], [np.zeros(10)], 5)
    # dense noise: loo's wording
    dense = R.BayesianLinearRegressor(np.zeros(D), R.Diagonal(np.ones(D)))(fxs[0].x, np.eye(150))
    with pytest.raises(NotImplementedError, match="block leave-out"):
        R.kfold_large(dense, np.zeros(150), 70)
    assert rec.calls == []
    # fold_size > N is one fold
    r = R.kfold_large(fxs[1], np.zeros(140), 1000)
    assert r.logpdf.shape == (1,) and rec.calls[-1][0] == "kfold_large" and rec.calls[-1][1][6] == 1000


def test_cross_validate_dispatches_on_the_fold_size(monkeypatch):
    rec = _Recorder()
    monkeypatch.setattr(R, "_handle", lambda: rec)
    rng = np.random.default_rng(6)
    N = 650
    fx, y = _problem(rng, 5, N), rng.standard_normal(N)
    r = R.cross_validate(fx, y, 10)              # F = 65
    assert rec.calls[-1][0] == "kfold_large" and rec.calls[-1][1][6] == 65 and r.logpdf.shape == (10,)
    r = R.cross_validate(fx, y, 11)              # F = ceil(650 / 11) = 60
    assert rec.calls[-1][0] == "kfold" and rec.calls[-1][1][6] == 60 and r.logpdf.shape == (11,)
    fx2, y2 = _problem(rng, 5, 640), rng.standard_normal(640)
    R.cross_validate(fx2, y2, 10)                # F = 64: still blr_kfold_batched_*
    assert rec.calls[-1][0] == "kfold" and rec.calls[-1][1][6] == 64
    R.cross_validate(fx, y, 5)                   # F = 130
    assert rec.calls[-1][0] == "kfold_large" and rec.calls[-1][1][6] == 130
    R.cross_validate(fx, y, 1)                   # one fold of everything
    assert rec.calls[-1][0] == "kfold_large" and rec.calls[-1][1][6] == N
    perm = rng.permutation(N)
    r = R.cross_validate(fx, y, 5, perm=perm)
    expect = np.empty(N)
    expect[perm] = np.arange(N)
    assert np.array_equal(r.mean, 10.0 + expect)
    for bad in (0, 2.5):
        with pytest.raises(ValueError):
            R.cross_validate(fx, y, bad)


def test_resident_kfold_large_passes_the_resident_pointers(monkeypatch):
    rec = _Recorder()
    monkeypatch.setattr(_abi, "default_handle", lambda: rec)
    rng = np.random.default_rng(8)
    D, N, F = 6, 170, 80
    Lw = R.PDMat(np.triu(rng.standard_normal((D, D))) + 3.0 * np.eye(D))
    st = R.ResidentPosterior(R.BayesianLinearRegressor(rng.standard_normal(D), Lw))
    X = np.asfortranarray(rng.standard_normal((D, N)))
    r = st.kfold_large(R.ColVecs(X), 0.5, rng.standard_normal(N), F)
    assert [k for k, _ in rec.calls] == ["kfold_large"] and isinstance(r, R.KFold) and r.logpdf.shape == (3,)
    a = rec.calls[0][1]
    assert a[1] == _abi.MEM_DEVICE and a[3:7] == (1, D, N, F) and a[12] == _abi.NOISE_ISOTROPIC
    assert a[15] == st._mw.ptr and a[17] == st._T.ptr and a[18] == D  # no copy of the state
    with pytest.raises(NotImplementedError):
        st.kfold_large(R.ColVecs(X), np.eye(N), np.zeros(N), F)
    with pytest.raises(ValueError):
        st.kfold_large(R.ColVecs(X), 0.5, np.zeros(N), 0)


@pytest.mark.parametrize("rowvecs", [False, True])
def test_perm_is_validated_gathered_and_scattered_back(monkeypatch, rowvecs):
    rec = _Recorder()
    monkeypatch.setattr(R, "_handle", lambda: rec)
    rng = np.random.default_rng(9)
    D, N, F = 3, 150, 70
    X = np.asfortranarray(rng.standard_normal((D, N)))
    s, y = np.exp(rng.standard_normal(N)), rng.standard_normal(N)
    f = R.BayesianLinearRegressor(np.zeros(D), R.Diagonal(np.ones(D)))
    x = R.RowVecs(np.ascontiguousarray(X.T)) if rowvecs else R.ColVecs(X)
    perm = rng.permutation(N)
    got = {}
    real = _Recorder.kfold_large

    def spy(self, *a):  # (the staged buffers are freed after the call: look at them now)
        got["X"] = _buf(rec, a[7], np.float64, D * N).copy()
        got["y"] = _buf(rec, a[10], np.float64, N).copy()
        got["s"] = _buf(rec, a[13], np.float64, N).copy()
        return real(self, *a)

    monkeypatch.setattr(_Recorder, "kfold_large", spy)
    r = R.kfold_large(f(x, R.Diagonal(s)), y, F, perm=perm)
    a = rec.calls[-1][1]
    assert a[2] == _abi.LAYOUT_COLVECS and a[8] == D   # both containers hold D x N column-major here
    assert np.array_equal(got["X"].reshape((D, N), order="F"), X[:, perm])
    assert np.array_equal(got["y"], y[perm]) and np.array_equal(got["s"], s[perm])
    # observation perm[n] was row n of the call: the recorder's 10 + n / 100 + n land at perm[n]
    expect = np.empty(N)
    expect[perm] = np.arange(N)
    assert np.array_equal(r.mean, 10.0 + expect) and np.array_equal(r.var, 100.0 + expect)
    for bad in (np.arange(N - 1), np.zeros(N, dtype=int)):
        with pytest.raises(ValueError):
            R.kfold_large(f(x, R.Diagonal(s)), y, F, perm=bad)


@pytest.fixture(scope="module")
def refits():
    """(D, N, F) -> the state, the closed form and the brute force, computed once"""
    out = {}
    for D, N, F in SHAPES:
        mw, U, X, s, y = state(rng_of(D + N), D, N)
        mwp, T = posterior_state(mw, U, X, s, y)
        out[(D, N, F)] = (mwp, T, X, s, y, closed_form_large(mwp, T, X, s, y, F), brute_force(mw, U.T @ U, X, s, y, F))
    return out


@pytest.mark.parametrize("D,N,F", SHAPES)
def test_closed_form_matches_brute_force_refits(refits, D, N, F):
    """The weight-space identities of the header in NumPy float64 against the chain rule with the oracle, rel 1e-10 of the output's
    scale per entry (measured: <= 3.1e-12, the mean at (32, 2200, 2100)); the cancellation of A - G_f stays <= 20 on these inputs."""
    mwp, T, X, s, y, (mean, var, lps, cancel), (m_o, v_o, lp_o) = refits[(D, N, F)]
    assert cancel <= 20.0, cancel
    np.testing.assert_allclose(lps, lp_o, rtol=1e-10)
    np.testing.assert_allclose(mean, m_o, rtol=1e-10, atol=1e-10 * np.max(np.abs(m_o)))
    np.testing.assert_allclose(var, v_o, rtol=1e-10)
    if F <= 64:  # the same quantities as the hat-matrix closed form of blr_kfold_batched_*
        m_h, v_h, lp_h, _ = closed_form(mwp, T, X, s, y, F)
        np.testing.assert_allclose(mean, m_h, rtol=1e-10, atol=1e-10 * np.max(np.abs(m_h)))
        np.testing.assert_allclose(var, v_h, rtol=1e-10)
        np.testing.assert_allclose(lps, lp_h, rtol=1e-10)


def test_fp32_yardstick_is_a_bound_of_fp32_size(refits):
    """The yardstick's bounds are those of a float32 computation: between 8 eps32 and 1e-3 of the output's scale on every shape."""
    eps = float(np.finfo(np.float32).eps)
    for (D, N, F), (mwp, T, X, s, y, _, _) in refits.items():
        truth, bounds = fp32_bounds_large(mwp, T, X, s, y, F)
        for t, b in zip(truth, bounds):
            scale = max(1.0, float(np.max(np.abs(t))))
            assert 8 * eps * scale <= b <= 1e-3 * scale, (D, N, F, b, scale)
