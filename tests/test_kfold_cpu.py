"""CPU-side checks of the exact leave-fold-out predictives (blr_kfold_batched_*, kfold, kfold_map, ResidentPosterior.kfold; DESIGN.md
K23): the symbols are declared, exported and bound, the header, the binding and the Julia shim agree on the arity, the argument checks
that need no device (they come before the handle check), the routing of the Python functions with the handle replaced by a recorder,
the closed form of tests/_kfold_ref.py (the yardstick of tests/test_kfold_gpu.py) against brute-force refits with the oracle, and the
register / scratch limits of kfold_kernel from the compiled code object."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import blr_amd
from blr_amd import _abi
from blr_amd import regressor as R

from _kfold_ref import brute_force, closed_form, posterior_state, rng_of, state
from _recorder import Recorder as _Recorder

SYMS = ("blr_kfold_batched_f64", "blr_kfold_batched_f32")
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
    assert _abi._SIGS[SYMS[0]] == _abi._SIGS[SYMS[1]]
    assert hasattr(_abi.Handle, "kfold")
    block = header[header.index("LEAVE-FOLD-OUT (K-fold) predictives"):header.index("int blr_kfold_batched_f64")]
    for word in ("1 <= F <= 64", "F > N is allowed", "16384", "kfold_degenerate", "bit-reproducible", "No float atomics", "NOT promised",
                 "correct, not fast", "SYNCHRONISES", "65535", "256 MiB", "MAX_CHUNK", "last_chunks", "stride of 0 shares"):
        assert word in block, word
    assert '"kfold_degenerate"' in header[header.index("Counters of the handle"):header.index("int blr_get_stat")]
    assert "kfold_degenerate" in _abi.Handle.get_stat.__doc__


def test_python_surface():
    for name in ("kfold", "kfold_map", "KFold"):
        assert getattr(blr_amd, name) is getattr(R, name)
        assert name in blr_amd.__all__ and name in R.__all__
    assert R.KFold._fields == ("mean", "var", "logpdf", "total")
    assert callable(blr_amd.ResidentPosterior.kfold)


def test_julia_shim_calls_both_symbols_with_the_header_arity(repo_root):
    jl = open(os.path.join(repo_root, "julia", "BLRMI355X.jl")).read()
    header = _header(repo_root)
    assert "function kfold!(" in jl
    for name in SYMS:
        m = re.search(rf"ccall\(\(:{name}, LIB\), Cint,\s*\(([^)]*)\)", jl)
        assert m, name
        types = [t for t in m.group(1).split(",") if t.strip()]
        assert len(types) == _arity(header, name) == ARITY, name


def _call(name, **kw):
    """blr_kfold_batched_* with a NULL handle and valid arguments except those in kw."""
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
    assert _call(name, D=8193) == -5
    assert _call(name, N=-1) == -6
    assert _call(name, N=(1 << 30) + 1) == -6
    assert _call(name, D=129, ldx=129, ldt=129, N=16385) == -6        # D > 128 goes through an N x N covariance
    assert _call(name, F=0) == -7
    assert _call(name, F=65) == -7
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
    assert _call(name, F=65, ldx=0) == -7
    # valid arguments and a NULL handle: -1
    assert _call(name) == -1
    assert _call(name, strideX=0, stridey=0, strides=0, stridemw=0, strideT=0) == -1   # shared inputs
    assert _call(name, km=None, kv=None, kl=None, tot=None, stride_km=0, stride_kv=0, stride_kl=0) == -1   # any output may be NULL
    assert _call(name, B=1, stride_km=0, stride_kv=0, stride_kl=0) == -1                # a single regressor: any output stride
    assert _call(name, noise_kind=_abi.NOISE_ISOTROPIC, strides=1) == -1
    assert _call(name, F=64, stride_kl=1) == -1                                         # F > N: one fold
    assert _call(name, F=1, stride_kl=5, kl=np.zeros(10)) == -1
    assert _call(name, layout=_abi.LAYOUT_ROWVECS, ldx=5) == -1
    assert _call(name, N=0, X=None, y=None, s=None) == -1
    assert _call(name, D=129, ldx=129, ldt=129, T=np.zeros(1), N=16384, X=np.zeros(1), B=1) == -1
    assert _call(name, N=1 << 30, X=np.zeros(1), B=1) == -1


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
    D, N, nb, F = 6, 11, 4, 4
    fxs = [_problem(rng, D, N) for _ in range(nb)]
    ys = [rng.standard_normal(N) for _ in range(nb)]
    out = R.kfold_map(fxs, ys, F)
    assert [k for k, _ in rec.calls] == ["posterior", "kfold"] and len(out) == nb
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
    fxs = [_problem(rng, D, n) for n in (5, 4, 5)]
    out = R.kfold_map(fxs, [rng.standard_normal(n) for n in (5, 4, 5)], 2)
    assert [k for k, _ in rec.calls] == ["posterior", "kfold"] * 3
    assert [r.logpdf.shape for r in out] == [(3,), (2,), (3,)]
    assert all(c[1][3] == 1 for c in rec.calls)
    rec.calls.clear()
    assert R.kfold_map([], [], 2) == [] and rec.calls == []
    with pytest.raises(ValueError):
        R.kfold_map(fxs, [np.zeros(5)], 2)
    for bad in (0, 65, 2.5):
        with pytest.raises(ValueError):
            R.kfold(fxs[0], np.zeros(5), bad)
    # dense noise: loo's wording
    dense = R.BayesianLinearRegressor(np.zeros(D), R.Diagonal(np.ones(D)))(fxs[0].x, np.eye(5))
    with pytest.raises(NotImplementedError, match="block leave-out"):
        R.kfold(dense, np.zeros(5), 2)
    assert rec.calls == []


def test_resident_kfold_passes_the_resident_pointers(monkeypatch):
    rec = _Recorder()
    monkeypatch.setattr(_abi, "default_handle", lambda: rec)
    rng = np.random.default_rng(8)
    D, N, F = 6, 7, 3
    Lw = R.PDMat(np.triu(rng.standard_normal((D, D))) + 3.0 * np.eye(D))
    st = R.ResidentPosterior(R.BayesianLinearRegressor(rng.standard_normal(D), Lw))
    X = np.asfortranarray(rng.standard_normal((D, N)))
    r = st.kfold(R.ColVecs(X), 0.5, rng.standard_normal(N), F)
    assert [k for k, _ in rec.calls] == ["kfold"] and isinstance(r, R.KFold) and r.logpdf.shape == (3,)
    a = rec.calls[0][1]
    assert a[1] == _abi.MEM_DEVICE and a[3:7] == (1, D, N, F) and a[12] == _abi.NOISE_ISOTROPIC
    assert a[15] == st._mw.ptr and a[17] == st._T.ptr and a[18] == D  # no copy of the state
    with pytest.raises(NotImplementedError):
        st.kfold(R.ColVecs(X), np.eye(N), np.zeros(N), F)


@pytest.mark.parametrize("rowvecs", [False, True])
def test_perm_gathers_the_inputs_and_scatters_mean_and_var(monkeypatch, rowvecs):
    rec = _Recorder()
    monkeypatch.setattr(R, "_handle", lambda: rec)
    rng = np.random.default_rng(9)
    D, N, F = 3, 7, 3
    X = np.asfortranarray(rng.standard_normal((D, N)))
    s, y = np.exp(rng.standard_normal(N)), rng.standard_normal(N)
    f = R.BayesianLinearRegressor(np.zeros(D), R.Diagonal(np.ones(D)))
    x = R.RowVecs(np.ascontiguousarray(X.T)) if rowvecs else R.ColVecs(X)
    perm = rng.permutation(N)
    got = {}
    real = _Recorder.kfold

    def spy(self, *a):  # (the staged buffers are freed after the call: look at them now)
        got["X"] = _buf(rec, a[7], np.float64, D * N).copy()
        got["y"] = _buf(rec, a[10], np.float64, N).copy()
        got["s"] = _buf(rec, a[13], np.float64, N).copy()
        return real(self, *a)

    monkeypatch.setattr(_Recorder, "kfold", spy)
    r = R.kfold(f(x, R.Diagonal(s)), y, F, perm=perm)
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
            R.kfold(f(x, R.Diagonal(s)), y, F, perm=bad)


@pytest.mark.parametrize("D,N,F", [(7, 40, 5), (33, 150, 16), (128, 200, 64)])
def test_closed_form_matches_brute_force_refits(D, N, F):
    """The identities of the header in NumPy float64 against the chain rule with the oracle, rel 1e-12; every fold's H~ has its
    largest eigenvalue <= 0.7 on these inputs, so G~ is well conditioned and the GPU tolerances do not hide cancellation."""
    mw, U, X, s, y = state(rng_of(0), D, N)
    mwp, T = posterior_state(mw, U, X, s, y)
    mean, var, lps, lam = closed_form(mwp, T, X, s, y, F)
    m_o, v_o, lp_o = brute_force(mw, U.T @ U, X, s, y, F)
    assert lam <= 0.7, lam
    np.testing.assert_allclose(lps, lp_o, rtol=1e-12)
    np.testing.assert_allclose(mean, m_o, rtol=1e-12, atol=1e-12 * np.max(np.abs(m_o)))
    np.testing.assert_allclose(var, v_o, rtol=1e-12)


def test_kfold_kernel_resources(tmp_path):
    """Registers and scratch of both kfold_kernel instantiations from the code object's notes: at most 256 registers, no scratch and no
    spilled register (DESIGN.md K23 states this build's figures)."""
    objdump = "/opt/rocm/lib/llvm/bin/llvm-objdump"
    readelf = "/opt/rocm/lib/llvm/bin/llvm-readelf"
    if not (os.path.exists(objdump) and os.path.exists(readelf)):
        pytest.skip("ROCm LLVM tools not installed")
    so = shutil.copy(_abi.LIB_PATH, tmp_path / "lib.so")
    subprocess.run([objdump, "--offloading", str(so)], check=True, capture_output=True, cwd=tmp_path)
    cos = [p for p in os.listdir(tmp_path) if "gfx950" in p]
    assert cos, "no gfx950 code object in the library"
    notes = "".join(subprocess.run([readelf, "--notes", str(tmp_path / c)], check=True, capture_output=True, text=True).stdout for c in sorted(cos))
    props, name = {}, None
    for line in notes.splitlines():
        m = re.match(r"\s+(?:- )?\.(name|vgpr_count|vgpr_spill_count|private_segment_fixed_size):\s+(\S+)", line)
        if m and m.group(1) == "name":
            name = m.group(2)
        elif m and name is not None:
            props.setdefault(name, {})[m.group(1)] = int(m.group(2))
    kf = {k: v for k, v in props.items() if "kfold_kernel" in k}
    assert len(kf) == 2, sorted(kf)  # two element types
    for k, v in kf.items():
        assert v["vgpr_count"] <= 256, (k, v)
        assert v["private_segment_fixed_size"] == 0, (k, v)
        assert v["vgpr_spill_count"] == 0, (k, v)
