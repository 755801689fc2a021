"""CPU-side checks of the exact leave-one-out predictives of multi-output states (blr_loo_multi_batched_*, loo_columns,
loo_columns_map, ResidentColumnsPosterior.loo): the symbols are declared, exported and bound, the header, the binding
and the Julia shim agree on the arity, the argument checks that need no device (they come before the handle check), the routing of
the Python functions with the handle replaced by a recorder, and loo_cols_kernel's register / scratch limits from the compiled code
object."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import blr_amd
from blr_amd import _abi
from blr_amd import regressor as R
from _recorder import Recorder as _Recorder

SYMS = ("blr_loo_multi_batched_f64", "blr_loo_multi_batched_f32")
ARITY = 33


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
    assert hasattr(_abi.Handle, "loo_multi_batched")
    block = header[header.index("predictives of a MULTI-OUTPUT state"):header.index("int blr_loo_multi_batched_f64")]
    assert ":55-58" in block and ":49-70" in block
    assert "correct, not fast" in block and "bit-reproducible" in block and "may synchronise" in block
    assert "counted ONCE" in block and "strideX = 0" in block and "strideY = 0" in block and "strideM = 0" in block


def test_pass_width_is_mirrored(repo_root):
    csrc = os.path.join(repo_root, "bayesianlinearregressors.jl_amd", "csrc")
    hpp = open(os.path.join(csrc, "blr_loo_multi.hpp")).read()
    assert re.search(r"constexpr int kLooColsPerPass = kMargColsPerPass;", hpp)
    m = re.search(r"constexpr int kMargColsPerPass = (\d+);", open(os.path.join(csrc, "blr_marg_multi.hpp")).read())
    assert m and int(m.group(1)) == _abi.LOO_COLS_PER_PASS == _abi.MARG_COLS_PER_PASS


def test_python_surface():
    for name in ("loo_columns", "loo_columns_map"):
        assert getattr(blr_amd, name) is getattr(R, name)
        assert name in blr_amd.__all__ and name in R.__all__
    assert callable(blr_amd.ResidentColumnsPosterior.loo)


def test_julia_shim_calls_both_symbols_with_the_header_arity(repo_root):
    jl = open(os.path.join(repo_root, "julia", "BLRMI355X.jl")).read()
    header = _header(repo_root)
    assert "function loo_multi_batched!(" in jl
    for name in SYMS:
        m = re.search(rf"ccall\(\(:{name}, LIB\), Cint,\s*\(([^)]*)\)", jl)
        assert m, name
        types = [t for t in m.group(1).split(",") if t.strip()]
        assert len(types) == _arity(header, name) == ARITY, name


def _call(name, **kw):
    """blr_loo_multi_batched_* with a NULL handle and valid arguments except those in kw."""
    lib = _abi.load_library()
    D, N, S, B = 4, 5, 3, 2
    a = dict(memspace=_abi.MEM_HOST, layout=_abi.LAYOUT_COLVECS, B=B, D=D, N=N, S=S, X=np.zeros((D, N * B)), ldx=D, strideX=D * N,
             Y=np.zeros(N * S * B), ldY=N, strideY=N * S, noise_kind=_abi.NOISE_ISOTROPIC, s=np.ones(B), strides=1, M=np.zeros(D * S * B),
             ldm=D, strideM=D * S, T=np.eye(D), ldt=D, strideT=0, loo_mean=np.zeros(N * S * B), ld_lm=N, stride_lm=N * S,
             loo_var=np.zeros(N * B), stride_lv=N, loo_logpdf=np.zeros(N * S * B), ld_ll=N, stride_ll=N * S, loo_total=np.zeros(S * B),
             stride_lt=S, info=np.zeros(B, dtype=np.int32))
    a.update(kw)
    p = _abi._ptr
    return getattr(lib, name)(None, a["memspace"], a["layout"], a["B"], a["D"], a["N"], a["S"], p(a["X"]), a["ldx"], a["strideX"],
                              p(a["Y"]), a["ldY"], a["strideY"], a["noise_kind"], p(a["s"]), a["strides"], p(a["M"]), a["ldm"],
                              a["strideM"], p(a["T"]), a["ldt"], a["strideT"], p(a["loo_mean"]), a["ld_lm"], a["stride_lm"],
                              p(a["loo_var"]), a["stride_lv"], p(a["loo_logpdf"]), a["ld_ll"], a["stride_ll"], p(a["loo_total"]),
                              a["stride_lt"], p(a["info"]))


@pytest.mark.parametrize("name", SYMS)
def test_argument_errors_without_a_device(name):
    # (the checks read no element of the data: the float64 buffers only provide non-NULL pointers for the f32 entry point too)
    assert _call(name, memspace=7) == -2
    assert _call(name, layout=2) == -3
    assert _call(name, B=-1) == -4
    assert _call(name, B=2**30 + 1) == -4
    assert _call(name, D=0) == -5
    assert _call(name, D=8193) == -5
    assert _call(name, N=-1) == -6
    assert _call(name, N=2**30 + 1) == -6
    assert _call(name, S=-1) == -7
    assert _call(name, S=2**20 + 1) == -7
    assert _call(name, X=None) == -8
    assert _call(name, ldx=3) == -9
    assert _call(name, layout=_abi.LAYOUT_ROWVECS, ldx=4) == -9
    assert _call(name, strideX=-1) == -10
    assert _call(name, Y=None) == -11
    assert _call(name, ldY=4) == -12                                  # ldY < N
    assert _call(name, strideY=-1) == -13
    assert _call(name, noise_kind=_abi.NOISE_DENSE) == -14            # dense noise
    assert _call(name, noise_kind=7) == -14
    assert _call(name, s=None) == -15
    assert _call(name, strides=-1) == -16
    assert _call(name, M=None) == -17
    assert _call(name, ldm=3) == -18                                  # ldm < D
    assert _call(name, strideM=-1) == -19
    assert _call(name, T=None) == -20
    assert _call(name, ldt=3) == -21                                  # ldt < D
    assert _call(name, strideT=-1) == -22
    assert _call(name, ld_lm=4) == -24                                # ld_lm < N
    assert _call(name, stride_lm=14) == -25                           # overlapping outputs for B = 2
    assert _call(name, stride_lv=4) == -27
    assert _call(name, ld_ll=4) == -29                                # ld_ll < N
    assert _call(name, stride_ll=14) == -30
    assert _call(name, stride_lt=2) == -32
    assert _call(name, info=None) == -33
    # the ranges come first, in the order of the arguments
    assert _call(name, memspace=7, layout=2, noise_kind=_abi.NOISE_DENSE) == -2
    assert _call(name, S=-1, ldY=0) == -7
    # nothing to do: a no-op, whatever else is passed
    assert _call(name, B=0, info=None, X=None) == 0
    assert _call(name, S=0, info=None, X=None, noise_kind=_abi.NOISE_DENSE) == 0
    # valid arguments and a NULL handle: -1
    assert _call(name) == -1
    assert _call(name, strideX=0, strideY=0, strideM=0, strides=0, strideT=0) == -1     # shared inputs
    assert _call(name, loo_mean=None, loo_var=None, loo_logpdf=None) == -1              # the totals alone (through workspace)
    assert _call(name, loo_mean=None, ld_lm=0, stride_lm=0, loo_logpdf=None, ld_ll=0, stride_ll=0, loo_total=None, stride_lt=0) == -1
    assert _call(name, B=1, stride_lm=0, stride_lv=0, stride_ll=0, stride_lt=0) == -1   # a single regressor: any output stride
    assert _call(name, N=0, X=None, Y=None, s=None, ldY=0, ld_lm=0, ld_ll=0) == -1      # N = 0 still writes totals and info
    assert _call(name, noise_kind=_abi.NOISE_DIAGONAL, s=np.ones(10), strides=5) == -1
    assert _call(name, layout=_abi.LAYOUT_ROWVECS, ldx=5) == -1


def _patch(monkeypatch, rec):
    monkeypatch.setattr(R, "_handle", lambda: rec)


def _problem(rng, D, N, S):
    f = R.BayesianLinearRegressor(rng.standard_normal(D), R.Diagonal(np.exp(0.1 * rng.standard_normal(D))))
    X = np.asfortranarray(rng.standard_normal((D, N)))
    return f(R.ColVecs(X), R.Diagonal(np.exp(rng.standard_normal(N)))), rng.standard_normal((N, S))


def _device_buffer_works_with(rec):
    """The recorder must provide what _DeviceBuffer uses; the routing tests below depend on that."""
    b = R._DeviceBuffer.of(rec, np.arange(3.0))
    out = np.empty(3)
    rec.memcpy_d2h(out, b.ptr)
    b.free()
    return np.array_equal(out, np.arange(3.0))


def test_equal_shapes_make_one_fit_and_one_loo_call(monkeypatch):
    rec = _Recorder()
    _patch(monkeypatch, rec)
    assert _device_buffer_works_with(rec)
    rng = np.random.default_rng(5)
    D, N, S, nb = 6, 5, 3, 4
    fxs, Ys = zip(*[_problem(rng, D, N, S) for _ in range(nb)])
    out = R.loo_columns_map(fxs, Ys)
    assert [k for k, _ in rec.calls] == ["fit", "loo_multi"] and len(out) == nb
    assert all(r.mean.shape == (N, S) and r.var.shape == (N,) and r.logpdf.shape == (N, S) and r.total.shape == (S,) for r in out)
    assert out[0].logpdf.dtype == np.float64
    fit, a = rec.calls[0][1], rec.calls[1][1]
    (dtype, memspace, layout, B, D_, N_, S_, dX, ldx, strideX, dY, ldY, strideY, noise_kind, ds, strides, dM, ldm, strideM, dT, ldt, strideT,
     d_lm, ld_lm, stride_lm, d_lv, stride_lv, d_ll, ld_ll, stride_ll, d_tot, stride_lt, d_info) = a
    assert (dtype, memspace, layout, B, D_, N_, S_) == (np.float64, _abi.MEM_DEVICE, _abi.LAYOUT_COLVECS, nb, D, N, S)
    assert (ldx, strideX, ldY, strideY, noise_kind, strides) == (D, D * N, N, N * S, _abi.NOISE_DIAGONAL, N)
    assert (ldm, strideM, ldt, strideT) == (D, D * S, D, D * D)
    assert (ld_lm, stride_lm, stride_lv, ld_ll, stride_ll, stride_lt) == (N, N * S, N, N, N * S, S)
    # the LOO call reads the device buffers the fit wrote (mw_post, T_post) and the inputs the fit read: nothing is staged twice
    assert (dX, dY, ds) == (fit[7], fit[10], fit[14]) and (dM, dT) == (fit[22], fit[25])
    assert fit[1] == _abi.MEM_DEVICE and fit[3] == nb and fit[6] == S
    # one data set: B = 1
    rec.calls.clear()
    r = R.loo_columns(fxs[0], Ys[0])
    assert [k for k, _ in rec.calls] == ["fit", "loo_multi"] and rec.calls[1][1][3] == 1 and r.mean.shape == (N, S)


def test_mixed_shapes_loop_and_errors(monkeypatch):
    rec = _Recorder()
    _patch(monkeypatch, rec)
    rng = np.random.default_rng(6)
    D = 6
    fxs, Ys = zip(*[_problem(rng, D, n, s) for n, s in ((5, 3), (4, 3), (5, 2))])
    out = R.loo_columns_map(fxs, Ys)
    assert [k for k, _ in rec.calls] == ["fit", "loo_multi"] * 3 and [c[1][3] for c in rec.calls] == [1] * 6
    assert [r.mean.shape for r in out] == [(5, 3), (4, 3), (5, 2)]
    rec.calls.clear()
    assert R.loo_columns_map([], []) == []
    with pytest.raises(ValueError, match="as many"):
        R.loo_columns_map(fxs, Ys[:2])
    with pytest.raises(ValueError, match="length"):
        R.loo_columns(fxs[0], Ys[1])
    with pytest.raises(NotImplementedError, match="block leave-out"):
        f = R.BayesianLinearRegressor(np.zeros(D), R.Diagonal(np.ones(D)))
        R.loo_columns(f(R.ColVecs(np.asfortranarray(rng.standard_normal((D, 4)))), np.eye(4) + 0.1), np.zeros((4, 2)))
    assert rec.calls == []


def test_resident_loo_passes_the_resident_pointers(monkeypatch):
    rec = _Recorder()
    monkeypatch.setattr(_abi, "default_handle", lambda: rec)
    rng = np.random.default_rng(7)
    D, N, S = 6, 5, 3
    Lw = R.PDMat(np.triu(rng.standard_normal((D, D))) + 3.0 * np.eye(D))
    st = R.ResidentColumnsPosterior([R.BayesianLinearRegressor(rng.standard_normal(D), Lw) for _ in range(S)])
    X = np.asfortranarray(rng.standard_normal((D, N)))
    r = st.loo(R.ColVecs(X), 0.5, rng.standard_normal((N, S)))
    assert [k for k, _ in rec.calls] == ["loo_multi"]
    a = rec.calls[0][1]
    assert a[1] == _abi.MEM_DEVICE and a[3:7] == (1, D, N, S) and a[13] == _abi.NOISE_ISOTROPIC
    assert a[16] == st._M.ptr and a[19] == st._T.ptr and (a[17], a[20]) == (D, D)
    assert (a[9], a[12], a[15], a[18], a[21]) == (0, 0, 0, 0, 0)  # one regressor: no strides
    assert r.mean.shape == (N, S) and r.var.shape == (N,) and r.logpdf.shape == (N, S) and r.total.shape == (S,)
    with pytest.raises(ValueError, match="x S"):
        st.loo(R.ColVecs(X), 0.5, np.zeros((N, S + 1)))
    with pytest.raises(NotImplementedError):
        st.loo(R.ColVecs(X), np.eye(N) + 0.1, np.zeros((N, S)))


def test_loo_cols_kernel_resources(tmp_path):
    """Registers and scratch of every loo_cols_kernel instantiation from the code object's notes: at most 256 registers, and the
    scratch per lane bounded at what this build gives -- the fp32 kernels and fp64 ColVecs none, fp64 RowVecs 236 B
    (58 spilled registers: the addresses of the strided loads beside the double-precision epilogue)."""
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
    loo = {k: v for k, v in props.items() if "loo_cols_kernel" in k}
    assert len(loo) == 4, sorted(loo)  # two element types, ColVecs and RowVecs
    for k, v in loo.items():
        f64_row = "loo_cols_kernelIdLi1E" in k
        assert v["vgpr_count"] <= 256, (k, v)
        assert v["private_segment_fixed_size"] <= (256 if f64_row else 0), (k, v)
        assert v["vgpr_spill_count"] <= (64 if f64_row else 0), (k, v)
    assert any("loo_cols_total_kernel" in k for k in props) and sum("loo_cols_finish_kernel" in k for k in props) == 2
