"""CPU-side checks of the batched multi-output posterior (blr_posterior_multi_batched_*, posterior_columns, logpdf_columns_map,
posterior_columns_map): the symbols are declared, exported and bound, the header, the binding and the Julia shim
agree on the arity, the argument checks that need no device (they come before the handle check), the routing of the Python
functions with the handle's methods replaced, and multi_cols_kernel's register / scratch limits from the compiled code object."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import blr_amd
from blr_amd import _abi
from blr_amd import regressor as R

SYMS = ("blr_posterior_multi_batched_f64", "blr_posterior_multi_batched_f32")
ARITY = 34


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
    assert hasattr(_abi.Handle, "posterior_multi_batched")
    block = header[header.index("S target columns per regressor in one call"):header.index("int blr_posterior_multi_batched_f64")]
    assert ":55-58" in block and ":60-69" in block and ":72-89" in block and "map over fxs with MATRIX targets" in block


def test_pass_width_is_mirrored(repo_root):
    hpp = open(os.path.join(repo_root, "bayesianlinearregressors.jl_amd", "csrc", "blr_multi.hpp")).read()
    m = re.search(r"constexpr int kMultiColsPerPass = (\d+);", hpp)
    assert m and int(m.group(1)) == _abi.MULTI_COLS_PER_PASS == 64


def test_python_surface():
    for name in ("posterior_columns", "logpdf_columns_map", "posterior_columns_map"):
        assert getattr(blr_amd, name) is getattr(R, name)
        assert name in blr_amd.__all__ and name in R.__all__


def test_julia_shim_calls_both_symbols_with_the_header_arity(repo_root):
    jl = open(os.path.join(repo_root, "julia", "BLRMI355X.jl")).read()
    header = _header(repo_root)
    assert "function posterior_multi_batched!(" in jl
    assert "function logpdf_map(fxs::AbstractVector{<:FiniteGP}, Ys::AbstractVector{<:AbstractMatrix" in jl
    for name in SYMS:
        m = re.search(rf"ccall\(\(:{name}, LIB\), Cint,\s*\(([^)]*)\)", jl)
        assert m, name
        types = [t for t in m.group(1).split(",") if t.strip()]
        assert len(types) == _arity(header, name) == ARITY, name


def _call(name, **kw):
    """blr_posterior_multi_batched_* with a NULL handle and valid arguments except those in kw."""
    lib = _abi.load_library()
    D, N, S, B = 4, 5, 3, 2
    a = dict(memspace=_abi.MEM_HOST, layout=_abi.LAYOUT_COLVECS, B=B, D=D, N=N, S=S, X=np.zeros((D, N * B)), ldx=D, strideX=D * N,
             Y=np.zeros(N * S * B), ldY=N, strideY=N * S, noise_kind=_abi.NOISE_ISOTROPIC, s=np.ones(B), strides=1,
             prior_kind=_abi.PRIOR_DENSE, mw=np.zeros(D), stridemw=0, Lw=np.eye(D), ldl=D, strideLw=0, mw_post=None, ldmp=D,
             stride_mwpost=D * S, T_post=None, ldt=D, strideT=D * D, Lw_post=None, ldlp=D, strideLp=D * D, logpdf=np.zeros(B * S),
             stride_lp=S, info=np.zeros(B, dtype=np.int32))
    a.update(kw)
    p = _abi._ptr
    return getattr(lib, name)(None, a["memspace"], a["layout"], a["B"], a["D"], a["N"], a["S"], p(a["X"]), a["ldx"], a["strideX"], p(a["Y"]),
                              a["ldY"], a["strideY"], a["noise_kind"], p(a["s"]), a["strides"], a["prior_kind"], p(a["mw"]), a["stridemw"],
                              p(a["Lw"]), a["ldl"], a["strideLw"], p(a["mw_post"]), a["ldmp"], a["stride_mwpost"], p(a["T_post"]), a["ldt"],
                              a["strideT"], p(a["Lw_post"]), a["ldlp"], a["strideLp"], p(a["logpdf"]), a["stride_lp"], p(a["info"]))


@pytest.mark.parametrize("name", SYMS)
def test_argument_errors_without_a_device(name):
    # (the checks read no element of the data: the float64 buffers only provide non-NULL pointers for the f32 entry point too)
    T = np.zeros((4, 4))
    M = np.zeros(4 * 3 * 2)
    mw, Lw = np.zeros(4), np.eye(4)
    assert _call(name, noise_kind=_abi.NOISE_DENSE) == -14             # dense noise
    assert _call(name, noise_kind=7) == -14
    assert _call(name, ldY=4) == -12                                   # ldY < N
    assert _call(name, mw_post=M, ldmp=3) == -24                       # ldmp < D
    assert _call(name, mw_post=M, stride_mwpost=11) == -25             # overlapping means for B = 2 (< ldmp * S)
    assert _call(name, stride_lp=2) == -33                             # overlapping evidences for B = 2 (< S)
    assert _call(name, mw=mw, mw_post=mw) == -23                       # mw_post == mw
    assert _call(name, Lw=Lw, T_post=Lw) == -26                        # T_post == Lw
    assert _call(name, info=None) == -34                               # NULL info
    assert _call(name, S=-1) == -7                                     # negative S
    assert _call(name, S=2**20 + 1) == -7
    assert _call(name, T_post=T, strideT=15) == -28
    assert _call(name, T_post=T, ldt=3) == -27
    assert _call(name, Lw_post=T, strideLp=15) == -31
    assert _call(name, Lw_post=T, ldlp=3) == -30
    assert _call(name, memspace=7) == -2
    assert _call(name, layout=2) == -3
    assert _call(name, B=-1) == -4
    assert _call(name, D=0) == -5
    assert _call(name, D=8193) == -5
    assert _call(name, N=-1) == -6
    assert _call(name, X=None) == -8
    assert _call(name, ldx=3) == -9
    assert _call(name, layout=_abi.LAYOUT_ROWVECS, ldx=4) == -9
    assert _call(name, strideX=-1) == -10
    assert _call(name, Y=None) == -11
    assert _call(name, strideY=-1) == -13
    assert _call(name, s=None) == -15
    assert _call(name, prior_kind=3) == -17
    assert _call(name, mw=None) == -18
    assert _call(name, Lw=None) == -20
    assert _call(name, ldl=3) == -21
    # nothing to do: a no-op, whatever else is passed
    assert _call(name, B=0, info=None, X=None) == 0
    assert _call(name, S=0, info=None, Y=None) == 0
    # valid arguments and a NULL handle: -1 (shared inputs and N = 0 are valid; a single regressor may have any output stride)
    assert _call(name) == -1
    assert _call(name, strideX=0, strideY=0, strides=0) == -1
    assert _call(name, N=0, X=None, Y=None, ldY=0) == -1
    assert _call(name, B=1, mw_post=M, stride_mwpost=0, stride_lp=0) == -1


class _Recorder:
    """stands in for the library handle: records the entry point and fills the status so that the unpacking goes through"""

    def __init__(self):
        self.calls = []

    def _rec(self, kind, args):
        self.calls.append((kind, args))
        args[-1][...] = 0  # info
        return 0

    def posterior_multi_batched(self, *args):
        return self._rec("multi_batched", args)

    def posterior_batched(self, *args):
        return self._rec("batched", args)

    def logpdf_multi(self, *args):
        return self._rec("logpdf_multi", args)

    def posterior(self, *args):
        self.calls.append(("single", args))
        return 0

    def posterior_dense_noise(self, *args):
        return self._rec("dense_noise", args)


def _problems(shapes, D=6, noise="diag", layout="col"):
    rng = np.random.default_rng(3)
    fxs, Ys = [], []
    for i, (N, S) in enumerate(shapes):
        f = R.BayesianLinearRegressor(rng.standard_normal(D), R.Diagonal(np.ones(D)))
        X = np.asfortranarray(rng.standard_normal((D, N)))
        x = R.ColVecs(X) if layout == "col" else R.RowVecs(np.asfortranarray(X.T))
        Sy = {"diag": np.exp(rng.standard_normal(N)), "iso": 0.5 + i, "dense": np.eye(N) * 2.0}[noise]
        fxs.append(f(x, Sy))
        Ys.append(rng.standard_normal((N, S)))
    return fxs, Ys


def test_equal_shapes_make_one_call(monkeypatch):
    rec = _Recorder()
    monkeypatch.setattr(R, "_handle", lambda: rec)
    fxs, Ys = _problems([(5, 3)] * 4)
    out = R.logpdf_columns_map(fxs, Ys)
    assert out.shape == (4, 3) and [k for k, _ in rec.calls] == ["multi_batched"]
    a = rec.calls[0][1]
    dtype, memspace, layout, B, D, N, S, X, ldx, strideX, Y, ldY, strideY, noise_kind, s, strides = a[:16]
    assert (memspace, layout, B, D, N, S, ldx, strideX, ldY, strideY, noise_kind, strides) == (
        _abi.MEM_HOST, _abi.LAYOUT_COLVECS, 4, 6, 5, 3, 6, 30, 5, 15, _abi.NOISE_DIAGONAL, 5)
    assert np.array_equal(Y[2].reshape((5, 3), order="F"), Ys[2]) and np.array_equal(X[1].reshape((6, 5), order="F"), fxs[1].x.X)
    mw_post, ldmp, stride_mwpost, T_post = a[22:26]
    assert mw_post is None and T_post is None and a[31].shape == (4, 3)
    assert a[32] == 3  # stride_lp
    # posteriors: means D x S per data set, one factor each; RowVecs and isotropic noise pack the same way
    rec.calls.clear()
    fxs, Ys = _problems([(4, 2)] * 3, noise="iso", layout="row")
    posts = R.posterior_columns_map(fxs, Ys)
    assert [k for k, _ in rec.calls] == ["multi_batched"]
    a = rec.calls[0][1]
    assert a[2] == _abi.LAYOUT_ROWVECS and a[22].shape == (3, 6 * 2) and (a[23], a[24]) == (6, 12) and a[25].shape == (3, 36)
    assert a[13] == _abi.NOISE_ISOTROPIC and a[14].reshape(-1).tolist() == [0.5, 1.5, 2.5] and a[15] == 1
    assert len(posts) == 3 and all(len(p) == 2 for p in posts)
    assert posts[1][0].Lw is posts[1][1].Lw and posts[0][0].Lw is not posts[1][0].Lw  # the columns of a data set share one factor
    # one data set: posterior_columns is the same call with B = 1
    rec.calls.clear()
    one = R.posterior_columns(fxs[0], Ys[0])
    assert [k for k, _ in rec.calls] == ["multi_batched"] and rec.calls[0][1][3] == 1 and len(one) == 2


def test_mixed_shapes_and_dense_noise_take_the_loop(monkeypatch):
    rec = _Recorder()
    monkeypatch.setattr(R, "_handle", lambda: rec)
    out = R.logpdf_columns_map(*_problems([(5, 3), (4, 3), (5, 3)]))  # N differs
    assert out.shape == (3, 3) and [k for k, _ in rec.calls] == ["batched"] * 3  # logpdf_columns' own route at D <= 128
    rec.calls.clear()
    with pytest.raises(ValueError, match="number of columns"):
        R.logpdf_columns_map(*_problems([(5, 3), (5, 2)]))  # S differs: no (B, S) array
    assert [k for k, _ in rec.calls] == ["batched"] * 2
    rec.calls.clear()
    R.logpdf_columns_map(*_problems([(5, 2), (5, 2)], noise="dense"))
    assert [k for k, _ in rec.calls] == ["dense_noise"] * 4
    rec.calls.clear()
    posts = R.posterior_columns_map(*_problems([(5, 2), (4, 2)]))
    assert [k for k, _ in rec.calls] == ["single"] * 4 and [len(p) for p in posts] == [2, 2]
    assert R.logpdf_columns_map([], []).shape == (0, 0) and R.posterior_columns_map([], []) == []
    with pytest.raises(ValueError, match="as many"):
        R.logpdf_columns_map(_problems([(5, 3)])[0], [])


def test_multi_cols_kernel_resources(tmp_path):
    """Registers and scratch of every multi_cols_kernel instantiation from the code object's notes: at most 256 registers (two
    workgroups per CU), and the scratch per lane recorded at what the build gives -- the fp32 kernels none, the fp64 kernels a few
    spilled address registers (ColVecs 92 B, RowVecs 12 B), bounded at 128 B as fused_small_kernel<double, 8, 4> is."""
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
    multi = {k: v for k, v in props.items() if "multi_cols_kernel" in k}
    assert len(multi) == 4, sorted(multi)  # two element types, ColVecs and RowVecs
    for k, v in multi.items():
        assert v["vgpr_count"] <= 256, (k, v)
        assert v["private_segment_fixed_size"] <= (128 if "multi_cols_kernelId" in k else 0), (k, v)
        assert v["vgpr_spill_count"] <= (32 if "multi_cols_kernelId" in k else 0), (k, v)
