"""CPU-side checks of the unequal-count update (blr_posterior_ragged_*, posterior_ragged, logpdf_ragged, the routing of
posterior_map / logpdf_map): the symbols are declared, exported and bound, the header, the binding and the Julia shim agree on
the arity, the argument checks that need no device (they come before the handle check), the routing of _fused_many with the
handle's methods replaced, and the new kernels' register / scratch limits from the compiled code object."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import blr_amd
from blr_amd import _abi
from blr_amd import regressor as R

SYMS = ("blr_posterior_ragged_f64", "blr_posterior_ragged_f32")
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
    assert hasattr(_abi.Handle, "posterior_ragged")
    block = header[header.index("UNEQUAL observation counts"):header.index("int blr_posterior_ragged_f64")]
    assert "bayesian_linear_regression.jl:55-58" in block and "map over fxs of different lengths" in block


def test_python_surface():
    for name in ("posterior_ragged", "logpdf_ragged"):
        assert getattr(blr_amd, name) is getattr(R, name)
        assert name in blr_amd.__all__ and name in R.__all__


def test_julia_shim_calls_both_symbols_with_the_header_arity(repo_root):
    jl = open(os.path.join(repo_root, "julia", "BLRMI355X.jl")).read()
    header = _header(repo_root)
    assert "function posterior_ragged!(" in jl
    for name in SYMS:
        m = re.search(rf"ccall\(\(:{name}, LIB\), Cint,\s*\(([^)]*)\)", jl)
        assert m, name
        types = [t for t in m.group(1).split(",") if t.strip()]
        assert len(types) == _arity(header, name) == ARITY, name


def _call(name, **kw):
    """blr_posterior_ragged_* with a NULL handle and valid arguments except those in kw."""
    lib = _abi.load_library()
    D = 4
    a = dict(memspace=_abi.MEM_HOST, layout=_abi.LAYOUT_COLVECS, B=2, D=D, offsets=np.array([0, 3, 5], dtype=np.int64), X=np.zeros((D, 5)),
             ldx=D, y=np.zeros(5), noise_kind=_abi.NOISE_ISOTROPIC, s=np.ones(2), strides=1, prior_kind=_abi.PRIOR_DENSE, mw=np.zeros(D),
             stridemw=0, Lw=np.eye(D), ldl=D, strideLw=0, mw_post=None, stride_mwpost=D, T_post=None, ldt=D, strideT=D * D, Lw_post=None,
             ldlp=D, strideLp=D * D, logpdf=np.zeros(2), info=np.zeros(2, dtype=np.int32))
    a.update(kw)
    p = _abi._ptr
    return getattr(lib, name)(None, a["memspace"], a["layout"], a["B"], a["D"], p(a["offsets"]), p(a["X"]), a["ldx"], p(a["y"]),
                              a["noise_kind"], p(a["s"]), a["strides"], a["prior_kind"], p(a["mw"]), a["stridemw"], p(a["Lw"]), a["ldl"],
                              a["strideLw"], p(a["mw_post"]), a["stride_mwpost"], p(a["T_post"]), a["ldt"], a["strideT"], p(a["Lw_post"]),
                              a["ldlp"], a["strideLp"], p(a["logpdf"]), p(a["info"]))


@pytest.mark.parametrize("name", SYMS)
def test_argument_errors_without_a_device(name):
    # (the checks read no element of the data: the float64 buffers only provide non-NULL pointers for the f32 entry point too)
    i64 = lambda *v: np.array(v, dtype=np.int64)  # noqa: E731
    T = np.zeros((4, 4))
    assert _call(name, offsets=i64(0, 3, 2)) == -6                 # a decreasing entry
    assert _call(name, offsets=i64(-1, 3, 5)) == -6                # offsets[0] < 0
    assert _call(name, offsets=None) == -6                         # NULL with B > 0
    assert _call(name, offsets=i64(0, 3, 3 + 2**30 + 1)) == -6     # a regressor beyond the bound on N
    assert _call(name, ldx=3) == -8                                # ColVecs: ldx < D
    assert _call(name, layout=_abi.LAYOUT_ROWVECS, ldx=4) == -8    # RowVecs: ldx < offsets[B]
    assert _call(name, layout=_abi.LAYOUT_ROWVECS, ldx=5) == -1
    assert _call(name, noise_kind=_abi.NOISE_DENSE) == -10
    assert _call(name, layout=2) == -3
    assert _call(name, noise_kind=7) == -10
    assert _call(name, prior_kind=3) == -13
    assert _call(name, T_post=T, strideT=15) == -23                # overlapping outputs for B = 2
    assert _call(name, mw_post=np.zeros(8), stride_mwpost=3) == -20
    assert _call(name, Lw_post=T, strideLp=15) == -26
    assert _call(name, T_post=T, ldt=3) == -22
    assert _call(name, D=0) == -5
    assert _call(name, D=8193) == -5
    assert _call(name, B=-1) == -4
    assert _call(name, memspace=7) == -2
    assert _call(name, X=None) == -7
    assert _call(name, y=None) == -9
    assert _call(name, ldl=3) == -17
    assert _call(name, info=None) == -28
    # no regressors: a no-op, whatever else is passed
    assert _call(name, B=0) == 0
    assert _call(name, B=0, offsets=None, X=None, y=None, info=None) == 0
    # valid arguments and a NULL handle: -1 (empty regressors and offsets[0] > 0 are valid)
    assert _call(name) == -1
    assert _call(name, offsets=i64(2, 2, 5)) == -1


class _Recorder:
    """stands in for the library handle: records the entry point and fills the status so that the unpacking goes through"""

    def __init__(self):
        self.calls = []

    def _rec(self, kind, args):
        self.calls.append((kind, args))
        args[-1][...] = 0  # info
        return 0

    def posterior_ragged(self, *args):
        return self._rec("ragged", args)

    def posterior_batched(self, *args):
        return self._rec("batched", args)

    def posterior(self, *args):
        self.calls.append(("single", args))
        return 0


def _problems(Ns, layouts=None, D=6, noise="diag"):
    rng = np.random.default_rng(3)
    fxs, ys = [], []
    for i, N in enumerate(Ns):
        f = R.BayesianLinearRegressor(rng.standard_normal(D), R.Diagonal(np.ones(D)))
        X = np.asfortranarray(rng.standard_normal((D, N)))
        x = R.ColVecs(X) if not layouts or layouts[i] == "col" else R.RowVecs(np.asfortranarray(X.T))
        fxs.append(f(x, np.exp(rng.standard_normal(N)) if noise == "diag" else 0.5 + i))
        ys.append(rng.standard_normal(N))
    return fxs, ys


def test_problems_differing_only_in_n_make_one_ragged_call(monkeypatch):
    rec = _Recorder()
    monkeypatch.setattr(R, "_handle", lambda: rec)
    fxs, ys = _problems([3, 0, 7, 5])
    out = R.logpdf_map(fxs, ys)
    assert len(out) == 4 and [k for k, _ in rec.calls] == ["ragged"]
    a = rec.calls[0][1]
    dtype, memspace, layout, B, D, offsets, X, ldx, y, noise_kind, s, strides = a[:12]
    assert (memspace, layout, B, D, ldx, noise_kind) == (_abi.MEM_HOST, _abi.LAYOUT_COLVECS, 4, 6, 6, _abi.NOISE_DIAGONAL)
    assert offsets.tolist() == [0, 3, 3, 10, 15]
    assert X.shape == (6 * 15,) and y.shape == (15,) and s.shape == (15,)
    assert np.array_equal(X.reshape((6, 15), order="F")[:, 3:10], fxs[2].x.X) and np.array_equal(y[10:], ys[3])
    # RowVecs problems are stacked by rows into one offsets[B] x D column-major matrix; isotropic noise: one variance per problem
    rec.calls.clear()
    fxs, ys = _problems([2, 4, 1], layouts=["row"] * 3, noise="iso")
    R.posterior_map(fxs, ys)
    assert [k for k, _ in rec.calls] == ["ragged"]
    a = rec.calls[0][1]
    assert a[2] == _abi.LAYOUT_ROWVECS and a[5].tolist() == [0, 2, 6, 7] and a[7] == 7 and a[6].shape == (7, 6) and a[6].flags.f_contiguous
    assert np.array_equal(a[6][2:6, :], fxs[1].x.X) and a[9] == _abi.NOISE_ISOTROPIC and a[10].tolist() == [0.5, 1.5, 2.5] and a[11] == 1


def test_equal_shapes_still_take_the_batched_call_and_mixed_layouts_go_one_by_one(monkeypatch):
    rec = _Recorder()
    monkeypatch.setattr(R, "_handle", lambda: rec)
    R.logpdf_map(*_problems([5, 5, 5]))
    assert [k for k, _ in rec.calls] == ["batched"]
    rec.calls.clear()
    R.logpdf_map(*_problems([5, 4, 5], layouts=["col", "row", "col"]))
    assert [k for k, _ in rec.calls] == ["single"] * 3


def test_packed_functions_check_their_arguments():
    f = R.BayesianLinearRegressor(np.zeros(3), R.Diagonal(np.ones(3)))
    X = np.zeros((3, 5), order="F")
    with pytest.raises(ValueError, match="offsets"):
        R.logpdf_ragged(f, R.ColVecs(X), [0, 2, 4], 1.0, np.zeros(5))
    with pytest.raises(ValueError, match="dense"):
        R.logpdf_ragged(f, R.ColVecs(X), [0, 2, 5], np.eye(5), np.zeros(5))
    with pytest.raises(ValueError):
        R.posterior_ragged([f], R.ColVecs(X), [0, 2, 5], 1.0, np.zeros(5))
    assert R.posterior_ragged(f, R.ColVecs(X[:, :0]), [0], 1.0, np.zeros(0)) == []


def test_ragged_kernels_keep_the_fused_kernels_occupancy(tmp_path):
    """Registers and scratch of every fused_ragged_kernel instantiation from the code object: at most 256 registers (the phase
    functions are compiled once for all their callers in the translation unit -- the kernel carries fused_small_kernel's launch
    bounds), and for <double, 8, 4> no more scratch per lane than tests/test_abi_cpu.py allows fused_small_kernel<double, 8, 4>."""
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
    ragged = {k: v for k, v in props.items() if "fused_ragged_kernel" in k}
    assert len(ragged) == 48, sorted(ragged)  # NB = 1 .. 8, two element types, loader MODE 0, 1, 4
    assert not any("fused_small_kernel" in k for k in ragged)
    for k, v in ragged.items():
        assert v["vgpr_count"] <= 256, (k, v)
    d84 = [v for k, v in ragged.items() if "fused_ragged_kernelIdLi8ELi4" in k]
    assert len(d84) == 1 and d84[0]["private_segment_fixed_size"] <= 128 and d84[0]["vgpr_spill_count"] <= 4, d84
