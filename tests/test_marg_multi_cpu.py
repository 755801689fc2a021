"""CPU-side checks of the batched multi-output marginals (blr_marginals_multi_batched_*, mean_and_var_columns, mean_columns,
mean_and_var_columns_map): the symbols are declared, exported and bound, the header, the binding and the Julia shim
agree on the arity, the argument checks that need no device (they come before the handle check), the routing of the Python
functions with the handle's methods replaced, and marginals_cols_kernel's register / scratch limits from the compiled code object."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import blr_amd
from blr_amd import _abi
from blr_amd import regressor as R

SYMS = ("blr_marginals_multi_batched_f64", "blr_marginals_multi_batched_f32")
ARITY = 26


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
    assert hasattr(_abi.Handle, "marginals_multi_batched")
    block = header[header.index("S mean columns and one variance per input"):header.index("int blr_marginals_multi_batched_f64")]
    assert ":33" in block and ":40-43" in block and ":47" in block and "regressors come from matrix targets" in block
    assert "correct, not fast" in block and "bit-reproducible" in block


def test_pass_width_is_mirrored(repo_root):
    hpp = open(os.path.join(repo_root, "bayesianlinearregressors.jl_amd", "csrc", "blr_marg_multi.hpp")).read()
    m = re.search(r"constexpr int kMargColsPerPass = (\d+);", hpp)
    assert m and int(m.group(1)) == _abi.MARG_COLS_PER_PASS


def test_python_surface():
    for name in ("mean_and_var_columns", "mean_columns", "mean_and_var_columns_map"):
        assert getattr(blr_amd, name) is getattr(R, name)
        assert name in blr_amd.__all__ and name in R.__all__


def test_julia_shim_calls_both_symbols_with_the_header_arity(repo_root):
    jl = open(os.path.join(repo_root, "julia", "BLRMI355X.jl")).read()
    header = _header(repo_root)
    assert "function marginals_multi_batched!(" in jl
    assert "function mean_and_var(fxs::AbstractVector{<:FiniteGP})" in jl
    for name in SYMS:
        m = re.search(rf"ccall\(\(:{name}, LIB\), Cint,\s*\(([^)]*)\)", jl)
        assert m, name
        types = [t for t in m.group(1).split(",") if t.strip()]
        assert len(types) == _arity(header, name) == ARITY, name


def _call(name, **kw):
    """blr_marginals_multi_batched_* with a NULL handle and valid arguments except those in kw."""
    lib = _abi.load_library()
    D, N, S, B = 4, 5, 3, 2
    a = dict(memspace=_abi.MEM_HOST, layout=_abi.LAYOUT_COLVECS, B=B, D=D, N=N, S=S, X=np.zeros((D, N * B)), ldx=D, strideX=D * N,
             noise_kind=_abi.NOISE_ISOTROPIC, s=np.ones(B), strides=1, prior_kind=_abi.PRIOR_DENSE, M=np.zeros(D * S * B), ldm=D,
             strideM=D * S, Lw=np.eye(D), ldl=D, strideLw=0, mean=np.zeros(N * S * B), ldmean=N, stridemean=N * S, var=np.zeros(N * B),
             stridevar=N, info=np.zeros(B, dtype=np.int32))
    a.update(kw)
    p = _abi._ptr
    return getattr(lib, name)(None, a["memspace"], a["layout"], a["B"], a["D"], a["N"], a["S"], p(a["X"]), a["ldx"], a["strideX"],
                              a["noise_kind"], p(a["s"]), a["strides"], a["prior_kind"], p(a["M"]), a["ldm"], a["strideM"], p(a["Lw"]),
                              a["ldl"], a["strideLw"], p(a["mean"]), a["ldmean"], a["stridemean"], p(a["var"]), a["stridevar"], p(a["info"]))


@pytest.mark.parametrize("name", SYMS)
def test_argument_errors_without_a_device(name):
    # (the checks read no element of the data: the float64 buffers only provide non-NULL pointers for the f32 entry point too)
    assert _call(name, noise_kind=_abi.NOISE_DENSE) == -11            # dense noise
    assert _call(name, noise_kind=7) == -11
    assert _call(name, ldm=3) == -16                                  # ldm < D
    assert _call(name, ldmean=4) == -22                               # ldmean < N
    assert _call(name, stridemean=14) == -23                          # overlapping means for B = 2 (< ldmean * S)
    assert _call(name, stridevar=4) == -25                            # overlapping variances for B = 2 (< N)
    assert _call(name, S=-1) == -7
    assert _call(name, S=2**20 + 1) == -7
    assert _call(name, info=None) == -26                              # NULL info
    assert _call(name, X=None) == -8                                  # NULL X
    assert _call(name, M=None) == -15                                 # NULL M with S > 0 and mean != NULL
    assert _call(name, s=None) == -12                                 # NULL s with var != NULL
    assert _call(name, Lw=None) == -18                                # NULL Lw with var != NULL
    assert _call(name, memspace=7) == -2
    assert _call(name, layout=2) == -3
    assert _call(name, B=-1) == -4
    assert _call(name, D=0) == -5
    assert _call(name, D=8193) == -5
    assert _call(name, N=-1) == -6
    assert _call(name, N=2**30 + 1) == -6
    assert _call(name, ldx=3) == -9
    assert _call(name, layout=_abi.LAYOUT_ROWVECS, ldx=4) == -9
    assert _call(name, strideX=-1) == -10
    assert _call(name, strides=-1) == -13
    assert _call(name, prior_kind=3) == -14
    assert _call(name, strideM=-1) == -17
    assert _call(name, ldl=3) == -19
    assert _call(name, strideLw=-1) == -20
    # nothing to do: a no-op, whatever else is passed
    assert _call(name, B=0, info=None, X=None) == 0
    assert _call(name, N=0, info=None, X=None) == 0
    assert _call(name, S=0, var=None, info=None, X=None) == 0
    # valid arguments and a NULL handle: -1
    assert _call(name) == -1
    assert _call(name, strideX=0, strideM=0, strides=0) == -1          # shared inputs
    assert _call(name, var=None, s=None, Lw=None) == -1                # mean only needs neither the noise nor the precision
    assert _call(name, S=0, M=None, mean=None) == -1                   # var only
    assert _call(name, mean=None, M=None) == -1                        # mean == NULL with S > 0: M is not read
    assert _call(name, B=1, stridemean=0, stridevar=0) == -1           # a single regressor may have any output stride
    assert _call(name, prior_kind=_abi.PRIOR_DIAGONAL, ldl=1) == -1


class _Recorder:
    """stands in for the library handle: records the entry point and fills the status so that the unpacking goes through"""

    def __init__(self):
        self.calls = []

    def marginals_multi_batched(self, *args):
        self.calls.append(("marg_multi", args))
        args[-1][...] = 0  # info
        return 0


def _columns(D, S, rng, shared=True):
    Lw = R.Diagonal(np.ones(D))
    return [R.BayesianLinearRegressor(rng.standard_normal(D), Lw if shared else R.Diagonal(np.ones(D))) for _ in range(S)]


def test_equal_shapes_make_one_call(monkeypatch):
    rec = _Recorder()
    monkeypatch.setattr(R, "_handle", lambda: rec)
    rng = np.random.default_rng(5)
    D, N, S = 6, 5, 3
    fss = [_columns(D, S, rng) for _ in range(4)]
    xs = [R.ColVecs(np.asfortranarray(rng.standard_normal((D, N)))) for _ in range(4)]
    out = R.mean_and_var_columns_map(fss, xs, Sy=[np.exp(rng.standard_normal(N)) for _ in range(4)])
    assert [k for k, _ in rec.calls] == ["marg_multi"] and len(out) == 4
    assert all(m.shape == (N, S) and v.shape == (N,) for m, v in out)
    a = rec.calls[0][1]
    dtype, memspace, layout, B, D_, N_, S_, X, ldx, strideX, noise_kind, s, strides, prior_kind, M, ldm, strideM = a[:17]
    assert (memspace, layout, B, D_, N_, S_, ldx, strideX, noise_kind, strides, prior_kind, ldm, strideM) == (
        _abi.MEM_HOST, _abi.LAYOUT_COLVECS, 4, D, N, S, D, D * N, _abi.NOISE_DIAGONAL, N, _abi.PRIOR_DIAGONAL, D, D * S)
    assert np.array_equal(M[2].reshape((D, S), order="F")[:, 1], fss[2][1].mw) and np.array_equal(X[1].reshape((D, N), order="F"), xs[1].X)
    mean, ldmean, stridemean, var, stridevar = a[20:25]
    assert (ldmean, stridemean, stridevar) == (N, N * S, N) and mean.shape == (4, N * S) and var.shape == (4, N)
    # one data set: B = 1; mean_columns passes no variance, no noise and no precision
    rec.calls.clear()
    m, v = R.mean_and_var_columns(fss[0], xs[0], 0.5)
    a = rec.calls[0][1]
    assert [k for k, _ in rec.calls] == ["marg_multi"] and a[3] == 1 and a[6] == S and a[10] == _abi.NOISE_ISOTROPIC
    assert m.shape == (N, S) and v.shape == (N,) and (a[15], a[21]) == (D, N)
    rec.calls.clear()
    m = R.mean_columns(fss[0], xs[0])
    a = rec.calls[0][1]
    assert m.shape == (N, S) and a[11] is None and a[17] is None and a[23] is None
    # a dense noise covariance is reduced to its diagonal; a BasisFunctionRegressor maps its inputs first
    rec.calls.clear()
    R.mean_and_var_columns(fss[0], xs[0], np.diag(np.arange(1.0, N + 1)))
    a = rec.calls[0][1]
    assert a[10] == _abi.NOISE_DIAGONAL and a[11].tolist() == list(np.arange(1.0, N + 1))
    rec.calls.clear()
    phi = lambda x: R.ColVecs(np.asfortranarray(2.0 * x.X))  # noqa: E731
    R.mean_and_var_columns([R.BasisFunctionRegressor(f, phi) for f in fss[0]], xs[0], 0.5)
    assert np.array_equal(rec.calls[0][1][7], 2.0 * xs[0].X)


def test_mixed_shapes_loop_and_errors(monkeypatch):
    rec = _Recorder()
    monkeypatch.setattr(R, "_handle", lambda: rec)
    rng = np.random.default_rng(6)
    D = 6
    fss = [_columns(D, 3, rng), _columns(D, 3, rng), _columns(D, 2, rng)]
    xs = [R.ColVecs(np.asfortranarray(rng.standard_normal((D, n)))) for n in (5, 4, 5)]
    out = R.mean_and_var_columns_map(fss, xs, Sy=0.5)
    assert [k for k, _ in rec.calls] == ["marg_multi"] * 3 and [c[1][3] for c in rec.calls] == [1, 1, 1]
    assert [m.shape for m, _ in out] == [(5, 3), (4, 3), (5, 2)]
    rec.calls.clear()
    with pytest.raises(ValueError, match="the columns must share one precision object"):
        R.mean_and_var_columns(_columns(D, 3, rng, shared=False), xs[0])
    with pytest.raises(ValueError, match="the columns must share one precision object"):
        R.mean_and_var_columns_map([_columns(D, 3, rng, shared=False)], xs[:1])
    assert rec.calls == []
    assert R.mean_and_var_columns_map([], []) == []
    with pytest.raises(ValueError, match="as many"):
        R.mean_and_var_columns_map(fss, xs[:2])


def test_marginals_cols_kernel_resources(tmp_path):
    """Registers and scratch of every marginals_cols_kernel instantiation from the code object's notes: at most 256 registers, and
    the scratch per lane bounded at what this build gives -- the fp32 kernels none, fp64 ColVecs none, fp64 RowVecs 52 B (a few
    spilled address registers), under the 128 B bound of the sibling multi_cols_kernel."""
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
    marg = {k: v for k, v in props.items() if "marginals_cols_kernel" in k}
    assert len(marg) == 4, sorted(marg)  # two element types, ColVecs and RowVecs
    for k, v in marg.items():
        f64 = "marginals_cols_kernelId" in k
        assert v["vgpr_count"] <= 256, (k, v)
        assert v["private_segment_fixed_size"] <= (64 if f64 else 0), (k, v)
        assert v["vgpr_spill_count"] <= (16 if f64 else 0), (k, v)
