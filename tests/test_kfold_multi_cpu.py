"""CPU-side checks of the K-fold predictives of multi-output states (blr_kfold_multi_batched_*, kfold_columns, kfold_columns_map,
ResidentColumnsPosterior.kfold): the symbols are declared, exported and bound with one arity in the header, the binding
and the Julia shim, every argument error comes back with its position from a NULL handle, the Python functions refuse what the entry
point does not take before they look for a device, the per-column closed form of tests/_kfold_multi_ref.py (the yardstick of
tests/test_kfold_multi_gpu.py) against brute-force refits with the oracle, and the register / scratch figures of the two new kernels
from the compiled code object."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import blr_amd
from blr_amd import _abi
from blr_amd import regressor as R

from _kfold_multi_ref import brute_force_columns, closed_form_columns, columns_state

SYMS = ("blr_kfold_multi_batched_f64", "blr_kfold_multi_batched_f32")
ARITY = 34


def _header(repo_root):
    return open(os.path.join(repo_root, "include", "blr_mi355x.h")).read()


def _params(text, name):
    m = re.search(rf"\bint\s+{name}\s*\(([^;]*?)\)\s*;", text, flags=re.S)
    assert m, name
    return [p.strip() for p in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).replace("\n", " ").split(",") if p.strip()]


def test_symbols_declared_exported_and_bound(repo_root):
    header = _header(repo_root)
    lib = _abi.load_library()
    for name in SYMS:
        assert hasattr(lib, name), name
        assert name in _abi.EXPORTED_SYMBOLS
        params = _params(header, name)
        argtypes = _abi._SIGS[name][0]
        assert len(params) == len(argtypes) == ARITY
        # header prototype <-> binding, position by position: pointer / 64-bit integer / int
        for pos, (p, t) in enumerate(zip(params, argtypes)):
            kind = "ptr" if "*" in p else ("i64" if p.startswith("int64_t") else "int")
            got = "ptr" if t is _abi._vp else ("i64" if t is _abi._i64 else "int")
            assert kind == got, (name, pos + 1, p)
    assert _abi._SIGS[SYMS[0]] == _abi._SIGS[SYMS[1]]
    names = [p.split()[-1].lstrip("*") for p in _params(header, SYMS[0])]
    assert names == ["h", "memspace", "layout", "B", "D", "N", "S", "F", "X", "ldx", "strideX", "Y", "ldY", "strideY", "noise_kind", "s",
                     "strides", "M", "ldm", "strideM", "T", "ldt", "strideT", "kf_mean", "ld_km", "stride_km", "kf_var", "stride_kv",
                     "kf_logpdf", "ld_kl", "stride_kl", "kf_total", "stride_kt", "info"]
    assert hasattr(_abi.Handle, "kfold_multi_batched")
    block = header[header.index("predictives of a MULTI-OUTPUT state: S target columns, one factor per fold"):header.index("int blr_kfold_multi_batched_f64")]
    for word in ("1 <= F <= 64", "F > N is allowed", "D > 128 is an argument error (5)", "2^28", "kfold_degenerate", "ONCE (not S times)",
                 "bit-reproducible", "No float atomics", "NOT promised", "65535", "256 MiB", "MAX_CHUNK", "last_chunks", "stride of 0 shares",
                 "B = 0 or S = 0", "only enqueues"):
        assert word in block, word


def test_python_surface():
    for name in ("kfold_columns", "kfold_columns_map"):
        assert getattr(blr_amd, name) is getattr(R, name)
        assert name in blr_amd.__all__ and name in R.__all__
    assert callable(blr_amd.ResidentColumnsPosterior.kfold)


def test_julia_shim_calls_both_symbols_with_the_header_arity(repo_root):
    jl = open(os.path.join(repo_root, "julia", "BLRMI355X.jl")).read()
    assert "function kfold_multi_batched!(" in jl
    for name in SYMS:
        m = re.search(rf"ccall\(\(:{name}, LIB\), Cint,\s*\(([^)]*)\)", jl)
        assert m, name
        assert len([t for t in m.group(1).split(",") if t.strip()]) == ARITY, name


def _call(name, **kw):
    """blr_kfold_multi_batched_* with a NULL handle and valid arguments except those in kw."""
    lib = _abi.load_library()
    D, N, B, S, F = 4, 5, 2, 3, 2
    a = dict(memspace=_abi.MEM_HOST, layout=_abi.LAYOUT_COLVECS, B=B, D=D, N=N, S=S, F=F, X=np.zeros((D, N * B)), ldx=D, strideX=D * N,
             Y=np.zeros(N * S * B), ldY=N, strideY=N * S, noise_kind=_abi.NOISE_DIAGONAL, s=np.ones(N * B), strides=N, M=np.zeros(D * S * B),
             ldm=D, strideM=D * S, T=np.eye(D), ldt=D, strideT=0, km=np.zeros(N * S * B), ld_km=N, stride_km=N * S, kv=np.zeros(N * B),
             stride_kv=N, kl=np.zeros(3 * S * B), ld_kl=3, stride_kl=3 * S, tot=np.zeros(S * B), stride_kt=S, info=np.zeros(B, dtype=np.int32))
    a.update(kw)
    p = _abi._ptr
    return getattr(lib, name)(None, a["memspace"], a["layout"], a["B"], a["D"], a["N"], a["S"], a["F"], p(a["X"]), a["ldx"], a["strideX"],
                              p(a["Y"]), a["ldY"], a["strideY"], a["noise_kind"], p(a["s"]), a["strides"], p(a["M"]), a["ldm"], a["strideM"],
                              p(a["T"]), a["ldt"], a["strideT"], p(a["km"]), a["ld_km"], a["stride_km"], p(a["kv"]), a["stride_kv"], p(a["kl"]),
                              a["ld_kl"], a["stride_kl"], p(a["tot"]), a["stride_kt"], p(a["info"]))


@pytest.mark.parametrize("name", SYMS)
def test_argument_errors_without_a_device(name):
    # (the checks read no element of the data: the float64 buffers only provide non-NULL pointers for the f32 entry point too)
    assert _call(name, memspace=7) == -2
    assert _call(name, layout=2) == -3
    assert _call(name, B=-1) == -4
    assert _call(name, B=(1 << 30) + 1) == -4
    assert _call(name, D=0) == -5
    assert _call(name, D=129, ldx=129, ldm=129, ldt=129) == -5       # no slow route
    assert _call(name, N=-1) == -6
    assert _call(name, N=(1 << 30) + 1) == -6
    assert _call(name, S=-1) == -7
    assert _call(name, S=(1 << 20) + 1) == -7
    assert _call(name, N=1 << 20, S=257, B=1) == -7                   # the means workspace of one regressor: S 64 ceil(N / 64) > 2^28
    assert _call(name, N=(1 << 20) + 1, S=256, B=1) == -7
    assert _call(name, F=0) == -8
    assert _call(name, F=65) == -8
    assert _call(name, X=None) == -9
    assert _call(name, ldx=3) == -10
    assert _call(name, layout=_abi.LAYOUT_ROWVECS, ldx=4) == -10
    assert _call(name, strideX=-1) == -11
    assert _call(name, Y=None) == -12
    assert _call(name, ldY=4) == -13
    assert _call(name, strideY=-1) == -14
    assert _call(name, noise_kind=_abi.NOISE_DENSE) == -15            # dense noise couples the folds
    assert _call(name, noise_kind=7) == -15
    assert _call(name, s=None) == -16
    assert _call(name, strides=-1) == -17
    assert _call(name, M=None) == -18
    assert _call(name, ldm=3) == -19
    assert _call(name, strideM=-1) == -20
    assert _call(name, T=None) == -21
    assert _call(name, ldt=3) == -22
    assert _call(name, strideT=-1) == -23
    assert _call(name, ld_km=4) == -25
    assert _call(name, stride_km=14) == -26                           # overlapping outputs for B = 2
    assert _call(name, stride_kv=4) == -28
    assert _call(name, ld_kl=2) == -30                                # nfolds = ceil(5 / 2) = 3
    assert _call(name, stride_kl=8) == -31
    assert _call(name, stride_kt=2) == -33
    assert _call(name, info=None) == -34
    # the ranges come first, in the order of the arguments
    assert _call(name, memspace=7, layout=2, F=0) == -2
    assert _call(name, S=-1, F=0) == -7
    assert _call(name, F=65, ldx=0) == -8
    # no-ops need neither a handle nor the pointers
    assert _call(name, B=0, X=None, info=None) == 0
    assert _call(name, S=0, X=None, info=None) == 0
    # valid arguments and a NULL handle: -1
    assert _call(name) == -1
    assert _call(name, strideX=0, strideY=0, strides=0, strideM=0, strideT=0) == -1    # shared inputs
    assert _call(name, km=None, kv=None, kl=None, tot=None, ld_km=0, stride_km=0, stride_kv=0, ld_kl=0, stride_kl=0, stride_kt=0) == -1
    assert _call(name, B=1, stride_km=0, stride_kv=0, stride_kl=0, stride_kt=0) == -1   # a single regressor: any output stride
    assert _call(name, noise_kind=_abi.NOISE_ISOTROPIC, strides=1) == -1
    assert _call(name, F=64, ld_kl=1, stride_kl=3) == -1                                # F > N: one fold
    assert _call(name, layout=_abi.LAYOUT_ROWVECS, ldx=5) == -1
    assert _call(name, N=0, X=None, Y=None, s=None, ldY=0, ld_km=0, ld_kl=0) == -1
    assert _call(name, D=128, ldx=128, ldm=128, ldt=128, X=np.zeros(1), M=np.zeros(1), T=np.zeros(1)) == -1
    assert _call(name, N=1 << 20, S=256, B=1, X=np.zeros(1), Y=np.zeros(1), ldY=1 << 20, ld_km=1 << 20, ld_kl=1 << 19) == -1


def _fx(rng, D, N, Sy=None):
    f = R.BayesianLinearRegressor(np.zeros(D), R.Diagonal(np.ones(D)))
    return f(R.ColVecs(np.asfortranarray(rng.standard_normal((D, N)))), R.Diagonal(np.ones(N)) if Sy is None else Sy)


def test_python_refuses_what_the_entry_point_does_not_take(monkeypatch):
    def no_device():
        raise AssertionError("looked for a device")

    monkeypatch.setattr(R, "_handle", no_device)
    monkeypatch.setattr(_abi, "default_handle", no_device)
    rng = np.random.default_rng(3)
    N, S = 6, 2
    Y = rng.standard_normal((N, S))
    with pytest.raises(NotImplementedError, match="kfold_columns.*block leave-out"):
        R.kfold_columns(_fx(rng, 4, N, np.eye(N)), Y, 2)
    with pytest.raises(ValueError, match=r"D = 129 is beyond the limit of blr_kfold_multi_batched_\* \(D <= 128\)"):
        R.kfold_columns(_fx(rng, 129, N), Y, 2)
    with pytest.raises(ValueError, match=r"D = 129 is beyond"):
        R.kfold_columns_map([_fx(rng, 129, N)], [Y], 2)
    for bad in (0, 65, 2.5):
        with pytest.raises(ValueError, match=r"fold_size must be an integer in 1\.\.64"):
            R.kfold_columns(_fx(rng, 4, N), Y, bad)
        with pytest.raises(ValueError, match=r"fold_size must be an integer in 1\.\.64"):
            R.kfold_columns_map([_fx(rng, 4, N)], [Y], bad)
    with pytest.raises(ValueError, match="N x S matrix"):
        R.kfold_columns(_fx(rng, 4, N), Y[:, 0], 2)
    for perm in (np.arange(N - 1), np.zeros(N, dtype=int)):
        with pytest.raises(ValueError, match="permutation"):
            R.kfold_columns(_fx(rng, 4, N), Y, 2, perm=perm)
    with pytest.raises(ValueError):
        R.kfold_columns_map([_fx(rng, 4, N)], [Y, Y], 2)
    assert R.kfold_columns_map([], [], 2) == []
    # nothing to do: the empty record without a call
    r = R.kfold_columns(_fx(rng, 4, N), np.zeros((N, 0)), 4)
    assert isinstance(r, R.KFold) and r.mean.shape == (N, 0) and r.var.shape == (N,) and r.logpdf.shape == (2, 0) and r.total.shape == (0,)


@pytest.mark.parametrize("D,N,F,S", [(7, 13, 5, 3), (7, 40, 1, 2), (33, 70, 16, 4)])
def test_closed_form_per_column_matches_brute_force_refits(D, N, F, S):
    """The identities of the header per column in NumPy float64 against the chain rule with the oracle, rel 1e-12 (as
    tests/test_kfold_cpu.py); one variance serves every column."""
    mw, U, X, s, Y, M, T = columns_state(0, D, N, S)
    mean, var, lps, lam = closed_form_columns(M, T, X, s, Y, F)
    m_o, v_o, lp_o = brute_force_columns(mw, U.T @ U, X, s, Y, F)
    assert lam <= 0.7, lam
    assert mean.shape == (N, S) and var.shape == (N,) and lps.shape == (-(-N // F), S)
    np.testing.assert_allclose(lps, lp_o, rtol=1e-12)
    np.testing.assert_allclose(mean, m_o, rtol=1e-12, atol=1e-12 * np.max(np.abs(m_o)))
    for c in range(S):
        np.testing.assert_allclose(var, v_o[:, c], rtol=1e-12)


def _kernel_props(tmp_path):
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
    return props


def test_kfold_multi_kernel_resources(tmp_path):
    """kfold_cols_kernel<double> and <float>: at most 256 registers (two workgroups per CU), 0 B of scratch, no spilled vector register.
    kfold_whiten_cols_kernel: the same for both ColVecs forms and the fp32 RowVecs form; the fp64 RowVecs form spills in this build
    (2 registers, 12 B of scratch: open) and is held to what it has.  kfold_kernel's own two instantiations are still
    the only ones of that name (tests/test_kfold_cpu.py pins their figures)."""
    props = _kernel_props(tmp_path)
    cols = {k: v for k, v in props.items() if "kfold_cols_kernel" in k}
    assert len(cols) == 2, sorted(cols)
    for k, v in cols.items():
        assert v["vgpr_count"] <= 256, (k, v)
        assert v["private_segment_fixed_size"] == 0, (k, v)
        assert v["vgpr_spill_count"] == 0, (k, v)
    wh = {k: v for k, v in props.items() if "kfold_whiten_cols_kernel" in k}
    assert len(wh) == 4, sorted(wh)
    for k, v in wh.items():
        assert v["vgpr_count"] <= 256, (k, v)
        if "IdLi1E" in k:  # <double, LAYOUT_ROWVECS>
            assert v["private_segment_fixed_size"] <= 16 and v["vgpr_spill_count"] <= 2, (k, v)
        else:
            assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0, (k, v)
    assert len([k for k in props if "kfold_kernel" in k]) == 2
