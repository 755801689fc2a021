"""CPU-side checks of the update / downdate of a resident multi-output state (blr_update_multi_factor_*, blr_downdate_multi_factor_*,
ResidentColumnsPosterior): the symbols are declared, exported and bound, the header, the binding and the Julia shim
agree on the arity, the argument checks that need no device (they come before the handle check), state_cols_kernel's registers,
scratch and LDS from the compiled code object, and the derivation itself in NumPy against the oracle."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import blr_amd
from blr_amd import _abi
from blr_amd import regressor as R
from oracle import blr_oracle as O

SYMS = ("blr_update_multi_factor_f64", "blr_update_multi_factor_f32", "blr_downdate_multi_factor_f64", "blr_downdate_multi_factor_f32")
ARITY = 25


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
    assert len({tuple(_abi._SIGS[n][0]) for n in SYMS}) == 1
    assert hasattr(_abi.Handle, "update_multi_factor") and hasattr(_abi.Handle, "downdate_multi_factor")
    block = header[header.index("resident MULTI-OUTPUT state"):header.index("int blr_update_multi_factor_f64")]
    assert "test/bayesian_linear_regression.jl:49-70" in block and ":93" in block and ":55-58" in block and "MATRIX targets" in block


def test_pass_width_is_mirrored(repo_root):
    hpp = open(os.path.join(repo_root, "bayesianlinearregressors.jl_amd", "csrc", "blr_state_cols.hpp")).read()
    m = re.search(r"constexpr int kStateColsPerPass = (\d+);", hpp)
    assert m and int(m.group(1)) == _abi.STATE_COLS_PER_PASS == 16


def test_python_surface():
    assert blr_amd.ResidentColumnsPosterior is R.ResidentColumnsPosterior
    assert "ResidentColumnsPosterior" in blr_amd.__all__
    for name in ("condition", "forget", "regressors", "mean_and_var", "mean", "state"):
        assert callable(getattr(R.ResidentColumnsPosterior, name)), name
    assert "_inputs" not in vars(R.ResidentColumnsPosterior)  # ResidentPosterior's helper is reused, not copied


def test_julia_shim_calls_the_symbols_with_the_header_arity(repo_root):
    jl = open(os.path.join(repo_root, "julia", "BLRMI355X.jl")).read()
    header = _header(repo_root)
    assert "function update_multi_factor!(" in jl and "function downdate_multi_factor!(" in jl
    for name in SYMS:
        m = re.search(rf"ccall\(\(:{name}, LIB\), Cint,\s*\(([^)]*)\)", jl)
        assert m, name
        types = [t for t in m.group(1).split(",") if t.strip()]
        assert len(types) == _arity(header, name) == ARITY, name


def _call(name, **kw):
    """blr_{update,downdate}_multi_factor_* with a NULL handle and valid arguments except those in kw."""
    lib = _abi.load_library()
    D, k, S, B = 4, 5, 3, 2
    a = dict(memspace=_abi.MEM_HOST, layout=_abi.LAYOUT_COLVECS, B=B, D=D, k=k, S=S, X=np.zeros((D, k * B)), ldx=D, strideX=D * k,
             Y=np.zeros(k * S * B), ldY=k, strideY=k * S, noise_kind=_abi.NOISE_ISOTROPIC, s=np.ones(B), strides=1,
             M=np.zeros(D * S * B), ldm=D, strideM=D * S, T=np.zeros(D * D * B), ldt=D, strideT=D * D, logpdf=np.zeros(B * S),
             stride_lp=S, info=np.zeros(B, dtype=np.int32))
    a.update(kw)
    p = _abi._ptr
    return getattr(lib, name)(None, a["memspace"], a["layout"], a["B"], a["D"], a["k"], a["S"], p(a["X"]), a["ldx"], a["strideX"], p(a["Y"]),
                              a["ldY"], a["strideY"], a["noise_kind"], p(a["s"]), a["strides"], p(a["M"]), a["ldm"], a["strideM"],
                              p(a["T"]), a["ldt"], a["strideT"], p(a["logpdf"]), a["stride_lp"], p(a["info"]))


@pytest.mark.parametrize("name", SYMS)
def test_argument_errors_without_a_device(name):
    # (the checks read no element of the data: the float64 buffers only provide non-NULL pointers for the f32 entry points too)
    assert _call(name, memspace=7) == -2
    assert _call(name, layout=2) == -3
    assert _call(name, B=-1) == -4
    assert _call(name, D=0) == -5
    assert _call(name, D=8193) == -5
    assert _call(name, k=-1) == -6
    assert _call(name, k=2**30 + 1) == -6
    assert _call(name, S=-1) == -7
    assert _call(name, S=2**20 + 1) == -7
    assert _call(name, X=None) == -8
    assert _call(name, ldx=3) == -9
    assert _call(name, layout=_abi.LAYOUT_ROWVECS, ldx=4) == -9
    assert _call(name, strideX=-1) == -10
    assert _call(name, Y=None) == -11
    assert _call(name, ldY=4) == -12                                   # ldY < k
    assert _call(name, strideY=-1) == -13
    assert _call(name, noise_kind=_abi.NOISE_DENSE) == -14             # dense noise
    assert _call(name, noise_kind=7) == -14
    assert _call(name, s=None) == -15
    assert _call(name, strides=-1) == -16
    assert _call(name, M=None) == -17
    assert _call(name, ldm=3) == -18                                   # ldm < D
    assert _call(name, strideM=11) == -19                              # overlapping means for B = 2 (< ldm * S)
    assert _call(name, T=None) == -20
    assert _call(name, ldt=3) == -21
    assert _call(name, strideT=15) == -22
    assert _call(name, stride_lp=2) == -24                             # overlapping evidences for B = 2 (< S)
    assert _call(name, info=None) == -25
    # nothing to do: a no-op, whatever else is passed
    assert _call(name, B=0, info=None, X=None) == 0
    assert _call(name, S=0, info=None, Y=None) == 0
    # valid arguments and a NULL handle: -1 (shared inputs and k = 0 are valid; a single regressor may have any stride; logpdf may be NULL)
    assert _call(name) == -1
    assert _call(name, strideX=0, strideY=0, strides=0) == -1
    assert _call(name, k=0, X=None, Y=None, ldY=0) == -1
    assert _call(name, B=1, strideM=0, stride_lp=0, strideT=0) == -1
    assert _call(name, logpdf=None, stride_lp=0) == -1


def _lds_bytes(elem, D):
    """state_cols_lds_bytes of blr_state_cols.hpp: header + max(stream buffers, packed factor)"""
    W, KC, header = _abi.STATE_COLS_PER_PASS, 16, 256 + 2 * 16 * 16 * 8
    return header + max(KC * (D + 1) + W * D, (D + 1) * (D + 2) // 2) * elem


def test_state_cols_kernel_resources(tmp_path, repo_root):
    """Registers and scratch of every state_cols_kernel instantiation from the code object's notes, and the LDS of a launch from the
    header's formula: no scratch, no spills, LDS within 160 KiB, and the occupancy DESIGN.md K19 states -- two workgroups per CU at
    fp64 and four at fp32 (D = 128), by LDS and by registers (eight / sixteen waves per CU: at most 256 / 128 registers)."""
    objdump = "/opt/rocm/lib/llvm/bin/llvm-objdump"
    readelf = "/opt/rocm/lib/llvm/bin/llvm-readelf"
    assert os.path.exists(objdump) and os.path.exists(readelf), "ROCm LLVM tools (the toolchain the library is built with)"
    so = shutil.copy(_abi.LIB_PATH, tmp_path / "lib.so")
    subprocess.run([objdump, "--offloading", str(so)], check=True, capture_output=True, cwd=tmp_path)
    cos = [p for p in os.listdir(tmp_path) if "gfx950" in p]
    assert cos, "no gfx950 code object in the library"
    notes = "".join(subprocess.run([readelf, "--notes", str(tmp_path / c)], check=True, capture_output=True, text=True).stdout for c in sorted(cos))
    props, name = {}, None
    for line in notes.splitlines():
        m = re.match(r"\s+(?:- )?\.(name|vgpr_count|vgpr_spill_count|private_segment_fixed_size|group_segment_fixed_size):\s+(\S+)", line)
        if m and m.group(1) == "name":
            name = m.group(2)
        elif m and name is not None:
            props.setdefault(name, {})[m.group(1)] = int(m.group(2))
    kernels = {k: v for k, v in props.items() if "state_cols_kernel" in k or "state_cols_global_kernel" in k}
    assert len(kernels) == 8, sorted(kernels)  # two kernels, two element types, update and downdate
    for k, v in kernels.items():
        assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0, (k, v)
        assert v["group_segment_fixed_size"] == 0, (k, v)  # all LDS is dynamic: the formula below is the whole of it
        if "state_cols_kernel" in k:
            assert v["vgpr_count"] <= (256 if "state_cols_kernelId" in k else 128), (k, v)
    hpp = open(os.path.join(repo_root, "bayesianlinearregressors.jl_amd", "csrc", "blr_state_cols.hpp")).read()
    assert "((size_t)kStateChunk * (D + 1) + (size_t)kStateColsPerPass * D) * elem" in hpp
    assert "return (D + 1) * (D + 2) / 2;" in hpp and "constexpr int kStateHeader = 256 + 2 * 16 * 16 * 8;" in hpp and "constexpr int kStateChunk = 16;" in hpp
    cu_lds = 160 * 1024
    assert all(_lds_bytes(e, D) <= cu_lds for e in (4, 8) for D in range(1, 129))
    assert cu_lds // _lds_bytes(8, 128) == 2 and cu_lds // _lds_bytes(4, 128) == 4
    assert 64 + 8192 * 8 <= cu_lds  # state_cols_global_kernel at the largest D


@pytest.mark.parametrize("down", [False, True])
@pytest.mark.parametrize("noise", ["diagonal", "isotropic"])
def test_derivation_reproduces_the_oracle(down, noise):
    """The formulas of the header in NumPy, for random (T, M, X, Y, s), against O.posterior_literal / O.logpdf_literal per column."""
    rng = np.random.Generator(np.random.PCG64(77 + down))
    D, k, S, N0 = 9, 4, 3, 12
    mw0 = rng.standard_normal((D, S))
    Lw = np.exp(0.2 * rng.standard_normal(D))
    X0 = rng.standard_normal((D, N0)) / np.sqrt(D)
    s0 = np.exp(0.3 * rng.standard_normal(N0)) if noise == "diagonal" else np.full(N0, 0.37)
    Y0 = rng.standard_normal((N0, S))
    X, s, Y = X0[:, :k], s0[:k], Y0[:k]
    rest = slice(k, N0)
    # the state before the call: the posterior given `rest` (update) or given everything (downdate)
    before = rest if not down else slice(0, N0)
    after = slice(0, N0) if not down else rest
    posts = [O.posterior_literal(mw0[:, c], Lw, X0[:, before], s0[before], Y0[before, c]) for c in range(S)]
    A = posts[0][2]
    T = np.linalg.cholesky(A).T
    M = np.stack([p[0] for p in posts], axis=1)
    W = X / np.sqrt(s)
    sgn = -1.0 if down else 1.0
    A1 = A + sgn * W @ W.T
    T1 = np.linalg.cholesky(A1).T
    for c in range(S):
        E = (Y[:, c] - X.T @ M[:, c]) / np.sqrt(s)
        u = np.linalg.solve(T1.T, W @ E)
        m1 = M[:, c] + sgn * np.linalg.solve(T1, u)
        quad = E @ E - sgn * (u @ u)
        lp = -0.5 * (k * np.log(2 * np.pi) + np.log(s).sum() + sgn * 2 * np.log(np.diag(T1) / np.diag(T)).sum() + quad)
        m_o, _, A_o = O.posterior_literal(mw0[:, c], Lw, X0[:, after], s0[after], Y0[after, c])
        np.testing.assert_allclose(T1.T @ T1, A_o, rtol=1e-11, atol=1e-12)
        np.testing.assert_allclose(m1, m_o, rtol=1e-9, atol=1e-11)
        # log p(Y_c | the state WITHOUT these k observations): before the call for the update, after it for the downdate
        lp_o = O.logpdf_literal(mw0[:, c], Lw, X0, s0, Y0[:, c]) - O.logpdf_literal(mw0[:, c], Lw, X0[:, rest], s0[rest], Y0[rest, c])
        assert lp == pytest.approx(lp_o, rel=1e-10, abs=1e-10)
