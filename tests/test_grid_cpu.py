"""CPU-side checks of the evidence grid (blr_logpdf_grid_*, logpdf_grid, posterior_best, logpdf_grid_map): the symbols are
declared, exported and bound, the header, the binding and the Julia shim agree on the arity, the argument checks that need no
device (they come before the handle check), the algebra the kernels implement against the oracle in numpy, and the new
kernels' register / LDS / scratch limits from the compiled code object."""
import math
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

SYMS = ("blr_logpdf_grid_f64", "blr_logpdf_grid_f32")
ARITY = 35


def _header(repo_root):
    return open(os.path.join(repo_root, "include", "blr_mi355x.h")).read()


def _arity(text, name):
    m = re.search(rf"\bint\s+{name}\s*\(([^)]*)\)", text)
    assert m, name
    return len([p for p in m.group(1).split(",") if p.strip()])


def test_symbols_declared_exported_and_bound(repo_root):
    header = _header(repo_root)
    lib = _abi.load_library()
    for name in SYMS:
        assert re.search(rf"\bint\s+{name}\s*\(", header), name
        assert hasattr(lib, name), name
        assert name in _abi.EXPORTED_SYMBOLS
        assert _arity(header, name) == len(_abi._SIGS[name][0]) == ARITY
    assert _abi._SIGS[SYMS[0]] == _abi._SIGS[SYMS[1]]
    assert hasattr(_abi.Handle, "logpdf_grid")
    assert "bayesian_linear_regression.jl:55-58" in header[header.index("GRID of (prior scale"):header.index("int blr_logpdf_grid_f64")]


def test_python_surface():
    for name in ("logpdf_grid", "posterior_best", "logpdf_grid_map", "EvidenceGrid"):
        assert getattr(blr_amd, name) is getattr(R, name)
        assert name in blr_amd.__all__ and name in R.__all__
    assert R.EvidenceGrid._fields == ("logpdf", "best", "alpha", "tau")


def test_julia_shim_calls_both_symbols_with_the_header_arity(repo_root):
    jl = open(os.path.join(repo_root, "julia", "BLRMI355X.jl")).read()
    header = _header(repo_root)
    assert "function logpdf_grid!(" in jl and "function logpdf_grid(" in jl
    for name in SYMS:
        m = re.search(rf"ccall\(\(:{name}, LIB\), Cint,\s*\(([^)]*)\)", jl)
        assert m, name
        types = [t for t in m.group(1).split(",") if t.strip()]
        assert len(types) == _arity(header, name), name


def _call(name, **kw):
    """blr_logpdf_grid_* with a NULL handle and valid arguments except those in kw."""
    lib = _abi.load_library()
    D, N, G = 4, 3, 5
    a = dict(memspace=_abi.MEM_HOST, layout=_abi.LAYOUT_COLVECS, B=1, D=D, N=N, X=np.zeros((D, N)), ldx=D, strideX=0, y=np.zeros(N),
             stridey=0, noise_kind=_abi.NOISE_ISOTROPIC, s=np.ones(1), strides=0, prior_kind=_abi.PRIOR_DENSE, mw=np.zeros(D), stridemw=0,
             Lw=np.eye(D), ldl=D, strideLw=0, G=G, alpha=np.ones(G), stride_alpha=0, tau=np.ones(G), stride_tau=0, logpdf=np.zeros(G),
             stride_lp=G, best=None, mw_best=None, stride_mwbest=D, T_best=None, ldt=D, strideT=D * D, info=np.zeros(G, dtype=np.int32),
             stride_info=G)
    a.update(kw)
    p = _abi._ptr
    return getattr(lib, name)(None, a["memspace"], a["layout"], a["B"], a["D"], a["N"], p(a["X"]), a["ldx"], a["strideX"], p(a["y"]),
                              a["stridey"], a["noise_kind"], p(a["s"]), a["strides"], a["prior_kind"], p(a["mw"]), a["stridemw"],
                              p(a["Lw"]), a["ldl"], a["strideLw"], a["G"], p(a["alpha"]), a["stride_alpha"], p(a["tau"]),
                              a["stride_tau"], p(a["logpdf"]), a["stride_lp"], p(a["best"]), p(a["mw_best"]), a["stride_mwbest"],
                              p(a["T_best"]), a["ldt"], a["strideT"], p(a["info"]), a["stride_info"])


@pytest.mark.parametrize("name", SYMS)
def test_argument_errors_without_a_device(name):
    # (the checks read no element: the float64 buffers only provide non-NULL pointers for the f32 entry point too)
    T = np.zeros((4, 4))
    assert _call(name, noise_kind=_abi.NOISE_DENSE) == -12
    assert _call(name, prior_kind=_abi.PRIOR_UPPER_FACTOR) == -15
    assert _call(name, ldx=3) == -8                               # ColVecs: ldx < D
    assert _call(name, layout=_abi.LAYOUT_ROWVECS, ldx=2) == -8   # RowVecs: ldx < N
    assert _call(name, stride_lp=4) == -27                        # stride_lp < G
    assert _call(name, B=2, T_best=T, strideT=15) == -33          # overlapping T_best
    assert _call(name, B=2, mw_best=np.zeros(8), stride_mwbest=3) == -30
    assert _call(name, T_best=T, ldt=3) == -32
    assert _call(name, info=None) == -34
    assert _call(name, stride_info=4) == -35
    assert _call(name, G=-1) == -21
    assert _call(name, stride_alpha=3) == -23
    assert _call(name, stride_tau=3) == -25
    assert _call(name, logpdf=None) == -26
    assert _call(name, D=0) == -5
    assert _call(name, D=8193) == -5
    assert _call(name, ldl=3) == -19
    assert _call(name, memspace=7) == -2
    # valid arguments and a NULL handle: -1
    assert _call(name) == -1
    assert _call(name, alpha=None, tau=None) == -1


def test_factor_prior_error_text():
    """the text posterior_from_stats uses: pass a carried-forward factor as U'U (read from the source: a NULL handle keeps no text)"""
    src = open(os.path.join(os.path.dirname(_abi.LIB_PATH), "blr_abi.hip")).read()
    body = src[src.index("int logpdf_grid(blr_handle* h"):]
    assert "pass a carried-forward factor as U'U" in body[:body.index("int S = 1")]


@pytest.mark.parametrize("D,N,noise,prior", [(7, 13, "diag", "dense"), (3, 11, "iso", "diag"), (32, 150, "diag", "diag"),
                                             (100, 150, "iso", "dense")])
def test_formula_block_agrees_with_the_oracle(D, N, noise, prior):
    """the algebra of csrc/blr_grid.hpp in numpy, fp64, against logpdf_literal / posterior_literal with Lw = alpha L0, Sy = tau S0"""
    rng = np.random.Generator(np.random.PCG64(4242 + D))
    X, mw, L0, s0 = O.generate_toy_problem(rng, N, D, dense_noise_cov=False)
    if noise == "iso":
        s0 = np.full(N, 0.8)
    if prior == "diag":
        L0 = np.diag(np.exp(0.3 * rng.standard_normal(D)))
    y = rng.standard_normal(N)
    W = 1.0 / s0
    G0 = (X * W) @ X.T
    d = y - X.T @ mw
    b0, q0, l0 = X @ (W * d), float(d @ (W * d)), float(np.sum(np.log(s0)))
    ld0 = np.linalg.slogdet(L0)[1]
    for a in 10.0 ** np.linspace(-2, 2, 5):
        for t in 10.0 ** np.linspace(-2, 2, 5):
            T = np.linalg.cholesky(a * L0 + G0 / t).T
            u = np.linalg.solve(T.T, b0 / t)
            lp = -0.5 * (N * math.log(2 * math.pi) + N * math.log(t) + l0 + q0 / t + 2 * np.sum(np.log(np.diag(T))) - D * math.log(a)
                         - ld0 - u @ u)
            m = mw + np.linalg.solve(T, u)
            lp_o = O.logpdf_literal(mw, a * L0, X, t * s0, y)
            m_o, _, A_o = O.posterior_literal(mw, a * L0, X, t * s0, y)
            assert abs(lp - lp_o) <= 1e-10 * abs(lp_o)
            assert np.linalg.norm(m - m_o) <= 1e-10 * np.linalg.norm(m_o)
            assert np.max(np.abs(T.T @ T - A_o)) <= 1e-10 * np.max(np.abs(A_o))


def test_grid_kernels_keep_two_workgroups_per_cu(tmp_path):
    """Registers, scratch and spills of the new kernels from the code object: at most 256 registers (two workgroups of four waves
    per CU; that twice the dynamic LDS of a launch fits a CU is a static_assert in csrc/blr_grid.hpp).  Scratch: the per-setting
    and the prior kernel at most the fused kernel's bound (128 B per lane, tests/test_abi_cpu.py); the statistics kernel -- a thin
    caller of phase_gram -- no more than the fused kernel of the same <T, NB, MODE>.  Vector spills: the accepted figure is what the
    kernels keep across their two phase calls (status pointers, the setting's scales), 12 at most (grid_eval_kernel<float, 8>;
    <double, 8>: 0); a statistics kernel at most 4, the fused kernel's bound in tests/test_abi_cpu.py."""
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
    grid = {k: v for k, v in props.items() if re.search(r"grid_(eval|stats|prior)_kernel", k)}
    assert len([k for k in grid if "grid_eval_kernel" in k]) == 16 and len([k for k in grid if "grid_stats_kernel" in k]) == 48
    for k, v in grid.items():
        assert v["vgpr_count"] <= 256, (k, v)
        if "grid_stats_kernel" in k:
            # a thin caller of phase_gram: whatever that phase keeps in scratch is booked on its callers -- no more than on the
            # fused kernel of the same <T, NB, MODE>
            twin = k.replace("17grid_stats_kernel", "18fused_small_kernel").replace("8GridArgs", "13PosteriorArgs")
            assert twin in props, twin
            assert v["private_segment_fixed_size"] <= props[twin]["private_segment_fixed_size"], (k, v, props[twin])
            assert v["vgpr_spill_count"] <= 4, (k, v)  # (the fused kernel's spill bound, tests/test_abi_cpu.py)
        else:
            # the fused kernel's own figure (tests/test_abi_cpu.py): the call frames of the phases, no spilled loop state
            assert v["private_segment_fixed_size"] <= 128, (k, v)
            assert v["vgpr_spill_count"] <= 12, (k, v)
    assert props[[k for k in grid if "grid_eval_kernelIdLi8" in k][0]]["vgpr_spill_count"] == 0


def _fx(D=3, N=4, Sy=0.5):
    rng = np.random.default_rng(0)
    f = R.BayesianLinearRegressor(np.zeros(D), R.Diagonal(np.ones(D)))
    return f(R.ColVecs(rng.standard_normal((D, N))), Sy)


def test_grid_rejects_dense_noise_and_length_mismatch():
    with pytest.raises(ValueError, match="dense"):
        R.logpdf_grid(_fx(Sy=np.eye(4)), np.zeros(4), [1.0], [1.0])
    with pytest.raises(ValueError):
        R.logpdf_grid(_fx(), np.zeros(5))
    with pytest.raises(ValueError):
        R.logpdf_grid_map([_fx(), _fx()], [np.zeros(4)])
    assert R.logpdf_grid_map([], []) == []
