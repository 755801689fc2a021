"""CPU-side checks of the leave-one-out predictives (blr_loo_batched_*, loo, loo_map, ResidentPosterior.loo): the symbols are
declared, exported and bound, the header, the binding and the Julia shim agree on the arity, and the argument checks that need
no device (they come before the handle check)."""
import os
import re

import numpy as np
import pytest

import blr_amd
from blr_amd import _abi
from blr_amd import regressor as R

SYMS = ("blr_loo_batched_f64", "blr_loo_batched_f32")
ARITY = 27


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
    assert _abi._SIGS["blr_loo_batched_f64"] == _abi._SIGS["blr_loo_batched_f32"]
    assert hasattr(_abi.Handle, "loo")


def test_python_surface():
    for name in ("loo", "loo_map", "LOO"):
        assert getattr(blr_amd, name) is getattr(R, name)
        assert name in blr_amd.__all__
    assert R.LOO._fields == ("mean", "var", "logpdf", "total")
    assert callable(getattr(blr_amd.ResidentPosterior, "loo", None))


def test_julia_shim_calls_both_symbols_with_the_header_arity(repo_root):
    jl = open(os.path.join(repo_root, "julia", "BLRMI355X.jl")).read()
    header = _header(repo_root)
    assert "function loo!(" in jl and "function loo(" in jl
    for name in SYMS:
        m = re.search(rf"ccall\(\(:{name}, LIB\), Cint,\s*\(([^)]*)\)", jl)
        assert m, name
        types = [t for t in m.group(1).split(",") if t.strip()]
        assert len(types) == _arity(header, name), name


def _call(name, **kw):
    """blr_loo_batched_* with a NULL handle and valid arguments except those in kw."""
    lib = _abi.load_library()
    X = np.zeros((4, 3))
    y, s, mw, T = np.zeros(3), np.ones(1), np.zeros(4), np.eye(4)
    info = np.zeros(1, dtype=np.int32)
    a = dict(memspace=_abi.MEM_HOST, layout=_abi.LAYOUT_COLVECS, B=1, D=4, N=3, X=X, ldx=4, strideX=0, y=y, stridey=0,
             noise_kind=_abi.NOISE_ISOTROPIC, s=s, strides=0, mw=mw, stridemw=0, T=T, ldt=4, strideT=0, lm=None, stride_lm=3,
             lv=None, stride_lv=3, ll=None, stride_ll=3, tot=None, info=info)
    a.update(kw)
    p = _abi._ptr
    return getattr(lib, name)(None, a["memspace"], a["layout"], a["B"], a["D"], a["N"], p(a["X"]), a["ldx"], a["strideX"], p(a["y"]),
                              a["stridey"], a["noise_kind"], p(a["s"]), a["strides"], p(a["mw"]), a["stridemw"], p(a["T"]), a["ldt"],
                              a["strideT"], p(a["lm"]), a["stride_lm"], p(a["lv"]), a["stride_lv"], p(a["ll"]), a["stride_ll"],
                              p(a["tot"]), p(a["info"]))


@pytest.mark.parametrize("name", SYMS)
def test_argument_errors_without_a_device(name):
    # (the checks read no element: the float64 buffers only provide non-NULL pointers for the f32 entry point too)
    assert _call(name, noise_kind=_abi.NOISE_DENSE) == -12
    assert _call(name, ldx=3) == -8                        # ColVecs: ldx < D
    assert _call(name, layout=_abi.LAYOUT_ROWVECS, ldx=2) == -8  # RowVecs: ldx < N
    assert _call(name, info=None) == -27
    assert _call(name, D=0) == -5
    assert _call(name, T=None) == -17
    assert _call(name, ldt=3) == -18
    assert _call(name, B=2, stridemw=3) == -16
    assert _call(name, memspace=7) == -2
    # valid arguments and a NULL handle: -1
    assert _call(name) == -1


def _fx(D=3, N=4, Sy=0.5):
    rng = np.random.default_rng(0)
    f = R.BayesianLinearRegressor(np.zeros(D), R.Diagonal(np.ones(D)))
    return f(R.ColVecs(rng.standard_normal((D, N))), Sy)


def test_loo_rejects_dense_noise_and_length_mismatch():
    fx = _fx(Sy=np.eye(4))
    with pytest.raises(NotImplementedError):
        R.loo(fx, np.zeros(4))
    with pytest.raises(ValueError):
        R.loo(_fx(), np.zeros(5))
    with pytest.raises(ValueError):
        R.loo_map([_fx(), _fx()], [np.zeros(4)])
    assert R.loo_map([], []) == []
