"""CPU-side checks of the downdate (blr_downdate_factor_*, ResidentPosterior.forget): the symbols are declared, exported and
bound with the update's signature, the Julia shim calls them with the header's arity, and the argument checks that need no
device."""
import os
import re

import numpy as np
import pytest

import blr_amd
from blr_amd import _abi
from blr_amd import regressor as R

SYMS = ("blr_downdate_factor_f64", "blr_downdate_factor_f32")


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
        # exactly the update's signature
        upd = name.replace("downdate", "update")
        assert _abi._SIGS[name] == _abi._SIGS[upd]
        assert _arity(header, name) == _arity(header, upd) == len(_abi._SIGS[name][0]) == 21
    assert hasattr(_abi.Handle, "downdate_factor")


def test_resident_posterior_forget_exists():
    assert callable(getattr(blr_amd.ResidentPosterior, "forget", None))
    assert blr_amd.ResidentPosterior is R.ResidentPosterior


def test_julia_shim_calls_both_symbols_with_the_header_arity(repo_root):
    jl = open(os.path.join(repo_root, "julia", "BLRMI355X.jl")).read()
    header = _header(repo_root)
    assert "function downdate_factor!(" in jl
    for name in SYMS:
        m = re.search(rf"ccall\(\(:{name}, LIB\), Cint,\s*\(([^)]*)\)", jl)
        assert m, name
        types = [t for t in m.group(1).split(",") if t.strip()]
        assert len(types) == _arity(header, name), name


def test_null_handle_returns_minus_one():
    lib = _abi.load_library()
    for name in SYMS:
        fn = getattr(lib, name)
        assert fn(None, _abi.MEM_DEVICE, _abi.LAYOUT_COLVECS, 1, 4, 1, None, 4, 0, None, 0, _abi.NOISE_ISOTROPIC, None, 0, None, 0,
                  None, 4, 0, None, None) == -1


def test_option_key_is_listed(repo_root):
    header = _header(repo_root)
    assert "NO_DOWNDATE_LDS" in header
    readme = open(os.path.join(repo_root, "README.md")).read()
    assert "NO_DOWNDATE_LDS" in readme
