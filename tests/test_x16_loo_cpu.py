"""blr_loo_batched_x16 without a GPU: the symbol is exported, bound and declared; loo / loo_map on ColVecs16 / RowVecs16
name their limits before any device is touched."""
import os
import re

import numpy as np
import pytest

import blr_amd as R
from blr_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_x16_loo_symbol_is_exported_bound_and_declared():
    header = open(os.path.join(ROOT, "include", "blr_mi355x.h")).read()
    decl = re.search(r"\nint blr_loo_batched_x16\(([^;]*)\);", header)
    assert decl and "blr_loo_batched_x16" in _abi.EXPORTED_SYMBOLS and callable(_abi.Handle.loo_batched_x16)
    assert len(decl.group(1).split(",")) == len(_abi._SIGS["blr_loo_batched_x16"][0]) == 28
    assert hasattr(_abi.load_library(), "blr_loo_batched_x16")


@pytest.mark.parametrize("call", [lambda fx, y: R.loo(fx, y), lambda fx, y: R.loo_map([fx], [y])], ids=["loo", "loo_map"])
def test_x16_loo_front_names_its_limits(call, monkeypatch):
    monkeypatch.setattr(R.regressor, "_handle", lambda: pytest.fail("a limit must be raised before the handle is asked for"))
    f = R.BayesianLinearRegressor(np.zeros(3, np.float32), R.Diagonal(np.ones(3, np.float32)))
    x, y = R.ColVecs16(np.zeros((3, 4), np.float16, order="F")), np.zeros(4, np.float32)
    with pytest.raises(ValueError, match="isotropic"):
        call(f(x, R.Diagonal(np.ones(4))), y)
    with pytest.raises(NotImplementedError, match="block"):
        call(f(x, np.eye(4)), y)
    big = R.BayesianLinearRegressor(np.zeros(129, np.float32), R.Diagonal(np.ones(129, np.float32)))
    with pytest.raises(ValueError, match="D <= 128"):
        call(big(R.RowVecs16(np.zeros((4, 129), np.float16)), 0.5), y)
    with pytest.raises(ValueError, match="mixed"):
        R.loo_map([f(x, 0.5), f(R.ColVecs(np.zeros((3, 4), np.float32, order="F")), 0.5)], [y, y])
