"""blr_posterior_ragged_x16 without a GPU: the symbol is exported, bound and declared; posterior_ragged / logpdf_ragged
on ColVecs16 / RowVecs16 name their limits before any device is touched; the map front still refuses unequal N on 16-bit inputs."""
import os
import re

import numpy as np
import pytest

import blr_amd as R
from blr_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_x16_ragged_symbol_is_exported_bound_and_declared():
    header = open(os.path.join(ROOT, "include", "blr_mi355x.h")).read()
    decl = re.search(r"\nint blr_posterior_ragged_x16\(([^;]*)\);", header)
    assert decl and "blr_posterior_ragged_x16" in _abi.EXPORTED_SYMBOLS and callable(_abi.Handle.posterior_ragged_x16)
    assert len(decl.group(1).split(",")) == len(_abi._SIGS["blr_posterior_ragged_x16"][0]) == 29
    assert hasattr(_abi.load_library(), "blr_posterior_ragged_x16")


@pytest.mark.parametrize("call", [R.posterior_ragged, R.logpdf_ragged])
def test_x16_ragged_front_names_its_limits(call, monkeypatch):
    monkeypatch.setattr(R.regressor, "_handle", lambda: pytest.fail("a limit must be raised before the handle is asked for"))
    f = R.BayesianLinearRegressor(np.zeros(3, np.float32), R.Diagonal(np.ones(3, np.float32)))
    x, y, offsets = R.ColVecs16(np.zeros((3, 4), np.float16, order="F")), np.zeros(4, np.float32), [0, 1, 4]
    with pytest.raises(ValueError, match="isotropic"):
        call(f, x, offsets, R.Diagonal(np.ones(4)), y)
    with pytest.raises(ValueError, match="isotropic"):
        call(f, x, offsets, np.ones(4), y)  # per observation
    with pytest.raises(ValueError, match=r"offsets\[-1\] != number of inputs"):
        call(f, x, [0, 1, 3], 0.5, y)
    big = R.BayesianLinearRegressor(np.zeros(129, np.float32), R.Diagonal(np.ones(129, np.float32)))
    with pytest.raises(ValueError, match="D <= 128"):
        call(big, R.RowVecs16(np.zeros((4, 129), np.float16)), offsets, 0.5, y)
    with pytest.raises(TypeError):  # the packed calls without a 16-bit entry point do not widen on the quiet
        R.mean_ragged(f, x, offsets)


def test_x16_map_front_still_refuses_unequal_counts():
    f = R.BayesianLinearRegressor(np.zeros(3, np.float32), R.Diagonal(np.ones(3, np.float32)))
    xs = [R.ColVecs16(np.zeros((3, n), np.float16, order="F")) for n in (4, 5)]
    with pytest.raises(ValueError, match="unequal N"):
        R.logpdf_map([f(x, 0.5) for x in xs], [np.zeros(4, np.float32), np.zeros(5, np.float32)])
