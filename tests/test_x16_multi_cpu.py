"""blr_posterior_multi_batched_x16 without a GPU: the symbol is declared, exported and bound with one arity, and the limits of the
Python column fronts on ColVecs16 / RowVecs16 inputs raise ValueError naming them (no widened fall-back)."""
import os
import re

import numpy as np
import pytest

import blr_amd as R
from blr_amd import _abi

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "blr_mi355x.h")
NAME = "blr_posterior_multi_batched_x16"


def test_symbol_declared_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(NAME + r"\s*\(([^)]*)\)", text)
    assert m, "the header does not declare it"
    assert NAME in _abi.EXPORTED_SYMBOLS
    assert len(_abi._SIGS[NAME][0]) == len(m.group(1).split(",")) == 35
    assert callable(getattr(_abi.Handle, "posterior_multi_batched_x16"))


def _fx(D, N, Sy=0.5, vecs=R.ColVecs16, fmt="f16", prior=None):
    X = np.ones((D, N), np.float16) if fmt == "f16" else R.bf16_bits(np.ones((D, N), np.float32))
    x = vecs(np.asfortranarray(X) if vecs is R.ColVecs16 else np.ascontiguousarray(X.T), fmt)
    return R.BayesianLinearRegressor(np.zeros(D, np.float32), prior if prior is not None else R.Diagonal(np.ones(D, np.float32)))(x, Sy)


@pytest.mark.parametrize("front", [R.posterior_columns_map, R.logpdf_columns_map])
@pytest.mark.parametrize("fxs,Ss,word", [
    ([_fx(129, 4)], [2], "D <= 128"),
    ([_fx(8, 4, Sy=R.Diagonal(np.ones(4, np.float32)))], [2], "isotropic"),
    ([_fx(8, 4), R.BayesianLinearRegressor(np.zeros(8), R.Diagonal(np.ones(8)))(R.ColVecs(np.ones((8, 4))), 0.5)], [2, 2], "mixed"),
    ([_fx(8, 4), _fx(8, 5)], [2, 2], "unequal N"),
    ([_fx(8, 4), _fx(8, 4)], [2, 3], "must agree"),
    ([_fx(8, 4), _fx(9, 4)], [2, 2], "must agree"),
    ([_fx(8, 4), _fx(8, 4, vecs=R.RowVecs16)], [2, 2], "must agree"),
    ([_fx(8, 4), _fx(8, 4, fmt="bf16")], [2, 2], "must agree"),
])
def test_limits_raise_value_error(front, fxs, Ss, word):
    Ys = [np.zeros((len(fx.x), S), np.float32) for fx, S in zip(fxs, Ss)]
    with pytest.raises(ValueError, match=word):
        front(fxs, Ys)


def test_single_data_set_fronts_reject_too():
    with pytest.raises(ValueError, match="D <= 128"):
        R.logpdf_columns(_fx(129, 4), np.zeros((4, 2), np.float32))
    with pytest.raises(ValueError, match="isotropic"):
        R.posterior_columns(_fx(8, 4, Sy=R.Diagonal(np.ones(4, np.float32))), np.zeros((4, 2), np.float32))
