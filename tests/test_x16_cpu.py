"""Host side of the 16-bit-feature front (no GPU): bf16 rounding bit for bit, exact widening, zero-copy containers."""
import numpy as np
import pytest

import blr_amd as R
from blr_amd import _abi
from blr_amd.regressor import _x16_layout, _x_layout


def _bf16_bits_restated(a):
    """round to nearest, ties to even, one value at a time on the bit pattern"""
    out = []
    for u in np.asarray(a, np.float32).view(np.uint32).tolist():
        if (u & 0x7F800000) == 0x7F800000 and (u & 0x007FFFFF):
            out.append((u >> 16) | 0x0040)  # NaN stays NaN (quiet)
            continue
        low, keep = u & 0xFFFF, u >> 16
        if low > 0x8000 or (low == 0x8000 and (keep & 1)):
            keep += 1
        out.append(keep & 0xFFFF)
    return np.array(out, dtype=np.uint16)


def test_bf16_bits_rounds_to_nearest_even():
    bits = np.array([0x3F808000, 0x3F818000, 0x3F808001, 0x3F807FFF, 0x00000001, 0x00008000, 0x00018000, 0x807FFFFF, 0x7F7FFFFF,
                     0x7F800000, 0xFF800000, 0x7FC00000, 0x7F800001, 0x00000000, 0x80000000], dtype=np.uint32)
    a = np.concatenate([bits.view(np.float32), np.random.default_rng(0).standard_normal(4096).astype(np.float32)])
    got = R.bf16_bits(a)
    assert got.dtype == np.uint16 and np.array_equal(got, _bf16_bits_restated(a))
    assert np.array_equal(got[:3], [0x3F80, 0x3F82, 0x3F81])  # tie to even down, tie to even up, just above the tie
    w = R.widen16(got, "bf16")
    assert w.dtype == np.float32 and np.array_equal(R.bf16_bits(w), got)  # idempotent
    assert np.isposinf(w[9]) and np.isneginf(w[10]) and np.isnan(w[11]) and np.isnan(w[12])
    h = a[15:].astype(np.float16)
    assert np.array_equal(R.widen16(h, "f16"), h.astype(np.float32))


@pytest.mark.parametrize("order", ["F", "C"])
@pytest.mark.parametrize("cls,plain", [(R.ColVecs16, R.ColVecs), (R.RowVecs16, R.RowVecs)])
def test_vecs16_keep_their_array_and_layout(cls, plain, order):
    M = np.asarray(np.arange(15, dtype=np.uint16).reshape(3, 5), order=order)
    x = cls(M)  # uint16 -> bf16
    assert x.fmt == "bf16" and x.X is M and len(x) == len(plain(M))
    got = _x16_layout(x)
    assert got[0] is M and got[1:] == _x_layout(plain(M.astype(np.float32, order="K")), np.float32)[1:]
    assert cls(M.astype(np.float16)).fmt == "f16"
    assert np.array_equal(x.widen().X, R.widen16(M, "bf16"))
    with pytest.raises(TypeError):
        cls(M.astype(np.float32))
    with pytest.raises(TypeError):
        cls(M, fmt="f16")


def test_x16_front_names_its_limits():
    f = R.BayesianLinearRegressor(np.zeros(3, np.float32), R.Diagonal(np.ones(3, np.float32)))
    x = R.ColVecs16(np.zeros((3, 4), np.float16, order="F"))
    y = np.zeros(4, np.float32)
    with pytest.raises(ValueError, match="isotropic"):
        R.logpdf(f(x, R.Diagonal(np.ones(4))), y)
    with pytest.raises(ValueError, match="mixed"):
        R.logpdf_map([f(x, 0.5), f(R.ColVecs(np.zeros((3, 4), np.float16)), 0.5)], [y, y])
    big = R.BayesianLinearRegressor(np.zeros(129, np.float32), R.Diagonal(np.ones(129, np.float32)))
    with pytest.raises(ValueError, match="D <= 128"):
        R.logpdf(big(R.RowVecs16(np.zeros((4, 129), np.float16)), 0.5), y)
    assert "blr_posterior_batched_x16" in _abi.EXPORTED_SYMBOLS and (_abi.X_BF16, _abi.X_F16) == (0, 1)
