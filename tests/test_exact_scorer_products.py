"""The fact the exact scorer's fp64 FMA rests on: the product of a stored value (bf16, f16 or f32) and an
f32 query value is exact in fp64.

The inner-product scorer (csrc/vs_device.h ``exact_score_rows``) accumulates ``fma(x, q, acc)`` where the
oracle computes ``acc + x * q`` with a rounded product.  The two agree bit for bit exactly when ``x * q``
needs no rounding: at most 24 + 24 significant bits, an exponent far inside fp64's range.  Checked here
with exact rational arithmetic over random and extreme values of each row dtype.
"""
from fractions import Fraction

import numpy as np
import pytest

from oracle import oracle as O


def _f32_extremes():
    """fp32 values at the edges: zeros, the subnormal range, the normal range's ends, odd mantissas."""
    bits = np.array([0x00000000, 0x80000000,  # +0, -0
                     0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF,  # smallest / largest subnormal
                     0x00800000, 0x80800000,  # smallest normal
                     0x7F7FFFFF, 0xFF7FFFFF,  # largest finite
                     0x3F800000, 0xBF800000, 0x3F800001, 0xBFFFFFFF,  # 1, -1, 1 + ulp, -(2 - ulp)
                     0x4B7FFFFF, 0x33800001, 0x7F000001, 0x00FFFFFF], dtype=np.uint32)
    return bits.view(np.float32)


def _random_f32(rng, n):
    """Finite fp32 values with uniformly random sign, exponent and mantissa bits (subnormals included)."""
    bits = rng.integers(0, 2 ** 32, size=n, dtype=np.uint64).astype(np.uint32)
    v = bits.view(np.float32)
    return v[np.isfinite(v)]


def _row_values(dtype, rng, n):
    """Values a stored row of ``dtype`` can hold, as fp32: extremes of the dtype plus random ones."""
    if dtype == "f32":
        return np.concatenate([_f32_extremes(), _random_f32(rng, n)])
    if dtype == "bf16":  # the upper 16 bits of an fp32: every finite pattern of the edges, random others
        hi = np.array([0x0000, 0x8000, 0x0001, 0x8001, 0x007F, 0x0080, 0x7F7F, 0xFF7F, 0x3F80, 0xBF80, 0x3FFF,
                       0x00FF], dtype=np.uint32)
        hi = np.concatenate([hi, rng.integers(0, 2 ** 16, size=n, dtype=np.uint64).astype(np.uint32)])
        v = (hi << np.uint32(16)).view(np.float32)
        return v[np.isfinite(v)]
    h = np.array([0x0000, 0x8000, 0x0001, 0x8001, 0x03FF, 0x83FF, 0x0400, 0x7BFF, 0xFBFF, 0x3C00, 0xBC00, 0x3C01],
                 dtype=np.uint16)
    h = np.concatenate([h, rng.integers(0, 2 ** 16, size=n, dtype=np.uint64).astype(np.uint16)])
    v = h.view(np.float16).astype(np.float32)  # (f16 -> f32 is exact, subnormals included)
    return v[np.isfinite(v)]


@pytest.mark.parametrize("dtype", ["bf16", "f16", "f32"])
def test_row_value_times_f32_query_is_exact_in_fp64(dtype):
    rng = np.random.default_rng({"bf16": 11, "f16": 12, "f32": 13}[dtype])
    x = _row_values(dtype, rng, 600)
    np.testing.assert_array_equal(O.round_dtype(x, dtype), x)  # values the dtype really holds
    q = np.concatenate([_f32_extremes(), _random_f32(rng, 600)])
    # every extreme against every extreme, and random pairs
    xe, qe = np.meshgrid(x[:18], q[:18], indexing="ij")
    n = min(x.size, q.size)
    xs = np.concatenate([xe.ravel(), x[:n], x[:n][::-1]])
    qs = np.concatenate([qe.ravel(), q[:n], q[:n]])
    with np.errstate(all="raise"):  # no overflow, underflow or invalid in the fp64 product
        p = xs.astype(np.float64) * qs.astype(np.float64)
    assert np.isfinite(p).all()
    for a, b, c in zip(xs.tolist(), qs.tolist(), p.tolist()):
        assert Fraction(c) == Fraction(a) * Fraction(b), (dtype, a, b, c)
    # the sign of a zero product is the product of the signs: what the separate multiply gives too
    z = p == 0.0
    assert np.array_equal(np.signbit(p[z]), np.signbit(xs[z]) ^ np.signbit(qs[z]))


def test_fma_equals_rounded_product_then_add():
    """With an exact product, acc + fl(x * q) is the single rounding of acc + x * q: the FMA's result."""
    rng = np.random.default_rng(14)
    x = _row_values("f32", rng, 400)
    q = _random_f32(rng, 400)
    n = min(x.size, q.size)
    x, q = x[:n], q[:n]
    acc = rng.standard_normal(n) * np.exp2(rng.integers(-60, 60, size=n).astype(np.float64))
    acc[:8] = [0.0, -0.0, 1.0, -1.0, 2.0 ** -1074, 2.0 ** 1000, -2.0 ** -1022, 3.0]
    got = acc + x.astype(np.float64) * q.astype(np.float64)
    for a, b, c, g in zip(acc.tolist(), x.tolist(), q.tolist(), got.tolist()):
        exact = Fraction(a) + Fraction(b) * Fraction(c)
        # the correctly rounded fp64 of the exact sum (Fraction -> float rounds to nearest even)
        assert g == float(exact), (a, b, c, g)
