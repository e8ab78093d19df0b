"""The arithmetic behind the range of the default product form (AMS_MATMUL_SPLIT_F16), restated in NumPy.

split1_f16 (ams_amd/csrc/split_bf16.hpp) turns an f32 weight v into two fp16 parts:
    hi = fp16(v)                                  (round to nearest even)
    lo = fp16(fma(hi, -2^11, v 2^11))             v 2^11 - hi 2^11 is exact in f32: v - hi has at most 12 significant bits
and the products use v ~ hi + lo 2^-11.  The freeze keeps a layer on that form only while its weights lie inside the range this file pins
(ams_student_freeze, weights_beyond_kernel): every |w| <= 65504 and finite, and the largest |w| at least LOW = 2^-10.

Error bound.  Let r = (v - hi) 2^11 (exact), so hi + lo 2^-11 - v = (lo - r) 2^-11.
  * v in [2^e, 2^(e+1)), e >= -14 (hi normal): |v - hi| <= 2^(e-11) (half an fp16 ulp), so |r| <= 2^e.  If |r| < 2^e its fp16 rounding
    error is at most half an ulp at |r|'s binade, <= 2^(e-12); |r| = 2^e is exact.  An r below fp16's normal range (< 2^-14) is rounded
    to a multiple of 2^-24: error <= 2^-25.  Hence |error| <= max(2^(e-23), 2^-36) <= max(2^-23 |v|, 2^-36), and since 2^-36 <= 2^-22 |v|
    for |v| >= 2^-14:   |hi + lo 2^-11 - v| <= 2^-22 |v|   on [2^-14, 65504].
  * |v| < 2^-14 (hi subnormal or zero): hi and lo are multiples of 2^-24, |v - hi| <= 2^-25, |r| <= 2^-14, and the error is up to 2^-36
    ABSOLUTE — relative to a layer whose largest weight is M that is 2^-36 / M, which passes f32's unit roundoff 2^-24 once M < 2^-12
    and reaches 2^-8 of M at M ~ 6e-9 (hi = 0, lo subnormal).
  * The freeze's threshold LOW = 2^-10 keeps every fp16 layer at <= max(2^-23, 2^-36 / 2^-10) = 2^-23 of its largest weight, a factor 4
    inside the point (2^-12) where the subnormal floor would pass 2^-24 of M.
  * 65520 is the midpoint between 65504 and 2^16: round-to-nearest-even gives hi = inf (and lo = -inf), the product NaN.
"""
import numpy as np
import pytest

LOW = 2.0 ** -10                 # ams_student_freeze: a layer whose largest |w| is below this leaves the fp16 form
F16_MAX = 65504.0


def split1_f16(v):
    """hi, lo as fp16 arrays, the way split1_f16 forms them (f32 input, RNE)."""
    v = np.asarray(v, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        hi = v.astype(np.float16)
        r = ((v.astype(np.float64) - hi.astype(np.float64)) * 2048.0).astype(np.float32)     # exact in f32 (see the module docstring)
        lo = r.astype(np.float16)
    return hi, lo


def joined(v):
    hi, lo = split1_f16(v)
    with np.errstate(invalid="ignore"):
        return hi.astype(np.float64) + lo.astype(np.float64) * 2.0 ** -11


def test_numpy_fp16_rounding_is_round_to_nearest_even():
    # (the restatement is only as good as this): ties go to the even significand, overflow rounds to inf at the midpoint 65520
    assert np.float32(1 + 2 ** -11).astype(np.float16) == np.float16(1.0)
    assert np.float32(1 + 3 * 2 ** -11).astype(np.float16) == np.float16(1 + 2 ** -9)
    assert np.float32(2 ** -25).astype(np.float16) == np.float16(0.0)             # tie between 0 and the smallest subnormal 2^-24
    assert np.float32(3 * 2 ** -25).astype(np.float16) == np.float16(2 ** -23)


def test_two_fp16_parts_keep_22_bits_on_the_normal_range():
    rng = np.random.default_rng(0)
    mag = np.exp2(rng.uniform(-14, np.log2(F16_MAX), 400000))
    edges = [2.0 ** -14, F16_MAX, 1.0, 2.0 - 2.0 ** -23, 2.0 ** 15 * (2 - 2.0 ** -10), 2.0 ** -13 * (1 + 2.0 ** -23)]
    # every binade's last f32 below the power of two (hi rounds up into the next binade) and fp16 ties
    edges += [np.nextafter(np.float32(2.0 ** e), np.float32(0)) for e in range(-13, 16)]
    edges += [2.0 ** e * (1 + 2.0 ** -11) for e in range(-14, 15)]
    v = np.concatenate([mag, np.asarray(edges, np.float64)]).astype(np.float32)
    v = np.concatenate([v, -v])
    a = np.abs(v.astype(np.float64))
    assert a.min() >= 2.0 ** -14 and a.max() <= F16_MAX
    err = np.abs(joined(v) - v.astype(np.float64))
    assert np.isfinite(err).all()
    assert np.all(err <= np.maximum(2.0 ** -23 * a, 2.0 ** -36)), "split error above max(2^-23 |v|, 2^-36)"
    assert np.all(err <= 2.0 ** -22 * a), "split error above 2^-22 |v| on [2^-14, 65504]: worst %g" % (err / a).max()
    # the bound is tight up to a factor of 2: the worst measured case sits above 2^-24 |v|
    assert (err / a).max() > 2.0 ** -24


def test_largest_fp16_value_splits_and_65520_overflows():
    hi, lo = split1_f16(np.float32(F16_MAX))
    assert float(hi) == F16_MAX and float(lo) == 0.0
    below = np.nextafter(np.float32(65520.0), np.float32(0))                         # 65519.996: still rounds down to 65504
    hi, lo = split1_f16(below)
    assert float(hi) == F16_MAX and np.isfinite(float(lo))
    assert abs(joined(below) - float(below)) <= 2.0 ** -22 * float(below)
    for v in (65520.0, -65520.0, 1e5):
        hi, lo = split1_f16(np.float32(v))
        assert np.isinf(float(hi)) and np.sign(float(hi)) == np.sign(v)
        assert not np.isfinite(joined(np.float32(v)))                              # inf + (-inf) 2^-11: NaN in the product


def _layer_error(M, rng, n=20000):
    """worst |split error| of a layer of n weights uniform in [-M, M] (its largest exactly M), relative to M"""
    w = (rng.uniform(-1.0, 1.0, n) * M).astype(np.float32)
    w[0] = np.float32(M)
    return float(np.abs(joined(w) - w.astype(np.float64)).max() / M)


@pytest.mark.parametrize("log2_max", [-15, -16, -20, -24, -27.5])
def test_layers_below_the_normal_range_lose_f32_level(log2_max):
    """A layer whose weights all lie below 2^-14 (its BN may scale them back up: the same function) multiplies with an error far above
    f32 level relative to its own scale.  Such a layer lies below LOW, so the freeze moves it to three bf16 parts."""
    M = 2.0 ** log2_max
    assert M < LOW
    rel = _layer_error(M, np.random.default_rng(1))
    assert rel > 2.0 ** -22, "layer max 2^%g: split error %g of the max" % (log2_max, rel)
    assert rel <= 2.0 ** -36 / M                                                     # the subnormal floor of the module docstring
    if log2_max <= -27:                                                              # weights ~ 6e-9: hi = 0, lo subnormal
        assert rel > 1e-4


@pytest.mark.parametrize("log2_max", [-10, -9, -6, -2, 0, 3, 10, 15.99])
def test_layers_at_or_above_the_threshold_stay_at_f32_level(log2_max):
    M = 2.0 ** log2_max
    assert LOW <= M <= F16_MAX
    rng = np.random.default_rng(2)
    assert _layer_error(M, rng) <= 2.0 ** -23
    # the worst weights of such a layer: tiny ones on fp16 subnormal midpoints, where the floor 2^-36 is reached exactly
    w = np.asarray([M, 2.0 ** -25 + 2.0 ** -36, 3 * 2.0 ** -25 - 2.0 ** -37, 0.0, -2.0 ** -30], np.float32)
    err = np.abs(joined(w) - w.astype(np.float64))
    assert err.max() <= max(2.0 ** -23 * M, 2.0 ** -36)
    assert err.max() / M <= 2.0 ** -23
