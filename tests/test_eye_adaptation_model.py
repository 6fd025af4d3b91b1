"""tests/eye_adaptation_model.py against answers worked out by hand from the rule in include/oxcull.h (oxc_apply_eye_adaptation).  No GPU."""
import math

import numpy as np

import eye_adaptation_model as M

F = np.float32
# Where an answer is compared with binary64 mathematics and not bit for bit, the bound is 1e-5 relative: the argument of the exp2 near -6
# is rounded to binary32 (half an ulp of 4.8e-7, 1.7e-7 relative in 2^x), and the division, the subtraction, the two products and the two
# closed forms around it each add at most 6e-8: under 1e-6 in all, ten times inside the bound.
ONE_ONE = np.array([0x3F800000, 0x3F800000], dtype=np.uint32)


def words(adapted, exposure=1.0):
    return np.array([adapted, exposure], dtype=np.float32).view(np.uint32)


def as_f32(w):
    return np.asarray(w, dtype=np.uint32).view(np.float32)


def grey_halves(values):
    """An RGBA16F image [1, n, 4] whose texel k is (v_k, v_k, v_k, 1): luminance v_k * (0.2127f + 0.7152f + 0.0722f) up to rounding."""
    v = np.asarray(values, dtype=np.float16)
    img = np.empty((1, v.size, 4), dtype=np.float16)
    img[0, :, :3] = v[:, None]
    img[0, :, 3] = 1.0
    return img.view(np.uint16)


def test_two_by_two_one_pixel_per_bin():
    # min -6, max 10: mapped = ((l + 6) / 16) * 254 + 1.  Grey v has luminance about 1.0001 v, l = log2(v) + 0.00014: v = 0 is dark (bin 0),
    # 2^-6 gives mapped 1.002 (bin 1), 4 gives 128.002 (bin 128), 1024 gives 255.002 (bin 255).
    img = grey_halves([0.0, 2.0 ** -6, 4.0, 1024.0]).reshape(2, 2, 4)
    hist, out = M.apply_eye_adaptation(img, 1, ONE_ONE, -6.0, 10.0, 1.0, 1.0)
    expect = np.zeros(256, dtype=np.uint32)
    expect[[0, 1, 128, 255]] = 1
    assert np.array_equal(hist, expect)
    # weighted_sum = 1 + 128 + 255 = 384, dark = 1: avg = 384 / 3 - 1 = 127;  desired = exp2((127 / 254) * 16 - 6) = exp2(2) = 4, exactly;
    # adapted = 1 + (4 - 1) * 1 = 4;  ev100 = log2(4 * (100 / 12.5)) = log2(32) = 5, exactly;  exposure = 1 / (32 * 1.2f)
    assert as_f32(out)[0] == F(4.0)
    assert as_f32(out)[1] == F(1.0) / (F(32.0) * F(1.2))


def test_dark_threshold_neighbours():
    # with the component's -11.5 .. 18: log2(0.001f) = -9.96578, mapped = (1.53422 / 29.5) * 254 + 1 = 14.21: bin 14; one ulp below is dark
    eps = F(0.001)
    below = np.nextafter(eps, F(0.0))
    assert M.bin_of([below, eps], -11.5, 18.0).tolist() == [0, 14]
    assert M.bin_of([F(-0.0), F(-5.0), F(0.0)], -11.5, 18.0).tolist() == [0, 0, 0]


def test_mapped_on_an_integer_and_one_ulp_below():
    # min 0, max 8: mapped = (l / 8) * 254 + 1 with an exact division.  l = 4 gives 0.5 * 254 + 1 = 128 exactly.
    # 16 - 3 ulp = 16 (1 - 1.79e-7) has log2 = 4 - 2.58e-7, which rounds to the binary32 below 4 (4 - 2.38e-7);  / 8 is exact: 0.5 - 2.98e-8;
    # * 254 = 127 - 7.57e-6, nearest binary32 127 - 7.63e-6;  + 1 = 128 - 7.63e-6 exactly, the binary32 below 128: bin 127.
    lum = F(16.0) - F(3.0) * F(2.0 ** -20)
    assert M.mapped_value([F(16.0)], 0.0, 8.0)[0] == F(128.0)
    assert M.mapped_value([lum], 0.0, 8.0)[0] == np.nextafter(F(128.0), F(0.0))
    assert M.bin_of([F(16.0), lum], 0.0, 8.0).tolist() == [128, 127]
    # the engine's range: powers of two land on ((k + 6) / 24) * 254 + 1
    assert M.bin_of([F(2.0 ** -6), F(64.0), F(2.0 ** 18), F(2.0 ** 19)], -6.0, 18.0).tolist() == [1, 128, 255, 255]


def test_all_dark_frame():
    img = np.zeros((3, 5), dtype=np.uint32)
    hist, out = M.apply_eye_adaptation(img, 0, ONE_ONE, -6.0, 18.0, 1.0, 1.0)
    assert hist[0] == 15 and hist[1:].sum() == 0
    # pixel_count - dark = 0 is clamped to 1: avg = 0 / 1 - 1 = -1;  desired = exp2(-24 / 254 - 6)
    desired = 2.0 ** (-24.0 / 254.0 - 6.0)
    assert abs(float(as_f32(out)[0]) / desired - 1.0) < 1e-5
    assert abs(float(as_f32(out)[1]) * (desired * 8.0 * 1.2) - 1.0) < 1e-5


def test_time_coeff_zero_keeps_the_adapted_luminance():
    img = grey_halves([0.5, 3.0, 100.0])
    for last in (0.37, 1.0, 2.0 ** -140, 65504.0):
        before = words(last)
        _, out = M.apply_eye_adaptation(img, 1, before, -6.0, 18.0, 1.0, 0.0)
        assert out[0] == before[0]
        assert abs(float(as_f32(out)[1]) * (float(F(last)) * 8.0 * 1.2) - 1.0) < 1e-5 or last < 2.0 ** -126


def test_time_coeff_one_goes_to_the_desired_luminance():
    # every pixel in bin 128 of -6 .. 18: avg = 127, desired = exp2(0.5 * 24 - 6) = 64;  adapted = 0.25 + (64 - 0.25) * 1 = 64
    img = grey_halves([64.0] * 6)
    hist, out = M.apply_eye_adaptation(img, 1, words(0.25), -6.0, 18.0, 1.0, 1.0)
    assert hist[128] == 6
    assert as_f32(out)[0] == F(64.0)
    assert as_f32(out)[1] == F(1.0) / (F(512.0) * F(1.2))  # ev100 = log2(64 * 8) = 9


def test_weighted_sum_wraps_modulo_two_to_the_32():
    hist = np.zeros(256, dtype=np.uint32)
    hist[128] = 2 ** 25 + 1  # 128 * (2^25 + 1) = 2^32 + 128 -> 128
    out = M.average(hist, 2 ** 25 + 1, ONE_ONE, -6.0, 18.0, 1.0, 1.0)
    # f32(2^25 + 1) = 2^25: avg = 128 / 2^25 - 1 = 2^-18 - 1
    avg = 2.0 ** -18 - 1.0
    desired = 2.0 ** (avg / 254.0 * 24.0 - 6.0)
    assert abs(float(as_f32(out)[0]) / desired - 1.0) < 1e-5


def test_non_finite_and_negative_channels():
    h = lambda *v: np.array(v, dtype=np.float16).view(np.uint16)  # noqa: E731
    img = np.stack([h(np.nan, 0, 0, 1), h(np.inf, 0, 0, 1), h(-1, 0, 0, 1), h(np.inf, -np.inf, 0, 1), h(0, 0, np.inf, 1), h(-0.0, -0.0, -0.0, 1)]).reshape(1, 6, 4)
    r, g, b = M.decode(img, 1)
    bins = M.bin_of(M.luminance(r, g, b), -6.0, 18.0)
    # NaN: fails the dark test, log2 gives -Inf, mapped -Inf, i32 saturates, clamp: 0.  +Inf: 255.  negative and -0: dark.  Inf - Inf: NaN.
    assert bins.tolist() == [0, 255, 0, 0, 255, 0]
    # B10G11R11: exponent 31 with a zero mantissa is +Inf, with a mantissa NaN; there is no sign
    w = np.array([[31 << 6, (31 << 6) | 1, (31 << 5) << 22, ((31 << 5) | 3) << 22, 0]], dtype=np.uint32)
    assert M.bin_of(M.luminance(*M.decode(w, 0)), -6.0, 18.0).tolist() == [255, 0, 255, 0, 0]
    # a NaN adapted luminance in the buffer comes out as the one quiet pattern;  the log2 rule gives -Inf for a NaN, exp2 of it 0.0 and the
    # division 1.0 / (0.0 * 1.2f) = +Inf: the exposure word of a NaN luminance is +Inf, not NaN
    _, out = M.apply_eye_adaptation(img, 1, np.array([0x7FC12345, 0x3F800000], dtype=np.uint32), -6.0, 18.0, 1.0, 0.5)
    assert out.tolist() == [0x7FC00000, 0x7F800000]
    assert M.stored(F(np.nan)) == 0x7FC00000 and M.stored(np.array([0xFFC00001], dtype=np.uint32).view(np.float32)[0]) == 0x7FC00000


def test_engine_defaults_on_a_mid_grey_frame():
    # 0.18 grey: luminance 0.18 * 1.0001, l = -2.4738, mapped = (3.5262 / 24) * 254 + 1 = 38.32: every pixel in bin 38;  avg = 37;
    # desired = exp2(37 / 254 * 24 - 6) = 0.17630;  from {1, 1} with time_coeff 1: adapted = desired;  exposure = 1 / (desired * 8 * 1.2)
    img = grey_halves([0.18] * 64).reshape(8, 8, 4)
    hist, out = M.apply_eye_adaptation(img, 1, ONE_ONE, -6.0, 18.0, 1.0, 1.0)
    assert hist[38] == 64
    desired = 2.0 ** (37.0 / 254.0 * 24.0 - 6.0)
    assert math.isclose(float(as_f32(out)[0]), desired, rel_tol=1e-5)
    assert math.isclose(float(as_f32(out)[1]), 1.0 / (desired * 9.6), rel_tol=1e-5)
    assert math.isclose(float(as_f32(out)[1]), 0.59085, rel_tol=1e-4)
