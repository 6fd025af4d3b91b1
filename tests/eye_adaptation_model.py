"""The numpy checker of oxc_apply_eye_adaptation: steps 1-9 of its header block in include/oxcull.h, vectorised over the image.  Every
binary32 operation is one numpy float32 operation in the order the header states; log2 and exp2 are the closed forms the other checkers
use.  Returns the histogram (uint32 [256]) and the exposure buffer's 8 bytes (uint32 [2])."""
from __future__ import annotations

import numpy as np

from pixel_rules import cvt_i32_sat, exp2_rule, f32a, from_half_bits, log2_rule, unpack_b10g11r11

F = np.float32
BINS = 256
LUMINANCE_EPSILON = F(0.001)
QUIET_NAN = np.uint32(0x7FC00000)
FORMAT_B10G11R11, FORMAT_R16G16B16A16 = 0, 1


def decode(image, source_format: int):
    """Step 1: the three channels of every texel as flat binary32 arrays.  Format 0: uint32 / int32 [H, W]; format 1: 16-bit [H, W, 4]."""
    if source_format == FORMAT_B10G11R11:
        return unpack_b10g11r11(np.ascontiguousarray(image).view(np.uint32).reshape(-1))
    halves = np.ascontiguousarray(image).view(np.uint16).reshape(-1, 4)
    return from_half_bits(halves[:, 0]), from_half_bits(halves[:, 1]), from_half_bits(halves[:, 2])


@np.errstate(all="ignore")
def luminance(r, g, b) -> np.ndarray:
    """Step 2."""
    return ((f32a(r) * F(0.2127) + f32a(g) * F(0.7152)) + f32a(b) * F(0.0722)).astype(np.float32)


@np.errstate(all="ignore")
def mapped_value(lum, min_exposure, max_exposure) -> np.ndarray:
    """Step 4 before the conversion: ((log2(lum) - min) / (max - min)) * 254 + 1."""
    lo = F(min_exposure)
    rng = F(F(max_exposure) - lo)
    return (((log2_rule(lum) - lo) / rng) * F(254.0) + F(1.0)).astype(np.float32)


@np.errstate(all="ignore")
def bin_of(lum, min_exposure, max_exposure) -> np.ndarray:
    """Steps 3 and 4: the bin of every luminance."""
    lum = np.atleast_1d(f32a(lum))
    bins = np.clip(cvt_i32_sat(mapped_value(lum, min_exposure, max_exposure)), 0, BINS - 1)
    return np.where(lum < LUMINANCE_EPSILON, 0, bins).astype(np.int64)


def histogram(image, source_format: int, min_exposure, max_exposure) -> np.ndarray:
    """Steps 1-5."""
    bins = bin_of(luminance(*decode(image, source_format)), min_exposure, max_exposure)
    return np.bincount(bins, minlength=BINS).astype(np.uint32)


def stored(x) -> np.uint32:
    """The word a binary32 result is stored as: a NaN is 0x7FC00000."""
    x = F(x)
    return QUIET_NAN if np.isnan(x) else np.asarray(x, dtype=np.float32).view(np.uint32)[()]


@np.errstate(all="ignore")
def average(hist, pixel_count: int, exposure_words, min_exposure, max_exposure, ev100_bias, time_coeff) -> np.ndarray:
    """Steps 6-9 from the histogram and the exposure buffer's two words (uint32); the two words stored."""
    hist = np.asarray(hist).astype(np.uint64)
    weighted_sum = int((hist * np.arange(BINS, dtype=np.uint64)).sum() & np.uint64(0xFFFFFFFF))  # every product and the sum modulo 2^32
    lo = F(min_exposure)
    rng = F(F(max_exposure) - lo)
    dark = F(np.uint32(hist[0]))
    avg = F(F(np.uint32(weighted_sum)) / np.fmax(F(F(np.uint32(pixel_count)) - dark), F(1.0))) - F(1.0)
    desired = exp2_rule(F(F(F(avg / F(254.0)) * rng) + lo))[0]
    last = np.asarray(exposure_words, dtype=np.uint32).view(np.float32)[0]
    adapted = F(last + F(F(desired - last) * F(time_coeff)))
    ev100 = log2_rule(F(adapted * F(F(F(100.0) * F(ev100_bias)) / F(12.5))))[0]
    exposure = F(F(1.0) / F(exp2_rule(ev100)[0] * F(1.2)))
    return np.array([stored(adapted), stored(exposure)], dtype=np.uint32)


def apply_eye_adaptation(image, source_format: int, exposure_words, min_exposure=-6.0, max_exposure=18.0, ev100_bias=1.0, time_coeff=1.0):
    """The whole call: (histogram uint32 [256], exposure buffer uint32 [2])."""
    image = np.asarray(image)
    pixel_count = image.shape[0] * image.shape[1]
    hist = histogram(image, source_format, min_exposure, max_exposure)
    return hist, average(hist, pixel_count, exposure_words, min_exposure, max_exposure, ev100_bias, time_coeff)
