"""tests/fxaa_model.py, the checker of oxc_apply_fxaa, on the CPU: known answers derived by hand, and a comparison with a second, scalar
transcription of passes/fxaa/fxaa.slang in binary64, written from the Slang and not from the checker."""
import math

import numpy as np
import pytest

import fxaa_frames as XF
import fxaa_model as XM
from pixel_rules import pack_ufloat

FORMATS = pytest.mark.parametrize("fmt", [0, 1], ids=["b10g11r11", "rgba16f"])


def transposed(image):
    return np.ascontiguousarray(np.swapaxes(image, 0, 1))


# ---- known answers ------------------------------------------------------------------------------------------------------------------------------
@FORMATS
def test_a_constant_image_is_unchanged(fmt):
    for colour in ((0.5, 0.25, 2.0), (0.0, 0.0, 0.0), (1.0 / 1024, 3.0, 60000.0)):
        image = XF.constant_image(13, 9, fmt, colour)
        out, stats = XM.apply_fxaa(image, fmt)
        assert np.array_equal(out, image) and stats == [13 * 9, 0, 0, 0]


@FORMATS
def test_a_black_image_is_unchanged(fmt):
    image = np.zeros((7, 5, 4), dtype=np.uint16) if fmt else np.zeros((7, 5), dtype=np.uint32)
    out, stats = XM.apply_fxaa(image, fmt)
    assert np.array_equal(out, image) and stats == [35, 0, 0, 0]


def codes_of(channel, value, fmt):
    """The stored code of one channel (0 r, 1 g, 2 b, 3 alpha) of the binary64 `value`."""
    if fmt:
        return int(np.float32(value).astype(np.float16).view(np.uint16))
    return int(pack_ufloat(np.float32(value), 5 if channel == 2 else 6)[0])


def channels_of(image, fmt):
    """[H, W, channels] of stored codes."""
    if fmt:
        return image.astype(np.int64)
    w = image.astype(np.int64)
    return np.stack([w & 0x7FF, (w >> 11) & 0x7FF, w >> 22], axis=-1)


@FORMATS
def test_vertical_step_edge(fmt):
    """A 16 x 8 image, DARK (D, luma Ld) in the columns 0 .. 7 and BRIGHT (B, luma Lb) in 8 .. 15.  Clamp addressing makes every row alike.
    Column 7: center = left = up = down = Ld, right = Lb, the corners Ld, Ld, Lb, Lb, so luma_range = Lb - Ld, above max(0.0312, Lb / 8).
    edge_horizontal = 0 and edge_vertical = 4 (Lb - Ld): the edge is vertical, step_length = 1 / 16; gradient1 = 0 and gradient2 = Lb - Ld, so
    side 2 (right) is the steepest, luma_local_average = (Ld + Lb) / 2, gradient_scaled = (Lb - Ld) / 4, and current_uv.x = 0.5: the texel
    boundary.  The search runs along y; every sample there is the mean colour (D + B) / 2, whose luma lies 0.038 above the local average,
    under gradient_scaled = 0.114: neither side is ever reached, all 12 steps run, both distances are 26.5 / 8, pixel_offset = -0.5 + 0.5 = 0.
    luma_average = (8 Ld + 4 Lb) / 12, so s1 = ((Lb - Ld) / 3) / (Lb - Ld) = 1 / 3, s2 = (-2 / 3 + 3) / 9 = 7 / 27 and final_offset =
    0.75 (7 / 27)^2 = 49 / 972 of a texel towards the bright side: column 7 becomes D + (B - D) * 49 / 972.  Column 8 mirrors it (side 1, left,
    is the steepest there; step_length = -1 / 16): B + (D - B) * 49 / 972.  Every other column has luma_range 0 and is unchanged; the alpha
    of RGBA16F is filtered like the colour.  In binary32 the result lies within one stored code of this."""
    image = XF.step_edge(16, 8, fmt, at=8)
    detail = {}
    out, stats = XM.apply_fxaa(image, fmt, detail)
    assert stats == [14 * 8, 2 * 8, 16 * 22, 16]
    assert not detail["horizontal"].any() and (detail["steepest1"] == (detail["xs"] == 8)).all()
    t = 49.0 / 972.0
    D, B = XF.DARK + (0.25,), XF.BRIGHT + (0.75,)
    got = channels_of(out, fmt)
    assert np.array_equal(np.delete(out, [7, 8], axis=1), np.delete(image, [7, 8], axis=1))
    for ch in range(4 if fmt else 3):
        for column, value in ((7, D[ch] + (B[ch] - D[ch]) * t), (8, B[ch] + (D[ch] - B[ch]) * t)):
            assert (np.abs(got[:, column, ch] - codes_of(ch, value, fmt)) <= 1).all(), (ch, column, value)
    # and the value itself, not only its neighbourhood: the red channel of column 7
    assert codes_of(0, 0.125 + 0.875 * t, fmt) in got[:, 7, 0]


@FORMATS
def test_the_transposed_image_gives_the_transposed_result(fmt):
    """A step edge has no ties, so this pins horizontal against vertical handling (and down = -1 against left = -1)."""
    for at in (8, 3):
        image = XF.step_edge(16, 8, fmt, at=at)
        a, b = {}, {}
        out, stats = XM.apply_fxaa(image, fmt, a)
        out_t, stats_t = XM.apply_fxaa(transposed(image), fmt, b)
        assert np.array_equal(transposed(out), out_t) and stats == stats_t
        assert not a["horizontal"].any() and b["horizontal"].all()


# ---- an independent transcription --------------------------------------------------------------------------------------------------------------
class Undecided(Exception):
    pass


def differs(a, b):
    """Guards a comparison: its sides must be at least 1e-4 relative apart."""
    if abs(a - b) <= 1e-4 * max(abs(a), abs(b)):
        raise Undecided()


def transcription(planes, x, y):
    """fs_main of fxaa.slang for one fragment, binary64 throughout: (rgba, searched).  `planes`: four [H][W] lists of Python floats.  The
    sampler is LinearSamplerClamped: unnormalised coordinate minus a half, floor, fraction, clamp to edge."""
    H, W = len(planes[0]), len(planes[0][0])

    def texel(ix, iy):
        ix, iy = min(max(ix, 0), W - 1), min(max(iy, 0), H - 1)
        return [p[iy][ix] for p in planes]

    def sample(u, v, offset=(0, 0)):
        gx, gy = u * W - 0.5 + offset[0], v * H - 0.5 + offset[1]
        ix, iy = math.floor(gx), math.floor(gy)
        fx, fy = gx - ix, gy - iy
        t00, t10, t01, t11 = texel(ix, iy), texel(ix + 1, iy), texel(ix, iy + 1), texel(ix + 1, iy + 1)
        return [(a * (1 - fx) + b * fx) * (1 - fy) + (c * (1 - fx) + d * fx) * fy for a, b, c, d in zip(t00, t10, t01, t11)]

    def rgb2luma(c):
        return math.sqrt(c[0] * 0.299 + c[1] * 0.587 + c[2] * 0.114)

    def quality(q):
        return 1.0 if q < 5 else ((2.0 if q < 10 else (4.0 if q < 11 else 8.0)) if q > 5 else 1.5)

    tex = ((x + 0.5) / W, (y + 0.5) / H)
    inverse_screen_size = (1.0 / W, 1.0 / H)
    color_center = sample(*tex)
    luma_center = rgb2luma(color_center)
    luma_down, luma_up = rgb2luma(sample(*tex, (0, -1))), rgb2luma(sample(*tex, (0, 1)))
    luma_left, luma_right = rgb2luma(sample(*tex, (-1, 0))), rgb2luma(sample(*tex, (1, 0)))
    luma_min = min(luma_center, min(min(luma_down, luma_up), min(luma_left, luma_right)))
    luma_max = max(luma_center, max(max(luma_down, luma_up), max(luma_left, luma_right)))
    luma_range = luma_max - luma_min
    threshold = max(0.0312, luma_max * 0.125)
    differs(luma_range, threshold)
    if luma_range < threshold:
        return color_center, False
    luma_down_left, luma_up_right = rgb2luma(sample(*tex, (-1, -1))), rgb2luma(sample(*tex, (1, 1)))
    luma_up_left, luma_down_right = rgb2luma(sample(*tex, (-1, 1))), rgb2luma(sample(*tex, (1, -1)))
    luma_down_up, luma_left_right = luma_down + luma_up, luma_left + luma_right
    luma_left_corners, luma_down_corners = luma_down_left + luma_up_left, luma_down_left + luma_down_right
    luma_right_corners, luma_up_corners = luma_down_right + luma_up_right, luma_up_right + luma_up_left
    edge_horizontal = abs(-2.0 * luma_left + luma_left_corners) + abs(-2.0 * luma_center + luma_down_up) * 2.0 + abs(-2.0 * luma_right + luma_right_corners)
    edge_vertical = abs(-2.0 * luma_up + luma_up_corners) + abs(-2.0 * luma_center + luma_left_right) * 2.0 + abs(-2.0 * luma_down + luma_down_corners)
    differs(edge_horizontal, edge_vertical)
    is_horizontal = edge_horizontal >= edge_vertical
    step_length = inverse_screen_size[1] if is_horizontal else inverse_screen_size[0]
    luma1, luma2 = (luma_down, luma_up) if is_horizontal else (luma_left, luma_right)
    gradient1, gradient2 = luma1 - luma_center, luma2 - luma_center
    differs(abs(gradient1), abs(gradient2))
    is1_steepest = abs(gradient1) >= abs(gradient2)
    gradient_scaled = 0.25 * max(abs(gradient1), abs(gradient2))
    if is1_steepest:
        step_length = -step_length
        luma_local_average = 0.5 * (luma1 + luma_center)
    else:
        luma_local_average = 0.5 * (luma2 + luma_center)
    current_uv = [tex[0], tex[1]]
    current_uv[1 if is_horizontal else 0] += step_length * 0.5
    offset = (inverse_screen_size[0], 0.0) if is_horizontal else (0.0, inverse_screen_size[1])
    uv1 = [current_uv[k] - offset[k] * quality(0) for k in (0, 1)]
    uv2 = [current_uv[k] + offset[k] * quality(0) for k in (0, 1)]
    luma_end1 = rgb2luma(sample(*uv1)) - luma_local_average
    luma_end2 = rgb2luma(sample(*uv2)) - luma_local_average

    def reached(luma_end):
        differs(abs(luma_end), gradient_scaled)
        return abs(luma_end) >= gradient_scaled

    reached1, reached2 = reached(luma_end1), reached(luma_end2)
    reached_both = reached1 and reached2
    if not reached1:
        uv1 = [uv1[k] - offset[k] * quality(1) for k in (0, 1)]
    if not reached2:
        uv2 = [uv2[k] + offset[k] * quality(1) for k in (0, 1)]
    if not reached_both:
        for i in range(2, 12):
            if not reached1:
                luma_end1 = rgb2luma(sample(*uv1)) - luma_local_average
            if not reached2:
                luma_end2 = rgb2luma(sample(*uv2)) - luma_local_average
            reached1, reached2 = reached(luma_end1), reached(luma_end2)
            reached_both = reached1 and reached2
            if not reached1:
                uv1 = [uv1[k] - offset[k] * quality(i) for k in (0, 1)]
            if not reached2:
                uv2 = [uv2[k] + offset[k] * quality(i) for k in (0, 1)]
            if reached_both:
                break
    distance1 = tex[0] - uv1[0] if is_horizontal else tex[1] - uv1[1]
    distance2 = uv2[0] - tex[0] if is_horizontal else uv2[1] - tex[1]
    differs(distance1, distance2)
    is_direction1 = distance1 < distance2
    distance_final = min(distance1, distance2)
    edge_thickness = distance1 + distance2
    differs(luma_center, luma_local_average)
    is_luma_center_smaller = luma_center < luma_local_average
    luma_end = luma_end1 if is_direction1 else luma_end2
    differs(luma_end, 0.0)
    correct_variation = (luma_end < 0.0) != is_luma_center_smaller
    pixel_offset = -distance_final / edge_thickness + 0.5
    final_offset = pixel_offset if correct_variation else 0.0
    luma_average = (1.0 / 12.0) * (2.0 * (luma_down_up + luma_left_right) + luma_left_corners + luma_right_corners)
    sub_pixel_offset1 = min(max(abs(luma_average - luma_center) / luma_range, 0.0), 1.0)
    sub_pixel_offset2 = (-2.0 * sub_pixel_offset1 + 3.0) * sub_pixel_offset1 * sub_pixel_offset1
    sub_pixel_offset_final = sub_pixel_offset2 * sub_pixel_offset2 * 0.75
    final_offset = max(final_offset, sub_pixel_offset_final)
    final_uv = [tex[0], tex[1]]
    final_uv[1 if is_horizontal else 0] += final_offset * step_length
    return sample(*final_uv), True


# of the searched, decided pixels' stored codes, how many differ from the transcription's (each by one code): measured against the
# transcription, never against the kernel
RECORDED = {0: (4, 3), 1: (22, 4)}  # fmt: (differing codes, channels per pixel)


@FORMATS
def test_against_the_transcription(fmt):
    image = XF.polygons(64, 48, fmt)
    H, W = image.shape[:2]
    out, stats = XM.apply_fxaa(image, fmt)
    got = channels_of(out, fmt)
    planes = [p.astype(np.float64).tolist() for p in XM.decode(image, fmt)]
    searched = undecided = compared = differing = 0
    worst = 0
    for y in range(H):
        for x in range(W):
            try:
                colour, was_searched = transcription(planes, x, y)
            except Undecided:
                undecided += 1
                continue
            if not was_searched:
                continue
            searched += 1
            for ch in range(4 if fmt else 3):
                d = abs(int(got[y, x, ch]) - codes_of(ch, colour[ch], fmt))
                compared += 1
                differing += d != 0
                worst = max(worst, d)
    print(f"format {fmt}: {searched} searched and decided, {undecided} undecided, {differing} of {compared} codes differ, at most by {worst}")
    # conditions on the image, not measurements (the undecided pixels are counted against the searched ones: an upper bound of their share)
    assert undecided <= 0.05 * (searched + undecided), (undecided, searched)
    assert searched >= 500, searched
    assert worst <= 1
    assert (differing, compared) == (RECORDED[fmt][0], searched * RECORDED[fmt][1])
