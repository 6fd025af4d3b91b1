"""tests/bloom_model.py against answers worked out by hand from the rule in include/oxcull.h (oxc_apply_bloom), and the binding's shape
against the header.  No GPU."""
import ctypes
import os
import subprocess

import numpy as np

import bloom_model as M
from oxylus_amd import lib as L

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULTS = dict(threshold=1.0, soft_threshold=0.125, clamp_value=4.0)


def uf11(e, m):
    return (e << 6) | m


def word(r, g, b):
    """A B10G11R11 word from its three fields."""
    return r | (g << 11) | (b << 22)


def grey_word(e, m6):
    """The word whose three channels hold exponent field e and the mantissa m6 / 64 (the UF10 channel truncates it to m6 >> 1)."""
    return word(uf11(e, m6), uf11(e, m6), (e << 5) | (m6 >> 1))


def constant(W, H, w):
    return np.full((H, W), w, dtype=np.uint32)


# ---- the binding -------------------------------------------------------------------------------------------------------------------------------
def test_the_library_exports_the_call_and_the_structs_match_the_header(tmp_path):
    L.build()
    assert hasattr(ctypes.CDLL(L.LIB_PATH), "oxc_apply_bloom")
    assert L.TUNE_BLOOM_TAIL_LEVEL == 16 and L.SCENE_HAS_BLOOM == 1 << 3
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "oxcull_debug.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %d %u\\n", '
                   "sizeof(oxc_bloom_context), sizeof(oxc_image_pyramid), offsetof(oxc_bloom_context, final_attachment), "
                   "offsetof(oxc_bloom_context, bloom_upsampled_attachment), offsetof(oxc_image_pyramid, bytes), (int)OXC_TUNE_BLOOM_TAIL_LEVEL, "
                   "OXC_SCENE_HAS_BLOOM); return 0; }\n")
    exe = str(tmp_path / "sz")
    subprocess.check_call(["gcc", "-std=c99", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe])
    size, pyramid, off_final, off_up, off_bytes, knob, flag = [int(x) for x in subprocess.check_output([exe]).split()]
    assert size == ctypes.sizeof(L.BloomContext)  # what struct_size must hold
    assert pyramid == ctypes.sizeof(L.ImagePyramid) == ctypes.sizeof(L.Image) + 8
    assert off_final == L.BloomContext.final_attachment.offset
    assert off_up == L.BloomContext.bloom_upsampled_attachment.offset
    assert off_bytes == L.ImagePyramid.bytes.offset
    assert (knob, flag) == (L.TUNE_BLOOM_TAIL_LEVEL, L.SCENE_HAS_BLOOM)
    for name in ("dptr", "width", "height", "levels", "level_offset"):  # oxc_image's fields where oxc_image has them
        assert getattr(L.ImagePyramid, name).offset == getattr(L.Image, name).offset


def test_the_python_twin_lays_a_pyramid_out():
    from oxylus_amd.renderer import bloom_layout

    assert bloom_layout(5, 7, 0) == (2, 3, 2, [0, 24], 28)
    assert bloom_layout(5, 7, 1) == (2, 3, 2, [0, 48], 56)
    assert bloom_layout(5, 7, 0, gap_texels=2) == (2, 3, 2, [8, 40], 52)
    w2, h2, levels, offsets, total = bloom_layout(3840, 2160, 0)
    assert (w2, h2, levels) == M.geometry(3840, 2160)[:3] and total == 4 * sum(w * h for w, h in M.geometry(3840, 2160)[3])


# ---- geometry ----------------------------------------------------------------------------------------------------------------------------------
def test_level_counts_and_extents():
    assert M.geometry(2, 2) == (1, 1, 1, [(1, 1)])
    assert M.geometry(3, 3) == (1, 1, 1, [(1, 1)])
    assert M.geometry(5, 7) == (2, 3, 2, [(2, 3), (1, 1)])
    # 65 = 2^6 + 1: seven levels; the height is 1 from the start
    assert M.geometry(130, 2) == (65, 1, 7, [(65, 1), (32, 1), (16, 1), (8, 1), (4, 1), (2, 1), (1, 1)])
    w2, h2, levels, extents = M.geometry(3840, 2160)
    assert (w2, h2, levels) == (1920, 1080, 11)  # 2^10 <= 1920 < 2^11
    assert extents[0] == (1920, 1080) and extents[4] == (120, 67) and extents[9] == (3, 2) and extents[10] == (1, 1)
    w2, h2, levels, extents = M.geometry(16383, 16383)
    assert (w2, h2, levels) == (8191, 8191, 13) and extents[12] == (1, 1)  # the largest side the limits allow
    # the integer count equals the reference's u32(log2f(f32(m))) + 1 on every power of two and its neighbours
    for m in [1, 2, 3, 4, 5, 7, 8, 9, 4095, 4096, 4097, 8191]:
        assert M.geometry(2 * m, 2)[2] == int(np.log2(np.float32(m)).astype(np.float32)) + 1


# ---- the bilinear ------------------------------------------------------------------------------------------------------------------------------
def row(values):
    p = np.array([values], dtype=np.float32)
    return (p, p, p)


def test_both_address_modes_at_minus_one_and_at_the_last_texel():
    # a 2-texel source under a 4-pixel output (the upsample's geometry).  x = 0, k = -1: uv = 0.125, ts = 0.25, p = -0.125, g = -0.25 - 0.5 =
    # -0.75: i = -1, f = 0.25.  x = 3, k = 1: p = 0.875 + 0.25 = 1.125, g = 2.25 - 0.5 = 1.75: i = 1 = size - 1, f = 0.75.  All exact.
    i, f = M.axis_tap(4, 2, -1)
    assert (i[0], f[0]) == (-1, F(0.25))
    i, f = M.axis_tap(4, 2, 1)
    assert (i[3], f[3]) == (1, F(0.75))
    src = row([8.0, 32.0])
    # border: texel -1 is 0: lerp(0, 8, 0.25) = 2;  texel 2 is 0: lerp(32, 0, 0.75) = 32 - 24 = 8
    assert M.bilinear(src, 4, 1, -1, 0, M.BORDER)[0][0, 0] == F(2.0)
    assert M.bilinear(src, 4, 1, 1, 0, M.BORDER)[0][0, 3] == F(8.0)
    # clamp: texel -1 is texel 0, texel 2 is texel 1
    assert M.bilinear(src, 4, 1, -1, 0, M.CLAMP)[0][0, 0] == F(8.0)
    assert M.bilinear(src, 4, 1, 1, 0, M.CLAMP)[0][0, 3] == F(32.0)
    # inside, both modes agree: x = 1, k = 0: g = 0.375 * 2 - 0.5 = 0.25: i = 0, f = 0.25: 8 + 24 * 0.25 = 14
    for mode in (M.BORDER, M.CLAMP):
        assert M.bilinear(src, 4, 1, 0, 0, mode)[0][0, 1] == F(14.0)


def test_the_tap_size_comes_from_the_output_extent():
    # a 5-texel source under a 2-pixel output (an odd side halved): x = 1, k = 2: uv = 0.75, ts = 0.5 (not 1 / 5), p = 1.75, g = 8.75 - 0.5 =
    # 8.25: far outside; k = -1: p = 0.25, g = 1.25 - 0.5 = 0.75: i = 0, f = 0.75
    i, f = M.axis_tap(2, 5, -1)
    assert (i[1], f[1]) == (0, F(0.75))
    assert M.axis_tap(2, 5, 2)[0][1] == 8


def test_nan_and_inf_through_one_tap():
    inf, nan = F(np.inf), F(np.nan)

    def rows(top, bottom):
        p = np.array([top, bottom], dtype=np.float32)
        return (p, p, p)

    # two rows under a one-pixel-high output: g.y = 0.5 * 2 - 0.5 = 0.5: rows 0 and 1, f.y = 0.5.  A 2-texel row under 4 pixels as above.
    # lerp(a, b, t) = a + (b - a) * t: an Inf in b comes through as Inf (t > 0), an Inf in a meets its own negative: NaN.
    src = rows([1.0, 1.0], [inf, 1.0])
    # border, x = 0, k = -1 (i = -1, f = 0.25): top = lerp(0, 1, 0.25) = 0.25, bottom = lerp(0, Inf, 0.25) = Inf, lerp(0.25, Inf, 0.5) = Inf
    assert M.bilinear(src, 4, 1, -1, 0, M.BORDER)[0][0, 0] == inf
    # x = 1, k = 0 (i = 0, f = 0.25): bottom = lerp(Inf, 1, 0.25) = Inf + -Inf = NaN
    assert np.isnan(M.bilinear(src, 4, 1, 0, 0, M.BORDER)[0][0, 1])
    # a NaN texel: x = 0, k = 1: g = 0.375 * 2 - 0.5 = 0.25: texels 0 and 1 of the top row
    assert np.isnan(M.bilinear(rows([nan, 1.0], [1.0, 1.0]), 4, 1, 1, 0, M.CLAMP)[0][0, 0])
    # a NaN texel of weight 0 still poisons: a 4-texel row under 4 pixels, x = 1, k = 0: g = 0.375 * 4 - 0.5 = 1.0: i = 1, f = 0, and
    # lerp(1, NaN, 0) = 1 + NaN * 0 = NaN.  One texel to the left it is out of reach: x = 0: i = 0, f = 0: texels 0 and 1.
    poisoned = rows([1.0, 1.0, nan, 1.0], [1.0, 1.0, nan, 1.0])
    for mode in (M.BORDER, M.CLAMP):
        assert np.isnan(M.bilinear(poisoned, 4, 1, 0, 0, mode)[0][0, 1])
        assert M.bilinear(poisoned, 4, 1, 0, 0, mode)[0][0, 0] == F(1.0)
    # the stores: NaN is the one pattern of each format, Inf stays Inf, a negative is 0 in B10G11R11
    plane = lambda v: np.array([[v]], dtype=np.float32)  # noqa: E731
    assert M.encode([plane(nan), plane(inf), plane(-2.0)], 0)[0, 0] == word(uf11(31, 63), uf11(31, 0), 0)
    assert M.encode([plane(nan), plane(inf), plane(-2.0)], 1)[0, 0].tolist() == [0x7E00, 0x7C00, 0xC000, 0x3C00]


def test_min_of_nan_and_the_clamp_value_is_the_clamp_value():
    # an image of NaN reds: every group's red is NaN, min(NaN, 4) = 4 -- the same D level 0 as an image of reds 64 (group 64, min 4)
    def image(red_half):
        img = np.zeros((8, 8, 4), dtype=np.uint16)
        img[..., 0] = red_half
        return img

    from_nan = M.prefilter(image(0x7E00), 1, 1.0, **DEFAULTS)
    from_big = M.prefilter(image(int(np.float16(64.0).view(np.uint16))), 1, 1.0, **DEFAULTS)
    assert np.array_equal(from_nan, from_big)
    assert from_big[2, 2, 0] != 0 and from_big[2, 2, 0] != 0x7E00


# ---- paper-worked cases ------------------------------------------------------------------------------------------------------------------------
def test_constant_image_below_the_threshold_is_black():
    # 0.5 everywhere: every group is at most 0.5; brightness - threshold <= -0.5, soft = clamp(-0.375, 0, 0.25) = 0, contribution =
    # max(0, negative) / brightness = 0: every texel of D level 0 is 0
    D0 = M.prefilter(constant(12, 10, grey_word(14, 0)), 0, 1.0, **DEFAULTS)
    assert D0.shape == (5, 6) and not D0.any()


def test_constant_image_above_the_threshold():
    # 2.0 everywhere, 16 x 16 -> 8 x 8 (powers of two: every coordinate exact, g = 2 x + 2 k + 0.5).  Interior (x, y in 2 .. 5: texels
    # 2 x - 4 .. 2 x + 5 inside 0 .. 15): every tap is lerp(2, 2, f) = 2, every group (((2 + 2) + 2) + 2) * 0.25 * 1 = 2, min(2, 4) = 2.
    # brightness 2, knee 0.125: soft = clamp(1.125, 0, 0.25) = 0.25 -> 0.015625 / 0.12501 = 0.125; contribution = max(0.125, 1) / 2 = 0.5:
    # prefilter(group) = 1.0, the input's contribution above the threshold.  All five weights are one w (about 1 / 3): the result is
    # 5 w / (5 w + 1e-5) = 1 - 6e-6, just below 1.0, and the pack truncates: exponent field 14, mantissa all ones, 0.9921875 (UF11) and
    # 0.984375 (UF10) -- one truncation below 1.0.
    D0 = M.prefilter(constant(16, 16, grey_word(16, 0)), 0, 1.0, **DEFAULTS)
    assert (D0[2:6, 2:6] == word(uf11(14, 63), uf11(14, 63), (14 << 5) | 31)).all()
    r, g, b = M.decode(D0, 0)
    assert r[3, 3] == F(0.9921875) and b[3, 3] == F(0.984375)
    # an edge pixel (0, 3): the taps at kx = -2 and -1 are wholly outside, so abde, degh and jklm are (0 + 2 + 0 + 2) * 0.25 = 1, on the
    # threshold (contribution 0.03125), and only bcef and efhi are 2: darker.  The corner (0, 0) loses the taps at ky = -2 and -1 as well:
    # only bcef is whole: darker again.
    for ch in (r, g, b):
        assert ch[3, 0] < ch[3, 3] and ch[0, 3] < ch[3, 3] and ch[3, 7] < ch[3, 3] and ch[7, 3] < ch[3, 3]
        assert ch[0, 0] < ch[3, 0] and ch[7, 7] < ch[3, 7] and ch[0, 0] > 0
        assert ch[3, 1] < ch[3, 3]  # x = 1 still loses the kx = -2 taps


def test_single_bright_texel_through_prefilter_and_one_downsample():
    # 32 x 32 black, texel (16, 16) red = 64 (UF11 exponent field 21).  D level 0 is 16 x 16 and every coordinate is exact: the tap (kx, ky)
    # of pixel (x, y) covers texels 2 (x + kx) + {0, 1} with weights 0.5, so it sees the texel when (kx, ky) = (8 - x, 8 - y), as 64 / 4 = 16.
    img = constant(32, 32, 0)
    img[16, 16] = word(uf11(21, 0), 0, 0)
    D0 = M.prefilter(img, 0, 1.0, **DEFAULTS)
    lit = {(8 - kx, 8 - ky) for kx, ky in M.TAPS13.values()}
    assert {(x, y) for y in range(16) for x in range(16) if D0[y, x]} == lit
    assert not (D0 >> 11).any()  # green and blue stay 0
    # A group that holds the tap is 16 * 0.25 = 4 = min(4, 4): weight w = 1 / (1 + 4 * 0.299) = 0.45537, contribution = max(soft, 3) / 4 = 0.75,
    # prefilter(group) * w = 3 w.  A group without it is 0: soft = 0, contribution = max(0, -1) / 1e-5 = 0, weight 1 / (1 + 0) = 1.
    #   (8, 8), tap e, in four groups: 12 w / (4 w + 1 + 1e-5) = 5.46445 / 2.82149 = 1.93673 -> exponent 15, mantissa floor(0.93673 * 64 = 59.95) = 59
    #   (8, 6), tap b, in two groups:  6 w / (2 w + 3 + 1e-5) = 2.73222 / 3.91075 = 0.69864 -> exponent 14, floor(0.39728 * 64 = 25.4) = 25
    #   (6, 6), tap c, and (7, 7), tap k, in one group: 3 w / (w + 4 + 1e-5) = 1.36611 / 4.45538 = 0.30662 -> exponent 13, floor(0.22648 * 64 = 14.5) = 14
    assert D0[8, 8] == uf11(15, 59)
    assert D0[6, 8] == D0[10, 8] == D0[8, 6] == D0[8, 10] == uf11(14, 25)
    assert D0[6, 6] == D0[7, 7] == D0[9, 9] == D0[10, 10] == D0[6, 10] == D0[9, 7] == uf11(13, 14)
    # One downsample, 16 x 16 -> 8 x 8.  Pixel (1, 1) covers texels 2 (1 + k) + {0, 1}: only its tap c = (2, 2) reaches lit texels, (6, 6) and
    # (7, 7), both A = 0.25 * (1 + 14 / 64): c = lerp(lerp(A, 0, 0.5), lerp(0, A, 0.5), 0.5) = A / 2, and the result is c * 0.03125 =
    # (1 + 14 / 64) * 2^-8, exactly: exponent field 7, mantissa 14.  Pixel (0, 0) reaches texels 0 .. 5 only: black.
    D1 = M.downsample(D0, 0, 8, 8)
    assert D1[1, 1] == uf11(7, 14) and D1[0, 0] == 0
    assert D1.shape == (8, 8) and D1[4, 4] != 0
    D, U = M.apply_bloom(img, 0, None)
    assert np.array_equal(D[0], D0) and np.array_equal(D[1], D1) and [d.shape for d in D] == [(16, 16), (8, 8), (4, 4), (2, 2), (1, 1)]
    assert U[4].shape == (1, 1) and U[4][0, 0] == 0 and U[0].shape == (16, 16)


def test_upsample_of_a_constant_level():
    # the 9-tap source is 2.0 everywhere (2 x 2), D level k - 1 is 0.5 everywhere (4 x 4).  Clamp: every tap is lerp(2, 2, f) = 2 and
    # color_sum = (2 * 0.25 + 8 * 0.125) + 8 * 0.0625 = (0.5 + 1) + 0.5 = 2.  radius 0: 0.5 + (2 - 0.5) * 0 = 0.5, D's own texels;
    # radius 1: 0.5 + 1.5 * 1 = 2, the filtered source; radius 0.75: 0.5 + 1.125 = 1.625 = 1 + 40 / 64.
    source, down = constant(2, 2, grey_word(16, 0)), constant(4, 4, grey_word(14, 0))
    assert np.array_equal(M.upsample(source, down, 0, 0.0), down)
    assert np.array_equal(M.upsample(source, down, 0, 1.0), constant(4, 4, grey_word(16, 0)))
    assert np.array_equal(M.upsample(source, down, 0, 0.75), constant(4, 4, grey_word(15, 40)))
    # RGBA16F: the same values as halves, alpha stored as 1.0 whatever the inputs' alpha holds
    h = lambda v: int(np.float16(v).view(np.uint16))  # noqa: E731
    texels = lambda n, v: np.tile(np.array([h(v), h(v), h(v), 0x1234], dtype=np.uint16), (n, n, 1))  # noqa: E731
    assert np.array_equal(M.upsample(texels(2, 2.0), texels(4, 0.5), 1, 0.75), np.tile(np.array([h(1.625)] * 3 + [0x3C00], dtype=np.uint16), (4, 4, 1)))


def test_a_level_one_texel_high():
    # h2 = 1.  Prefilter, an 8 x 2 source: v = 0.5, ts.y = 1, p.y = 0.5 + ky, g.y = 2 p.y - 0.5: ky = 0 gives 0.5 (rows 0 and 1), ky = 1 gives
    # 2.5, ky = -1 gives -1.5: every tap with ky != 0 lies outside and is 0 under the border mode.
    rng = np.random.default_rng(1)
    src = tuple(rng.uniform(0.5, 2.0, (2, 8)).astype(np.float32) for _ in range(3))
    for ky in (-2, -1, 1, 2):
        assert not np.any(M.bilinear(src, 4, 1, 1, ky, M.BORDER)[0])
    assert np.all(M.bilinear(src, 4, 1, 1, 0, M.BORDER)[0][:, :3] > 0)
    # Downsample, a 4 x 1 level under a 2 x 1 output: g.y = ky exactly: i = ky, f = 0.  ky = -1 takes rows -1 (border) and 0 with weight 0:
    # lerp(0, t, 0) = 0; ky = 1 takes rows 1 and 2: 0.
    one_row = tuple(p[:1, :4] for p in src)
    for ky in (-2, -1, 1, 2):
        assert not np.any(M.bilinear(one_row, 2, 1, 0, ky, M.BORDER)[0])
    # Upsample: the same rows clamp to row 0: every vertical neighbour is the row itself
    for ky in (-1, 1):
        assert np.array_equal(M.bilinear(one_row, 8, 1, 1, ky, M.CLAMP)[0], M.bilinear(one_row, 8, 1, 1, 0, M.CLAMP)[0])
    # the whole call on 130 x 2: seven levels of height 1, every byte defined
    img = np.full((2, 130), grey_word(16, 0), dtype=np.uint32)
    D, U = M.apply_bloom(img, 0, None)
    assert [d.shape for d in D] == [(1, 65), (1, 32), (1, 16), (1, 8), (1, 4), (1, 2), (1, 1)] == [u.shape for u in U]
    # the interior of D level 0: only d, e, f are inside: abde = (0 + 0 + 2 + 2) * 0.25 = 1, likewise the other three; jklm = 0: on the
    # threshold, contribution 0.03125: w = 1 / 2 up to rounding: 4 * 0.03125 w / (4 w + 1 + 1e-5) = 0.0625 / 3.00001 = 0.0208333 -> 2^-6 * 1.33333:
    # exponent field 9, mantissa floor(21.33) = 21
    assert D[0][0, 30] == grey_word(9, 21) and (D[0][0, 2:62] == D[0][0, 30]).all()


def test_exposure_scales_the_groups_before_the_clamp():
    # 0.5 everywhere with exposure 4 is 2.0 everywhere with exposure 1 (powers of two: exact); without the flag the buffer is not looked at
    words = np.array([0x7FC00000, np.float32(4.0).view(np.uint32)], dtype=np.uint32)
    a = M.apply_bloom(constant(16, 16, grey_word(14, 0)), 0, words)
    b = M.apply_bloom(constant(16, 16, grey_word(16, 0)), 0, None)
    assert all(np.array_equal(x, y) for x, y in zip(a[0] + a[1], b[0] + b[1]))
    assert M.exposure_of(None) == F(1.0) and M.exposure_of(words) == F(4.0)
