"""tests/highlight_model.py, the checker of oxc_pick_transform and oxc_apply_highlight, without a GPU: against a plain binary64 transcription
of the three highlight shaders, against the golden fixture, the alpha-255 round trip the kernel's copy path rests on, and the library's
exports."""
import dataclasses
import math

import numpy as np

import highlight_frames as HF
import highlight_model as HM
from oxylus_amd import lib as L

F = np.float32


def test_library_exports_the_two_entry_points(liboxcull):
    for name in ("oxc_pick_transform", "oxc_apply_highlight"):
        assert name in L.EXPORTS and hasattr(liboxcull, name)


# ---- a binary64 transcription of highlight_mask, highlight_dilate_horizontal and highlight_composite, pixel by pixel ------------------------------
def _to_linear64(c):
    return c / 12.92 if c < 0.04045 else (abs(c + 0.055) / 1.055) ** 2.4


def _decode64(byte, srgb):
    c = byte / 255.0
    return (c / 12.92 if c <= 0.04045 else ((c + 0.055) / 1.055) ** 2.4) if srgb else c


def _encode64(v, srgb):
    """(the byte, the distance of the rounded value from the rounding threshold)."""
    v = min(max(v, 0.0), 1.0)
    if srgb:
        v = v * 12.92 if v <= 0.0031308 else 1.055 * v ** (1.0 / 2.4) - 0.055
    s = min(max(v, 0.0), 1.0) * 255.0 + 0.5
    return int(math.floor(s)), min(s - math.floor(s), math.ceil(s) - s) if s != math.floor(s) else 0.0


def transcription(f: HF.Frame):
    """(u32 image, per-pixel least distance from a rounding threshold)."""
    W, H = f.extent
    selected = [int(v) for v in f.selected if int(v) != HM.EMPTY]
    mask = np.zeros((H, W))
    for y in range(H):
        for x in range(W):
            texel = int(f.vis[y, x])
            if texel == HM.EMPTY:
                continue
            if texel >> 8 == HM.TERRAIN_INSTANCE:
                t = f.terrain_transform_index
            elif texel >> 8 >= f.meshlet_instance_count:
                t = 0
            else:
                t = int(f.mesh_instances[int(f.meshlet_instances[texel >> 8, 0]), 3])
            mask[y, x] = 1.0 if t != HM.EMPTY and t in selected else 0.0
    rx, ry = max(1, f.dilate_radius), max(1, f.outline_width)
    horizontal = np.zeros((H, W))
    for y in range(H):
        for x in range(W):
            horizontal[y, x] = max(mask[y, min(max(x + d, 0), W - 1)] for d in range(-rx, rx + 1))
    srgb = f.color_format != HM.RGBA8_UNORM
    order = (2, 1, 0) if f.color_format == HM.BGRA8_SRGB else (0, 1, 2)
    outline = [_to_linear64(float(F(c))) for c in f.outline_color[:3]] + [float(F(f.outline_color[3]))]
    out, margin = np.zeros((H, W), np.uint32), np.ones((H, W))
    for y in range(H):
        for x in range(W):
            max_mask = max(horizontal[min(max(y + d, 0), H - 1), x] for d in range(-ry, ry + 1))
            word = int(f.color[y, x])
            back = [_decode64((word >> (8 * order[c])) & 0xFF, srgb) for c in range(3)] + [(word >> 24) / 255.0]
            final = back
            if max_mask - mask[y, x] > 0.01:
                occluded = float(f.depth[y, x]) > float(F(0.00001))
                if occluded and f.occluded_mode == 0:
                    final = back
                elif occluded and f.occluded_mode == 1:
                    final = [b + (o - b) * 0.35 for b, o in zip(back, outline)]
                else:
                    final = outline
            blended = [final[c] * final[3] for c in range(3)] + [final[3] + (1.0 - final[3])]
            stored = 0
            for c in range(3):
                byte, dist = _encode64(blended[c], srgb)
                stored |= byte << (8 * order[c])
                margin[y, x] = min(margin[y, x], dist)
            byte, dist = _encode64(blended[3], False)
            out[y, x] = stored | (byte << 24)
            margin[y, x] = min(margin[y, x], dist)
    return out, margin, mask.astype(bool)


def test_checker_against_the_binary64_transcription():
    """Every format and mode on a 33 x 19 frame.  The binary32 checker and the binary64 transcription may differ only where a stored value
    lies within 1e-4 of a rounding threshold; such pixels are left out, and they are few.  Most of them are exact ties: the outline's blue is
    0.0, so mode 1 stores byte * 0.65 + 0.5 in format 2, an integer for bytes 10, 30, 50 .."""
    base = HF.frame((33, 19), selected=(11, 13, HF.TERRAIN_TRANSFORM))
    for fmt in HF.FORMATS:
        for mode in HF.MODES:
            f = dataclasses.replace(base, color_format=fmt, occluded_mode=mode, dilate_radius=3, outline_width=2)
            want, margin, mask = transcription(f)
            st = {}
            got = HF.want_composite(f, stats=st)
            assert np.array_equal(HF.want_mask(f), mask)
            clear = margin > 1e-4
            assert clear.mean() > 0.9 and np.array_equal(got[clear], want[clear]), (fmt, mode, np.argwhere(clear & (got != want))[:4])
            assert st["selected"] > 20 and st["edge_occluded"] > 10 and st["edge_free"] > 3 and st["translucent"] > 10 and (clear & st["edge"]).sum() > 10


def test_golden_fixture():
    g = np.load(HF.GOLDEN)
    f = HF.golden_frame()
    for name in ("vis", "depth", "color", "meshlet_instances", "mesh_instances", "selected"):
        assert np.array_equal(np.asarray(getattr(f, name)).view(np.uint32), g["in_" + name].view(np.uint32)), name
    mask = HF.want_mask(f)
    assert np.array_equal(HM.mask_words(mask), g["mask_bits"]) and np.array_equal(HM.mask_image(mask), g["mask_attachment"])
    assert 0 < mask.sum() < mask.size
    for fmt in HF.FORMATS:
        for mode in HF.MODES:
            st = {}
            got = HF.want_composite(dataclasses.replace(f, color_format=fmt, occluded_mode=mode), mask, st)
            assert np.array_equal(got, g[f"dst_format{fmt}_mode{mode}"]), (fmt, mode)
            assert st["edge_occluded"] and st["edge_free"] and st["plain"]


def test_an_opaque_pixel_off_the_outline_comes_back_with_its_bytes():
    """H5: alpha byte 255, every value of a channel, every format: decode, blend with alpha 1.0 and store return the word.  The kernel copies
    such words on this ground."""
    v = np.arange(256, dtype=np.uint32)
    words = np.stack([v | (v[::-1] << np.uint32(8)) | (((v * 7 + 3) & 0xFF) << np.uint32(16)) | np.uint32(0xFF000000),
                      v * np.uint32(0x010101) | np.uint32(0xFF000000)]).astype(np.uint32)
    assert all(set(((words >> np.uint32(8 * c)) & 0xFF).reshape(-1).tolist()) == set(range(256)) for c in range(3))
    nothing = np.zeros(words.shape, bool)
    for fmt in HF.FORMATS:
        for mode in HF.MODES:
            got = HM.composite(nothing, np.ones(words.shape, np.float32), words, color_format=fmt, occluded_mode=mode)
            assert np.array_equal(got, words), fmt


def test_a_translucent_pixel_is_premultiplied_onto_black():
    """alpha 128 of 255: colour * alpha, alpha + (1 - alpha) = 1."""
    word = np.array([[0x80FF8000]], np.uint32)
    got = int(HM.composite(np.zeros((1, 1), bool), np.zeros((1, 1), np.float32), word, color_format=HM.RGBA8_UNORM)[0, 0])
    a = F(128) / F(255)
    assert got == (0xFF000000 | (int(np.floor(F(1.0) * a * F(255) + F(0.5))) << 16) | (int(np.floor(F(128) / F(255) * a * F(255) + F(0.5))) << 8))


def test_outline_colour_rule():
    """srgb_to_linear as written: strict below 0.04045, the absolute value of the base; a NaN's log2 is -Inf (pow gives 0), Inf stays Inf."""
    below = np.nextafter(F(0.04045), F(0))
    got = HM.srgb_to_linear([0.0, below, F(0.04045), 1.0, -1.0, np.nan, np.inf])
    assert got[0] == 0 and got[1] == below / F(12.92) and got[2] != F(0.04045) / F(12.92) and abs(got[2] - 0.04045 / 12.92) < 1e-6
    assert got[3] == 1.0 and got[4] == F(-1.0) / F(12.92) and got[5] == 0.0 and got[6] == np.inf


def test_mask_words_and_their_reading():
    rng = np.random.default_rng(1)
    for W in (1, 63, 64, 65, 129):
        mask = rng.random((3, W)) < 0.5
        words = HM.mask_words(mask)
        assert words.shape == (3, (W + 63) // 64) and np.array_equal(HM.mask_of_words(words, W), mask)
        assert W % 64 == 0 or not (words[:, -1] >> np.uint64(W % 64)).any()
        if W % 64:  # the composite ignores what a caller left past the width
            words[:, -1] |= ~np.uint64(0) << np.uint64(W % 64)
            assert np.array_equal(HM.mask_of_words(words, W), mask)


def test_transform_rule():
    f = HF.golden_frame()
    vis = np.array([HM.EMPTY, HF.TERRAIN_TEXEL | 9, 0x00000105, (4 << 8) | 1, (f.meshlet_instance_count << 8), 0x7FFFFF00], np.uint32)
    got = HM.texel_transform(vis, **f.records)
    assert got.tolist() == [HM.EMPTY, HF.TERRAIN_TRANSFORM, 11, HM.EMPTY, 0, 0]
    # a record whose transform is ~0u is never selected, nor is an empty texel, whatever the list holds
    mask = HM.selection_mask(vis.reshape(1, -1), [HM.EMPTY, 0, 11, 11], **f.records)
    assert mask.tolist() == [[False, False, True, False, True, True]]
