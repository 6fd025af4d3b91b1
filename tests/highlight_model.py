"""The checker of oxc_pick_transform and oxc_apply_highlight (include/oxcull.h, rules P, M1 - M2, H1 - H5): numpy in binary32, the shared
numeric rules from pixel_rules.  The mask and both dilations are computed the Slang's way -- a float image of 0.0 and 1.0, a maximum over
clamped taps, edge_intensity > 0.01 -- and never on bits, so that the equivalences the header claims in H1 and H2 are tested by every
comparison with the library and not assumed."""
from __future__ import annotations

import numpy as np

from pixel_rules import F, pack_unorm4x8, pow_rule, srgb_decode, srgb_encode

EMPTY = 0xFFFFFFFF
TERRAIN_INSTANCE = 0xFFFFFE
MASK, COMPOSITE, ALL = 1, 2, 3
RGBA8_SRGB, BGRA8_SRGB, RGBA8_UNORM = 0, 1, 2
OUTLINE = (1.0, 0.53, 0.0, 1.0)   # ViewportPanel.cpp:1307


# ---- P, M1, M2 ------------------------------------------------------------------------------------------------------------------------------
def texel_transform(vis, meshlet_instance_count, meshlet_instances, mesh_instances, terrain_transform_index) -> np.ndarray:
    """P: the transform index behind every texel of `vis` (any shape), as uint32."""
    vis = np.asarray(vis, dtype=np.uint32)
    instance = (vis >> np.uint32(8)).astype(np.int64)
    known = (vis != EMPTY) & (instance != TERRAIN_INSTANCE) & (instance < meshlet_instance_count)
    out = np.zeros(vis.shape, np.uint32)   # the all-zero MeshInstance beyond the count
    if known.any():
        chain = np.asarray(meshlet_instances, dtype=np.uint32).reshape(-1, 2)[instance[known], 0]
        out[known] = np.asarray(mesh_instances, dtype=np.uint32).reshape(-1, 5)[chain, 3]
    out[instance == TERRAIN_INSTANCE] = np.uint32(terrain_transform_index & 0xFFFFFFFF)
    out[vis == EMPTY] = EMPTY
    return out


def pick(vis, x, y, **records) -> int:
    return int(texel_transform(np.asarray(vis)[y, x], **records))


def selection_mask(vis, transform_indices, **records) -> np.ndarray:
    """M1: bool [H, W]."""
    t = texel_transform(vis, **records)
    listed = np.asarray(transform_indices, dtype=np.uint32).reshape(-1)
    listed = listed[listed != EMPTY]
    return (np.asarray(vis, dtype=np.uint32) != EMPTY) & (t != EMPTY) & np.isin(t, listed)


def mask_words(mask) -> np.ndarray:
    """M2: uint64 [H, ceil(W / 64)], bit x % 64 of word x / 64; the bits past W are zero."""
    H, W = mask.shape
    words = (W + 63) // 64
    padded = np.zeros((H, words * 64), np.uint64)
    padded[:, :W] = mask
    return (padded.reshape(H, words, 64) << np.arange(64, dtype=np.uint64)).sum(axis=-1, dtype=np.uint64)


def mask_of_words(words, W) -> np.ndarray:
    """The composite's reading of mask_bits: bool [H, W]; the bits past W are ignored."""
    words = np.asarray(words).view(np.uint64)
    bits = (words[:, :, None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)
    return bits.reshape(words.shape[0], -1)[:, :W].astype(bool)


def mask_image(mask) -> np.ndarray:
    return np.where(mask, np.uint8(255), np.uint8(0))


# ---- H1 - H5 --------------------------------------------------------------------------------------------------------------------------------
def srgb_to_linear(c) -> np.ndarray:
    """common/color.slang:75-77 as written: a strict comparison, the absolute value of the base."""
    c = np.atleast_1d(np.asarray(c, dtype=np.float32))
    with np.errstate(all="ignore"):
        return np.where(c < F(0.04045), c / F(12.92), pow_rule(np.abs(c + F(0.055)) / F(1.055), F(2.4))).astype(np.float32)


def decode(color, color_format):
    """H3: (r, g, b, a) in binary32 of the u32 image."""
    w = np.asarray(color).view(np.uint32)
    byte = [(w >> np.uint32(8 * k)) & np.uint32(0xFF) for k in range(4)]
    if color_format == BGRA8_SRGB:
        byte[0], byte[2] = byte[2], byte[0]
    rgb = [srgb_decode(b) if color_format != RGBA8_UNORM else b.astype(np.float32) / F(255.0) for b in byte[:3]]
    return rgb + [byte[3].astype(np.float32) / F(255.0)]


def store(rgba, color_format) -> np.ndarray:
    """oxc_apply_tonemap step 11."""
    r, g, b = (srgb_encode(c) for c in rgba[:3]) if color_format != RGBA8_UNORM else rgba[:3]
    if color_format == BGRA8_SRGB:
        r, b = b, r
    return pack_unorm4x8(r, g, b, rgba[3])


def dilate(mask_f, radius, axis) -> np.ndarray:
    """One pass of the separable dilation as the Slang runs it: r = max(1, radius), the maximum of the taps -r .. r clamped to the image."""
    r = max(1, int(radius))
    n = mask_f.shape[axis]
    at = np.arange(n)
    out = np.zeros_like(mask_f)
    for d in range(-r, r + 1):
        out = np.maximum(out, np.take(mask_f, np.clip(at + d, 0, n - 1), axis=axis))
    return out


@np.errstate(all="ignore")
def composite(mask, depth, color, color_format=RGBA8_SRGB, outline_color=OUTLINE, dilate_radius=8, outline_width=5, occluded_mode=2, stats=None) -> np.ndarray:
    """H1 - H5: the u32 image the composite stores.  `stats` receives the boolean images `edge` and `occluded` and the class counts
    `selected`, `edge_occluded`, `edge_free`, `plain` (no edge) and `translucent` (no edge, alpha byte below 255)."""
    mask_f = np.where(mask, F(1.0), F(0.0)).astype(np.float32)
    max_mask = dilate(dilate(mask_f, dilate_radius, 1), outline_width, 0)
    edge = (max_mask - mask_f) > F(0.01)
    back = decode(color, color_format)
    depth = np.asarray(depth, dtype=np.float32)
    occluded = depth > F(0.00001)
    oc = np.asarray(outline_color, dtype=np.float32)
    final_outline = list(srgb_to_linear(oc[:3])) + [oc[3]]
    src = []
    for ch in range(4):
        o = np.full(depth.shape, final_outline[ch], np.float32)
        if occluded_mode == 0:
            lit = np.where(occluded, back[ch], o)
        elif occluded_mode == 1:
            lit = np.where(occluded, back[ch] + (o - back[ch]) * F(0.35), o)
        else:
            lit = o
        src.append(np.where(edge, lit, back[ch]).astype(np.float32))
    out = [src[ch] * src[3] for ch in range(3)] + [src[3] + (F(1.0) - src[3])]
    if stats is not None:
        alpha = np.asarray(color).view(np.uint32) >> np.uint32(24)
        stats.update(edge=edge, occluded=occluded, selected=int(np.count_nonzero(mask)), edge_occluded=int((edge & occluded).sum()),
                     edge_free=int((edge & ~occluded).sum()), plain=int((~edge).sum()), translucent=int((~edge & (alpha != 255)).sum()))
    return store(out, color_format)
