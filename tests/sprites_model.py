"""The checker of oxc_draw_sprites, oxc_pick_sprite and the two host helpers: rules S1 - S7 of include/oxcull.h in numpy binary32, one sprite and
one triangle at a time in the stated order.  It has no bins, no tiles and no lists.  The raster rules come from raster_model (vertex multiply,
snap, setup, cover, depth) and from vsm_draw_model (the clip class and the clipper, the Python copy of oxcull_raster_device.hpp's), the
pack and unpack rules from pixel_rules; none is written a second time here.  CPU only."""
import numpy as np

import pixel_rules as PR
import raster_model as RM
from vsm_draw_model import clip_class, clip_polygon

F = np.float32
VIS, COLOR, ALL = 1, 2, 3
SORT_Y, FLIP_X = 1, 2
EMPTY = 0xFFFFFFFF
B10G11R11, RGBA16F = 0, 1
POSITIONS = ((-0.5, -0.5), (0.5, -0.5), (0.5, 0.5), (0.5, 0.5), (-0.5, 0.5), (-0.5, -0.5))  # 2d_forward.slang:44-45
MAX_SPRITES = 1 << 20


# ---- the host helpers ------------------------------------------------------------------------------------------------------------------------
def pack_sprite(render_flags, position_y, transform_id, material_id, distance):
    """RenderQueue2D::add: (material_id16_ypos16, flags16_distance16, transform_id)."""
    half = lambda v: int(PR.channel_half(F(v)))  # noqa: E731
    return (material_id & 0xFFFF) | (half(position_y) << 16), (render_flags & 0xFFFF) | (half(distance) << 16), transform_id & 0xFFFFFFFF


def half_sort_key(b):
    return (~b & 0xFFFF) if b & 0x8000 else (b | 0x8000)


def sort_key(words) -> int:
    """SpriteGPUData::operator>'s 64-bit key: distance bits above the y key."""
    w0, w1 = int(words[0]), int(words[1])
    return ((w1 >> 16) << 32) | (half_sort_key(w0 >> 16) if w1 & SORT_Y else 0)


def sort_sprites(sprites) -> np.ndarray:
    """Descending by key, equal keys in submission order (stated: stable)."""
    sprites = np.asarray(sprites, np.uint32).reshape(-1, 3)
    order = sorted(range(len(sprites)), key=lambda i: -sort_key(sprites[i]))
    return sprites[order].copy()


# ---- S1 - S4: one sprite ---------------------------------------------------------------------------------------------------------------------
def dequantize_half(h):
    """com::dequantize_half: a denormal half is a signed zero, everything else its value."""
    h = np.asarray(h, np.uint16)
    v = PR.from_half_bits(h)
    return np.where((h & np.uint16(0x7C00)) == 0, np.copysign(F(0.0), v), v).astype(np.float32)


def material_words(materials, index, material_count):
    """(color [4], cutoff) of material `index`; the all-zero Material beyond material_count.  materials: uint16 [M, 28]."""
    rec = np.zeros(28, np.uint16) if index >= material_count else np.asarray(materials, np.uint16).reshape(-1, 28)[index]
    return dequantize_half(rec[0:4]), dequantize_half(rec[9])


def sprite_setup(words, materials, material_count, transforms, transform_count, pv, W, H):
    """S1 - S4 up to the setup: None for a dropped or discarded sprite, else (color, transform_id, [set-up triangles in drawing order])."""
    w0, w1, tid = (int(v) for v in words)
    if tid >= transform_count:
        return None
    color, cutoff = material_words(materials, w0 & 0xFFFF, material_count)
    with np.errstate(invalid="ignore"):
        if color[3] <= cutoff:
            return None
    world16 = np.asarray(transforms, F).reshape(-1, 16)[tid]
    flip = F(-1.0) if (w1 & 0xFFFF) & FLIP_X else F(1.0)
    with np.errstate(all="ignore"):
        clips = [RM.mul_point(pv, RM.mul_point(world16, (F(x) * flip, F(y), F(0.0)))[:3]) for x, y in POSITIONS]
        tris = []
        for t in range(2):
            tri = np.array(clips[3 * t:3 * t + 3], F)
            cls = int(clip_class(tri[None])[0])
            for piece in ([] if cls == 2 else [tri] if cls == 0 else clip_polygon(tri)):
                snapped = RM.snap(piece, W, H)
                if snapped is None:
                    continue
                X, Y, z = snapped
                # cullMode eNone: raster_model.setup orients a negative area (corners 1 and 2 exchanged); a positive area given with those
                # corners exchanged comes back in its own order
                s = RM.setup(snapped, W, H) or RM.setup(([X[0], X[2], X[1]], [Y[0], Y[2], Y[1]], [z[0], z[2], z[1]]), W, H)
                if s is not None:
                    tris.append(s)
    return color, tid, tris


def fragments(t, W, H):
    """(kept [H, W] bool, depth [H, W] binary32) of one set-up triangle: covered and depth in (0, 1], raster_model's own draw."""
    image = np.zeros((H, W), np.uint64)
    RM.draw_triangle(t, 1, image)
    return image != 0, (image >> np.uint64(32)).astype(np.uint32).view(np.float32)


# ---- S5 - S7 ---------------------------------------------------------------------------------------------------------------------------------
def decode(color, fmt):
    if fmt == B10G11R11:
        return list(PR.unpack_b10g11r11(color))
    return [PR.from_half_bits(color[..., k]) for k in range(4)]


def encode(ch, fmt, like):
    if fmt == B10G11R11:
        return PR.pack_b10g11r11(ch[0], ch[1], ch[2]).reshape(like.shape).astype(np.uint32)
    return np.stack([PR.channel_half(c) for c in ch], axis=-1).astype(np.uint16)


@np.errstate(all="ignore")
def draw(sprites, materials, transforms, pv, W, H, depth, vis=None, color=None, stages=ALL, clear=True, source_format=B10G11R11, first_sprite=0,
         sprite_count=None, material_count=None, transform_count=None, stats=None, requantize=True) -> dict:
    """oxc_draw_sprites.  sprites uint32 [n, 3], materials uint16 [M, 28], transforms float32 [T, 16]; depth float32 [H, W]; vis uint32 [H, W]
    (VIS); color uint32 [H, W] or uint16 [H, W, 4] (COLOR).  Returns the images after the call.  stats["blends"][k]: how often each pixel
    took a fragment of sprite k in the last stage run.  requantize=False keeps the colour in binary32 between fragments and encodes once at
    the end -- NOT the rule; the tests use it to show that a frame can tell the difference."""
    sprites = np.asarray(sprites, np.uint32).reshape(-1, 3)
    sprite_count = len(sprites) - first_sprite if sprite_count is None else sprite_count
    material_count = len(np.asarray(materials).reshape(-1, 28)) if material_count is None else material_count
    transform_count = len(np.asarray(transforms).reshape(-1, 16)) if transform_count is None else transform_count
    out = dict(depth=np.array(depth, F))
    if stages & VIS:
        out["vis"] = np.full((H, W), EMPTY, np.uint32) if clear else np.array(vis, np.uint32)
    if stages & COLOR:
        out["color"] = np.array(color)
    setups = [sprite_setup(sprites[first_sprite + k], materials, material_count, transforms, transform_count, pv, W, H) for k in range(sprite_count)]
    pieces = [None if s is None else [fragments(t, W, H) for t in s[2]] for s in setups]
    for stage in (VIS, COLOR):
        if not stages & stage:
            continue
        ch = decode(out["color"], source_format) if stage == COLOR else None
        touched = np.zeros((H, W), bool)  # a pixel no fragment reached keeps its stored word, whatever its bits
        blends = {}
        for k, s in enumerate(setups):
            if s is None:
                continue
            rgba, tid, _ = s
            a, oma = rgba[3], F(1.0) - rgba[3]
            count = np.zeros((H, W), np.int32)
            for kept, d in pieces[k]:
                passed = kept & (d >= out["depth"])  # S5: false for a NaN on either side
                out["depth"] = np.where(passed, d, out["depth"]).astype(np.float32)
                count += passed
                if stage == VIS:
                    out["vis"] = np.where(passed, np.uint32(tid), out["vis"]).astype(np.uint32)
                    continue
                new = [rgba[c] * a + ch[c] * oma for c in range(3)] + ([a + ch[3] * oma] if source_format == RGBA16F else [])  # S6
                ch = [np.where(passed, n, o).astype(np.float32) for n, o in zip(new, ch)]
                touched |= passed
                if requantize:
                    ch = decode(encode(ch, source_format, out["color"]), source_format)
            blends[k] = count
        if stage == COLOR:
            enc = encode(ch, source_format, out["color"])
            out["color"] = np.where(touched if enc.ndim == 2 else touched[..., None], enc, out["color"]).astype(enc.dtype)
        if stats is not None:
            stats["blends"] = blends
    return out


def pick(vis, x, y) -> int:
    """mouse_picking_2d.slang: the texel itself."""
    return int(np.asarray(vis, np.uint32)[y, x])
