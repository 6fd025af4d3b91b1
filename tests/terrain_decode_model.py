"""The numpy checker of oxc_decode_terrain: steps D1-D8 of its header block in include/oxcull.h.  Every binary32 operation is one numpy float32
operation in the order the header states.  It joins rules that already have a Python copy and adds none of its own for them: the normal
halves and the flushing dequantize_half come from visbuffer_decode_model and smoothstep from terrain_maps_model, whose passes define them;
the unsaturated sRGB encode, unorm8, lerp, the clamp bilinear's axis, unproject, vec3_to_oct, saturate and the B10G11R11 pack from pixel_rules.  Images are numpy arrays in the header's layouts: vis uint32 [H, W], depth float32 [H, W], normalmap uint16 [h, w, 2],
splatmap uint32 [h, w], materials uint8 [56 * material_count], hit uint32 [4]; the outputs as visbuffer_decode_model.decode returns them.
`decode` returns new arrays and leaves its arguments unchanged.  `counts`, when given, receives how often each class and branch was taken
(COUNTS); `pre`, when given, the values before quantisation at the terrain pixels."""
from __future__ import annotations

import dataclasses

import numpy as np

from pixel_rules import axis_clamp, count, lerp, normalize, pack_b10g11r11, pack_unorm4x8, saturate, srgb_unorm_encode, unorm8, unproject, vec3_to_oct
from terrain_maps_model import smoothstep
from visbuffer_decode_model import IMAGES, MATERIAL_BYTES, dequantize_half_flush, normal_half

F = np.float32
TERRAIN_INSTANCE_ID = 0xFFFFFE
TERRAIN_TEXEL = np.uint32(TERRAIN_INSTANCE_ID << 8)
INVALID_LAYER = 0xFFFFFFFF
RING_COLOUR = (F(1.0), F(0.55), F(0.1))
SRGB_KNEE = F(0.0031308)
COUNTS = (("pixels_not_terrain", "pixels_terrain", "weight_sum_kept", "weight_sum_default", "ring_off", "ring_invalid_hit", "ring_on", "ring_pixels_touched",
           "srgb_linear", "srgb_power") + tuple(f"layer{i}_{k}" for i in range(4) for k in ("skipped", "invalid", "out_of_range", "valid")))


@dataclasses.dataclass
class Terrain:
    """GPU::TerrainData (scene.slang:634-647) with the record's own defaults."""
    world_min: tuple = (0.0, 0.0)
    world_size: tuple = (1.0, 1.0)
    inv_world_size: tuple = (1.0, 1.0)
    patch_count: tuple = (1, 1)
    base_height: float = 0.0
    height_scale: float = 1.0
    target_edge_pixels: float = 16.0
    max_tessellation: float = 64.0
    layer_tiling: float = 8.0
    triplanar_begin: float = 0.5
    layer_material_indices: tuple = (INVALID_LAYER,) * 4
    brush_radius: float = 0.0


def is_terrain(vis) -> np.ndarray:
    return (np.asarray(vis).view(np.uint32) >> np.uint32(8)) == np.uint32(TERRAIN_INSTANCE_ID)


# ---- D2 - D4 -------------------------------------------------------------------------------------------------------------------------------------
@np.errstate(all="ignore")
def world_of(ipv, xs, ys, W: int, H: int, depth):
    """D2: the world position of pixels (xs, ys) with their depth texels."""
    u, v = (xs.astype(np.float32) + F(0.5)) / F(W), (ys.astype(np.float32) + F(0.5)) / F(H)
    return unproject(np.asarray(ipv, np.float32), u, v, np.asarray(depth, np.float32))


@np.errstate(all="ignore")
def sample_maps(T: Terrain, normalmap, splatmap, wx, wz):
    """D3's two samples: (n.x, n.y, [w0, w1, w2, w3]) by the clamp bilinear of step B3."""
    h, w = splatmap.shape
    u = ((wx - F(T.world_min[0])) * F(T.inv_world_size[0])).astype(np.float32)
    v = ((wz - F(T.world_min[1])) * F(T.inv_world_size[1])).astype(np.float32)
    x0, x1, fx = axis_clamp(u, w)
    y0, y1, fy = axis_clamp(v, h)
    bil = lambda t: lerp(lerp(t[y0, x0], t[y0, x1], fx), lerp(t[y1, x0], t[y1, x1], fx), fy)  # noqa: E731
    nm = np.ascontiguousarray(normalmap).view(np.float16).astype(np.float32)
    sp = np.asarray(splatmap, np.uint32)
    channels = [((sp >> np.uint32(8 * k)) & np.uint32(0xFF)).astype(np.float32) / F(255.0) for k in range(4)]
    return bil(nm[..., 0]), bil(nm[..., 1]), [bil(c) for c in channels]


@np.errstate(all="ignore")
def geometric_normal_of(nx, ny):
    return normalize((nx, np.sqrt(saturate(F(1.0) - (nx * nx + ny * ny))), ny))


@np.errstate(all="ignore")
def weights_of(w, counts=None):
    """D4."""
    weight_sum = ((w[0] + w[1]) + w[2]) + w[3]
    kept = weight_sum > F(1e-4)
    count(counts, "weight_sum_kept", kept.sum())
    count(counts, "weight_sum_default", (~kept).sum())
    return [np.where(kept, w[k] / weight_sum, F(1.0 if k == 0 else 0.0)).astype(np.float32) for k in range(4)], weight_sum


# ---- D5 ------------------------------------------------------------------------------------------------------------------------------------------
def layer_factors(T: Terrain, materials, material_count: int):
    """Per layer (kind, the nine factors albedo rgba, emissive rgb, roughness, metallic as the record orders its halves)."""
    out = []
    recs = None if materials is None or not material_count else np.ascontiguousarray(materials).view(np.uint16).reshape(-1, MATERIAL_BYTES // 2)
    for i in range(4):
        index = int(T.layer_material_indices[i]) & 0xFFFFFFFF
        if index == INVALID_LAYER:
            out.append(("invalid", None))
        elif index >= int(material_count):
            out.append(("out_of_range", dequantize_half_flush(np.zeros(9, np.uint16))))
        else:
            out.append(("valid", dequantize_half_flush(recs[index, :9])))
    return out


@np.errstate(all="ignore")
def blend_layers(T: Terrain, weights, materials, material_count: int, counts=None) -> dict:
    n = len(weights[0])
    z = lambda: np.zeros(n, np.float32)  # noqa: E731
    s = {"albedo": [z() for _ in range(4)], "emissive": [z() for _ in range(3)], "metallic": z(), "roughness": z(), "occlusion": z()}
    add = lambda acc, factor, weight, on: np.where(on, acc + F(factor) * weight, acc).astype(np.float32)  # noqa: E731
    for i, (kind, f) in enumerate(layer_factors(T, materials, material_count)):
        weight = weights[i]
        skip = weight <= F(0.0)
        on = ~skip
        count(counts, f"layer{i}_skipped", skip.sum())
        count(counts, f"layer{i}_{kind}", on.sum())
        if kind == "invalid":
            f = [1.0, 1.0, 1.0, 1.0, None, None, None, 1.0, 0.0]
        for k in range(4):
            s["albedo"][k] = add(s["albedo"][k], f[k], weight, on)
        if kind != "invalid":
            for k in range(3):
                s["emissive"][k] = add(s["emissive"][k], f[4 + k], weight, on)
        s["metallic"] = add(s["metallic"], f[8], weight, on)
        s["roughness"] = add(s["roughness"], f[7], weight, on)
        s["occlusion"] = np.where(on, s["occlusion"] + weight, s["occlusion"]).astype(np.float32)
    return s


# ---- D7 ------------------------------------------------------------------------------------------------------------------------------------------
def ring_width_of(brush_radius) -> np.float32:
    return np.fmax(F(brush_radius) * F(0.02), F(0.05))


@np.errstate(all="ignore")
def ring_of(T: Terrain, hit, wx, wz):
    """ring per pixel; the caller has checked brush_radius > 0 and hit.valid."""
    hp = np.asarray(hit, np.uint32).view(np.float32)
    dx, dz = wx - hp[0], wz - hp[2]
    distance = np.sqrt(dx * dx + dz * dz)
    return (F(1.0) - smoothstep(F(0.0), ring_width_of(T.brush_radius), np.abs(distance - F(T.brush_radius)))).astype(np.float32)


# ---- the call ------------------------------------------------------------------------------------------------------------------------------------
@np.errstate(all="ignore")
def decode(T: Terrain, vis, depth, inv_projection_view, normalmap, splatmap, materials=None, material_count: int = 0, hit=None, init: dict = None,
           counts=None, pre: dict = None) -> dict:
    """-> {"albedo", "normal", "emissive", "mro"}: `init` (zeros when None) with the terrain pixels written."""
    vis = np.ascontiguousarray(vis).view(np.uint32)
    H, W = vis.shape
    img = {"albedo": np.zeros((H, W), np.uint32), "normal": np.zeros((H, W, 4), np.uint16), "emissive": np.zeros((H, W), np.uint32), "mro": np.zeros((H, W), np.uint32)}
    if init is not None:
        img = {k: np.array(init[k], dtype=img[k].dtype).reshape(img[k].shape) for k in IMAGES}
    # D1
    terrain = is_terrain(vis)
    ys, xs = np.nonzero(terrain)
    count(counts, "pixels_not_terrain", (~terrain).sum())
    count(counts, "pixels_terrain", terrain.sum())
    ring_state = "ring_off" if not F(T.brush_radius) > F(0.0) else ("ring_on" if int(np.asarray(hit, np.uint32)[3]) != 0 else "ring_invalid_hit")
    count(counts, ring_state)
    if len(ys) == 0:
        return img
    # D2 - D5
    wx, wy, wz = world_of(inv_projection_view, xs, ys, W, H, np.asarray(depth, np.float32)[ys, xs])
    nx, ny, w = sample_maps(T, np.asarray(normalmap), np.asarray(splatmap), wx, wz)
    geometric = geometric_normal_of(nx, ny)
    weights, weight_sum = weights_of(w, counts)
    s = blend_layers(T, weights, materials, material_count, counts)
    # D6
    shading = normalize(geometric)
    # D7
    ring = None
    if ring_state == "ring_on":
        ring = ring_of(T, hit, wx, wz)
        count(counts, "ring_pixels_touched", (ring > 0).sum())
        for k in range(3):
            s["albedo"][k] = lerp(s["albedo"][k], RING_COLOUR[k], ring)
    # D8
    for k in range(3):
        linear = s["albedo"][k] <= SRGB_KNEE
        count(counts, "srgb_linear", linear.sum())
        count(counts, "srgb_power", (~linear).sum())
    a = s["albedo"]
    img["albedo"][ys, xs] = unorm8(srgb_unorm_encode(a[0])) | (unorm8(srgb_unorm_encode(a[1])) << np.uint32(8)) | (unorm8(srgb_unorm_encode(a[2])) << np.uint32(16)) | (unorm8(a[3]) << np.uint32(24))
    sx, sy = vec3_to_oct(shading)
    gx, gy = vec3_to_oct(geometric)
    img["normal"][ys, xs] = np.stack([normal_half(sx), normal_half(sy), normal_half(gx), normal_half(gy)], axis=-1)
    img["emissive"][ys, xs] = pack_b10g11r11(*s["emissive"])
    img["mro"][ys, xs] = pack_unorm4x8(s["metallic"], s["roughness"], s["occlusion"], np.zeros_like(s["occlusion"]))
    if pre is not None:
        pre.update(ys=ys, xs=xs, world=(wx, wy, wz), n=(nx, ny), weight_sum=weight_sum, weights=weights, geometric=geometric, shading=shading, ring=ring,
                   albedo=a, emissive=s["emissive"], metallic=s["metallic"], roughness=s["roughness"], occlusion=s["occlusion"])
    return img
