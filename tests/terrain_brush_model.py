"""The numpy checker of oxc_apply_terrain_brush: steps B1-B10 of its header block in include/oxcull.h.  Every binary32 operation is one numpy
float32 operation in the order the header states.  It joins rules that already have a Python copy and adds none of its own for them:
noised (T3) and the unorm16 load come from terrain_maps_model, whose pass defines them; lerp, clamp, the unorm8 store, the clamp bilinear's
axis, saturate, the saturating conversions and pow from pixel_rules.  Images are numpy arrays in the header's layouts: heightmap uint16 [H, W], height_edit float32 [H, W], splat_edit uint32 [H, W],
hit and region uint32 [4].  A stage returns new arrays and leaves its arguments unchanged.  `counts`, when given, receives how often each
branch was taken: miss_clip, miss_parallel, miss_no_crossing, hit_step (a dict: march step -> hits), texels_outside, texels_zero_falloff,
texels_written and mode_<name> (texels written per mode)."""
from __future__ import annotations

import dataclasses

import numpy as np

from pixel_rules import axis_clamp, clamp, count, cvt_i32_sat, cvt_u32_sat, lerp, pow_rule, saturate, unorm8
from terrain_maps_model import load_unorm16, noised

F = np.float32
TRACE, APPLY, BOTH = 1, 2, 3
RAISE, SMOOTH, FLATTEN, NOISE, PAINT_LAYER = range(5)
MODE_NAMES = ("raise", "smooth", "flatten", "noise", "paint_layer")
MARCH_STEPS, REFINE_STEPS = 512, 24
COUNTS = ("miss_clip", "miss_parallel", "miss_no_crossing", "texels_outside", "texels_zero_falloff", "texels_written") + tuple("mode_" + m for m in MODE_NAMES)


@dataclasses.dataclass
class Params:
    """GPU::TerrainBrushParams (scene.slang:606-621)."""
    ray_origin: tuple = (0.0, 0.0, 0.0)
    radius_texels: float = 0.0
    ray_direction: tuple = (0.0, -1.0, 0.0)
    strength: float = 0.0
    resolution: tuple = (1, 1)
    world_min: tuple = (0.0, 0.0)
    world_size: tuple = (1.0, 1.0)
    inv_world_size: tuple = (1.0, 1.0)
    patch_count: tuple = (1, 1)
    base_height: float = 0.0
    height_scale: float = 1.0
    falloff: float = 1.0
    flatten_height: float = 0.0
    mode: int = RAISE
    layer: int = 0


def _f3(v):
    return [F(c) for c in v]


# ---- B1 - B3 -------------------------------------------------------------------------------------------------------------------------------------
@np.errstate(all="ignore")
def direction_of(B: Params):
    x, y, z = _f3(B.ray_direction)
    ln = np.sqrt((x * x + y * y) + z * z)
    return x / ln, y / ln, z / ln


@np.errstate(all="ignore")
def clip_to_footprint(B: Params, origin, direction, counts=None):
    """-> (span.x, span.y); the parallel-and-outside return is counted as miss_parallel."""
    near, far = F(0.0), F(1e9)
    for o, d, lo, size in ((origin[0], direction[0], B.world_min[0], B.world_size[0]), (origin[2], direction[2], B.world_min[1], B.world_size[1])):
        o, d, lo = F(o), F(d), F(lo)
        hi = lo + F(size)
        if np.abs(d) < F(1e-6):
            if o < lo or o > hi:
                count(counts, "miss_parallel")
                return F(1.0), F(0.0)
            continue
        t0, t1 = (lo - o) / d, (hi - o) / d
        near = np.fmax(near, np.fmin(t0, t1))
        far = np.fmin(far, np.fmax(t0, t1))
    return near, far


@np.errstate(all="ignore")
def sample_height(B: Params, heightmap, wx, wz):
    W, H = int(B.resolution[0]), int(B.resolution[1])
    u = ((wx - F(B.world_min[0])) * F(B.inv_world_size[0])).astype(np.float32)
    v = ((wz - F(B.world_min[1])) * F(B.inv_world_size[1])).astype(np.float32)
    x0, x1, fx = axis_clamp(u, W)
    y0, y1, fy = axis_clamp(v, H)
    t = load_unorm16(heightmap)
    n = lerp(lerp(t[y0, x0], t[y0, x1], fx), lerp(t[y1, x0], t[y1, x1], fx), fy)
    return (F(B.base_height) + n * F(B.height_scale)).astype(np.float32)


@np.errstate(all="ignore")
def gap_at(B: Params, heightmap, d, t):
    o = _f3(B.ray_origin)
    t = np.atleast_1d(np.asarray(t, np.float32))
    px, py, pz = (o[0] + d[0] * t).astype(np.float32), (o[1] + d[1] * t).astype(np.float32), (o[2] + d[2] * t).astype(np.float32)
    return (py - sample_height(B, heightmap, px, pz)).astype(np.float32)


# ---- B4 - B6 -------------------------------------------------------------------------------------------------------------------------------------
@np.errstate(all="ignore")
def march_parameters(span_x, span_y):
    step = (span_y - span_x) / F(MARCH_STEPS)
    t = (span_x + step * np.arange(MARCH_STEPS + 1, dtype=np.float32)).astype(np.float32)
    t[0] = span_x
    return t


@np.errstate(all="ignore")
def trace(B: Params, heightmap, counts=None, info=None):
    """The trace stage: (hit uint32 [4], region uint32 [4]).  `info`, when given, receives step (0 on a miss), span and the hit's t."""
    hit, region = np.zeros(4, np.uint32), np.zeros(4, np.uint32)
    d = direction_of(B)
    o = _f3(B.ray_origin)
    parallel = {}
    span_x, span_y = clip_to_footprint(B, o, d, parallel)
    if info is not None:
        info.update(step=0, span=(span_x, span_y))
    if not span_x <= span_y:
        count(counts, "miss_parallel" if parallel else "miss_clip")
        return hit, region
    t = march_parameters(span_x, span_y)
    gaps = gap_at(B, heightmap, d, t)
    crossing = (gaps[1:] <= 0) & (gaps[:-1] > 0)
    if not crossing.any():
        count(counts, "miss_no_crossing")
        return hit, region
    i = int(np.argmax(crossing)) + 1
    if counts is not None:
        counts.setdefault("hit_step", {})
        counts["hit_step"][i] = counts["hit_step"].get(i, 0) + 1
    lo, hi = t[i - 1], t[i]
    for _ in range(REFINE_STEPS):
        mid = (lo + hi) * F(0.5)
        if gap_at(B, heightmap, d, mid)[0] > 0:
            lo = mid
        else:
            hi = mid
    w = [o[k] + d[k] * hi for k in range(3)]
    hit[:3] = np.asarray(w, np.float32).view(np.uint32)
    hit[3] = 1
    radius = F(B.radius_texels) + F(1.0)
    for k, c in enumerate((w[0], w[2])):
        center = ((c - F(B.world_min[k])) * F(B.inv_world_size[k])) * F(B.resolution[k])
        scale = F(B.patch_count[k]) / F(B.resolution[k])
        region[k] = int(cvt_u32_sat(np.fmax(np.floor(center - radius), F(0.0))))
        region[2 + k] = int(cvt_u32_sat(np.fmax(np.floor((center - radius) * scale), F(0.0))))
    if info is not None:
        info.update(step=i, t=hi, gaps=gaps)
    return hit, region


# ---- B7 - B10 ------------------------------------------------------------------------------------------------------------------------------------
def footprint_threads(radius_texels) -> int:
    """Threads a side: 2 * u32(ceil(radius_texels)) + 1 in whole 16 x 16 groups."""
    return -(-(2 * int(np.ceil(F(radius_texels))) + 1) // 16) * 16


@np.errstate(all="ignore")
def falloff_of(B: Params, distance):
    """B8 for an array of distances."""
    distance = np.atleast_1d(np.asarray(distance, np.float32))
    if not F(B.radius_texels) > 0:
        return np.zeros(distance.shape, np.float32)
    t = saturate(F(1.0) - distance / F(B.radius_texels))
    smoothed = (((t * t) * t) * (t * (t * F(6.0) - F(15.0)) + F(10.0))).astype(np.float32)
    return pow_rule(smoothed, np.fmax(F(B.falloff), F(1e-3))).reshape(distance.shape)


@np.errstate(all="ignore")
def apply(B: Params, hit, heightmap, height_edit, splat_edit, counts=None):
    """The apply stage on the hit record as it is: (height_edit, splat_edit) after it; an edit image the mode does not touch may be None."""
    out_h = None if height_edit is None else height_edit.copy()
    out_s = None if splat_edit is None else splat_edit.copy()
    hit = np.asarray(hit, np.uint32)
    if hit[3] == 0:
        return out_h, out_s
    W, H = int(B.resolution[0]), int(B.resolution[1])
    wp = hit[:3].copy().view(np.float32)
    cx = ((wp[0] - F(B.world_min[0])) * F(B.inv_world_size[0])) * F(W)
    cy = ((wp[2] - F(B.world_min[1])) * F(B.inv_world_size[1])) * F(H)
    radius = int(cvt_i32_sat(np.ceil(F(B.radius_texels))))
    n = footprint_threads(B.radius_texels)
    ty, tx = (g.reshape(-1) for g in np.mgrid[0:n, 0:n].astype(np.int64))
    sx, sy = int(cvt_i32_sat(np.floor(cx))) - radius + tx, int(cvt_i32_sat(np.floor(cy))) - radius + ty
    inside = (sx >= 0) & (sy >= 0) & (sx < W) & (sy < H)
    count(counts, "texels_outside", (~inside).sum())
    x, y = sx[inside], sy[inside]
    dx, dy = (x.astype(np.float32) + F(0.5)) - cx, (y.astype(np.float32) + F(0.5)) - cy
    falloff = falloff_of(B, np.sqrt(dx * dx + dy * dy))
    keep = falloff > 0
    count(counts, "texels_zero_falloff", (~keep).sum())
    count(counts, "texels_written", keep.sum())
    count(counts, "mode_" + MODE_NAMES[int(B.mode)], keep.sum())
    x, y = x[keep], y[keep]
    amount = (falloff[keep] * F(B.strength)).astype(np.float32)
    if int(B.mode) == PAINT_LAYER:
        k = saturate(amount)
        pw = splat_edit[y, x].astype(np.uint32)
        target = [F(1.0) if int(B.layer) == c + 1 else F(0.0) for c in range(3)] + [F(1.0)]
        word = np.zeros(pw.shape, np.uint32)
        for c in range(4):
            p = ((pw >> np.uint32(8 * c)) & np.uint32(0xFF)).astype(np.float32) / F(255.0)
            word |= unorm8(lerp(p, target[c], k)) << np.uint32(8 * c)
        out_s[y, x] = word
        return out_h, out_s
    loaded = load_unorm16(heightmap)
    load = lambda ox, oy: loaded[np.clip(y + oy, 0, H - 1), np.clip(x + ox, 0, W - 1)]  # noqa: E731
    height = load(0, 0)
    mode = int(B.mode)
    if mode == SMOOTH:
        total = np.zeros(height.shape, np.float32)
        for oy in range(-2, 3):
            for ox in range(-2, 3):
                total = total + load(ox, oy)
        delta = (total / F(25.0) - height) * amount
    elif mode == FLATTEN:
        delta = (F(B.flatten_height) - height) * amount
    elif mode == NOISE:
        delta = noised(x.astype(np.float32) * F(0.05), y.astype(np.float32) * F(0.05), 0)[0] * amount
    else:
        delta = amount
    out_h[y, x] = clamp(height_edit[y, x] + delta.astype(np.float32), -1.0, 1.0)
    return out_h, out_s


# ---- the call ------------------------------------------------------------------------------------------------------------------------------------
def terrain_brush(B: Params, images: dict, stages=BOTH, counts=None, info=None) -> dict:
    """The stages of `stages` in their order on `images` (heightmap, height_edit, splat_edit, hit, region): the images after the call."""
    out = dict(images)
    if stages & TRACE:
        out["hit"], out["region"] = trace(B, out["heightmap"], counts, info)
    if stages & APPLY:
        out["height_edit"], out["splat_edit"] = apply(B, out["hit"], out.get("heightmap"), out.get("height_edit"), out.get("splat_edit"), counts)
    return out
