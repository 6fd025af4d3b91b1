"""The numpy checker of oxc_generate_terrain_maps: steps T1-T12 of its header block in include/oxcull.h, vectorised over the texels (patches)
a call writes.  Every binary32 operation is one numpy float32 operation in the order the header states; exp, pow, the cos / sin of an angle,
frac, lerp, clamp and the unorm8 store are the shared rules of pixel_rules; the terrain-only rules (smoothstep, the unorm16 pair, noised)
live here.  Images are numpy arrays in the layouts of the header: heightmap uint16 [H, W], ridgemap uint16 [H, W] of binary16 bits, normalmap uint16
[H, W, 2], splatmap uint32 [H, W], height_edit float32 [H, W], splat_edit uint32 [H, W], patch_minmax float32 [py, px, 2].  A stage returns
new arrays and leaves its arguments unchanged.  `counts`, when given, receives how many texels (or cells) took each side of the branches
the tests must not leave empty; `pre`, when given, the values before their quantisation."""
from __future__ import annotations

import dataclasses

import numpy as np

from pixel_rules import channel_half, clamp, cos_sin_angle_rule, count, cvt_u32_sat, exp_rule, f32a, frac, from_half_bits, lerp, pow_rule, saturate, sign, unorm8

F = np.float32
TAU_F = F(6.283185307179586476925286766559)
EPSILON = F(1e-10)
K0, K1 = F(0.3183099), F(0.3678794)
S0, S1 = F(0.06711056), F(0.00583715)
WEIGHT_BIAS = F(0.01111)
GENERATE, DERIVE, MINMAX, ALL = 1, 2, 4, 7
CLASSES = ("smooth_start_linear", "smooth_start_quadratic", "weight_zero_cells", "weight_positive_cells", "normalize_safe_zero", "normalize_safe_kept",
           "height_clipped_low", "height_clipped_high", "height_inside", "grass_dominant", "rock_dominant", "drainage_dominant", "snow_dominant")


@dataclasses.dataclass
class Erosion:
    """GPU::TerrainErosion with the record's defaults."""
    scale: float = 0.15
    strength: float = 0.22
    gully_weight: float = 0.5
    detail: float = 1.5
    rounding: tuple = (0.1, 0.0, 0.1, 2.0)
    onset: tuple = (1.25, 1.25, 2.8, 1.5)
    assumed_slope: tuple = (0.7, 1.0)
    cell_scale: float = 0.7
    gain: float = 0.5
    lacunarity: float = 2.0
    normalization: float = 0.5
    octaves: int = 5
    seed: int = 0


@dataclasses.dataclass
class Generate:
    """GPU::TerrainGenerate with the record's defaults (the resolution travels beside it)."""
    erosion: Erosion = dataclasses.field(default_factory=Erosion)
    height_offset: tuple = (-0.65, 0.0)
    domain_size: float = 2.0
    height_frequency: float = 3.0
    height_amplitude: float = 0.125
    height_lacunarity: float = 2.0
    height_gain: float = 0.1
    height_octaves: int = 3


@dataclasses.dataclass
class Derive:
    """GPU::TerrainDerive with the record's defaults; texel_world_size and height_range as Terrain::bake fills them."""
    texel_world_size: tuple = (0.5, 0.5)
    height_range: float = 400.0
    slope_rock_begin: float = 0.55
    slope_rock_end: float = 0.8
    altitude_snow_begin: float = 0.7
    altitude_snow_end: float = 0.85
    ridge_drainage_scale: float = 1.0


# ---- the small rules ---------------------------------------------------------------------------------------------------------------------------
def ease_out(t):
    v = F(1.0) - saturate(t)
    return (F(1.0) - v * v).astype(np.float32)


@np.errstate(all="ignore")
def smooth_start(t, s, counts=None):
    linear = t >= s
    count(counts, "smooth_start_linear", linear)
    count(counts, "smooth_start_quadratic", ~linear)
    return np.where(linear, t - F(0.5) * s, ((F(0.5) * t) * t) / s).astype(np.float32)


@np.errstate(all="ignore")
def smoothstep(e0, e1, x):
    s = saturate((x - F(e0)) / (F(e1) - F(e0)))
    return ((s * s) * (F(3.0) - F(2.0) * s)).astype(np.float32)


@np.errstate(all="ignore")
def unorm16(e) -> np.ndarray:
    return cvt_u32_sat(np.floor(saturate(e) * F(65535.0) + F(0.5))).astype(np.uint16)


def load_unorm16(q) -> np.ndarray:
    return (np.asarray(q).astype(np.float32) / F(65535.0)).astype(np.float32)


def seed_offset(seed: int):
    fs = np.uint32(seed & 0xFFFFFFFF).astype(np.float32)
    return fs * S0, fs * S1


# ---- T2 - T4 -----------------------------------------------------------------------------------------------------------------------------------
@np.errstate(all="ignore")
def hash2(x, y, seed: int):
    sx, sy = seed_offset(seed)
    qx, qy = (x + sx) * K0 + K1, (y + sy) * K1 + K0
    t = frac((qx * qy) * (qx + qy))
    return (F(-1.0) + F(2.0) * frac((F(16.0) * K0) * t)).astype(np.float32), (F(-1.0) + F(2.0) * frac((F(16.0) * K1) * t)).astype(np.float32)


@np.errstate(all="ignore")
def noised(px, py, seed: int):
    px, py = f32a(px), f32a(py)
    ix, iy = np.floor(px), np.floor(py)
    fx, fy = px - ix, py - iy
    u = lambda f: ((f * f) * f) * (f * (f * F(6.0) - F(15.0)) + F(10.0))  # noqa: E731
    du = lambda f: ((F(30.0) * f) * f) * (f * (f - F(2.0)) + F(1.0))  # noqa: E731
    ux, uy, dux, duy = u(fx), u(fy), du(fx), du(fy)
    ga, gb = hash2(ix, iy, seed), hash2(ix + F(1.0), iy, seed)
    gc, gd = hash2(ix, iy + F(1.0), seed), hash2(ix + F(1.0), iy + F(1.0), seed)
    va = ga[0] * fx + ga[1] * fy
    vb = gb[0] * (fx - F(1.0)) + gb[1] * fy
    vc = gc[0] * fx + gc[1] * (fy - F(1.0))
    vd = gd[0] * (fx - F(1.0)) + gd[1] * (fy - F(1.0))
    k = ((va - vb) - vc) + vd
    uxy = ux * uy
    value = ((va + ux * (vb - va)) + uy * (vc - va)) + uxy * k
    d = lambda c, dc, w, v: (((ga[c] + ux * (gb[c] - ga[c])) + uy * (gc[c] - ga[c])) + uxy * (((ga[c] - gb[c]) - gc[c]) + gd[c])) + dc * ((w * k + v) - va)  # noqa: E731
    return value.astype(np.float32), d(0, dux, uy, vb).astype(np.float32), d(1, duy, ux, vc).astype(np.float32)


@np.errstate(all="ignore")
def fractal_noise(px, py, G: Generate):
    r = [np.zeros(np.shape(px), np.float32) for _ in range(3)]
    amplitude, freq = F(1.0), F(G.height_frequency)
    for i in range(int(G.height_octaves)):
        o = noised(px * freq, py * freq, int(G.erosion.seed) + i)
        af = amplitude * freq
        r = [r[0] + o[0] * amplitude, r[1] + o[1] * af, r[2] + o[2] * af]
        amplitude = amplitude * F(G.height_gain)
        freq = freq * F(G.height_lacunarity)
    return r


# ---- T7 ------------------------------------------------------------------------------------------------------------------------------------------
@np.errstate(all="ignore")
def phacelle(ppx, ppy, gx, gy, E: Erosion, seed: int, counts=None, ties=None):
    """-> (ph.x, ph.y, side.x, side.y)."""
    ln = np.sqrt(gx * gx + gy * gy)
    keep = ln > EPSILON
    count(counts, "normalize_safe_zero", ~keep)
    count(counts, "normalize_safe_kept", keep)
    nx, ny = np.where(keep, gx / ln, F(0.0)).astype(np.float32), np.where(keep, gy / ln, F(0.0)).astype(np.float32)
    cell = F(E.cell_scale)
    side_x, side_y = ((ny * F(-1.0)) * cell) * TAU_F, ((nx * F(1.0)) * cell) * TAU_F
    phase_offset = F(0.25) * TAU_F
    cx, cy = np.floor(ppx), np.floor(ppy)
    fx, fy = ppx - cx, ppy - cy
    dir_x = np.zeros(np.shape(ppx), np.float32)
    dir_y, weight_sum = dir_x.copy(), dir_x.copy()
    for a in range(-1, 3):
        for b in range(-1, 3):
            ga, gb = F(a), F(b)
            hx, hy = hash2(cx + ga, cy + gb, seed)
            dx, dy = (fx - ga) - hx * F(0.5), (fy - gb) - hy * F(0.5)
            sq = dx * dx + dy * dy
            weight = np.fmax(F(0.0), exp_rule((-sq) * F(2.0)) - WEIGHT_BIAS)
            count(counts, "weight_zero_cells", weight == 0)
            count(counts, "weight_positive_cells", weight > 0)
            weight_sum = weight_sum + weight
            w = (dx * side_x + dy * side_y) + phase_offset
            cs, sn = cos_sin_angle_rule(w)
            dir_x, dir_y = dir_x + cs * weight, dir_y + sn * weight
    den = np.fmax(weight_sum, EPSILON)
    ipx, ipy = dir_x / den, dir_y / den
    mag = np.fmax(F(1.0) - F(E.normalization), np.sqrt(ipx * ipx + ipy * ipy))
    if ties is not None:
        ties["normalize_safe_length"].append(ln)
    return (ipx / mag).astype(np.float32), (ipy / mag).astype(np.float32), side_x.astype(np.float32), side_y.astype(np.float32)


# ---- T1, T5 - T9 -----------------------------------------------------------------------------------------------------------------------------
def written(origin, dispatch, extent, group):
    """The indices origin + [0, roundup(dispatch, group)) below `extent` on one axis, ascending by thread: the u32 sum, the thread count capped
    at roundup(extent, group)."""
    n = min(-(-int(dispatch) // group) * group, -(-int(extent) // group) * group)
    v = (int(origin) + np.arange(n, dtype=np.int64)) & 0xFFFFFFFF
    return v[v < extent]


@np.errstate(all="ignore")
def generate_values(G: Generate, resolution, tx, ty, counts=None, ties=None):
    """Steps T1 - T9 before the store for the texels (tx, ty) (integer arrays): (height before height_edit, ridge)."""
    E = G.erosion
    tx, ty = np.asarray(tx), np.asarray(ty)
    px = (((tx.astype(np.float32) + F(0.5)) / F(resolution[0])) * F(G.domain_size)).astype(np.float32)
    py = (((ty.astype(np.float32) + F(0.5)) / F(resolution[1])) * F(G.domain_size)).astype(np.float32)
    r = fractal_noise(px, py, G)
    amp = F(G.height_amplitude)
    bx0, by, bz = r[0] * amp, r[1] * amp, r[2] * amp
    fade_target = clamp(bx0 / (amp * F(0.6)), -1.0, 1.0)
    bx = (bx0 * F(0.5) + F(0.5)).astype(np.float32)

    rounding, onset = [F(v) for v in E.rounding], [F(v) for v in E.onset]
    strength = F(E.strength) * F(E.scale)
    freq = F(1.0) / (F(E.scale) * F(E.cell_scale))
    target = clamp(fade_target, -1.0, 1.0)
    height = bx
    slope_length = np.fmax(np.sqrt(by * by + bz * bz), EPSILON)
    magnitude, rounding_mult = F(0.0), F(1.0)
    rounding_for_input = lerp(rounding[1], rounding[0], saturate(target + F(0.5))) * rounding[2]
    combi_mask = ease_out(smooth_start(slope_length * onset[0], rounding_for_input * onset[0], counts))
    ridge_mask = ease_out(slope_length * onset[2])
    ridge_target = target
    as0, as1 = F(E.assumed_slope[0]), F(E.assumed_slope[1])
    gx, gy = lerp(by, (by / slope_length) * as0, as1), lerp(bz, (bz / slope_length) * as0, as1)
    gw = F(E.gully_weight)
    for i in range(int(E.octaves)):
        phx, phy, side_x, side_y = phacelle(px * freq, py * freq, gx, gy, E, int(E.seed) + i, counts, ties)
        if ties is not None:
            ties["phacelle_y"].append(phy)
        phz, phw = side_x * (-freq), side_y * (-freq)
        sloping = np.abs(phy)
        sg = sign(phy)
        gx = (gx + ((sg * phz) * strength) * gw).astype(np.float32)
        gy = (gy + ((sg * phw) * strength) * gw).astype(np.float32)
        faded = lerp(target, phx * gw, combi_mask)
        height = (height + faded * strength).astype(np.float32)
        magnitude = magnitude + strength
        target = faded
        rounding_for_octave = lerp(rounding[1], rounding[0], saturate(phx + F(0.5))) * rounding_mult
        new_mask = ease_out(smooth_start(sloping * onset[1], rounding_for_octave * onset[1], counts))
        combi_mask = ((F(1.0) - pow_rule(F(1.0) - saturate(combi_mask), F(E.detail)).reshape(np.shape(combi_mask))) * new_mask).astype(np.float32)
        ridge_target = lerp(ridge_target, phx, ridge_mask)
        ridge_mask = (ridge_mask * ease_out(sloping * onset[3])).astype(np.float32)
        strength = strength * F(E.gain)
        freq = freq * F(E.lacunarity)
        rounding_mult = rounding_mult * rounding[3]
    delta = height - bx
    ridge = ridge_target * (F(1.0) - ridge_mask)
    offset = lerp(F(G.height_offset[0]), -fade_target, F(G.height_offset[1])) * magnitude
    return ((bx + delta) + offset).astype(np.float32), ridge.astype(np.float32)


@np.errstate(all="ignore")
def generate(G: Generate, resolution, height_edit, heightmap, ridgemap, texel_origin=(0, 0), dispatch_texels=None, counts=None, pre=None):
    """The generate stage: (heightmap, ridgemap) after it."""
    heightmap, ridgemap = heightmap.copy(), ridgemap.copy()
    dispatch_texels = resolution if dispatch_texels is None else dispatch_texels
    xs, ys = written(texel_origin[0], dispatch_texels[0], resolution[0], 16), written(texel_origin[1], dispatch_texels[1], resolution[1], 16)
    if xs.size == 0 or ys.size == 0:
        return heightmap, ridgemap
    ty, tx = (g.reshape(-1) for g in np.meshgrid(ys, xs, indexing="ij"))
    h, ridge = generate_values(G, resolution, tx, ty, counts)
    total = h + height_edit[ty, tx]
    count(counts, "height_clipped_low", total <= 0)
    count(counts, "height_clipped_high", total >= 1)
    count(counts, "height_inside", (total > 0) & (total < 1))
    if pre is not None:
        pre.update(tx=tx, ty=ty, height=h, ridge=ridge)
    heightmap[ty, tx] = unorm16(total)
    ridgemap[ty, tx] = channel_half(ridge)
    return heightmap, ridgemap


# ---- T10, T11 ------------------------------------------------------------------------------------------------------------------------------------
@np.errstate(all="ignore")
def derive(D: Derive, resolution, heightmap, ridgemap, splat_edit, normalmap, splatmap, texel_origin=(0, 0), dispatch_texels=None, counts=None, pre=None):
    """The derive stage on the heightmap and ridgemap as they are: (normalmap, splatmap) after it."""
    normalmap, splatmap = normalmap.copy(), splatmap.copy()
    dispatch_texels = resolution if dispatch_texels is None else dispatch_texels
    W, H = int(resolution[0]), int(resolution[1])
    xs, ys = written(texel_origin[0], dispatch_texels[0], W, 16), written(texel_origin[1], dispatch_texels[1], H, 16)
    if xs.size == 0 or ys.size == 0:
        return normalmap, splatmap
    ty, tx = (g.reshape(-1) for g in np.meshgrid(ys, xs, indexing="ij"))
    load = lambda dx, dy: load_unorm16(heightmap[np.clip(ty + dy, 0, H - 1), np.clip(tx + dx, 0, W - 1)])  # noqa: E731
    h00, h10, h20 = load(-1, -1), load(0, -1), load(1, -1)
    h01, h21 = load(-1, 0), load(1, 0)
    h02, h12, h22 = load(-1, 1), load(0, 1), load(1, 1)
    hr = F(D.height_range)
    dhdx = ((((h20 + F(2.0) * h21) + h22) - ((h00 + F(2.0) * h01) + h02)) * hr) / (F(8.0) * F(D.texel_world_size[0]))
    dhdz = ((((h02 + F(2.0) * h12) + h22) - ((h00 + F(2.0) * h10) + h20)) * hr) / (F(8.0) * F(D.texel_world_size[1]))
    vx, vy, vz = -dhdx, np.full(dhdx.shape, F(1.0)), -dhdz
    ln = np.sqrt((vx * vx + vy * vy) + vz * vz)
    nx, ny, nz = (vx / ln).astype(np.float32), (vy / ln).astype(np.float32), (vz / ln).astype(np.float32)
    if pre is not None:
        pre.update(tx=tx, ty=ty, normal_x=nx, normal_z=nz)
    normalmap[ty, tx, 0] = channel_half(nx)
    normalmap[ty, tx, 1] = channel_half(nz)
    height = load(0, 0)
    ridge = from_half_bits(ridgemap[ty, tx])
    slope = saturate(F(1.0) - ny)
    rock = smoothstep(D.slope_rock_begin, D.slope_rock_end, slope)
    snow = smoothstep(D.altitude_snow_begin, D.altitude_snow_end, height) * (F(1.0) - rock)
    drainage = (saturate((-ridge) * F(D.ridge_drainage_scale)) * (F(1.0) - rock)) * (F(1.0) - snow)
    grass = saturate(((F(1.0) - rock) - snow) - drainage)
    pw = splat_edit[ty, tx].astype(np.uint32)
    p = [((pw >> np.uint32(8 * k)) & np.uint32(0xFF)).astype(np.float32) / F(255.0) for k in range(4)]
    painted = (saturate(((F(1.0) - p[0]) - p[1]) - p[2]), p[0], p[1], p[2])
    out = [lerp(a, b, p[3]) for a, b in zip((grass, rock, drainage, snow), painted)]
    layers = np.stack(out)
    for k, name in enumerate(("grass_dominant", "rock_dominant", "drainage_dominant", "snow_dominant")):
        count(counts, name, (np.argmax(np.nan_to_num(layers), axis=0) == k) & (np.nan_to_num(layers[k]) > 0.5))
    splatmap[ty, tx] = unorm8(out[0]) | (unorm8(out[1]) << np.uint32(8)) | (unorm8(out[2]) << np.uint32(16)) | (unorm8(out[3]) << np.uint32(24))
    return normalmap, splatmap


# ---- T12 -----------------------------------------------------------------------------------------------------------------------------------------
@np.errstate(all="ignore")
def patch_range(patch: int, scale, extent: int):
    """(begin, end) of one axis."""
    begin = int(cvt_u32_sat(np.floor(F(patch) * scale)))
    end = min(int(cvt_u32_sat(np.ceil(F(patch + 1) * scale))) + 1, int(extent))
    return begin, end


def minmax(resolution, patch_count, heightmap, patch_minmax, patch_origin=(0, 0), dispatch_patches=None):
    """The minmax stage: patch_minmax after it."""
    patch_minmax = patch_minmax.copy()
    dispatch_patches = patch_count if dispatch_patches is None else dispatch_patches
    scale = [F(resolution[k]) / F(patch_count[k]) for k in range(2)]
    loaded = load_unorm16(heightmap)
    for py in written(patch_origin[1], dispatch_patches[1], patch_count[1], 8):
        by, ey = patch_range(int(py), scale[1], resolution[1])
        for px in written(patch_origin[0], dispatch_patches[0], patch_count[0], 8):
            bx, ex = patch_range(int(px), scale[0], resolution[0])
            window = loaded[by:ey, bx:ex] if (ey > by and ex > bx) else np.zeros((0,), np.float32)
            patch_minmax[py, px, 0] = np.fmin(F(1.0), window.min()) if window.size else F(1.0)
            patch_minmax[py, px, 1] = np.fmax(F(0.0), window.max()) if window.size else F(0.0)
    return patch_minmax


# ---- the call ------------------------------------------------------------------------------------------------------------------------------------
def terrain_maps(G: Generate, D: Derive, resolution, patch_count, images: dict, stages=ALL, region=(0, 0, 0, 0), dispatch_texels=None, dispatch_patches=None,
                 counts=None) -> dict:
    """The stages of `stages` in their order on `images` (the seven arrays under the context's field names): the images after the call."""
    out = dict(images)
    if stages & GENERATE:
        out["heightmap"], out["ridgemap"] = generate(G, resolution, out["height_edit"], out["heightmap"], out["ridgemap"], region[:2], dispatch_texels, counts)
    if stages & DERIVE:
        out["normalmap"], out["splatmap"] = derive(D, resolution, out["heightmap"], out["ridgemap"], out["splat_edit"], out["normalmap"], out["splatmap"], region[:2],
                                                   dispatch_texels, counts)
    if stages & MINMAX:
        out["patch_minmax"] = minmax(resolution, patch_count, out["heightmap"], out["patch_minmax"], region[2:], dispatch_patches)
    return out
