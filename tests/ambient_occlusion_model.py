"""Checker of oxc_generate_ambient_occlusion: the three VBGTAO pipelines of RendererInstance::generate_ambient_occlusion (Passes/PBR.cpp:
179-311; vbgtao_prefilter / vbgtao_main / vbgtao_denoise) restated in numpy, vectorised over pixels, step by step from the rules
include/oxcull.h states: binary32 in the Slang's evaluation order, no contraction, IEEE division and square root, gathers as clamped integer
texels, the manual bilinear at two levels in place of the trilinear sampler, the resolve's rotation pair, and the closed forms of log2 and
pow in binary64.  Written from the header, not from the kernels.  Every intermediate the call writes is returned."""
from __future__ import annotations

import numpy as np

from pixel_rules import (cos_sin_turn, cvt_i32_sat, cvt_u32_sat, dot, f32a, frac, from_half_bits, length, log2_rule, normalize, oct_to_vec3, pack_unorm4x8, pow_rule,
                         saturate, sign, to_half_bits)

F = np.float32
HALF_PI, PI = F(1.57079632679), F(3.1415926535897932384626433832795)
SECTORS = 32
LEVELS = 5
PIXEL_TOO_CLOSE = F(1.3)
MIP_OFFSET = F(3.30)
R2 = (F(0.75487766624669276005), F(0.5698402909980532659114))
GOLDEN = F(0.6180339887498948482)
COUNTER_NAMES = ("non_sky_pixels", "samples", "mip0", "mip1", "mip2", "mip3", "mip4", "fractional", "result_one", "result_partial", "result_zero",
                 "zero_width", "sign_minus", "sign_zero", "sign_plus")
PRESETS = {"low": (1, 2), "medium": (2, 2), "high": (3, 3), "ultra": (9, 3)}  # slice_count, samples_per_slice_side


# ---- small rules ----------------------------------------------------------------------------------------------------------------------------
@np.errstate(all="ignore")
def fast_acos(x):
    x = f32a(x)
    a = np.abs(x)
    res = F(-0.156583) * a + HALF_PI
    res = res * np.sqrt(saturate(F(1.0) - a))
    return np.where(x >= 0, res, PI - res).astype(np.float32)


def unpack_unorm4x8(w):
    w = np.asarray(w, dtype=np.uint32)
    return tuple(((w >> np.uint32(8 * k)) & np.uint32(0xFF)).astype(np.float32) / F(255.0) for k in range(4))


def noise_pair(entry, noise_index):
    """load_noise: the R2 pair of table entry `entry` (u16) and the temporal index."""
    idx = (np.asarray(entry).astype(np.int64) + 288 * (int(noise_index) % 64)).astype(np.float32)  # below 2^24: exact
    return frac(F(0.5) + idx * R2[0]), frac(F(0.5) + idx * R2[1])


# ---- per-call constants (host) -----------------------------------------------------------------------------------------------------------------
def falloff_constants(effect_radius):
    """(falloff_mul, falloff_add) of an already scaled effect radius, in the Slang's order."""
    er = F(effect_radius)
    falloff_range = F(0.615) * er
    falloff_from = er * (F(1.0) - F(0.615))
    return F(-1.0) / falloff_range, falloff_from / falloff_range + F(1.0)


PREFILTER_RADIUS = (F(0.75) * F(0.5)) * F(1.457)


# ---- prefilter ------------------------------------------------------------------------------------------------------------------------------
@np.errstate(all="ignore")
def weighted_average(d0, d1, d2, d3):
    mul, add = falloff_constants(PREFILTER_RADIUS)
    mn = np.fmin(np.fmin(d0, d1), np.fmin(d2, d3))
    w = [saturate((d - mn) * mul + add) for d in (d0, d1, d2, d3)]
    total = ((w[0] + w[1]) + w[2]) + w[3]
    return ((((w[0] * d0) + (w[1] * d1)) + (w[2] * d2)) + (w[3] * d3)) / total


def level_extent(W, H, k):
    return max(1, W >> k), max(1, H >> k)


@np.errstate(all="ignore")
def prefilter(depth, projection):
    """Five float32 levels.  One thread per 2 x 2 source texels on a grid padded to 8 x 8 threads; every thread works from its clamped gather,
    whether or not its destination texels exist."""
    depth = np.ascontiguousarray(depth, dtype=np.float32)
    H, W = depth.shape
    pm = f32a(projection)
    mul, add = pm[14], pm[10]  # glm projection[3][2], projection[2][2]
    TW, TH = (W + 15) // 16 * 8, (H + 15) // 16 * 8
    bx, by = np.meshgrid(np.arange(TW), np.arange(TH))
    x0, x1 = np.minimum(2 * bx, W - 1), np.minimum(2 * bx + 1, W - 1)
    y0, y1 = np.minimum(2 * by, H - 1), np.minimum(2 * by + 1, H - 1)
    lin = lambda t: mul / (t + add)  # noqa: E731
    d00, d10, d01, d11 = lin(depth[y0, x0]), lin(depth[y0, x1]), lin(depth[y1, x0]), lin(depth[y1, x1])
    levels = [lin(depth)]
    cur = weighted_average(d00, d10, d01, d11)  # .w, .z, .x, .y
    for k in range(1, LEVELS):
        w, h = level_extent(W, H, k)
        levels.append(np.ascontiguousarray(cur[:h, :w]))
        if k < LEVELS - 1:
            cur = weighted_average(cur[0::2, 0::2], cur[0::2, 1::2], cur[1::2, 0::2], cur[1::2, 1::2])
    return levels


# ---- main -----------------------------------------------------------------------------------------------------------------------------------
@np.errstate(all="ignore")
def calculate_edges(level0, xs, ys):
    """(packed edges, depth_center) for pixels (xs, ys) of level 0."""
    H, W = level0.shape
    cx = lambda v: np.clip(v, 0, W - 1)  # noqa: E731
    cy = lambda v: np.clip(v, 0, H - 1)  # noqa: E731
    center = level0[ys, xs]
    left, right = level0[ys, cx(xs - 1)], level0[ys, cx(xs + 1)]
    top, bottom = level0[cy(ys - 1), xs], level0[cy(ys + 1), xs]
    e = [left - center, right - center, top - center, bottom - center]
    slr = (e[1] - e[0]) * F(0.5)
    stb = (e[3] - e[2]) * F(0.5)
    adj = [e[0] + slr, e[1] + -slr, e[2] + stb, e[3] + -stb]
    e = [np.fmin(np.abs(a), np.abs(b)) for a, b in zip(e, adj)]
    scale = center * F(0.011)
    e = [saturate((F(1.0) + F(0.25)) - v / scale) for v in e]
    return pack_unorm4x8(*e), center


@np.errstate(all="ignore")
def update_sectors(min_horizon, max_horizon):
    """(mask, zero width) of one arc, into an empty bitmask."""
    angle = cvt_u32_sat(np.ceil(saturate(f32a(max_horizon) - f32a(min_horizon)) * F(SECTORS)))
    start = np.minimum(cvt_u32_sat(saturate(min_horizon) * F(SECTORS)), SECTORS - 1)
    bits = np.int64(0xFFFFFFFF) >> (SECTORS - np.maximum(angle, 1))
    mask = (bits << start) & np.int64(0xFFFFFFFF)
    return np.where(angle == 0, 0, mask).astype(np.int64), angle == 0


@np.errstate(all="ignore")
def bilinear(level, u, v):
    H, W = level.shape
    gx, gy = u * F(W) - F(0.5), v * F(H) - F(0.5)
    ix, iy = np.floor(gx), np.floor(gy)
    fx, fy = gx - ix, gy - iy
    jx, jy = cvt_i32_sat(ix), cvt_i32_sat(iy)
    x0, x1 = np.clip(jx, 0, W - 1), np.clip(jx + 1, 0, W - 1)
    y0, y1 = np.clip(jy, 0, H - 1), np.clip(jy + 1, 0, H - 1)
    t00, t10, t01, t11 = level[y0, x0], level[y0, x1], level[y1, x0], level[y1, x1]
    top = t00 + (t10 - t00) * fx
    bottom = t01 + (t11 - t01) * fx
    return top + (bottom - top) * fy


@np.errstate(all="ignore")
def sample_level(levels, u, v, lvl):
    """The filtered sample: bilinear at floor(l) and at min(floor(l) + 1, 4), always both, lerp by the fraction."""
    fl = np.floor(lvl)
    l0 = fl.astype(np.int64)
    l1 = np.minimum(l0 + 1, LEVELS - 1)
    a, b = np.empty_like(u), np.empty_like(u)
    for k in range(LEVELS):
        m = l0 == k
        a[m] = bilinear(levels[k], u[m], v[m])
        m = l1 == k
        b[m] = bilinear(levels[k], u[m], v[m])
    return a + (b - a) * (lvl - fl)


def decode_normal_view(normal_u16x4, view):
    """normalize(mul(view, (oct_to_vec3(.ba), 0)).xyz), the w = 0 term left out."""
    h = np.ascontiguousarray(np.asarray(normal_u16x4)).view(np.uint16)
    n = oct_to_vec3(from_half_bits(h[..., 2]), from_half_bits(h[..., 3]))
    m = f32a(view)
    return normalize(tuple((m[0 + r] * n[0] + m[4 + r] * n[1]) + m[8 + r] * n[2] for r in range(3)))


@np.errstate(all="ignore")
def main_pass(levels, normal, hilbert, view, projection, resolution, far_clip, thickness, slice_count, samples_per_slice_side, effect_radius,
              noise_index, stats=None):
    """(depth_differences u32 [H, W], noisy_occlusion u16 [H, W])."""
    level0 = levels[0]
    H, W = level0.shape
    pm = f32a(projection)
    p00, p11 = pm[0], pm[5]
    rx, ry = F(resolution[0]), F(resolution[1])
    er = F(effect_radius) * F(1.457)
    fmul, fadd = falloff_constants(er)
    half_er = F(0.5) * er
    radius = (half_er * np.abs(p00), half_er * np.abs(p11))
    far_thr = F(far_clip) * F(0.999)
    thickness = F(thickness)
    scf, spf = F(slice_count), F(samples_per_slice_side)

    gy, gx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    edges, center = calculate_edges(level0, gx, gy)
    ao = np.ones((H, W), dtype=np.float32)
    ys, xs = np.nonzero(~(center >= far_thr))  # a NaN depth is not sky
    N = len(xs)
    per = {"samples": np.zeros(N, np.int64), "fractional": np.zeros(N, np.int64), "zero_width": np.zeros(N, np.int64),
           "mip": np.zeros((5, N), np.int64), "sign": np.zeros((3, N), np.int64)}
    if N:
        uvx, uvy = (xs.astype(np.float32) + F(0.5)) / rx, (ys.astype(np.float32) + F(0.5)) / ry
        ld = center[ys, xs] * F(0.99999)
        origin = (((uvx * F(2.0) - F(1.0)) / p00) * ld, ((uvy * F(2.0) - F(1.0)) / p11) * ld, -ld)
        vd = normalize((-origin[0], -origin[1], -origin[2]))
        nrm = decode_normal_view(np.asarray(normal).reshape(H, W, 4)[ys, xs], view)
        n0, n1 = noise_pair(np.asarray(hilbert).reshape(64, 64)[ys % 64, xs % 64], noise_index)
        srx, sry = radius[0] / ld, radius[1] / ld
        min_s = PIXEL_TOO_CLOSE / np.fmax(srx * rx, PIXEL_TOO_CLOSE)
        visibility = np.zeros(N, dtype=np.float32)
        for si in range(int(slice_count)):
            st = F(si)
            sl = (st + n0) / scf
            c, s = cos_sin_turn(sl * F(0.5))
            dv = c * vd[0] + s * vd[1]
            ortho = normalize((c - dv * vd[0], s - dv * vd[1], F(0.0) - dv * vd[2]))
            axis = normalize((s * vd[2], -(c * vd[2]), c * vd[1] - s * vd[0]))
            na = dot(nrm, axis)
            pn = (nrm[0] - axis[0] * na, nrm[1] - axis[1] * na, nrm[2] - axis[2] * na)
            pnl = np.fmax(length(pn), F(1e-6))
            sg = sign(dot(ortho, pn))
            cos_norm = saturate(dot(pn, vd) / pnl)
            n = sg * fast_acos(cos_norm)
            per["sign"][0] += sg < 0
            per["sign"][1] += sg == 0
            per["sign"][2] += sg > 0
            smx, smy = c * srx, (-s) * sry
            bitmask = np.zeros(N, dtype=np.int64)
            occlusion = np.zeros(N, dtype=np.float32)
            for ti in range(int(samples_per_slice_side)):
                tt = F(ti)
                sn = frac(n1 + (st + tt * spf) * GOLDEN)
                sv = (tt + sn) / spf
                sv = sv * sv
                sv = sv + min_s
                ox, oy = sv * smx, sv * smy
                px_, py_ = ox * rx, oy * ry
                lvl = np.fmin(np.fmax(log2_rule(np.sqrt(px_ * px_ + py_ * py_)) - MIP_OFFSET, F(0.0)), F(LEVELS - 1))
                fl = np.floor(lvl).astype(np.int64)
                for k in range(5):
                    per["mip"][k] += 2 * (fl == k)
                per["samples"] += 2
                per["fractional"] += 2 * (lvl != np.floor(lvl))
                for side in (F(1.0), F(-1.0)):
                    pu, pv = (uvx + ox, uvy + oy) if side > 0 else (uvx - ox, uvy - oy)
                    d = sample_level(levels, pu, pv, lvl)
                    sp = (((pu * F(2.0) - F(1.0)) / p00) * d, ((pv * F(2.0) - F(1.0)) / p11) * d, -d)
                    delta = (sp[0] - origin[0], sp[1] - origin[1], sp[2] - origin[2])
                    back = (delta[0] - vd[0] * thickness, delta[1] - vd[1] * thickness, delta[2] - vd[2] * thickness)
                    hf = fast_acos(dot(normalize(delta), vd))
                    hb = fast_acos(dot(normalize(back), vd))
                    hf = saturate((((side * -hf) + n) + HALF_PI) / PI)
                    hb = saturate((((side * -hb) + n) + HALF_PI) / PI)
                    lo, hi = (hb, hf) if side > 0 else (hf, hb)
                    mask, zero = update_sectors(lo, hi)
                    per["zero_width"] += zero
                    falloff = saturate(length(delta) * fmul + fadd)
                    new = mask & ~bitmask
                    count = np.zeros(N, dtype=np.int64)
                    for b in range(32):
                        count += (new >> b) & 1
                    occlusion = occlusion + (falloff * count.astype(np.float32)) / F(SECTORS)
                    bitmask = bitmask | mask
            visibility = visibility + saturate(F(1.0) - occlusion)
        ao[ys, xs] = saturate(visibility / scf)
    noisy = to_half_bits(ao)
    if stats is not None:
        cls = np.zeros((H, W), dtype=np.int8)  # 0 sky, 1 exactly 1.0, 2 inside (0, 1), 3 exactly 0.0 (of the stored half)
        hv = from_half_bits(noisy)[ys, xs]
        cls[ys, xs] = np.where(hv == 1, 1, np.where(hv == 0, 3, 2))
        stats.update(per, result_class=cls, xs=xs, ys=ys)
    return edges, noisy


# ---- denoise --------------------------------------------------------------------------------------------------------------------------------
@np.errstate(all="ignore")
def denoise(noisy_bits, edges, final_power):
    H, W = edges.shape
    vis = from_half_bits(noisy_bits).reshape(H, W)
    gy, gx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    at = lambda img, dx, dy: img[np.clip(gy + dy, 0, H - 1), np.clip(gx + dx, 0, W - 1)]  # noqa: E731
    left_e, right_e, top_e, bottom_e = (unpack_unorm4x8(at(edges, dx, dy)) for dx, dy in ((-1, 0), (1, 0), (0, -1), (0, 1)))
    ce = unpack_unorm4x8(edges)
    lw, rw, tw, bw = ce[0] * left_e[1], ce[1] * right_e[0], ce[2] * top_e[3], ce[3] * bottom_e[2]
    k = F(0.425)
    tlw = k * (tw * top_e[0] + lw * left_e[2])
    trw = k * (tw * top_e[1] + rw * right_e[2])
    blw = k * (bw * bottom_e[0] + lw * left_e[3])
    brw = k * (bw * bottom_e[1] + rw * right_e[3])
    cw = F(1.2)
    terms = ((0, 0, cw), (-1, 0, lw), (1, 0, rw), (0, -1, tw), (0, 1, bw), (-1, -1, tlw), (1, -1, trw), (-1, 1, blw), (1, 1, brw))
    total = None
    weight = None
    for dx, dy, w in terms:
        t = at(vis, dx, dy) * w
        total = t if total is None else total + t
        weight = np.full((H, W), w, dtype=np.float32) if weight is None else weight + w
    v = np.fmax(total / weight, F(0.0))
    return to_half_bits(pow_rule(v.reshape(-1), final_power).reshape(H, W))


# ---- the call -------------------------------------------------------------------------------------------------------------------------------
def generate(depth, normal, hilbert, view, projection, resolution, far_clip, thickness=0.25, slice_count=3, samples_per_slice_side=3,
             effect_radius=0.5, noise_index=0, final_power=2.2, stats=None) -> dict:
    """One oxc_generate_ambient_occlusion call: {"levels": five float32 arrays, "depth_differences": uint32 [H, W], "noisy_occlusion": uint16
    [H, W], "ambient_occlusion": uint16 [H, W]}."""
    levels = prefilter(depth, projection)
    edges, noisy = main_pass(levels, normal, hilbert, view, projection, resolution, far_clip, thickness, slice_count, samples_per_slice_side,
                             effect_radius, noise_index, stats)
    return {"levels": levels, "depth_differences": edges, "noisy_occlusion": noisy, "ambient_occlusion": denoise(noisy, edges, final_power)}


def counters(stats) -> dict:
    """The fifteen counters of oxc_debug_ambient_occlusion_stats from a `stats` dict of generate."""
    cls = stats["result_class"]
    vals = [int((cls != 0).sum()), int(stats["samples"].sum())] + [int(stats["mip"][k].sum()) for k in range(5)] + [int(stats["fractional"].sum())]
    vals += [int((cls == 1).sum()), int((cls == 2).sum()), int((cls == 3).sum()), int(stats["zero_width"].sum())]
    vals += [int(stats["sign"][k].sum()) for k in range(3)]
    return dict(zip(COUNTER_NAMES, vals))
