"""Checker of oxc_contact_shadows: the contact_shadows pass (RendererInstance.cpp:990-1020, passes/contact_shadows.slang + raymarch.slang in
the one configuration the engine uses) restated in numpy binary32, vectorised over pixels, from the rules include/oxcull.h states: the
Slang's evaluation order, no contraction, IEEE division and square root, the manual bilinear in place of the hardware sampler, clamp to
edge, saturating float -> integer conversions.  Written from the header, not from the kernel."""
from __future__ import annotations

import numpy as np

from pixel_rules import cvt_i32_sat, cvt_u32_sat, f32a, sign

F = np.float32
BIAS_SCALE = F(1.0) + F(0.000002)  # rule 6: rounded to binary32 once
EDGE_SPAN = F(0.3) - F(1.0)        # rule 7: smoothstep's edge1 - edge0
# outcome of a pixel
SKY, MISS, HIT_ZERO, HIT_PARTIAL, HIT_ONE, REJECTED = 0, 1, 2, 3, 4, 5
# how the step count came about
N_LOWER, N_BETWEEN, N_UPPER = 0, 1, 2
COUNTER_NAMES = ("non_sky_pixels", "taps", "miss", "hit_zero", "hit_partial", "hit_one", "rejected", "n_lower", "n_between", "n_upper", "end_clip",
                 "start_moved")


def mul_point(m, x, y, z):
    """mul(M, (x, y, z, 1)) of a column-major float[16]: four rows, each ((M[r][0] x + M[r][1] y) + M[r][2] z) + M[r][3]."""
    m = f32a(m)
    return tuple(((m[0 + r] * x + m[4 + r] * y) + m[8 + r] * z) + m[12 + r] for r in range(4))


def mul_vec4(m, x, y, z, w):
    """mul(M, (x, y, z, w)): ((M[r][0] x + M[r][1] y) + M[r][2] z) + M[r][3] w."""
    m = f32a(m)
    return tuple(((m[0 + r] * x + m[4 + r] * y) + m[8 + r] * z) + m[12 + r] * w for r in range(4))


def ray_vector(sun_dir, shadow_length):
    """normalize(sun_dir) * shadow_length, once per call."""
    s = f32a(sun_dir)
    length = np.sqrt((s[0] * s[0] + s[1] * s[1]) + s[2] * s[2])
    return (s / length) * F(shadow_length)


def depth_thickness(thickness, near_clip):
    return F(thickness) * (F(1.0) / F(near_clip))


@np.errstate(all="ignore")
def clip_ray(cs, end):
    """Rule 3's two clips.  cs, end: 3-tuples of float32 arrays.  Returns (start, ray_end, clip, moved): the clipped start, the clipped
    end, the end clip's factor min(1.0, ...) and the start clip's factor max(0.0, m)."""
    one, neg, zero = F(1.0), F(-1.0), F(0.0)
    delta = tuple(e - c for e, c in zip(end, cs))
    near = tuple(np.where(d < 0, one, neg) for d in delta[:2])
    m = np.fmax((near[0] - cs[0]) / delta[0], (near[1] - cs[1]) / delta[1])
    moved = np.fmax(zero, m)
    start = tuple(c + d * moved for c, d in zip(cs, delta))
    delta = tuple(e - s for e, s in zip(end, start))
    far = (np.where(delta[0] >= 0, one, neg), np.where(delta[1] >= 0, one, neg), np.where(delta[2] >= 0, one, zero))
    q = tuple((f - s) / d for f, s, d in zip(far, start, delta))
    clip = np.fmin(one, np.fmin(np.fmin(q[0], q[1]), q[2]))
    ray_end = tuple(s + d * clip for s, d in zip(start, delta))
    return start, ray_end, clip, moved


@np.errstate(all="ignore")
def ray_length_u32(start, ray_end, W, H):
    """u32(floor(length(len_px))) of rule 4, before the two clamps."""
    lx = ((ray_end[0] * F(0.5) + F(0.5)) - (start[0] * F(0.5) + F(0.5))) * F(W)
    ly = ((ray_end[1] * F(0.5) + F(0.5)) - (start[1] * F(0.5) + F(0.5))) * F(H)
    return cvt_u32_sat(np.floor(np.sqrt(lx * lx + ly * ly)))


def step_count(len_u, steps):
    """n = max(2, min(steps, len_u)) and how it came about."""
    lim = np.minimum(np.int64(steps), len_u)
    n = np.maximum(2, lim)
    cls = np.where(lim < 2, N_LOWER, np.where(len_u >= steps, N_UPPER, N_BETWEEN))
    return n, cls


@np.errstate(all="ignore")
def tap(depth, ux, uy):
    """Rule 6 at interp_uv * size = (ux, uy): (linear_depth, unfiltered_depth) and the texel coordinates read (x0, x1, y0, y1, nx, ny)."""
    H, W = depth.shape
    gx, gy = ux - F(0.5), uy - F(0.5)
    ix, iy = np.floor(gx), np.floor(gy)
    fx, fy = gx - ix, gy - iy
    jx, jy = cvt_i32_sat(ix), cvt_i32_sat(iy)
    x0, x1 = np.clip(jx, 0, W - 1), np.clip(jx + 1, 0, W - 1)
    y0, y1 = np.clip(jy, 0, H - 1), np.clip(jy + 1, 0, H - 1)
    nx, ny = np.clip(cvt_i32_sat(np.floor(ux)), 0, W - 1), np.clip(cvt_i32_sat(np.floor(uy)), 0, H - 1)
    t00, t10, t01, t11 = depth[y0, x0], depth[y0, x1], depth[y1, x0], depth[y1, x1]
    top = t00 + (t10 - t00) * fx
    bottom = t01 + (t11 - t01) * fx
    bil = top + (bottom - top) * fy
    return F(1.0) / bil, F(1.0) / depth[ny, nx], (x0, x1, y0, y1, nx, ny)


@np.errstate(all="ignore")
def shadow_of(frac):
    """smoothstep(1.0, 0.3, frac) of rule 7."""
    s = np.fmin(np.fmax((f32a(frac) - F(1.0)) / EDGE_SPAN, F(0.0)), F(1.0))
    return (s * s) * (F(3.0) - F(2.0) * s)


def contact_shadows(depth, inv_projection_view, view, projection, near_clip, sun_dir, steps=8, thickness=0.1, shadow_length=0.01, stats=None):
    """float32 [H, W] depth -> float32 [H, W] contact shadow term.  `stats` (a dict) receives per-pixel arrays: outcome, n (0 for sky),
    n_class (-1 for sky), taps, end_clip, start_moved; and clamped_taps, the number of taps whose four-texel footprint reached past the
    left / right / top / bottom border and was clamped."""
    depth = np.ascontiguousarray(depth, dtype=np.float32)
    H, W = depth.shape
    out = np.ones((H, W), dtype=np.float32)
    ys, xs = np.nonzero(~(depth == 0))  # NaN is not sky
    ys, xs = ys.astype(np.int64), xs.astype(np.int64)
    with np.errstate(all="ignore"):
        d = depth[ys, xs]
        csx = ((xs.astype(np.float32) + F(0.5)) / F(W)) * F(2.0) - F(1.0)
        csy = ((ys.astype(np.float32) + F(0.5)) / F(H)) * F(2.0) - F(1.0)
        cs = (csx, csy, d)
        hx, hy, hz, hw = mul_point(inv_projection_view, *cs)
        ray = ray_vector(sun_dir, shadow_length)
        end_ws = (hx / hw + ray[0], hy / hw + ray[1], hz / hw + ray[2])
        v = mul_point(view, *end_ws)
        p = mul_vec4(projection, *v)
        e = (p[0] / p[3], p[1] / p[3], p[2] / p[3])
        sg = sign(e[2])
        end = tuple(c + (ee - c) * sg for c, ee in zip(cs, e))
        start, ray_end, clip, moved = clip_ray(cs, end)
        len_u = ray_length_u32(start, ray_end, W, H)
        n, ncls = step_count(len_u, steps)
        dt = depth_thickness(thickness, near_clip)
        direction = tuple(r - s for r, s in zip(ray_end, start))
        fn = n.astype(np.float32)

        count = len(xs)
        alive = np.ones(count, dtype=bool)
        intersected = np.zeros(count, dtype=bool)
        distance = np.zeros(count, dtype=np.float32)
        penetration = np.zeros(count, dtype=np.float32)
        taps = np.zeros(count, dtype=np.int64)
        clamped = {"left": 0, "right": 0, "top": 0, "bottom": 0}  # taps whose 2 x 2 footprint was pulled back inside at that side
        for step in range(int(n.max()) if count else 0):
            k = np.nonzero(alive & (step < n))[0]
            if not len(k):
                break
            t = (F(step) + F(1.0)) / fn[k]
            c = tuple(s[k] + dd[k] * t for s, dd in zip(start, direction))
            ux, uy = (c[0] * F(0.5) + F(0.5)) * F(W), (c[1] * F(0.5) + F(0.5)) * F(H)
            ray_depth = F(1.0) / c[2]
            linear, unfiltered, _ = tap(depth, ux, uy)
            jx, jy = cvt_i32_sat(np.floor(ux - F(0.5))), cvt_i32_sat(np.floor(uy - F(0.5)))
            for side, over in (("left", jx < 0), ("right", jx + 1 > W - 1), ("top", jy < 0), ("bottom", jy + 1 > H - 1)):
                clamped[side] += int(over.sum())
            dist =np.fmax(linear, unfiltered) * BIAS_SCALE - ray_depth
            pen = ray_depth - np.fmin(linear, unfiltered)
            distance[k], penetration[k] = dist, pen
            taps[k] += 1
            hit_now = dist < 0
            intersected[k] = hit_now
            alive[k[hit_now]] = False
        hit = intersected & (penetration < dt) & (distance < dt)
        value = F(1.0) - shadow_of(penetration / dt)
        res = np.where(hit, value, F(1.0)).astype(np.float32)
    out[ys, xs] = res
    if stats is not None:
        oc = np.full((H, W), SKY, dtype=np.int8)
        oc[ys, xs] = np.where(~intersected, MISS, np.where(~hit, REJECTED, np.where(res == 0, HIT_ZERO, np.where(res == 1, HIT_ONE, HIT_PARTIAL))))
        full = {"n": (n, 0), "n_class": (ncls, -1), "taps": (taps, 0), "end_clip": (clip < 1, False), "start_moved": (moved > 0, False)}
        stats["outcome"] = oc
        stats["clamped_taps"] = clamped
        for name, (vals, fill) in full.items():
            a = np.full((H, W), fill, dtype=np.asarray(vals).dtype if name in ("end_clip", "start_moved") else np.int64)
            a[ys, xs] = vals
            stats[name] = a
    return out


def counters(stats) -> dict:
    """The twelve counters of oxc_debug_contact_shadows_stats from a `stats` dict of contact_shadows."""
    oc, nc = stats["outcome"], stats["n_class"]
    vals = (int((oc != SKY).sum()), int(stats["taps"].sum()), int((oc == MISS).sum()), int((oc == HIT_ZERO).sum()), int((oc == HIT_PARTIAL).sum()),
            int((oc == HIT_ONE).sum()), int((oc == REJECTED).sum()), int((nc == N_LOWER).sum()), int((nc == N_BETWEEN).sum()), int((nc == N_UPPER).sum()),
            int(stats["end_clip"].sum()), int(stats["start_moved"].sum()))
    return dict(zip(COUNTER_NAMES, vals))
