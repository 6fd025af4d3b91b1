"""The numpy checker of oxc_apply_fxaa: rules 1-8 of its header block in include/oxcull.h, vectorised over the image (the search over the
searching pixels, one masked pass per step).  Every binary32 operation is one numpy float32 operation in the order the header states.  An
image is uint32 [H, W] (B10G11R11) or uint16 [H, W, 4] (R16G16B16A16 Sfloat).  `apply_fxaa` returns the output image and the four counters of
oxc_debug_fxaa_stats; with `detail` it also leaves the per-pixel decisions there for the tests' not-degenerate assertions."""
from __future__ import annotations

import numpy as np

from pixel_rules import axis_clamp, channel_half, from_half_bits, lerp, pack_b10g11r11, unpack_b10g11r11

F = np.float32
FORMAT_B10G11R11, FORMAT_R16G16B16A16 = 0, 1
EDGE_THRESHOLD_MIN, EDGE_THRESHOLD_MAX = F(0.0312), F(0.125)
QUALITY = [F(q) for q in (1, 1, 1, 1, 1, 1.5, 2, 2, 2, 2, 4, 8)]
ITERATIONS = 12
SUBPIXEL_QUALITY = F(0.75)
ONE_TWELFTH = F(1.0) / F(12.0)


def decode(image, fmt: int):
    """Four float32 planes [H, W]: r, g, b, alpha (1.0 for B10G11R11)."""
    image = np.ascontiguousarray(image)
    if fmt == FORMAT_B10G11R11:
        w = image.view(np.uint32)
        r, g, b = (c.reshape(w.shape) for c in unpack_b10g11r11(w.reshape(-1)))
        return r, g, b, np.ones(w.shape, dtype=np.float32)
    halves = image.view(np.uint16)
    return tuple(from_half_bits(halves[..., c]) for c in range(4))


def encode(rgba, fmt: int) -> np.ndarray:
    r, g, b, a = (np.asarray(c, dtype=np.float32) for c in rgba)
    if fmt == FORMAT_B10G11R11:
        return pack_b10g11r11(r.reshape(-1), g.reshape(-1), b.reshape(-1)).astype(np.uint32).reshape(r.shape)
    return np.stack([channel_half(r), channel_half(g), channel_half(b), channel_half(a)], axis=-1).astype(np.uint16)


@np.errstate(all="ignore")
def luma_of(r, g, b):
    return np.sqrt((r * F(0.299) + g * F(0.587)) + b * F(0.114)).astype(np.float32)


def bilinear(planes, u, v):
    """Sample(sampler, (u, v)) of every plane, clamp mode; u, v float32 [n]."""
    H, W = planes[0].shape
    x0, x1, fx = axis_clamp(u, W)
    y0, y1, fy = axis_clamp(v, H)
    return tuple(lerp(lerp(p[y0, x0], p[y0, x1], fx), lerp(p[y1, x0], p[y1, x1], fx), fy) for p in planes)


@np.errstate(all="ignore")
def apply_fxaa(image, fmt: int, detail: dict = None):
    """(the output image, [early-out pixels, searched pixels, search taps issued, pixels that ran all 12 steps without reaching both ends])."""
    image = np.asarray(image)
    H, W = image.shape[:2]
    r, g, b, alpha = decode(image, fmt)
    rgb = (r, g, b)
    luma = luma_of(r, g, b)
    ys, xs = np.mgrid[0:H, 0:W]

    def tap(dx, dy):  # rule 2
        return luma[np.clip(ys + dy, 0, H - 1), np.clip(xs + dx, 0, W - 1)]

    center, down, up, left, right = luma, tap(0, -1), tap(0, 1), tap(-1, 0), tap(1, 0)
    luma_min = np.fmin(center, np.fmin(np.fmin(down, up), np.fmin(left, right)))
    luma_max = np.fmax(center, np.fmax(np.fmax(down, up), np.fmax(left, right)))
    luma_range = luma_max - luma_min
    early = luma_range < np.fmax(EDGE_THRESHOLD_MIN, luma_max * EDGE_THRESHOLD_MAX)  # rule 4
    out = [c.copy() for c in (r, g, b, alpha)]

    s = ~early
    sy, sx = ys[s], xs[s]
    n = int(s.sum())
    stats = [int(early.sum()), n, 0, 0]
    if detail is not None:
        detail.update(early=early, luma=luma, luma_range=luma_range, luma_max=luma_max)
    if n:
        center, down, up, left, right, luma_range = center[s], down[s], up[s], left[s], right[s], luma_range[s]
        down_left, up_right, up_left, down_right = tap(-1, -1)[s], tap(1, 1)[s], tap(-1, 1)[s], tap(1, -1)[s]
        tex_x, tex_y = (sx.astype(np.float32) + F(0.5)) / F(W), (sy.astype(np.float32) + F(0.5)) / F(H)
        inv_x, inv_y = F(1.0) / F(W), F(1.0) / F(H)
        # rule 5
        down_up, left_right = down + up, left + right
        left_corners, down_corners = down_left + up_left, down_left + down_right
        right_corners, up_corners = down_right + up_right, up_right + up_left
        edge_h = (np.abs(F(-2.0) * left + left_corners) + np.abs(F(-2.0) * center + down_up) * F(2.0)) + np.abs(F(-2.0) * right + right_corners)
        edge_v = (np.abs(F(-2.0) * up + up_corners) + np.abs(F(-2.0) * center + left_right) * F(2.0)) + np.abs(F(-2.0) * down + down_corners)
        horizontal = edge_h >= edge_v
        step = np.where(horizontal, inv_y, inv_x).astype(np.float32)
        luma1, luma2 = np.where(horizontal, down, left), np.where(horizontal, up, right)
        gradient1, gradient2 = luma1 - center, luma2 - center
        steepest1 = np.abs(gradient1) >= np.abs(gradient2)
        gradient_scaled = F(0.25) * np.fmax(np.abs(gradient1), np.abs(gradient2))
        step = np.where(steepest1, -step, step).astype(np.float32)
        average = np.where(steepest1, F(0.5) * (luma1 + center), F(0.5) * (luma2 + center)).astype(np.float32)
        cur_x = np.where(horizontal, tex_x, tex_x + step * F(0.5)).astype(np.float32)
        cur_y = np.where(horizontal, tex_y + step * F(0.5), tex_y).astype(np.float32)
        # rule 6
        off_x, off_y = np.where(horizontal, inv_x, F(0.0)).astype(np.float32), np.where(horizontal, F(0.0), inv_y).astype(np.float32)
        uv1 = [cur_x - off_x * QUALITY[0], cur_y - off_y * QUALITY[0]]
        uv2 = [cur_x + off_x * QUALITY[0], cur_y + off_y * QUALITY[0]]
        end1 = luma_of(*bilinear(rgb, *uv1)) - average
        end2 = luma_of(*bilinear(rgb, *uv2)) - average
        taps = 2 * n
        reached1, reached2 = np.abs(end1) >= gradient_scaled, np.abs(end2) >= gradient_scaled
        both = reached1 & reached2

        def advance(uv, mask, sign, q):
            uv[0] = np.where(mask, uv[0] + sign * (off_x * q), uv[0]).astype(np.float32)
            uv[1] = np.where(mask, uv[1] + sign * (off_y * q), uv[1]).astype(np.float32)

        advance(uv1, ~reached1, F(-1.0), QUALITY[1])
        advance(uv2, ~reached2, F(1.0), QUALITY[1])
        live = ~both  # the pixels inside the loop
        samples1, samples2 = np.ones(n, dtype=np.int64), np.ones(n, dtype=np.int64)
        for i in range(2, ITERATIONS):
            if not live.any():
                break
            m1, m2 = live & ~reached1, live & ~reached2
            end1 = np.where(m1, luma_of(*bilinear(rgb, *uv1)) - average, end1).astype(np.float32)
            end2 = np.where(m2, luma_of(*bilinear(rgb, *uv2)) - average, end2).astype(np.float32)
            taps += int(m1.sum()) + int(m2.sum())
            samples1, samples2 = samples1 + m1, samples2 + m2
            reached1 = np.where(live, np.abs(end1) >= gradient_scaled, reached1)
            reached2 = np.where(live, np.abs(end2) >= gradient_scaled, reached2)
            both = reached1 & reached2
            advance(uv1, live & ~reached1, F(-1.0), QUALITY[i])
            advance(uv2, live & ~reached2, F(1.0), QUALITY[i])
            live = live & ~both
        stats[2], stats[3] = taps, int(live.sum())  # `live` after step 11: the loop ran out
        # rule 7
        distance1 = np.where(horizontal, tex_x - uv1[0], tex_y - uv1[1]).astype(np.float32)
        distance2 = np.where(horizontal, uv2[0] - tex_x, uv2[1] - tex_y).astype(np.float32)
        direction1 = distance1 < distance2
        distance_final = np.fmin(distance1, distance2)
        thickness = distance1 + distance2
        center_smaller = center < average
        correct = np.where(direction1, (end1 < 0) != center_smaller, (end2 < 0) != center_smaller)
        pixel_offset = (-distance_final) / thickness + F(0.5)
        final_offset = np.where(correct, pixel_offset, F(0.0)).astype(np.float32)
        luma_average = ONE_TWELFTH * ((F(2.0) * (down_up + left_right) + left_corners) + right_corners)
        s1 = np.fmin(np.fmax(np.abs(luma_average - center) / luma_range, F(0.0)), F(1.0))
        s2 = ((F(-2.0) * s1 + F(3.0)) * s1) * s1
        sub_final = (s2 * s2) * SUBPIXEL_QUALITY
        final_offset = np.fmax(final_offset, sub_final)
        final_x = np.where(horizontal, tex_x, tex_x + final_offset * step).astype(np.float32)
        final_y = np.where(horizontal, tex_y + final_offset * step, tex_y).astype(np.float32)
        for plane, value in zip(out, bilinear((r, g, b, alpha), final_x, final_y)):
            plane[s] = value
        if detail is not None:
            detail.update(ys=sy, xs=sx, horizontal=horizontal, steepest1=steepest1, edge_h=edge_h, edge_v=edge_v, gradient1=gradient1, gradient2=gradient2,
                          final_offset=final_offset, ran_out=live, reached1=reached1, reached2=reached2, samples1=samples1, samples2=samples2)
    return encode(out, fmt), stats  # rule 8
