"""The numpy checker of oxc_apply_tonemap: steps 1-11 of its header block in include/oxcull.h, vectorised over the image.  Every binary32
operation is one numpy float32 operation in the order the header states; log2 / exp2 / pow, the exp and cos rules and the sRGB encode come
from pixel_rules.  The pixel-independent constants of step 5 are evaluated once by `constants()`, in
binary32 in the Slang's order -- the same way the library's host code does.  The source is uint32 [H, W] (B10G11R11) or uint16 [H, W, 4]
(R16G16B16A16 Sfloat); the bloom is U level 0 in the same format; the result is uint32 [H, W].  `stats`, when given, receives how many
values took each side of every branch of the rule."""
from __future__ import annotations

import numpy as np

from pixel_rules import cos_turn_rule, count, cvt_i32_sat, exp2_rule, exp_rule, f32a, from_half_bits, log2_rule, pack_unorm4x8, pow_rule, saturate, unpack_b10g11r11
from pixel_rules import srgb_encode as shared_srgb_encode

F = np.float32
NONE, ACES, AGX, GT7 = 0, 1, 2, 3
OUT_RGBA8_SRGB, OUT_BGRA8_SRGB, OUT_RGBA8_UNORM = 0, 1, 2
HAS_EYE_ADAPTATION, HAS_BLOOM, HAS_FILM_GRAIN, HAS_CHROMATIC_ABERRATION, HAS_VIGNETTE, TRANSPARENT_BACKGROUND = 1 << 2, 1 << 3, 1 << 6, 1 << 7, 1 << 8, 1 << 11
PI_F = F(3.1415926535897932384626433832795)
SIMPLEX_F2 = F((np.sqrt(3.0) - 1.0) / 2.0)  # the binary32 nearest the real value
SIMPLEX_G2 = F((3.0 - np.sqrt(3.0)) / 6.0)

ACES_IN = [[0.59719, 0.35458, 0.04823], [0.07600, 0.90834, 0.01566], [0.02840, 0.13383, 0.83777]]
ACES_OUT = [[1.60475, -0.53108, -0.07367], [-0.10208, 1.10813, -0.00605], [-0.00327, -0.07276, 1.07602]]
REC709_TO_XYZ = [[0.4124564, 0.3575761, 0.1804375], [0.2126729, 0.7151522, 0.0721750], [0.0193339, 0.1191920, 0.9503041]]
XYZ_TO_REC709 = [[3.2404542, -1.5371385, -0.4985314], [-0.9692660, 1.8760108, 0.0415560], [0.0556434, -0.2040259, 1.0572252]]
REC2020_TO_XYZ = [[0.636958, 0.1446169, 0.168881], [0.2627002, 0.6779981, 0.0593017], [0.0, 0.0280727, 1.0609851]]
XYZ_TO_REC2020 = [[1.7166512, -0.3556708, -0.2533663], [-0.6666844, 1.6164812, 0.0157685], [0.0176399, -0.0427706, 0.9421031]]
# eotfSt2084 / inverseEotfSt2084 (tonemap.slang:403-408)
PQ_M1, PQ_M2_BASE, PQ_C1, PQ_C2, PQ_C3, PQ_C = F(0.1593017578125), F(78.84375), F(0.8359375), F(18.8515625), F(18.6875), F(10000.0)
REFERENCE_LUMINANCE, SDR_PAPER_WHITE = F(100.0), F(250.0)


def _count_sides(stats, name, mask):
    count(stats, name, mask)
    count(stats, "not " + name, ~np.asarray(mask))


def mat(rows):
    return [[F(v) for v in row] for row in rows]


@np.errstate(all="ignore")
def mul_mv(M, v):
    """mul(M, v): row r is (M[r][0] * v.x + M[r][1] * v.y) + M[r][2] * v.z."""
    return tuple(((M[r][0] * v[0] + M[r][1] * v[1]) + M[r][2] * v[2]).astype(np.float32) for r in range(3))


def mul_mm(A, B):
    """mul(A, B): element (r, c) is (A[r][0] * B[0][c] + A[r][1] * B[1][c]) + A[r][2] * B[2][c]."""
    return [[F(F(F(A[r][0] * B[0][c]) + F(A[r][1] * B[1][c])) + F(A[r][2] * B[2][c])) for c in range(3)] for r in range(3)]


# ---- the closed forms in the shape of their argument ---------------------------------------------------------------------------------------------
def log2_r(x):
    return log2_rule(x).reshape(np.shape(x))


def _pow(v, p):
    return pow_rule(np.asarray(v, dtype=np.float32).reshape(-1), p).reshape(np.shape(v))


def _exp2(x):
    return exp2_rule(np.asarray(x, dtype=np.float32).reshape(-1)).reshape(np.shape(x))


# ---- step 5: the constants ----------------------------------------------------------------------------------------------------------------------
def inverse3(m):
    """inverse() of tonemap.slang:131-155 in binary32."""
    (a, b, c), (d, e, f), (g, h, i) = m
    A = F(F(e * i) - F(f * h))
    B = F(-F(F(d * i) - F(f * g)))
    C = F(F(d * h) - F(e * g))
    D = F(-F(F(b * i) - F(c * h)))
    E = F(F(a * i) - F(c * g))
    Fc = F(-F(F(a * h) - F(b * g)))
    G = F(F(b * f) - F(c * e))
    H = F(-F(F(a * f) - F(c * d)))
    I = F(F(a * e) - F(b * d))  # noqa: E741
    det = F(F(F(a * A) + F(b * B)) + F(c * C))
    inv = F(F(1.0) / det)
    return [[F(A * inv), F(D * inv), F(G * inv)], [F(B * inv), F(E * inv), F(H * inv)], [F(C * inv), F(Fc * inv), F(I * inv)]]


def unproject_xy(xy):
    """color_Unproject: color_XyYToXYZ((x, y, 1.0))."""
    x, y = xy
    Y = F(1.0)
    return (F(F(x * Y) / y), Y, F(F(F(F(F(1.0) - x) - y) * Y) / y))


def primaries_to_matrix(r, g, b, w):
    R, G, B, Wh = unproject_xy(r), unproject_xy(g), unproject_xy(b), unproject_xy(w)
    temp = [[R[0], G[0], B[0]], [F(1.0), F(1.0), F(1.0)], [R[2], G[2], B[2]]]
    inv = inverse3(temp)
    scale = [F(F(F(inv[k][0] * Wh[0]) + F(inv[k][1] * Wh[1])) + F(inv[k][2] * Wh[2])) for k in range(3)]
    return [[F(R[k] * scale[0]), F(G[k] * scale[1]), F(B[k] * scale[2])] for k in range(3)]


def compression_matrix(r, g, b, w, compression):
    s = F(F(1.0) / F(F(1.0) - compression))
    lerp2 = lambda a, c: (F(a[0] + F(F(c[0] - a[0]) * s)), F(a[1] + F(F(c[1] - a[1]) * s)))  # noqa: E731
    return primaries_to_matrix(lerp2(w, r), lerp2(w, g), lerp2(w, b), w)


@np.errstate(all="ignore")
def inverse_eotf(v, k):
    """inverseEotfSt2084 (tonemap.slang:426-442)."""
    v = f32a(v)
    y = (v * REFERENCE_LUMINANCE) / PQ_C
    ym = _pow(y, PQ_M1)
    return _exp2(k["pq_m2"] * (log2_r(PQ_C1 + PQ_C2 * ym) - log2_r(F(1.0) + PQ_C3 * ym)))


@np.errstate(all="ignore")
def rgb_to_ictcp(rgb, k):
    r, g, b = rgb
    l = ((r * F(1688.0) + g * F(2146.0)) + b * F(262.0)) / F(4096.0)  # noqa: E741
    m = ((r * F(683.0) + g * F(2951.0)) + b * F(462.0)) / F(4096.0)
    s = ((r * F(99.0) + g * F(309.0)) + b * F(3688.0)) / F(4096.0)
    lp, mp, sp = inverse_eotf(l, k), inverse_eotf(m, k), inverse_eotf(s, k)
    return ((F(2048.0) * lp + F(2048.0) * mp) / F(4096.0), ((F(6610.0) * lp - F(13613.0) * mp) + F(7003.0) * sp) / F(4096.0),
            ((F(17933.0) * lp - F(17390.0) * mp) - F(543.0) * sp) / F(4096.0))


def constants(chromatic_aberration_amount=0.0) -> dict:
    """Everything of steps 4 and 7 that does not depend on the pixel, once, in binary32 in the Slang's order."""
    k = {}
    # AgX_DS (tonemap.slang:227-262)
    xr, xg, xb, xw = (F(0.64), F(0.33)), (F(0.3), F(0.6)), (F(0.15), F(0.06)), (F(0.3127), F(0.3290))
    srgb_to_xyz = primaries_to_matrix(xr, xg, xb, xw)
    adjusted_to_xyz = compression_matrix(xr, xg, xb, xw, F(0.15))
    k["agx_in"] = mul_mm(srgb_to_xyz, inverse3(adjusted_to_xyz))
    k["agx_out"] = inverse3(k["agx_in"])
    peak, linear = F(1.0), F(0.10)
    k["agx_s"] = F(peak * linear)
    k["agx_span"] = F(peak - k["agx_s"])
    k["agx_neg_c"] = F(-F(peak / k["agx_span"]))
    k["agx_peak"] = peak
    # GT7ToneMapping::initializeAsSDR (tonemap.slang:576-624)
    k["gt_sdr"] = F(F(1.0) / F(SDR_PAPER_WHITE / REFERENCE_LUMINANCE))
    target = k["gt_target"] = F(SDR_PAPER_WHITE / REFERENCE_LUMINANCE)
    alpha, mid, lin, toe = F(0.25), F(0.538), F(0.444), F(1.280)
    kk = F(F(lin - F(1.0)) / F(alpha - F(1.0)))
    k["gt_mid"], k["gt_toe"] = mid, toe
    k["gt_ka"] = F(F(target * lin) + F(target * kk))
    k["gt_kb"] = F(F(F(-target) * kk) * exp_rule(F(lin / kk)))
    k["gt_kc"] = F(F(-1.0) / F(kk * target))
    k["gt_lin_peak"] = F(lin * target)
    k["gt_mid_span"] = F(mid - F(0.0))
    k["gt_blend"], k["gt_one_minus_blend"] = F(0.6), F(F(1.0) - F(0.6))
    k["gt_fade_start"], k["gt_fade_end"] = F(0.98), F(1.16)
    k["gt_fade_span"] = F(F(1.16) - F(0.98))
    k["pq_m2"] = F(PQ_M2_BASE * F(1.0))
    k["pq_inv_m2"] = F(F(1.0) / k["pq_m2"])
    k["pq_inv_m1"] = F(F(1.0) / PQ_M1)
    t = np.array([target], dtype=np.float32)
    k["gt_target_ucs"] = F(rgb_to_ictcp((t, t, t), k)[0][0])
    # FfxLensGetRGMag (lens.slang:51-67)
    A, B = F(1.5220), F(F(0.00459) * F(chromatic_aberration_amount))
    idx = [F(A + F(B / F(w * w))) for w in (F(0.612), F(0.549), F(0.464))]
    with np.errstate(all="ignore"):
        k["red_mag"] = F(F(idx[0] - F(1.0)) / F(idx[2] - F(1.0)))
        k["green_mag"] = F(F(idx[1] - F(1.0)) / F(idx[2] - F(1.0)))
    return k


# ---- step 4: the tone curves --------------------------------------------------------------------------------------------------------------------
@np.errstate(all="ignore")
def aces_fitted(c, stats=None):
    v = mul_mv(mat(ACES_IN), c)
    fit = []
    for x in v:
        a = x * (x + F(0.0245786)) - F(0.000090537)
        b = x * (F(0.983729) * x + F(0.4329510)) + F(0.238081)
        fit.append((a / b).astype(np.float32))
    out = mul_mv(mat(ACES_OUT), fit)
    for x in out:
        _count_sides(stats, "aces below 0", x < 0)
        _count_sides(stats, "aces above 1", x > 1)
    return tuple(saturate(x) for x in out)


@np.errstate(all="ignore")
def dual_section(x, k, stats=None):
    linear = x < k["agx_s"]
    _count_sides(stats, "agx linear", linear)
    curved = k["agx_peak"] - k["agx_span"] * exp_rule((k["agx_neg_c"] * (x - k["agx_s"])) / k["agx_peak"])
    return np.where(linear, x, curved).astype(np.float32)


@np.errstate(all="ignore")
def agx_ds(c, k, stats=None):
    w = tuple(np.fmax(x, F(0.0)) for x in c)
    w = mul_mv(k["agx_in"], w)
    w = tuple(np.fmin(np.fmax(dual_section(x, k, stats), F(0.0)), F(1.0)) for x in w)
    d = (w[0] * F(0.2126729) + w[1] * F(0.7151522)) + w[2] * F(0.0721750)
    w = tuple(np.fmin(np.fmax(d + (x - d) * F(1.3), F(0.0)), F(1.0)) for x in w)
    return mul_mv(k["agx_out"], w)


@np.errstate(all="ignore")
def smooth_step(x, edge0, edge1, span, stats=None, name=None):
    t = (x - edge0) / span
    below, above = x < edge0, x > edge1
    if name:
        _count_sides(stats, name + " below", below)
        _count_sides(stats, name + " above", above)
    return np.where(below, F(0.0), np.where(above, F(1.0), (t * t) * (F(3.0) - F(2.0) * t))).astype(np.float32)


@np.errstate(all="ignore")
def gt_curve(x, k, stats=None):
    """GTToneMappingCurveV2::evaluateCurve (tonemap.slang:358-380)."""
    x = f32a(x)
    negative = x < F(0.0)
    weight_linear = smooth_step(x, F(0.0), k["gt_mid"], k["gt_mid_span"], stats, "gt weight")
    weight_toe = F(1.0) - weight_linear
    shoulder = k["gt_ka"] + k["gt_kb"] * exp_rule(x * k["gt_kc"])
    toe = x < k["gt_lin_peak"]
    _count_sides(stats, "gt negative", negative)
    _count_sides(stats, "gt toe or linear", toe & ~negative)
    toe_mapped = k["gt_mid"] * _pow(x / k["gt_mid"], k["gt_toe"])
    return np.where(negative, F(0.0), np.where(toe, weight_toe * toe_mapped + weight_linear * x, shoulder)).astype(np.float32)


@np.errstate(all="ignore")
def eotf(n, k, stats=None):
    """eotfSt2084 (tonemap.slang:387-424)."""
    n = f32a(n)
    _count_sides(stats, "eotf below 0", n < 0)
    _count_sides(stats, "eotf above 1", n > 1)
    n = np.where(n < F(0.0), F(0.0), n)
    n = np.where(n > F(1.0), F(1.0), n).astype(np.float32)
    np_ = _pow(n, k["pq_inv_m2"])
    l = np_ - PQ_C1  # noqa: E741
    _count_sides(stats, "eotf l below 0", l < 0)
    l = np.where(l < F(0.0), F(0.0), l).astype(np.float32)  # noqa: E741
    l = l / (PQ_C2 - PQ_C3 * np_)  # noqa: E741
    l = _pow(l, k["pq_inv_m1"])  # noqa: E741
    return ((l * PQ_C) / REFERENCE_LUMINANCE).astype(np.float32)


@np.errstate(all="ignore")
def ictcp_to_rgb(ucs, k, stats=None):
    i, ct, cp = ucs
    l = (i + F(0.00860904) * ct) + F(0.11103) * cp  # noqa: E741
    m = (i - F(0.00860904) * ct) - F(0.11103) * cp
    s = (i + F(0.560031) * ct) - F(0.320627) * cp
    ll, ml, sl = eotf(l, k, stats), eotf(m, k, stats), eotf(s, k, stats)
    return (np.fmax((F(3.43661) * ll - F(2.50645) * ml) + F(0.0698454) * sl, F(0.0)), np.fmax((F(-0.79133) * ll + F(1.9836) * ml) - F(0.192271) * sl, F(0.0)),
            np.fmax((F(-0.0259499) * ll - F(0.0989137) * ml) + F(1.12486) * sl, F(0.0)))


@np.errstate(all="ignore")
def gt7_apply(rgb, k, stats=None):
    """GT7ToneMapping::applyToneMapping (tonemap.slang:632-665) on linear Rec.2020."""
    ucs = rgb_to_ictcp(rgb, k)
    skewed = tuple(gt_curve(x, k, stats) for x in rgb)
    skewed_ucs = rgb_to_ictcp(skewed, k)
    chroma = F(1.0) - smooth_step(ucs[0] / k["gt_target_ucs"], k["gt_fade_start"], k["gt_fade_end"], k["gt_fade_span"], stats, "gt chroma")
    scaled = ictcp_to_rgb((skewed_ucs[0], ucs[1] * chroma, ucs[2] * chroma), k, stats)
    out = []
    for ch in range(3):
        blended = k["gt_one_minus_blend"] * skewed[ch] + k["gt_blend"] * scaled[ch]
        _count_sides(stats, "gt above target", blended > k["gt_target"])
        out.append((k["gt_sdr"] * np.fmin(blended, k["gt_target"])).astype(np.float32))
    return tuple(out)


def gt7(c, k, stats=None):
    rec2020 = mul_mv(mat(XYZ_TO_REC2020), mul_mv(mat(REC709_TO_XYZ), c))
    return mul_mv(mat(XYZ_TO_REC709), mul_mv(mat(REC2020_TO_XYZ), gt7_apply(rec2020, k, stats)))


def tone_curve(c, tonemap_type: int, k, stats=None):
    if tonemap_type == ACES:
        return aces_fitted(c, stats)
    if tonemap_type == AGX:
        return agx_ds(c, k, stats)
    if tonemap_type == GT7:
        return gt7(c, k, stats)
    return c


# ---- sampling -----------------------------------------------------------------------------------------------------------------------------------
def decode(image, fmt: int):
    """(r, g, b, a) planes: format 0 has alpha 1.0, format 1 the binary16 decode."""
    image = np.ascontiguousarray(image)
    if fmt == 0:
        w = image.view(np.uint32)
        r, g, b = (c.reshape(w.shape) for c in unpack_b10g11r11(w.reshape(-1)))
        return r, g, b, np.ones(w.shape, dtype=np.float32)
    halves = image.view(np.uint16)
    return tuple(from_half_bits(halves[..., c]) for c in range(4))


@np.errstate(all="ignore")
def bilinear_repeat(plane, u, v):
    """The manual bilinear of oxc_apply_bloom with the repeat address mode: g = uv * size - 0.5, i = floor(g) converted saturating,
    f = g - floor(g); texel coordinates floor_mod(i, size) and that plus one, wrapped."""
    sh, sw = plane.shape
    out = []
    for coord, size in ((u, sw), (v, sh)):
        g = (coord * F(size) - F(0.5)).astype(np.float32)
        fl = np.floor(g)
        i0 = np.mod(cvt_i32_sat(fl), size)
        out.append((i0, np.mod(i0 + 1, size), (g - fl).astype(np.float32)))
    (x0, x1, fx), (y0, y1, fy) = out
    lerp = lambda a, b, t: (a + (b - a) * t).astype(np.float32)  # noqa: E731
    return lerp(lerp(plane[y0, x0], plane[y0, x1], fx), lerp(plane[y1, x0], plane[y1, x1], fx), fy)


# ---- the lens (steps 7-9) -----------------------------------------------------------------------------------------------------------------------
def pcg3d16(x, y, z):
    """pcg3d16 (lens.slang:9-19) in wrapping u32."""
    M = np.uint64(0xFFFFFFFF)
    x, y, z = ((np.asarray(v).astype(np.uint64) * np.uint64(12829) + np.uint64(47989)) & M for v in (x, y, z))
    x = (x + y * z) & M
    y = (y + z * x) & M
    z = (z + x * y) & M
    x = (x + y * z) & M
    y = (y + z * x) & M
    z = (z + x * y) & M
    return x >> np.uint64(16), y >> np.uint64(16), z >> np.uint64(16)


@np.errstate(all="ignore")
def chromatic_aberration(src_rgb, W, H, xs, ys, k):
    cx, cy = W // 2, H // 2
    rcp_x, rcp_y = F(1.0) / F(2 * cx), F(1.0) / F(2 * cy)
    dx, dy = (xs - cx).astype(np.float32), (ys - cy).astype(np.float32)
    shift = lambda d, mag, c, rcp: (((d * mag + F(c)) + F(0.5)) * rcp).astype(np.float32)  # noqa: E731
    red = bilinear_repeat(src_rgb[0], shift(dx, k["red_mag"], cx, rcp_x), shift(dy, k["red_mag"], cy, rcp_y))
    green = bilinear_repeat(src_rgb[1], shift(dx, k["green_mag"], cx, rcp_x), shift(dy, k["green_mag"], cy, rcp_y))
    blue = bilinear_repeat(src_rgb[2], xs.astype(np.float32) * rcp_x, ys.astype(np.float32) * rcp_y)
    return red, green, blue


@np.errstate(all="ignore")
def vignette_factor(W, H, xs, ys, amount):
    cx, cy = W // 2, H // 2
    pi_over_4 = F(PI_F * F(0.25))
    mask = []
    for d, c in ((np.abs(xs - cx), cx), (np.abs(ys - cy), cy)):
        m = cos_turn_rule((d.astype(np.float32) / F(c)) * F(amount) * pi_over_4)
        m = m * m
        mask.append(m * m)
    return np.fmin(np.fmax(mask[0] * mask[1], F(0.0)), F(1.0)).astype(np.float32)


def grain_divisor(scale) -> int:
    d = int(cvt_i32_sat(np.float32(F(scale) / F(8.0))))
    return 1 if d == 0 else d


@np.errstate(all="ignore")
def film_grain(xs, ys, scale, seed, stats=None):
    div = grain_divisor(scale)
    rx, ry, _ = pcg3d16(xs // div, ys // div, np.full(xs.shape, int(seed) & 0xFFFFFFFF, dtype=np.uint64))
    fine = [(r.astype(np.float32) * F(1.0 / 65536.0) - F(0.5)).astype(np.float32) for r in (rx, ry)]
    px, py = xs.astype(np.float32) / F(scale) + fine[0], ys.astype(np.float32) / F(scale) + fine[1]
    u = (px + py) * SIMPLEX_F2
    pix, piy = np.rint(px + u), np.rint(py + u)  # round half to even
    v = (pix + piy) * SIMPLEX_G2
    fx, fy = px - (pix - v), py - (piy - v)
    length = np.sqrt(fx * fx + fy * fy)
    return (F(1.0) - F(2.0) * _exp2((-length) * F(3.0))).astype(np.float32)


# ---- step 11: the store -------------------------------------------------------------------------------------------------------------------------
@np.errstate(all="ignore")
def srgb_encode(c, stats=None):
    """The shared srgb_encode; `stats` receives which side of its comparison each value took."""
    _count_sides(stats, "srgb linear", saturate(c) <= F(0.0031308))
    return shared_srgb_encode(c)


def store(rgb, alpha, output_format: int, stats=None) -> np.ndarray:
    r, g, b = (srgb_encode(c, stats) for c in rgb) if output_format != OUT_RGBA8_UNORM else rgb
    if output_format == OUT_BGRA8_SRGB:
        r, b = b, r
    return pack_unorm4x8(r, g, b, alpha)


# ---- the whole call -----------------------------------------------------------------------------------------------------------------------------
@np.errstate(all="ignore")
def apply_tonemap(image, fmt: int, output_format: int, scene_flags: int, tonemap_type: int, bloom=None, exposure_words=None, exposure=1.0,
                  chromatic_aberration_amount=0.5, vignette_amount=0.5, film_grain_scale=1.0, film_grain_amount=0.5, film_grain_seed=0, bloom_intensity=0.1,
                  stats=None) -> np.ndarray:
    """uint32 [H, W].  `bloom`: U level 0 (W // 2 x H // 2, the source's format), read with HAS_BLOOM; `exposure_words`: the exposure buffer's
    two uint32, read with HAS_EYE_ADAPTATION."""
    image = np.asarray(image)
    H, W = image.shape[:2]
    k = constants(chromatic_aberration_amount if scene_flags & HAS_CHROMATIC_ABERRATION else 0.0)
    r, g, b, a = decode(image, fmt)
    ys, xs = np.mgrid[0:H, 0:W].astype(np.int64)
    e = np.asarray(exposure_words, dtype=np.uint32).view(np.float32)[1] if scene_flags & HAS_EYE_ADAPTATION else F(exposure)
    c = [(p * e).astype(np.float32) for p in (r, g, b)]
    if scene_flags & HAS_BLOOM:
        u = ((xs.astype(np.float32) + F(0.5)) / F(W)).astype(np.float32)
        v = ((ys.astype(np.float32) + F(0.5)) / F(H)).astype(np.float32)
        planes = decode(bloom, fmt)
        assert planes[0].shape == (H // 2, W // 2)
        c = [(c[ch] + bilinear_repeat(planes[ch], u, v) * F(bloom_intensity)).astype(np.float32) for ch in range(3)]
    c = list(tone_curve(tuple(c), tonemap_type, k, stats))
    if scene_flags & HAS_CHROMATIC_ABERRATION:
        c = list(chromatic_aberration((r, g, b), W, H, xs, ys, k))
    if scene_flags & HAS_VIGNETTE:
        factor = vignette_factor(W, H, xs, ys, vignette_amount)
        c = [(p * factor).astype(np.float32) for p in c]
    if scene_flags & HAS_FILM_GRAIN:
        grain = film_grain(xs, ys, film_grain_scale, film_grain_seed, stats)
        c = [(p + (grain * np.fmin(p, F(1.0) - p)) * F(film_grain_amount)).astype(np.float32) for p in c]
    alpha = a if scene_flags & TRANSPARENT_BACKGROUND else np.ones((H, W), dtype=np.float32)
    return store(tuple(c), alpha, output_format, stats)
