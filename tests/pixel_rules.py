"""The numeric rules the checkers share, one copy each: the Python counterpart of include/oxcull_pixel_device.hpp and oxcull_device.hpp.
Binary32 in the stated evaluation order, no contraction, IEEE division and square root, the closed forms of log2 / exp2 / pow and of the
rotation pair in binary64 rounded once, saturating conversions, the half and small-float packers.  A checker (tests/*_model.py) imports
what it uses from here; no checker takes a numeric rule from another checker, and none defines a function under a name this module has
(tests/test_pixel_rules.py holds both).  What a checker still imports from another checker is a step or a constant of that checker's
own pass.
Shapes: the closed forms (log2, exp2, pow, the small-float packers) return at least one dimension, as they always have; every rule of the
section "the per-pixel rules of oxcull_pixel_device.hpp" returns the shape of its input, a scalar's included, and a caller that wants
one dimension more asks for it itself."""
from __future__ import annotations

import numpy as np

F = np.float32
HALF_NAN = 0x7E00
SQRT2_F = F(1.41421356)
INV_LN2 = float.fromhex("0x1.71547652b82fep+0")
LN2 = float.fromhex("0x1.62e42fefa39efp-1")
LOG_C = [1.0 / k for k in (3.0, 5.0, 7.0, 9.0, 11.0, 13.0, 15.0, 17.0)]  # the binary64 quotients
EXP_C = [1.0, 1.0, 1.0 / 2.0, 1.0 / 6.0, 1.0 / 24.0, 1.0 / 120.0, 1.0 / 720.0, 1.0 / 5040.0, 1.0 / 40320.0, 1.0 / 362880.0, 1.0 / 3628800.0,
         1.0 / 39916800.0, 1.0 / 479001600.0, 1.0 / 6227020800.0]
PIO2 = float.fromhex("0x1.921fb54442d18p+0")
INV_TWO_PI = float.fromhex("0x1.45f306dc9c883p-3")
SIN_C = [float.fromhex(h) for h in ("-0x1.5555555555555p-3", "0x1.1111111111111p-7", "-0x1.a01a01a01a01ap-13", "0x1.71de3a556c734p-19")]
COS_C = [float.fromhex(h) for h in ("-0x1.0000000000000p-1", "0x1.5555555555555p-5", "-0x1.6c16c16c16c17p-10", "0x1.a01a01a01a01ap-16",
                                    "-0x1.27e4fb7789f5cp-22")]


def f32a(v) -> np.ndarray:
    return np.asarray(v, dtype=np.float32)


def _u32(a) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(a)).view(np.uint32)


# ---- small rules ----------------------------------------------------------------------------------------------------------------------------
def saturate(x):
    """min(max(x, 0), 1): a NaN gives 0."""
    return np.fmin(np.fmax(f32a(x), F(0.0)), F(1.0))


def sign(a):
    a = f32a(a)
    return np.where(a > 0, F(1.0), np.where(a < 0, F(-1.0), F(0.0))).astype(np.float32)


def cvt_i32_sat(v) -> np.ndarray:
    """float -> i32, saturating, NaN -> 0 (truncation inside the range; every caller passes a floor)."""
    v = np.asarray(v, dtype=np.float64)
    return np.where(np.isnan(v), 0.0, np.clip(v, -2147483648.0, 2147483647.0)).astype(np.int64)


def cvt_u32_sat(v) -> np.ndarray:
    v = np.asarray(v, dtype=np.float64)
    return np.where(np.isnan(v), 0.0, np.clip(v, 0.0, 4294967295.0)).astype(np.int64)


# ---- log2, exp2 and pow ---------------------------------------------------------------------------------------------------------------------
@np.errstate(all="ignore")
def log2_f64(x) -> np.ndarray:
    """The binary64 value of the log2 rule before its rounding, for binary32 x.  x < 2^-126 (zero, denormal, negative) or NaN: -Inf;
    +Inf: +Inf."""
    x = np.atleast_1d(f32a(x))
    bits = x.view(np.uint32)
    e = ((bits >> np.uint32(23)) & np.uint32(0xFF)).astype(np.int64) - 127
    m = ((bits & np.uint32(0x7FFFFF)) | np.uint32(0x3F800000)).view(np.float32)  # in [1, 2)
    big = m > SQRT2_F
    m = np.where(big, m * F(0.5), m)  # exact
    e = e + big
    f = m.astype(np.float64) - 1.0
    s = f / (2.0 + f)
    z = s * s
    p = LOG_C[7]
    for c in LOG_C[6::-1]:
        p = p * z + c
    p = p * z + 1.0
    r = e.astype(np.float64) + ((2.0 * s) * p) * INV_LN2
    r = np.where(x >= F(2.0 ** -126), r, -np.inf)
    return np.where(x == F(np.inf), np.inf, r)


def log2_rule(x) -> np.ndarray:
    return log2_f64(x).astype(np.float32)


@np.errstate(all="ignore")
def exp2_f64_round(y) -> np.ndarray:
    """exp2 of a binary64 y rounded to binary32 once: the second half of the pow rule."""
    y = np.atleast_1d(np.asarray(y, dtype=np.float64))
    k = np.floor(y + 0.5)
    r = y - k
    t = r * LN2
    q = EXP_C[13]
    for c in EXP_C[12::-1]:
        q = q * t + c
    ki = np.where(np.isfinite(k), np.clip(k, -160, 160), 0).astype(np.int64)
    scale = ((ki + 1023).astype(np.uint64) << np.uint64(52)).view(np.float64)
    res = (q * scale).astype(np.float32)
    res = np.where(y <= -160.0, F(0.0), np.where(y >= 160.0, F(np.inf), res))
    return np.where(np.isnan(y), F(np.nan), res).astype(np.float32)


def exp2_rule(t) -> np.ndarray:
    return exp2_f64_round(np.atleast_1d(f32a(t)).astype(np.float64))


@np.errstate(all="ignore")
def pow_rule(v, p) -> np.ndarray:
    """pow(v, p) for binary32 v >= 0 (the caller's max(.., 0) has run) and a binary32 exponent, array or scalar: exp2((double)p * L(v)) in
    binary64, rounded once."""
    return exp2_f64_round(np.atleast_1d(f32a(p)).astype(np.float64) * log2_f64(v))


# ---- the rotation pair ----------------------------------------------------------------------------------------------------------------------
def cos_sin_turn(t):
    """(cos, sin) of 2 pi t for binary32 t in [0, 1): exact reduction to an octant, binary64 Horner, one rounding to binary32."""
    t = np.asarray(t, dtype=np.float32)
    q4 = t * F(4.0)        # exact
    k = np.floor(q4)
    f = q4 - k             # exact, in [0, 1)
    swap = f > F(0.5)
    g = np.where(swap, F(1.0) - f, f)  # exact, in [0, 0.5]
    a = g.astype(np.float64) * PIO2
    z = a * a
    ps = ((SIN_C[3] * z + SIN_C[2]) * z + SIN_C[1]) * z + SIN_C[0]
    s = a + (a * z) * ps
    pc = (((COS_C[4] * z + COS_C[3]) * z + COS_C[2]) * z + COS_C[1]) * z + COS_C[0]
    c = 1.0 + z * pc
    sf, cf = s.astype(np.float32), c.astype(np.float32)
    sq, cq = np.where(swap, cf, sf), np.where(swap, sf, cf)
    ki = k.astype(np.int64)
    cos = np.where(ki == 0, cq, np.where(ki == 1, -sq, np.where(ki == 2, -cq, sq)))
    sin = np.where(ki == 0, sq, np.where(ki == 1, cq, np.where(ki == 2, -sq, -cq)))
    return cos.astype(np.float32), sin.astype(np.float32)


# ---- the per-pixel rules of oxcull_pixel_device.hpp ------------------------------------------------------------------------------------------
def count(counts, name, n=1):
    """counts[name] += n, n a number or a mask (its true elements); nothing where counts is None."""
    if counts is not None:
        counts[name] = counts.get(name, 0) + int(np.asarray(n).sum())


def frac(x):
    """x - floor(x)."""
    return (x - np.floor(x)).astype(np.float32)


@np.errstate(all="ignore")
def lerp(a, b, t):
    """lerp_f: a + (b - a) * t."""
    return (a + (b - a) * t).astype(np.float32)


def clamp(x, lo, hi):
    """min(max(x, lo), hi): a NaN gives lo."""
    return np.fmin(np.fmax(f32a(x), F(lo)), F(hi))


@np.errstate(all="ignore")
def exp_rule(x):
    """exp_rule: exp(x) = exp2_f64_round((double)x * log2(e))."""
    x = f32a(x)
    return exp2_f64_round(x.astype(np.float64) * INV_LN2).reshape(x.shape)


@np.errstate(all="ignore")
def cos_sin_angle_rule(a):
    """cos_sin_angle_rule: (cos(a), sin(a)) of a binary32 angle, both NaN for a non-finite a; else u = (double)|a| / (2 pi), t = (float)(u -
    floor(u)), t == 1 becomes 0, the pair of the turn t, the sine negated for a < 0."""
    a = f32a(a)
    u = np.abs(a).astype(np.float64) * INV_TWO_PI
    u = np.where(np.isfinite(u), u, 0.0)
    t = (u - np.floor(u)).astype(np.float32)
    t = np.where(t == F(1.0), F(0.0), t).astype(np.float32)
    cs, sn = cos_sin_turn(t)
    sn = np.where(a < 0, -sn, sn)
    ok = np.isfinite(a)
    return np.where(ok, cs, F(np.nan)).astype(np.float32), np.where(ok, sn, F(np.nan)).astype(np.float32)


def cos_turn_rule(a):
    """cos_turn_rule: cos(a) of a binary32 angle, the cosine of cos_sin_angle_rule bit for bit."""
    return cos_sin_angle_rule(a)[0]


@np.errstate(all="ignore")
def srgb_decode(byte):
    """srgb_decode: c = f32(byte) / 255; c <= 0.04045 ? c / 12.92 : pow_rule((c + 0.055) / 1.055, 2.4)."""
    c = np.asarray(byte).astype(np.float32) / F(255.0)
    return np.where(c <= F(0.04045), c / F(12.92), pow_rule((c + F(0.055)) / F(1.055), F(2.4)).reshape(c.shape)).astype(np.float32)


@np.errstate(all="ignore")
def srgb_encode(c):
    """srgb_encode: c = saturate(c); c <= 0.0031308 ? c * 12.92 : 1.055 * pow_rule(c, 0.4166666666666667f) - 0.055."""
    c = saturate(c)
    return np.where(c <= F(0.0031308), c * F(12.92), F(1.055) * pow_rule(c, F(0.4166666666666667)).reshape(c.shape) - F(0.055)).astype(np.float32)


@np.errstate(all="ignore")
def srgb_unorm_encode(x):
    """The encode inside srgb_unorm, not saturated: x <= 0.0031308 ? 12.92 * x : 1.055 * pow_rule(x, 1.0f / 2.4f) - 0.055."""
    x = f32a(x)
    return np.where(x <= F(0.0031308), F(12.92) * x, F(1.055) * pow_rule(x, F(1.0) / F(2.4)).reshape(x.shape) - F(0.055)).astype(np.float32)


@np.errstate(all="ignore")
def unorm8(e):
    """pack_unorm, one channel of pack_unorm4x8: u32(floor(saturate(e) * 255.0 + 0.5)); a NaN gives 0."""
    return cvt_u32_sat(np.floor(saturate(e) * F(255.0) + F(0.5))).astype(np.uint32)


@np.errstate(all="ignore")
def axis_clamp(p, n: int):
    """axis_at<false>: (i0, i1, f) of the manual bilinear at the normalised coordinate p of a side of n texels, g = p * n - 0.5, f = g -
    floor(g), both indices in [0, n - 1] for every bit pattern of p."""
    g = (p * F(n) - F(0.5)).astype(np.float32)
    fl = np.floor(g)
    i = cvt_i32_sat(fl)
    return np.clip(i, 0, n - 1), np.clip(i + 1, 0, n - 1), (g - fl).astype(np.float32)


# ---- vectors and matrices -------------------------------------------------------------------------------------------------------------------
def cross(a, b):
    """cross(a, b).x = a.y * b.z - a.z * b.y and its rotations, each product rounded before the subtraction."""
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def length(a):
    return np.sqrt(dot(a, a))


def normalize(a):
    ln = length(a)
    return (a[0] / ln, a[1] / ln, a[2] / ln)


def _m(m, r, c):
    return m[..., c * 4 + r]


def mul_mp(m, p):
    """mul(M, float4(p, 1)), every row ((m0 p0 + m1 p1) + m2 p2) + m3, in the dtype of its operands (the checkers run it in binary32, a
    tolerance measurement in binary64); m column-major [..., 16], p [..., 3] -> [..., 4]."""
    return np.stack([((m[..., r] * p[..., 0] + m[..., 4 + r] * p[..., 1]) + m[..., 8 + r] * p[..., 2]) + m[..., 12 + r] for r in range(4)], axis=-1)


def unproject(m, u, v, d):
    """Camera::unproject_uv (scene.slang:189-193): (M (uv * 2 - 1, d, 1)).xyz / w, rows ((m0 a + m1 b) + m2 c) + m3."""
    nx, ny = u * F(2.0) - F(1.0), v * F(2.0) - F(1.0)
    h = [((_m(m, i, 0) * nx + _m(m, i, 1) * ny) + _m(m, i, 2) * d) + _m(m, i, 3) for i in range(4)]
    return h[0] / h[3], h[1] / h[3], h[2] / h[3]


# ---- octahedral normals ---------------------------------------------------------------------------------------------------------------------
def oct_to_vec3(ex, ey):
    """com::oct_to_vec3 (common/encoding.slang:7-15)."""
    vz = (F(1.0) - np.abs(ex)) - np.abs(ey)
    sx = np.where(ex >= 0, F(1.0), F(-1.0))
    sy = np.where(ey >= 0, F(1.0), F(-1.0))
    neg = vz < 0
    vx = np.where(neg, (F(1.0) - np.abs(ey)) * sx, ex)
    vy = np.where(neg, (F(1.0) - np.abs(ex)) * sy, ey)
    return normalize((vx, vy, vz))


def vec3_to_oct(v):
    """com::vec3_to_oct (common/encoding.slang:17-21): what visbuffer_decode stores."""
    s = F(1.0) / ((np.abs(v[0]) + np.abs(v[1])) + np.abs(v[2]))
    px, py = v[0] * s, v[1] * s
    sx = np.where(px >= 0, F(1.0), F(-1.0))
    sy = np.where(py >= 0, F(1.0), F(-1.0))
    return np.where(v[2] <= 0, (F(1.0) - np.abs(py)) * sx, px), np.where(v[2] <= 0, (F(1.0) - np.abs(px)) * sy, py)


def decode_normal(normal_u16x4):
    """.b and .a of the R16G16B16A16Sfloat image as binary32 (exact), then flat_N = normalize(oct_to_vec3(.ba))."""
    h = np.ascontiguousarray(np.asarray(normal_u16x4)).view(np.uint16)
    ex, ey = h[..., 2].view(np.float16).astype(np.float32), h[..., 3].view(np.float16).astype(np.float32)
    return normalize(oct_to_vec3(ex, ey))


# ---- halves and packed formats --------------------------------------------------------------------------------------------------------------
def to_half_bits(x) -> np.ndarray:
    """binary32 -> binary16, round to nearest even, denormals kept."""
    with np.errstate(all="ignore"):
        return f32a(x).astype(np.float16).view(np.uint16)


def from_half_bits(h) -> np.ndarray:
    return np.asarray(h, dtype=np.uint16).view(np.float16).astype(np.float32)


def channel_half(x) -> np.ndarray:
    """binary16 bits, round to nearest even, denormals kept, every NaN 0x7E00."""
    x = f32a(x)
    return np.where(np.isnan(x), np.uint16(HALF_NAN), to_half_bits(x)).astype(np.uint16)


@np.errstate(all="ignore")
def pack_unorm4x8(e0, e1, e2, e3) -> np.ndarray:
    """byte k = u32(floor(saturate(e_k) * 255.0 + 0.5)), component 0 in the low byte."""
    out = np.zeros(np.shape(e0), dtype=np.uint32)
    for k, e in enumerate((e0, e1, e2, e3)):
        out |= unorm8(e) << np.uint32(8 * k)
    return out


def pack_ufloat(v, mbits: int) -> np.ndarray:
    """binary32 -> the unsigned small float with 5 exponent bits and `mbits` mantissa bits (UF11: 6, UF10: 5), rule 8 of the header."""
    v = np.atleast_1d(np.asarray(v, dtype=np.float32))
    bits = v.view(np.uint32).astype(np.int64)
    top = (1 << mbits) - 1
    e = (bits >> 23) - 127 + 15
    m = bits & 0x7FFFFF
    normal = (e << mbits) | (m >> (23 - mbits))
    sh = np.clip((23 - mbits) + (1 - e), 0, 63)
    denormal = np.where(sh > 24, 0, (0x800000 | m) >> sh)
    out = np.where(e >= 31, (30 << mbits) | top, np.where(e >= 1, normal, denormal))
    out = np.where(bits == 0x7F800000, 31 << mbits, out)
    out = np.where((bits >> 31) != 0, 0, out)
    return np.where(np.isnan(v), (31 << mbits) | top, out).astype(np.uint32)


def unpack_ufloat(v, mbits: int) -> np.ndarray:
    """The unsigned small float with 5 exponent bits and `mbits` mantissa bits -> binary32, exact."""
    v = np.atleast_1d(np.asarray(v)).astype(np.uint32)
    e, m = v >> np.uint32(mbits), v & np.uint32((1 << mbits) - 1)
    normal = (((e + np.uint32(112)) << np.uint32(23)) | (m << np.uint32(23 - mbits))).astype(np.uint32).view(np.float32)
    out = np.where(e == 0, m.astype(np.float32) * F(2.0 ** -(14 + mbits)), normal)
    return np.where(e == 31, np.where(m != 0, F(np.nan), F(np.inf)), out).astype(np.float32)


def pack_b10g11r11(r, g, b) -> np.ndarray:
    return pack_ufloat(r, 6) | (pack_ufloat(g, 6) << np.uint32(11)) | (pack_ufloat(b, 5) << np.uint32(22))


def unpack_b10g11r11(w):
    w = np.asarray(w).astype(np.uint32)
    return unpack_ufloat(w & np.uint32(0x7FF), 6), unpack_ufloat((w >> np.uint32(11)) & np.uint32(0x7FF), 6), unpack_ufloat(w >> np.uint32(22), 5)
