"""The numpy checker of oxc_generate_sky_ibl: steps 11-15 of its header block in include/oxcull.h, vectorised over the texels of the cube
and their 64 samples ([texels, 64] arrays).  Every binary32 operation is one numpy float32 operation in the order the header states, the
closed forms of acos / atan2 are the same binary64 operations the device runs.  The shared rules -- the cos / sin of an angle, frac, lerp and the clamp
bilinear's axis among them -- come from pixel_rules; intersect and the host constants are local copies of the LUT checker's own steps (no
checker takes a numeric rule from another).  An image is
uint16 [..., 4] of binary16 bits; the cube is [6, S, S, 4].  `counts`, when given, receives how many texels or samples took each side of the
branches the tests must not leave empty."""
from __future__ import annotations

import math

import numpy as np

from pixel_rules import axis_clamp, channel_half, cos_sin_angle_rule, count, cross, dot, f32a, frac, from_half_bits, length, lerp, normalize, saturate

F = np.float32
PI_F, TAU_F = F(3.1415926535897932384626433832795), F(6.283185307179586476925286766559)
PI_D, PIO2_D, PIO4_D = (float.fromhex(h) for h in ("0x1.921fb54442d18p+1", "0x1.921fb54442d18p+0", "0x1.921fb54442d18p-1"))
ATAN_FOLD = float.fromhex("0x1.a827999fcef32p-2")  # sqrt(2) - 1
ATAN_C = [1.0 / k for k in range(1, 40, 2)]        # the binary64 quotients 1, 1/3 .. 1/39
HALF_MAX = F(65504.0)
SAMPLES = 64
GOLDEN, VDC_SCALE = F(0.61803398875), F(2.3283064365386963e-10)
NOISE = (F(0.06711056), F(0.00583715), F(52.9829189))
UP_LIMIT, SIDE_LIMIT, PLANE_LIMIT, BLEND = F(0.999), F(1e-5), F(1e-20), F(0.02)
# CUBE_MAP_FACE_ROTATION (sky_ibl.slang:21-30), the nine scalars of every face in the constructor's order: row r is scalars 3 r .. 3 r + 2
CUBE_FACE = np.array([[+0, +0, -1, +0, -1, +0, -1, +0, +0], [+0, +0, +1, +0, -1, +0, +1, +0, +0], [+1, +0, +0, +0, +0, -1, +0, +1, +0],
                      [+1, +0, +0, +0, +0, +1, +0, -1, +0], [+1, +0, +0, +0, -1, +0, +0, +0, -1], [-1, +0, +0, +0, -1, +0, +0, +0, +1]], dtype=np.float32)
CLASSES = ("samples_hit_planet", "samples_miss_planet", "side_vec_fallback", "side_vec_normalized", "light_on_plane_fallback", "light_on_plane_normalized",
           "up_is_x", "up_is_y", "has_history", "no_history", "clamped_at_half_max", "sanitized_sample")


# ---- step 11: the closed forms ---------------------------------------------------------------------------------------------------------------------
@np.errstate(all="ignore")
def atan2_f64(y, x) -> np.ndarray:
    """A(y, x) of step 11 on binary64 arrays."""
    y, x = np.broadcast_arrays(np.asarray(y, dtype=np.float64), np.asarray(x, dtype=np.float64))
    ax, ay = np.abs(x), np.abs(y)
    bigger = ax > ay
    mx, mn = np.where(bigger, ax, ay), np.where(bigger, ay, ax)
    a = mn / mx
    fold = a > ATAN_FOLD
    t = np.where(fold, (a - 1.0) / (a + 1.0), a)
    z = t * t
    p = ATAN_C[19]
    for c in ATAN_C[18::-1]:
        p = c - p * z
    r = t * p
    r = np.where(fold, PIO4_D + r, r)
    r = np.where(ay > ax, PIO2_D - r, r)
    r = np.where(x < 0.0, PI_D - r, r)
    r = np.where(y < 0.0, -r, r)
    r = np.where(mx == 0.0, 0.0, r)
    return np.where(np.isnan(x) | np.isnan(y), np.nan, r)


@np.errstate(all="ignore")
def atan2_rule(y, x) -> np.ndarray:
    return atan2_f64(f32a(y).astype(np.float64), f32a(x).astype(np.float64)).astype(np.float32)


@np.errstate(all="ignore")
def acos_rule(x) -> np.ndarray:
    x = f32a(x)
    xd = x.astype(np.float64)
    r = atan2_f64(np.sqrt(1.0 - xd * xd), xd).astype(np.float32)
    return np.where(np.abs(x) <= F(1.0), r, F(np.nan)).astype(np.float32)


def radical_inverse_vdc(i) -> np.ndarray:
    """sky_ibl.slang:32-39: the five swaps as written, then f32(bits) * 2.3283064365386963e-10."""
    b = np.asarray(i, dtype=np.uint64) & 0xFFFFFFFF
    m = 0xFFFFFFFF
    b = ((b << 16) | (b >> 16)) & m
    b = (((b & 0x55555555) << 1) | ((b & 0xAAAAAAAA) >> 1)) & m
    b = (((b & 0x33333333) << 2) | ((b & 0xCCCCCCCC) >> 2)) & m
    b = (((b & 0x0F0F0F0F) << 4) | ((b & 0xF0F0F0F0) >> 4)) & m
    b = (((b & 0x00FF00FF) << 8) | ((b & 0xFF00FF00) >> 8)) & m
    return b.astype(np.uint32).astype(np.float32) * VDC_SCALE


# ---- local copies of the LUT checker's rules -------------------------------------------------------------------------------------------------------
def safe_sqrt(x):
    return np.sqrt(np.fmax(F(0.0), x))


@np.errstate(all="ignore")
def intersect_has(o, d, radius):
    """Rule 1, whether there is a value."""
    a, b, c = dot(d, d), F(2.0) * dot(d, o), dot(o, o) - radius * radius
    delta = b * b - (F(4.0) * a) * c
    sq, den = np.sqrt(delta), F(2.0) * a
    s0, s1 = (-b + F(-1.0) * sq) / den, (-b + sq) / den
    return ~(delta < 0) & ~((s0 < 0) & (s1 < 0))


def sample_rgba(lut, u, v):
    """SampleLevel(LinearSamplerClamped, (u, v), 0) of a uint16 [H, W, 4] image: the manual bilinear, clamp mode, on the four decoded halves."""
    H, W = lut.shape[:2]
    planes = [from_half_bits(lut[..., c]) for c in range(4)]
    x0, x1, fx = axis_clamp(u, W)
    y0, y1, fy = axis_clamp(v, H)
    return tuple(lerp(lerp(p[y0, x0], p[y0, x1], fx), lerp(p[y1, x0], p[y1, x1], fx), fy) for p in planes)


@np.errstate(all="ignore")
def constants(planet_radius, atmos_radius, camera_y) -> dict:
    """The host constants: binary64 from the binary32 arguments, each rounded to binary32 once."""
    ar, pr = float(F(atmos_radius)), float(F(planet_radius))
    k = {"H": F(math.sqrt(max(0.0, ar * ar - pr * pr)))}
    min_altitude = pr + float(F(0.001))
    k["eye_altitude"] = F(np.fmax(np.float64(F(camera_y)) * float(F(0.01)) + min_altitude, min_altitude))
    h = np.float64(k["eye_altitude"])
    horizon = np.sqrt(np.fmax(0.0, h * h - pr * pr))
    beta = np.arccos(horizon / h)
    k["beta"], k["zenith_horizon_angle"] = F(beta), F(math.pi - beta)
    return k


# ---- steps 12 - 15 -----------------------------------------------------------------------------------------------------------------------------------
@np.errstate(all="ignore")
def output_dirs(cube_size: int):
    """Step 12's output_dir of every texel, three [6 S S] arrays in the cube's order, with (face, y, x)."""
    S = int(cube_size)
    face, y, x = (a.reshape(-1) for a in np.mgrid[0:6, 0:S, 0:S])
    u, v = (x.astype(np.float32) + F(0.5)) / F(S), (y.astype(np.float32) + F(0.5)) / F(S)
    vec = (u * F(2.0) - F(1.0), v * F(2.0) - F(1.0), np.full(u.shape, F(-1.0)))
    m = CUBE_FACE[face]
    return normalize(tuple((m[:, 3 * r] * vec[0] + m[:, 3 * r + 1] * vec[1]) + m[:, 3 * r + 2] * vec[2] for r in range(3))), (face, y, x)


@np.errstate(all="ignore")
def cosine_hemisphere_sample(i, rotation):
    """Step 13's local, for sample indices i and rotations broadcastable against them."""
    u1 = (f32a(i) + F(0.5)) / F(SAMPLES)
    u2 = frac(radical_inverse_vdc(i) + rotation)
    r, phi = np.sqrt(u1), TAU_F * u2
    cs, sn = cos_sin_angle_rule(phi)
    return r * cs, r * sn, np.sqrt(np.fmax(F(0.0), F(1.0) - u1))


@np.errstate(all="ignore")
def sky_view_uv(K, view_size, hit, view_zenith_cos_angle, light_on_plane):
    """sky_view_params_to_lut_uv with the host constants."""
    zha, beta = K["zenith_horizon_angle"], K["beta"]
    angle = acos_rule(view_zenith_cos_angle)
    ca = angle / zha
    ca = F(1.0) - ca
    ca = safe_sqrt(ca)
    ca = F(1.0) - ca
    cb = (angle - zha) / beta
    cb = safe_sqrt(cb)
    uy = np.where(hit, cb * F(0.5) + F(0.5), ca * F(0.5)).astype(np.float32)
    theta = atan2_rule(-light_on_plane[1], -light_on_plane[0])
    ux = (theta + PI_F) / (F(2.0) * PI_F)
    fw, fh = F(view_size[0]), F(view_size[1])
    return (ux + F(0.5) / fw) * (fw / (fw + F(1.0))), (uy + F(0.5) / fh) * (fh / (fh + F(1.0)))


@np.errstate(all="ignore")
def illuminance(K, planet_radius, sky_view, eye, d, sun_dir, counts=None, uv_out=None):
    """Step 14 for directions d (three arrays): the sanitized sample, three arrays."""
    sun_dir = tuple(F(s) for s in sun_dir)
    height = length(eye)
    up = tuple(e / height for e in eye)
    c = dot(d, up)
    side_raw = cross(up, d)
    keep_side = length(side_raw) > SIDE_LIMIT
    side_n = normalize(side_raw)
    side = tuple(np.where(keep_side, s, F(f)).astype(np.float32) for s, f in zip(side_n, (1.0, 0.0, 0.0)))
    count(counts, "side_vec_fallback", ~keep_side)
    count(counts, "side_vec_normalized", keep_side)
    forward = normalize(cross(side, up))
    sun = normalize(sun_dir)
    lx, ly = dot(sun, forward), dot(sun, side)
    len_sq = lx * lx + ly * ly
    inv = F(1.0) / np.sqrt(len_sq)
    keep = len_sq > PLANE_LIMIT
    count(counts, "light_on_plane_fallback", ~keep)
    count(counts, "light_on_plane_normalized", keep)
    lop = (np.where(keep, lx * inv, F(1.0)).astype(np.float32), np.where(keep, ly * inv, F(0.0)).astype(np.float32))
    hit = intersect_has(eye, d, F(planet_radius))
    count(counts, "samples_hit_planet", hit)
    count(counts, "samples_miss_planet", ~hit)
    u, v = sky_view_uv(K, (sky_view.shape[1], sky_view.shape[0]), hit, c, lop)
    if uv_out is not None:
        uv_out.extend((u, v, hit))
    r, g, b, a = sample_rgba(sky_view, u, v)
    raw = (r * a, g * a, b * a)
    count(counts, "sanitized_sample", ~(np.isfinite(raw[0]) & np.isfinite(raw[1]) & np.isfinite(raw[2])))
    return tuple(np.where(np.isfinite(x), x, F(0.0)).astype(np.float32) for x in raw)


@np.errstate(all="ignore")
def sun_color(K, planet_radius, atmos_radius, transmittance, h, mu):
    """Rule 3: the transmittance sample at (h, mu)."""
    pr, ar = F(planet_radius), F(atmos_radius)
    rho = safe_sqrt(h * h - pr * pr)
    discriminant = (h * h) * (mu * mu - F(1.0)) + ar * ar
    d = np.fmax(F(0.0), -h * mu + safe_sqrt(discriminant))
    d_min, d_max = ar - h, rho + K["H"]
    return sample_rgba(transmittance, (d - d_min) / (d_max - d_min), rho / K["H"])[:3]


@np.errstate(all="ignore")
def sky_ibl(planet_radius, atmos_radius, sky_view, transmittance, cube, camera_position, sun_dir, sun_intensity, sun_ambient_strength, frame_index,
            counts=None) -> np.ndarray:
    """One call: the cube after it, uint16 [6, S, S, 4]; `cube` is the cube before it and is not changed."""
    cube = np.asarray(cube, dtype=np.uint16)
    S = cube.shape[1]
    K = constants(planet_radius, atmos_radius, camera_position[1])
    out_dir, (face, y, x) = output_dirs(S)
    n = face.size
    zero = np.zeros(n, np.float32)
    up_x = ~(np.abs(out_dir[1]) < UP_LIMIT)
    count(counts, "up_is_x", up_x)
    count(counts, "up_is_y", ~up_x)
    up = (np.where(up_x, F(1.0), F(0.0)).astype(np.float32), np.where(up_x, F(0.0), F(1.0)).astype(np.float32), zero)
    tangent = normalize(cross(up, out_dir))
    bitangent = cross(out_dir, tangent)
    history = [from_half_bits(cube[..., c]).reshape(-1) for c in range(4)]
    has_history = (history[3] > 0) & np.isfinite(history[0]) & np.isfinite(history[1]) & np.isfinite(history[2])
    count(counts, "has_history", has_history)
    count(counts, "no_history", ~has_history)
    px = x.astype(np.float32) + face.astype(np.float32) * F(37.0)
    py = y.astype(np.float32) + face.astype(np.float32) * F(17.0)
    base_rotation = frac(NOISE[2] * frac(px * NOISE[0] + py * NOISE[1]))
    turned = frac(base_rotation + np.uint32(int(frame_index) & 0xFFFFFFFF).astype(np.float32) * GOLDEN)
    rotation = np.where(has_history, turned, base_rotation).astype(np.float32)

    i = np.arange(SAMPLES, dtype=np.uint32)[None, :]
    local = cosine_hemisphere_sample(i, rotation[:, None])
    col = lambda v: tuple(c[:, None] for c in v)  # noqa: E731
    T, B, O = col(tangent), col(bitangent), col(out_dir)
    d = normalize(tuple((local[0] * T[k] + local[1] * B[k]) + local[2] * O[k] for k in range(3)))
    eye = (F(0.0), K["eye_altitude"], F(0.0))
    samples = illuminance(K, planet_radius, sky_view, eye, d, sun_dir, counts)

    sun_in = tuple(F(s) for s in sun_dir)
    sun_cos_zenith = (sun_in[0] * F(0.0) + sun_in[1] * F(1.0)) + sun_in[2] * F(0.0)
    colour = sun_color(K, planet_radius, atmos_radius, transmittance, eye[1], sun_cos_zenith)
    sun_facing = saturate(dot(out_dir, sun_in))
    out = []
    clamped = np.zeros(n, bool)
    for c in range(3):
        total = np.zeros(n, np.float32)
        for k in range(SAMPLES):  # ascending sample order
            total = total + samples[c][:, k]
        estimate = total / F(64.0)
        sun_term = (((F(sun_ambient_strength) * colour[c]) * F(sun_intensity)) * sun_facing) / PI_F
        v = estimate + sun_term
        v = np.where(np.isfinite(v), v, F(0.0)).astype(np.float32)
        v = np.where(v > 0, v, F(0.0)).astype(np.float32)
        clamped |= ~(v < HALF_MAX)
        v = np.where(v < HALF_MAX, v, HALF_MAX).astype(np.float32)
        out.append(np.where(has_history, lerp(history[c], v, BLEND), v).astype(np.float32))
    count(counts, "clamped_at_half_max", clamped)
    words = np.stack([channel_half(c) for c in (*out, np.ones(n, np.float32))], axis=-1).astype(np.uint16)
    return words.reshape(6, S, S, 4)
