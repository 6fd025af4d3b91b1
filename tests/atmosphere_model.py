"""The numpy checker of oxc_generate_sky_luts and oxc_draw_atmosphere: the host constants and rules 1-10 of their header block in
include/oxcull.h, vectorised over the texels of a LUT (and, for the multiscattering pass, over the 64 directions), one masked pass per
integration step.  Every binary32 operation is one numpy float32 operation in the order the header states; pow, the exp and cos rules, lerp and the
clamp bilinear's axis come from pixel_rules.  A LUT is uint16 [H, W, 4] (the aerial
one [D, H, W, 4]) of binary16 bits.  `counts`, when given, receives how many texels, rays or steps took each side of the branches the tests
must not leave empty."""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np

from pixel_rules import axis_clamp, channel_half, cos_turn_rule, count, dot, exp_rule, f32a, from_half_bits, length, lerp, normalize, pow_rule, saturate, unproject

F = np.float32
PI_F, TAU_F = F(3.1415926535897932384626433832795), F(6.283185307179586476925286766559)
PLANET_RADIUS_OFFSET = F(0.001)
HALF_MAX, HALF_MIN_NORMAL = F(65504.0), F(6.103515625e-5)
INV_4PI = F(1.0) / (F(4.0) * PI_F)
RAYLEIGH_K = F(3.0) / (F(16.0) * PI_F)
THIRD = F(1.0) / F(3.0)
TRANSMITTANCE_STEPS = 1000


@dataclass
class Atmosphere:
    """GPU::Atmosphere (SceneGPU.hpp:158-181) with the record's own defaults; every float is used as the binary32 nearest to it."""
    rayleigh_scatter: tuple = (0.005802, 0.013558, 0.033100)
    rayleigh_density: float = 8.0
    mie_scatter: tuple = (0.003996, 0.003996, 0.003996)
    mie_density: float = 1.2
    mie_extinction: float = 0.004440
    mie_asymmetry: float = 3.6
    ozone_absorption: tuple = (0.000650, 0.001881, 0.000085)
    ozone_height: float = 25.0
    ozone_thickness: float = 15.0
    terrain_albedo: tuple = (0.3, 0.3, 0.3)
    planet_radius: float = 6360.0
    atmos_radius: float = 6460.0
    aerial_perspective_start_km: float = 8.0
    aerial_perspective_exposure: float = 1.0
    transmittance_lut_size: tuple = (256, 64, 1)
    sky_view_lut_size: tuple = (312, 192, 1)
    multiscattering_lut_size: tuple = (32, 32, 1)
    aerial_perspective_lut_size: tuple = (32, 32, 32)

    def f(self, name):
        v = getattr(self, name)
        return tuple(F(x) for x in v) if isinstance(v, (tuple, list)) else F(v)


# ---- the transcendentals ------------------------------------------------------------------------------------------------------------------------
def _pow(v, p):
    v = f32a(v)
    return pow_rule(v.reshape(-1), p).reshape(v.shape)


def safe_sqrt(x):
    return np.sqrt(np.fmax(F(0.0), x))


# ---- the host constants -------------------------------------------------------------------------------------------------------------------------
def _lit(x) -> float:
    """A decimal literal of the host evaluation: the binary32 nearest to it, widened."""
    return float(F(x))


@np.errstate(all="ignore")
def constants(A: Atmosphere, camera_y=None) -> dict:
    """Binary64 from the binary32 arguments, each value rounded to binary32 once."""
    ar, pr, g = float(A.f("atmos_radius")), float(A.f("planet_radius")), np.float64(A.f("mie_asymmetry"))
    k = {"H": F(math.sqrt(max(0.0, ar * ar - pr * pr)))}
    arg = lambda v: F(np.float64(v))  # noqa: E731
    k["g_hg"] = exp_rule(arg(-(_lit(0.0990567) / (g - _lit(1.67154)))))[()]
    k["g_d"] = exp_rule(arg(-(_lit(2.20679) / (g + _lit(3.91029))) - _lit(0.428934)))[()]
    k["alpha"] = exp_rule(arg(_lit(3.62489) - (_lit(8.29288) / (g + _lit(5.52825)))))[()]
    k["w_d"] = exp_rule(arg(-(_lit(0.599085) / (g - _lit(0.641583))) - _lit(0.665888)))[()]
    if camera_y is not None:
        min_altitude = pr + _lit(0.001)
        k["eye_altitude"] = F(np.fmax(np.float64(F(camera_y)) * _lit(0.01) + min_altitude, min_altitude))
        h = np.float64(k["eye_altitude"])
        horizon = np.sqrt(np.fmax(0.0, h * h - pr * pr))
        beta = np.arccos(horizon / h)
        k["beta"], k["zenith_horizon_angle"] = F(beta), F(math.pi - beta)
    return k


# ---- the shared rules ---------------------------------------------------------------------------------------------------------------------------
@np.errstate(all="ignore")
def intersect(o, d, radius):
    """Rule 1: (has, value); value 0.0 where there is none."""
    a, b, c = dot(d, d), F(2.0) * dot(d, o), dot(o, o) - radius * radius
    delta = b * b - (F(4.0) * a) * c
    sq, den = np.sqrt(delta), F(2.0) * a
    s0, s1 = (-b + F(-1.0) * sq) / den, (-b + sq) / den
    has = ~(delta < 0) & ~((s0 < 0) & (s1 < 0))
    value = np.where(s0 < 0, np.fmax(F(0.0), s1), np.where(s1 < 0, np.fmax(F(0.0), s0), np.fmax(F(0.0), np.fmin(s0, s1))))
    return has, np.where(has, value, F(0.0)).astype(np.float32)


@np.errstate(all="ignore")
def medium(A: Atmosphere, altitude):
    """Rule 2: (rayleigh, mie, scattering_sum, extinction_sum), each three planes."""
    rd, md = exp_rule(-altitude / A.f("rayleigh_density")), exp_rule(-altitude / A.f("mie_density"))
    od = np.fmax(F(0.0), F(1.0) - np.abs(altitude - A.f("ozone_height")) / A.f("ozone_thickness"))
    rayleigh = tuple(c * rd for c in A.f("rayleigh_scatter"))
    mie = tuple(c * md for c in A.f("mie_scatter"))
    me = A.f("mie_extinction") * md
    ozone = tuple(c * od for c in A.f("ozone_absorption"))
    return rayleigh, mie, tuple(r + m for r, m in zip(rayleigh, mie)), tuple((r + me) + o for r, o in zip(rayleigh, ozone))


def sample_rgb(lut, u, v):
    """SampleLevel(LinearSamplerClamped, (u, v), 0).rgb of a uint16 [H, W, 4] LUT: the manual bilinear, clamp mode, on the decoded halves."""
    H, W = lut.shape[:2]
    planes = [from_half_bits(lut[..., c]) for c in range(3)]
    x0, x1, fx = axis_clamp(u, W)
    y0, y1, fy = axis_clamp(v, H)
    return tuple(lerp(lerp(p[y0, x0], p[y0, x1], fx), lerp(p[y1, x0], p[y1, x1], fx), fy) for p in planes)


@np.errstate(all="ignore")
def sun_transmittance(A, K, lut, h, mu):
    """Rule 3."""
    pr, ar = A.f("planet_radius"), A.f("atmos_radius")
    rho = safe_sqrt(h * h - pr * pr)
    discriminant = (h * h) * (mu * mu - F(1.0)) + ar * ar
    d = np.fmax(F(0.0), -h * mu + safe_sqrt(discriminant))
    d_min, d_max = ar - h, rho + K["H"]
    return sample_rgb(lut, (d - d_min) / (d_max - d_min), rho / K["H"])


@np.errstate(all="ignore")
def draine_phase(alpha, g, c):
    first = (F(1.0) - g * g) / _pow((F(1.0) + g * g) - (F(2.0) * g) * c, F(1.5))
    second = (F(1.0) + (alpha * c) * c) / (F(1.0) + (alpha * THIRD) * (F(1.0) + (F(2.0) * g) * g))
    return (INV_4PI * first) * second


@np.errstate(all="ignore")
def integrate(A, K, lut, eye, d, sun, sun_intensity, step_count, t_max=None, planet_luminance=False, counts=None):
    """Rule 5: (luminance, multiscattering_as_1, transmittance), three planes each.  eye, d, sun: triples broadcastable to one shape;
    step_count a binary32 scalar or array; t_max None for the Slang's -1.0."""
    shape = np.broadcast(*eye, *d, *sun, step_count).shape
    eye, d, sun = (tuple(np.broadcast_to(f32a(c), shape) for c in v) for v in (eye, d, sun))
    step_count = np.broadcast_to(f32a(step_count), shape)
    pr, ar, si = A.f("planet_radius"), A.f("atmos_radius"), F(sun_intensity)
    dead = dot(eye, eye) <= pr * pr
    has_p, val_p = intersect(eye, d, pr)
    if t_max is None:
        has_a, val_a = intersect(eye, d, ar)
        dead = dead | ~has_a
        span = np.where(has_p, np.fmax(F(0.0), val_p), val_a).astype(np.float32)
    else:
        span = np.broadcast_to(f32a(t_max), shape)
    count(counts, "rays_hit_planet", has_p & ~dead)
    count(counts, "rays_miss_planet", ~has_p & ~dead)
    cos_theta = dot(sun, d)
    rayleigh_phase = RAYLEIGH_K * (F(1.0) + cos_theta * cos_theta)
    mie_phase = lerp(draine_phase(F(0.0), K["g_hg"], cos_theta), draine_phase(K["alpha"], K["g_d"], cos_theta), K["w_d"])
    lum = [np.zeros(shape, np.float32) for _ in range(3)]
    as1 = [np.zeros(shape, np.float32) for _ in range(3)]
    tr = [np.ones(shape, np.float32) for _ in range(3)]
    old = np.zeros(shape, np.float32)
    for s in range(int(np.max(np.where(dead, F(0.0), step_count), initial=0.0))):
        sf = F(s)
        active = (sf < step_count) & ~dead
        shift = (span * (sf + F(0.3))) / step_count
        step_length = shift - old
        old = shift
        pos = tuple(e + shift * c for e, c in zip(eye, d))
        h = length(pos)
        altitude = h - pr
        rayleigh, mie, scattering, extinction = medium(A, altitude)
        up = tuple(p / h for p in pos)
        sun_theta = dot(sun, up)
        t_sun = sun_transmittance(A, K, lut, h, sun_theta)
        shadowed, _ = intersect(tuple(p - PLANET_RADIUS_OFFSET * u for p, u in zip(pos, up)), sun, pr)
        earth_shadow = np.where(shadowed, F(0.0), F(1.0)).astype(np.float32)
        count(counts, "steps_earth_shadow_0", shadowed & active)
        count(counts, "steps_earth_shadow_1", ~shadowed & active)
        for c in range(3):
            phase = mie[c] * mie_phase + rayleigh[c] * rayleigh_phase
            sun_luminance = (earth_shadow * t_sun[c]) * phase + F(0.0) * scattering[c]
            t = exp_rule(-step_length * extinction[c])
            integral = (sun_luminance - sun_luminance * t) / extinction[c]
            ms_integral = (scattering[c] - scattering[c] * t) / extinction[c]
            lum[c] = np.where(active, lum[c] + si * (integral * tr[c]), lum[c]).astype(np.float32)
            as1[c] = np.where(active, as1[c] + ms_integral * tr[c], as1[c]).astype(np.float32)
            tr[c] = np.where(active, tr[c] * t, tr[c]).astype(np.float32)
    if planet_luminance:
        bounce = has_p & (span == val_p) & ~dead
        count(counts, "ground_bounce_taken", bounce)
        count(counts, "ground_bounce_not_taken", ~bounce)
        pos = tuple(e + span * c for e, c in zip(eye, d))
        h = length(pos)
        up = tuple(p / h for p in pos)
        sun_theta = dot(sun, up)
        nol = saturate(dot(normalize(sun), normalize(up)))
        t_sun = sun_transmittance(A, K, lut, h, sun_theta)
        albedo = A.f("terrain_albedo")
        for c in range(3):
            lum[c] = np.where(bounce, lum[c] + si * ((((t_sun[c] * tr[c]) * nol) * albedo[c]) / PI_F), lum[c]).astype(np.float32)
    return lum, as1, tr


@np.errstate(all="ignore")
def move_to_top_atmosphere(pos, d, ar):
    """Rule 6: (ok, the moved position)."""
    h = length(pos)
    above = h > ar
    has, value = intersect(pos, d, ar)
    moved = tuple((p + c * value) + (p / h) * -PLANET_RADIUS_OFFSET for p, c in zip(pos, d))
    return ~above | has, tuple(np.where(above & has, m, p).astype(np.float32) for m, p in zip(moved, pos))


def _pack(r, g, b, a) -> np.ndarray:
    return np.stack([channel_half(c) for c in (r, g, b, a)], axis=-1).astype(np.uint16)


def _texel_uv(W, H):
    ys, xs = np.mgrid[0:H, 0:W]
    return (xs.astype(np.float32) + F(0.5)) / F(W), (ys.astype(np.float32) + F(0.5)) / F(H)


# ---- oxc_generate_sky_luts ----------------------------------------------------------------------------------------------------------------------
@np.errstate(all="ignore")
def transmittance_lut(A: Atmosphere, steps: int = TRANSMITTANCE_STEPS) -> np.ndarray:
    """Rule 7."""
    W, H = A.transmittance_lut_size[:2]
    K = constants(A)
    u, v = _texel_uv(W, H)
    h, pr, ar = K["H"], A.f("planet_radius"), A.f("atmos_radius")
    rho = h * v
    lut_x = np.sqrt(rho * rho + pr * pr)
    d_min, d_max = ar - lut_x, rho + h
    d = d_min + u * (d_max - d_min)
    lut_y = np.where(d == 0, F(1.0), ((h * h - rho * rho) - d * d) / ((F(2.0) * lut_x) * d)).astype(np.float32)
    lut_y = np.fmin(np.fmax(lut_y, F(-1.0)), F(1.0))
    zero = np.zeros_like(lut_x)
    sun = (zero, np.sqrt(F(1.0) - lut_y * lut_y), lut_y)
    pos = (zero, zero, lut_x)
    per_step = intersect(pos, sun, ar)[1] / F(steps)
    depth = [zero, zero, zero]
    for _ in range(steps):
        pos = tuple(p + s * per_step for p, s in zip(pos, sun))
        extinction = medium(A, length(pos) - pr)[3]
        depth = [o + e * per_step for o, e in zip(depth, extinction)]
    return _pack(*(exp_rule(-o) for o in depth), np.ones_like(lut_x))


@np.errstate(all="ignore")
def multiscatter_lut(A: Atmosphere, transmittance: np.ndarray, hemisphere, counts=None) -> np.ndarray:
    """Rule 8; `hemisphere` float32 [64, 3]."""
    W, H = A.multiscattering_lut_size[:2]
    K = constants(A)
    hemisphere = f32a(hemisphere).reshape(64, 3)
    u, v = _texel_uv(W, H)
    pr, ar = A.f("planet_radius"), A.f("atmos_radius")
    altitude = ((pr + v * (ar - pr)) + PLANET_RADIUS_OFFSET)[..., None]
    c = (u * F(2.0) - F(1.0))[..., None]
    zero = np.zeros_like(c)
    sun = (zero, c, safe_sqrt(F(1.0) - c * c))
    d = tuple(hemisphere[:, k].reshape(1, 1, 64) for k in range(3))
    lum, as1, _ = integrate(A, K, transmittance, (zero, altitude, zero), d, sun, F(10.0), F(32.0), None, True, counts)
    out = []
    sphere = F(4.0) * PI_F
    inv_count = F(1.0) / F(64.0)
    for k in range(3):
        total_l, total_m = np.zeros((H, W), np.float32), np.zeros((H, W), np.float32)
        for i in range(64):  # ascending direction order
            total_m = total_m + as1[k][..., i]
            total_l = total_l + lum[k][..., i]
        total_l = total_l * (sphere * inv_count)
        total_m = total_m * inv_count
        out.append((total_l * (F(1.0) / sphere)) * (F(1.0) / (F(1.0) - total_m)))
    return _pack(*out, np.ones((H, W), np.float32))


# ---- oxc_draw_atmosphere ------------------------------------------------------------------------------------------------------------------------
@np.errstate(all="ignore")
def sky_view_lut(A: Atmosphere, transmittance, camera_position, sun_dir, sun_intensity, counts=None) -> np.ndarray:
    """Rule 9."""
    W, H = A.sky_view_lut_size[:2]
    K = constants(A, camera_position[1])
    u, v = _texel_uv(W, H)
    fw, fh = F(W), F(H)
    u = (u - F(0.5) / fw) * (fw / (fw - F(1.0)))
    v = (v - F(0.5) / fh) * (fh / (fh - F(1.0)))
    zha, beta, h = K["zenith_horizon_angle"], K["beta"], K["eye_altitude"]
    above = v < F(0.5)
    count(counts, "sky_view_above_horizon", above)
    count(counts, "sky_view_below_horizon", ~above)
    ca = v * F(2.0)
    ca = F(1.0) - ca
    ca = ca * ca
    ca = F(1.0) - ca
    cb = v * F(2.0) - F(1.0)
    cb = cb * cb
    angle = np.where(above, zha * ca, zha + beta * cb).astype(np.float32)
    longitude = u * TAU_F
    cz = cos_turn_rule(angle)
    sz = safe_sqrt(F(1.0) - cz * cz) * np.where(angle > 0, F(1.0), F(-1.0)).astype(np.float32)
    cl = cos_turn_rule(longitude)
    sl = safe_sqrt(F(1.0) - cl * cl) * np.where(longitude <= PI_F, F(1.0), F(-1.0)).astype(np.float32)
    d = (sz * cl, cz, sz * sl)
    zero = np.zeros((H, W), np.float32)
    ok, eye = move_to_top_atmosphere((zero, zero + h, zero), d, A.f("atmos_radius"))
    if h > A.f("atmos_radius"):
        count(counts, "sky_view_moved_to_top", ok)
        count(counts, "sky_view_missed_atmosphere", ~ok)
    up = tuple(e / h for e in eye)
    sun_in = tuple(F(s) for s in sun_dir)
    szc = dot(sun_in, up)
    sun = normalize((safe_sqrt(F(1.0) - szc * szc), szc, zero))
    lum, _, _ = integrate(A, K, transmittance, eye, d, sun, sun_intensity, F(48.0), None, False, counts)
    lum = [np.fmax(c, F(0.0)) for c in lum]
    lum = [np.where(np.isfinite(c), c, F(0.0)).astype(np.float32) for c in lum]
    mult = np.fmin(np.fmax(np.fmax(lum[0], np.fmax(lum[1], lum[2])), HALF_MIN_NORMAL), HALF_MAX)
    out = _pack(lum[0] / mult, lum[1] / mult, lum[2] / mult, mult)
    out[~ok] = 0
    return out


@np.errstate(all="ignore")
def aerial_lut(A: Atmosphere, transmittance, camera_position, inv_projection_view, sun_dir, sun_intensity, counts=None) -> np.ndarray:
    """Rule 10; inv_projection_view column-major [16]."""
    W, H, D = A.aerial_perspective_lut_size
    K = constants(A, camera_position[1])
    m = f32a(inv_projection_view).reshape(16)
    u, v = _texel_uv(W, H)
    world = unproject(m, u, v, F(1.0))
    cam = tuple(F(c) for c in camera_position)
    d = normalize(tuple(w - c for w, c in zip(world, cam)))
    d = tuple(np.broadcast_to(c[None], (D, H, W)) for c in d)
    z = np.arange(D, dtype=np.float32).reshape(D, 1, 1)
    slab = (z + F(0.5)) * (F(1.0) / F(D))
    slab = slab * slab
    slab = slab * F(D)
    per_slice_depth = F(W // D)
    t_max = np.broadcast_to(slab * per_slice_depth, (D, H, W)).astype(np.float32)
    h, ar = K["eye_altitude"], A.f("atmos_radius")
    zero = np.zeros((D, H, W), np.float32)
    eye = (zero, zero + h, zero)
    zeroed = np.zeros((D, H, W), bool)
    if h >= ar:
        ok, moved = move_to_top_atmosphere(eye, d, ar)
        to_atmosphere = length(tuple(p - q for p, q in zip(eye, moved)))
        rejected = ok & (t_max < to_atmosphere)
        count(counts, "aerial_moved_to_top", ok & ~rejected)
        count(counts, "aerial_missed_atmosphere", ~ok)
        count(counts, "aerial_rejected_by_t_max", rejected)
        zeroed = ~ok | rejected
        t_max = np.fmax(F(0.0), t_max - to_atmosphere)
        eye = moved
    step_count = np.broadcast_to(np.fmax(F(1.0), (z + F(1.0)) * F(2.0)), (D, H, W))
    lum, _, tr = integrate(A, K, transmittance, eye, d, tuple(F(s) for s in sun_dir), sun_intensity, step_count, t_max, False, counts)
    out = _pack(lum[0], lum[1], lum[2], (tr[0] * THIRD + tr[1] * THIRD) + tr[2] * THIRD)
    out[zeroed] = 0
    return out
