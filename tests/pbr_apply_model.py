"""Checker of oxc_apply_pbr: the no-atmosphere branch of RendererInstance::apply_pbr (Passes/PBR.cpp:313-534, passes/pbr_apply_no_atmos.slang
with pbr.slang) restated in numpy from the numbered rule include/oxcull.h states -- binary32 in the Slang's evaluation order, no contraction,
IEEE division and square root, pow / exp2 / cos the closed forms in binary64 rounded once.  Pixels are vectorised, lights are walked in
order.  Written from the header, not from the kernel.  Returns the final image and fills `stats`."""
from __future__ import annotations

import numpy as np

from pixel_rules import (COS_C, SIN_C, channel_half, clamp, dot, exp2_rule, f32a, from_half_bits, normalize, oct_to_vec3, pack_b10g11r11, pow_rule, saturate,
                         srgb_decode, unpack_b10g11r11)
from pixel_rules import unpack_ufloat  # noqa: F401  (the decode behind unpack_b10g11r11; the tests name it)

F = np.float32
HAS_DIRECTIONAL_LIGHT, HAS_ATMOSPHERE, HAS_CONTACT_SHADOWS, HAS_SKY, TRANSPARENT_BACKGROUND = 1 << 0, 1 << 1, 1 << 9, 1 << 10, 1 << 11
KIND_DIRECTIONAL, KIND_POINT, KIND_SPOT = 0, 1, 2
PI = F(3.1415926535897932)
FD_LAMBERT = F(1.0) / PI
MIN_ALPHA = F(0.0025)
TWO_OVER_PI = float.fromhex("0x1.45f306dc9c883p-1")
PIO2_HI = float.fromhex("0x1.921fb54p+0")          # pi / 2 to 29 significant bits
PIO2_LO = float.fromhex("0x1.10b4611a62633p-30")   # the rest
# GGX_directional_albedo's nine float4 constants, pbr.slang:40-42
ALBEDO_FIT = np.array([[0.1003, 0.9345, 1.0, 1.0], [-0.6303, -2.323, -1.765, 0.2281], [9.748, 2.229, 8.263, 15.94], [-2.038, -3.748, 11.53, -55.83],
                       [29.34, 1.424, 28.96, 13.08], [-8.245, -0.7684, -7.507, 41.26], [-26.44, 1.436, -36.11, 54.9], [19.99, 0.2913, 15.86, 300.2],
                       [-5.448, 0.6286, 33.37, -285.1]], dtype=np.float32)
COUNTER_NAMES = ("transparent_empty", "sky", "fallthrough_empty", "lit_nol_positive", "lit_nol_zero", "light_kind_skipped", "light_attenuation_out",
                 "light_ndotl_out", "light_shaded")
LIGHT_FIELDS = dict(position=slice(0, 3), intensity=3, color=slice(4, 7), range=7, direction=slice(8, 11), inner_cone_angle=11, outer_cone_angle=12)


# ---- the closed forms ------------------------------------------------------------------------------------------------------------------------
@np.errstate(all="ignore")
def cos_reduced_rule(x) -> np.ndarray:
    """The cos rule of this pass alone (its device function lives in oxcull_pbr_apply.hip, not in the shared header): two-constant reduction,
    the polynomials of the rotation rule, one rounding; NaN beyond 2^24 and for non-finite x."""
    x = np.atleast_1d(f32a(x))
    ax = np.abs(x)
    ok = ax <= F(2.0 ** 24)
    a = np.where(ok, ax, F(0.0)).astype(np.float64)
    q = np.floor(a * TWO_OVER_PI + 0.5)
    r = (a - q * PIO2_HI) - q * PIO2_LO
    z = r * r
    ps = ((SIN_C[3] * z + SIN_C[2]) * z + SIN_C[1]) * z + SIN_C[0]
    s = r + (r * z) * ps
    pc = (((COS_C[4] * z + COS_C[3]) * z + COS_C[2]) * z + COS_C[1]) * z + COS_C[0]
    c = 1.0 + z * pc
    n = q.astype(np.int64) & 3
    v = np.where(n == 0, c, np.where(n == 1, -s, np.where(n == 2, -c, s)))
    return np.where(ok, v.astype(np.float32), F(np.nan)).astype(np.float32)


# ---- decodes and packers ---------------------------------------------------------------------------------------------------------------------
def unpack_lights(lights, count: int = None) -> dict:
    """uint8 / uint32 records -> the fields as float32 arrays [n] / [n, 3] and kind uint32 [n]."""
    w = np.ascontiguousarray(np.asarray(lights)).view(np.uint32).reshape(-1, 16)
    if count is not None:
        w = w[:count]
    out = {k: w[:, s].view(np.float32) for k, s in LIGHT_FIELDS.items()}
    out["kind"] = w[:, 13].copy()
    return out


# ---- pbr.slang ---------------------------------------------------------------------------------------------------------------------------------
@np.errstate(all="ignore")
def ggx_directional_albedo(NoV, alpha):
    x, y = NoV, alpha
    x2, y2 = x * x, y * y
    c = ALBEDO_FIT
    r = [(((((((c[0, k] + c[1, k] * x) + c[2, k] * y) + (c[3, k] * x) * y) + c[4, k] * x2) + c[5, k] * y2) + (c[6, k] * x2) * y) + (c[7, k] * x) * y2)
         + (c[8, k] * x2) * y2 for k in range(4)]
    return clamp(r[0] / r[2], 0.0, 1.0), clamp(r[1] / r[3], 0.0, 1.0)


@np.errstate(all="ignore")
def attenuate_point(dist, rng):
    """lights_attenuate_point, pbr.slang:89-100; `rng` a binary32 scalar."""
    d2 = dist * dist + F(0.1)
    if rng <= F(0.0):
        return F(1.0) / d2
    win = dist / rng
    win = ((win * win) * win) * win
    win = np.fmax(F(0.0), F(1.0) - win)
    win = win * win
    return win / d2


@np.errstate(all="ignore")
def smoothstep(e0, e1, x):
    s = saturate((x - e0) / (e1 - e0))
    return (s * s) * (F(3.0) - F(2.0) * s)


@np.errstate(all="ignore")
def brdf(S, l):
    """Rule 10.  S: the pixel's surface terms; l: three arrays or scalars.  -> (diffuse, specular), each a list of three arrays."""
    N, V = S["N"], S["V"]
    VL = (V[0] + l[0], V[1] + l[1], V[2] + l[2])
    use = dot(VL, VL) > F(1e-8)
    Hn = normalize(VL)
    H = tuple(np.where(use, Hn[c], N[c]) for c in range(3))
    NoL = saturate(dot(N, l))
    NoH = saturate(dot(N, H))
    LoH = saturate(dot(l, H))
    a2 = S["alpha2"]
    f = (NoH * a2 - NoH) * NoH + F(1.0)
    D = a2 / ((PI * f) * f + F(1e-7))
    NoV = S["NoV"]
    GGXV = NoL * np.sqrt((NoV * NoV) * (F(1.0) - a2) + a2)
    GGXL = NoV * np.sqrt((NoL * NoL) * (F(1.0) - a2) + a2)
    Vis = saturate(F(0.5) / ((GGXV + GGXL) + F(1e-7)))
    p5 = pow_rule(saturate(F(1.0) - LoH), F(5.0))
    diffuse, specular = [], []
    for c in range(3):
        Fc = S["F0"][c] + (F(1.0) - S["F0"][c]) * p5
        specular.append(((D * Vis) * Fc) * S["ec"][c])
        diffuse.append((((F(1.0) - S["metallic"]) * (F(1.0) - Fc)) * S["albedo"][c]) * FD_LAMBERT)
    return diffuse, specular


@np.errstate(all="ignore")
def apply_pbr(depth, albedo, normal, emissive, mro, ao, resolved, contact, scene_flags, inv_projection_view, camera_position, sun_dir, sun_intensity,
              lights=None, light_count=None, base_ambient_color=(0.03, 0.03, 0.03), sky_solid_color=(0.0, 0.0, 0.0, 1.0),
              sky_ambient_color=(0.0, 0.0, 0.0), sky_has_texture=False, stats: dict = None) -> np.ndarray:
    """depth float32 [H, W]; albedo / emissive / mro uint32 [H, W]; normal uint16 [H, W, 4]; ao uint16 [H, W]; resolved / contact float32 [H, W]
    or None when their flag is clear -> uint32 [H, W] (B10G11R11), or uint16 [H, W, 4] with TransparentBackground."""
    flags = int(scene_flags)
    assert not flags & HAS_ATMOSPHERE
    depth = np.ascontiguousarray(depth, dtype=np.float32)
    H, W = depth.shape
    has_sun, has_contact, has_sky, transparent = bool(flags & HAS_DIRECTIONAL_LIGHT), bool(flags & HAS_CONTACT_SHADOWS), bool(flags & HAS_SKY), bool(flags & TRANSPARENT_BACKGROUND)
    u32 = lambda a: np.ascontiguousarray(np.asarray(a)).view(np.uint32).reshape(H, W)  # noqa: E731
    albedo, emissive, mro = u32(albedo), u32(emissive), u32(mro)
    normal = np.ascontiguousarray(np.asarray(normal)).view(np.uint16).reshape(H, W, 4)
    ao = np.ascontiguousarray(np.asarray(ao)).view(np.uint16).reshape(H, W)
    m = f32a(inv_projection_view)
    cam, L = f32a(camera_position), tuple(f32a(sun_dir))
    st = dict.fromkeys(COUNTER_NAMES, 0)
    out = np.zeros((H, W, 4), np.uint16) if transparent else np.zeros((H, W), np.uint32)

    def store(ys, xs, rgb):
        if transparent:
            out[ys, xs] = np.stack([channel_half(rgb[0]), channel_half(rgb[1]), channel_half(rgb[2]), np.full(len(ys), 0x3C00, np.uint16)], axis=-1)
        else:
            out[ys, xs] = pack_b10g11r11(rgb[0], rgb[1], rgb[2])

    # 1. transparent empty: all four channels 0 (the image starts as zeros)
    todo = np.ones((H, W), dtype=bool)
    if transparent:
        todo = ~(depth == 0)
        st["transparent_empty"] = int((~todo).sum())
    ys, xs = np.nonzero(todo)
    if len(ys):
        d = depth[ys, xs]
        # 2. decode
        aw = albedo[ys, xs]
        alb = [srgb_decode((aw >> np.uint32(8 * c)) & np.uint32(0xFF)) for c in range(3)]
        nh = from_half_bits(normal[ys, xs])
        mapped, smooth = oct_to_vec3(nh[:, 0], nh[:, 1]), oct_to_vec3(nh[:, 2], nh[:, 3])
        emission = unpack_b10g11r11(emissive[ys, xs])
        mw = mro[ys, xs]
        byte = lambda k: ((mw >> np.uint32(8 * k)) & np.uint32(0xFF)).astype(np.float32) / F(255.0)  # noqa: E731
        metallic = clamp(byte(0), 0.0, 1.0)
        roughness = clamp(byte(1), 0.045, 1.0)
        occlusion = byte(2) * from_half_bits(ao[ys, xs])
        # 3. position
        u, v = (xs.astype(np.float32) + F(0.5)) / F(W), (ys.astype(np.float32) + F(0.5)) / F(H)
        nx, ny = u * F(2.0) - F(1.0), v * F(2.0) - F(1.0)
        h = [((m[r] * nx + m[4 + r] * ny) + m[8 + r] * d) + m[12 + r] for r in range(4)]
        world = (h[0] / h[3], h[1] / h[3], h[2] / h[3])
        # 4. frame
        V = normalize((cam[0] - world[0], cam[1] - world[1], cam[2] - world[2]))
        N = normalize(mapped)
        nV = (-V[0], -V[1], -V[2])
        two_d = F(2.0) * dot(N, nV)
        R = (nV[0] - two_d * N[0], nV[1] - two_d * N[1], nV[2] - two_d * N[2])
        NoV = np.abs(dot(N, V)) + F(1e-5)
        NoL = np.fmax(dot(N, L), F(0.0))
        # 5. sky
        sky = (d == 0) & has_sky
        if sky.any():
            rgb = [np.full(int(sky.sum()), F(1.0) if sky_has_texture else F(sky_solid_color[c]), np.float32) for c in range(3)]
            store(ys[sky], xs[sky], rgb)
        st["sky"] = int(sky.sum())
        lit = ~sky
        st["fallthrough_empty"] = int((lit & (d == 0)).sum())
        st["lit_nol_positive"] = int((lit & ~(d == 0) & (NoL > 0)).sum())
        st["lit_nol_zero"] = int((lit & ~(d == 0) & ~(NoL > 0)).sum())
        # 6. terms
        ds = f32a(resolved)[ys, xs] if has_sun else np.ones(len(ys), np.float32)
        cs = f32a(contact)[ys, xs] if has_contact else np.ones(len(ys), np.float32)
        visibility = ds * cs
        direct = F(sun_intensity) if has_sun else F(0.0)
        env = f32a(sky_ambient_color) if has_sky else f32a(base_ambient_color)
        # 7. surface
        F0 = [F(0.04) + (alb[c] - F(0.04)) * metallic for c in range(3)]
        alpha = np.fmax(roughness * roughness, MIN_ALPHA)
        alpha2 = alpha * alpha
        ABx, ABy = ggx_directional_albedo(NoV, alpha)
        Ess = saturate(ABx + ABy)
        ec = [F(1.0) + (F0[c] * (F(1.0) - Ess)) / np.fmax(Ess, F(1e-4)) for c in range(3)]
        S = dict(N=N, V=V, albedo=alb, F0=F0, ec=ec, metallic=metallic, NoV=NoV, alpha2=alpha2)
        # 8. ambient
        spec_occlusion = saturate((pow_rule(NoV + occlusion, exp2_rule(F(-16.0) * roughness - F(1.0))) - F(1.0)) + occlusion)
        indirect = []
        for c in range(3):
            kS = F0[c] * ABx + ABy
            kD = (F(1.0) - metallic) * (F(1.0) - kS)
            ibl_diffuse = ((kD * env[c]) * alb[c]) * FD_LAMBERT
            ibl_specular = (kS * env[c]) * spec_occlusion
            indirect.append(ibl_diffuse * occlusion + ibl_specular)
        # 9. lights
        total = [np.zeros(len(ys), np.float32) for _ in range(3)]
        n_lights = 0 if lights is None else (len(np.asarray(lights).reshape(-1).view(np.uint8)) // 64 if light_count is None else int(light_count))
        if n_lights:
            lt = unpack_lights(lights, n_lights)
            n_lit = int(lit.sum())
            for i in range(n_lights):
                kind = int(lt["kind"][i])
                if kind not in (KIND_POINT, KIND_SPOT):
                    st["light_kind_skipped"] += n_lit
                    continue
                pos = lt["position"][i]
                lv = (pos[0] - world[0], pos[1] - world[1], pos[2] - world[2])
                dist = np.sqrt(dot(lv, lv))
                Ll = (lv[0] / dist, lv[1] / dist, lv[2] / dist)
                att = attenuate_point(dist, lt["range"][i])
                if kind == KIND_SPOT:
                    sd = normalize(tuple(lt["direction"][i]))
                    cos_angle = dot((-Ll[0], -Ll[1], -Ll[2]), sd)
                    att = att * smoothstep(cos_reduced_rule(lt["outer_cone_angle"][i])[0], cos_reduced_rule(lt["inner_cone_angle"][i])[0], cos_angle)
                intensity = lt["intensity"][i]
                out_att = (att <= 0) | bool(intensity <= 0)
                NdotL = saturate(dot(N, Ll))
                out_ndl = ~out_att & (NdotL <= 0)
                shaded = ~out_att & ~out_ndl
                st["light_attenuation_out"] += int((out_att & lit).sum())
                st["light_ndotl_out"] += int((out_ndl & lit).sum())
                st["light_shaded"] += int((shaded & lit).sum())
                diffuse, specular = brdf(S, Ll)
                for c in range(3):
                    radiance = (lt["color"][i][c] * att) * intensity
                    total[c] = np.where(shaded, total[c] + ((diffuse[c] + specular[c]) * radiance) * NdotL, total[c])
        # 11. sun
        horizon = saturate(F(1.0) + F(1.3) * dot(R, smooth))
        horizon = horizon * horizon
        diffuse, specular = brdf(S, L)
        surface = [np.where(NoL > 0, (((diffuse[c] + specular[c] * horizon) * direct) * NoL) * visibility, F(0.0)) for c in range(3)]
        # 12. store
        rgb = [(((surface[c] + total[c]) + indirect[c]) + emission[c])[lit] for c in range(3)]
        store(ys[lit], xs[lit], rgb)
        st.update(ys=ys, xs=xs, lit=lit, NoL=NoL, world=world, N=N, V=V)
    if stats is not None:
        stats.update(st)
    return out


def counters(stats) -> dict:
    """The device's counters (oxc_debug_pbr_apply_stats) from the checker's stats."""
    return {k: int(stats[k]) for k in COUNTER_NAMES}
