"""Checker of oxc_apply_pbr_atmosphere: the atmosphere branch of RendererInstance::apply_pbr (Passes/PBR.cpp:318-434, passes/pbr_apply.slang with
pbr.slang and sky.slang) in numpy, following steps A - K of its header block in include/oxcull.h.  What the other checkers already implement
is imported and left as it is: the surface, BRDF and the lights from pbr_apply_model, the record, the host constants, intersect and the
transmittance sample from atmosphere_model, the .rgba clamp bilinear and sky_view_params_to_lut_uv from sky_ibl_model; the numeric rules
(exp, the sRGB decode, clamp, lerp, the bilinear's axis) from pixel_rules.  New here: the sun
term per channel (C), the sky pixel with draw_sun (D), sample_aerial_perspective (E), the face-local cube sample (F) and the sky ambient (G).
Returns the image and a dict of counts: the pixel classes, the aerial branches and the four light outcomes."""
from __future__ import annotations

import numpy as np

import atmosphere_model as AM
import pbr_apply_model as PM
import sky_ibl_model as SM
from pbr_apply_model import HAS_CONTACT_SHADOWS, HAS_DIRECTIONAL_LIGHT, TRANSPARENT_BACKGROUND
from pixel_rules import (axis_clamp, channel_half, clamp, count, cross, dot, exp2_rule, exp_rule, f32a, from_half_bits, length, lerp, normalize, oct_to_vec3,
                         pack_b10g11r11, pow_rule, saturate, srgb_decode, unpack_b10g11r11)

F = np.float32
HALF_SLICE = F(0.70710678118654752)
COUNT_NAMES = ("transparent_empty", "sky_hit", "sky_in_disc", "sky_outside_disc", "lit_nol_positive", "lit_nol_zero", "aerial_near_slice", "aerial_zero_depth",
               "light_kind_skipped", "light_attenuation_out", "light_ndotl_out", "light_shaded")


# ---- the host constants ------------------------------------------------------------------------------------------------------------------------
@np.errstate(all="ignore")
def host_constants(A: AM.Atmosphere, camera_position, sun_dir) -> dict:
    """eye_altitude, beta, zenith_horizon_angle and H as oxc_draw_atmosphere forms them, and the binary32 constants of the header block."""
    K = AM.constants(A, camera_position[1])
    L = tuple(F(v) for v in sun_dir)
    K["min_altitude"] = A.f("planet_radius") + F(0.001)
    K["sun_cos_theta"] = (L[0] * F(0.0) + L[1] * F(1.0)) + L[2] * F(0.0)
    K["horizon_darkening"] = PM.smoothstep(F(-0.1), F(0.3), K["sun_cos_theta"])
    K["min_cos"] = PM.cos_reduced_rule((F(1.0) * PM.PI) / F(180.0))[0]
    lut = tuple(F(n) for n in A.aerial_perspective_lut_size)
    K["aerial_depth"] = lut[2]
    K["inv_per_slice_depth"] = F(1.0) / (lut[0] / lut[2])
    K["inv_aerial_depth"] = F(1.0) / lut[2]
    K["near_depth_fade_out"] = F(1.0) / F(0.001)
    return K


# ---- D: draw_sun ---------------------------------------------------------------------------------------------------------------------------------
@np.errstate(all="ignore")
def draw_sun(min_cos, ct):
    """pbr_apply.slang:26-38 for ct = dot(-V, L): (value, inside the disc)."""
    ct = f32a(ct)
    inside = ct >= min_cos  # false for a NaN
    offset = min_cos - ct
    g = exp_rule(-offset * F(50000.0)) * F(0.5)
    inv = (F(1.0) / (F(0.02) + offset * F(300.0))) * F(0.01)
    return np.where(inside, F(1.0), g + inv).astype(np.float32), inside


# ---- E: sample_aerial_perspective ------------------------------------------------------------------------------------------------------------------
@np.errstate(all="ignore")
def aerial_perspective(A, K, aerial, u, v, rel, counts=None):
    """aerial.rgb * aerial.a of sky.slang:258-293 at the pixel's uv for rel = (world - camera_position) * 0.01f; `aerial` uint16 [D, H, W, 4]."""
    relative_depth = np.fmax(F(0.0), length(rel) - A.f("aerial_perspective_start_km"))
    linear_slice = relative_depth * K["inv_per_slice_depth"]
    linear_w = linear_slice * K["inv_aerial_depth"]
    non_linear_w = np.sqrt(linear_w)
    non_linear_slice = non_linear_w * K["aerial_depth"]
    near = non_linear_slice < HALF_SLICE
    weight = np.where(near, saturate((non_linear_slice * non_linear_slice) * F(2.0)), F(1.0)).astype(np.float32)
    weight = weight * saturate(relative_depth * K["near_depth_fade_out"])
    count(counts, "aerial_near_slice", near)
    count(counts, "aerial_zero_depth", relative_depth == 0)
    D = aerial.shape[0]
    z0, z1, fz = axis_clamp(non_linear_w, D)
    t0 = [np.zeros(len(u), np.float32) for _ in range(4)]
    t1 = [np.zeros(len(u), np.float32) for _ in range(4)]
    for z in range(D):  # the bilinear .rgba of slice i0 and of slice i1
        for t, zi in ((t0, z0), (t1, z1)):
            m = zi == z
            if m.any():
                for c, plane in enumerate(SM.sample_rgba(aerial[z], u[m], v[m])):
                    t[c][m] = plane
    a = [lerp(t0[c], t1[c], fz) for c in range(4)]
    rgb = [a[c] * weight for c in range(3)]
    w = F(1.0) - (weight * (F(1.0) - a[3]))
    rgb = [c * A.f("aerial_perspective_exposure") for c in rgb]
    return [c * w for c in rgb]


# ---- F: the cube sample ----------------------------------------------------------------------------------------------------------------------------
@np.errstate(all="ignore")
def cube_coords(r):
    """(face, s, t) of rule F for directions r (three arrays)."""
    rx, ry, rz = (np.atleast_1d(f32a(c)) for c in r)
    ax, ay, az = np.abs(rx), np.abs(ry), np.abs(rz)
    is_z = (az >= ax) & (az >= ay)
    is_y = ~is_z & (ay >= ax)
    is_x = ~is_z & ~is_y
    neg = np.where(is_z, rz < 0, np.where(is_y, ry < 0, rx < 0))  # a negative zero and a NaN count as positive
    face = np.where(is_z, 4, np.where(is_y, 2, 0)) + neg
    sc = np.where(is_z, np.where(neg, -rx, rx), np.where(is_y, rx, np.where(neg, rz, -rz))).astype(np.float32)
    tc = np.where(is_y, np.where(neg, -rz, rz), -ry).astype(np.float32)
    ma = np.abs(np.where(is_z, rz, np.where(is_y, ry, rx))).astype(np.float32)
    assert (is_x | is_y | is_z).all()
    return face, (sc / ma) * F(0.5) + F(0.5), (tc / ma) * F(0.5) + F(0.5)


@np.errstate(all="ignore")
def cube_sample(cube, r):
    """The clamp bilinear .rgba of the selected face alone; `cube` uint16 [6, S, S, 4] -> four arrays."""
    face, s, t = cube_coords(r)
    out = [np.zeros(len(face), np.float32) for _ in range(4)]
    for f in range(6):
        m = face == f
        if m.any():
            for c, plane in enumerate(SM.sample_rgba(cube[f], s[m], t[m])):
                out[c][m] = plane
    return out


# ---- the call ------------------------------------------------------------------------------------------------------------------------------------
@np.errstate(all="ignore")
def apply_pbr_atmosphere(depth, albedo, normal, emissive, mro, ao, resolved, contact, scene_flags, inv_projection_view, camera_position, sun_dir, sun_intensity,
                         A: AM.Atmosphere, transmittance, sky_view, aerial, cube, lights=None, light_count=None, counts: dict = None, detail: dict = None):
    """The G-buffer images as pbr_apply_model.apply_pbr takes them; the four sky images uint16 [H, W, 4], [H, W, 4], [D, H, W, 4] and
    [6, S, S, 4] -> (uint32 [H, W] (B10G11R11) or uint16 [H, W, 4] with TransparentBackground, counts).  `detail` receives per-pixel arrays."""
    flags = int(scene_flags)
    depth = np.ascontiguousarray(depth, dtype=np.float32)
    H, W = depth.shape
    has_sun, has_contact, transparent = bool(flags & HAS_DIRECTIONAL_LIGHT), bool(flags & HAS_CONTACT_SHADOWS), bool(flags & TRANSPARENT_BACKGROUND)
    u32 = lambda a: np.ascontiguousarray(np.asarray(a)).view(np.uint32).reshape(H, W)  # noqa: E731
    albedo, emissive, mro = u32(albedo), u32(emissive), u32(mro)
    normal = np.ascontiguousarray(np.asarray(normal)).view(np.uint16).reshape(H, W, 4)
    ao = np.ascontiguousarray(np.asarray(ao)).view(np.uint16).reshape(H, W)
    u16 = lambda a: np.ascontiguousarray(np.asarray(a)).view(np.uint16)  # noqa: E731
    transmittance, sky_view, aerial, cube = u16(transmittance), u16(sky_view), u16(aerial), u16(cube)
    m = f32a(inv_projection_view)
    cam, L, Li = f32a(camera_position), tuple(f32a(sun_dir)), F(sun_intensity)
    K = host_constants(A, camera_position, sun_dir)
    st = dict.fromkeys(COUNT_NAMES, 0) if counts is None else counts
    for k in COUNT_NAMES:
        st.setdefault(k, 0)
    out = np.zeros((H, W, 4), np.uint16) if transparent else np.zeros((H, W), np.uint32)

    def store(ys, xs, rgb):
        if transparent:
            out[ys, xs] = np.stack([channel_half(rgb[0]), channel_half(rgb[1]), channel_half(rgb[2]), np.full(len(ys), 0x3C00, np.uint16)], axis=-1)
        else:
            out[ys, xs] = pack_b10g11r11(rgb[0], rgb[1], rgb[2])

    # A. transparent empty, then steps 2 - 4
    todo = np.ones((H, W), dtype=bool)
    if transparent:
        todo = ~(depth == 0)
        st["transparent_empty"] += int((~todo).sum())
    ys, xs = np.nonzero(todo)
    if not len(ys):
        return out, st
    d = depth[ys, xs]
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
    u, v = (xs.astype(np.float32) + F(0.5)) / F(W), (ys.astype(np.float32) + F(0.5)) / F(H)
    nx, ny = u * F(2.0) - F(1.0), v * F(2.0) - F(1.0)
    h = [((m[r] * nx + m[4 + r] * ny) + m[8 + r] * d) + m[12 + r] for r in range(4)]
    world = (h[0] / h[3], h[1] / h[3], h[2] / h[3])
    V = normalize((cam[0] - world[0], cam[1] - world[1], cam[2] - world[2]))
    N = normalize(mapped)
    nV = (-V[0], -V[1], -V[2])
    two_d = F(2.0) * dot(N, nV)
    R = (nV[0] - two_d * N[0], nV[1] - two_d * N[1], nV[2] - two_d * N[2])
    NoV = np.abs(dot(N, V)) + F(1e-5)
    NoL = np.fmax(dot(N, L), F(0.0))
    # B. visibility
    ds = f32a(resolved)[ys, xs] if has_sun else np.ones(len(ys), np.float32)
    cs = f32a(contact)[ys, xs] if has_contact else np.ones(len(ys), np.float32)
    visibility = ds * cs
    # C. sun
    world_eye_y = np.fmax(world[1] * F(0.01) + K["min_altitude"], K["min_altitude"])
    sun_t = AM.sun_transmittance(A, K, transmittance, world_eye_y, np.full(len(ys), K["sun_cos_theta"], np.float32))
    hd = K["horizon_darkening"]
    direct = [(sun_t[c] * Li) * hd for c in range(3)]
    # D. sky pixels
    sky = d == 0
    lit = ~sky
    if sky.any():
        nVs = tuple(c[sky] for c in nV)
        zero, one = np.zeros(int(sky.sum()), np.float32), np.ones(int(sky.sum()), np.float32)
        up = (zero, one, zero)
        eye = (zero, zero + K["eye_altitude"], zero)
        right = normalize(cross(up, nVs))
        forward = normalize(cross(right, up))
        lx, ly = dot(L, forward), dot(L, right)
        ln = np.sqrt(lx * lx + ly * ly)
        hit = SM.intersect_has(eye, nVs, A.f("planet_radius"))
        su, sv = SM.sky_view_uv(K, (sky_view.shape[1], sky_view.shape[0]), hit, dot(nVs, up), (lx / ln, ly / ln))
        s = list(SM.sample_rgba(sky_view, su, sv))
        disc, inside = draw_sun(K["min_cos"], dot(nVs, L))
        li = disc * Li
        for c in range(3):
            s[c] = np.where(hit, s[c], s[c] + li * sun_t[c][sky]).astype(np.float32)
        sky_rgb = [s[c] * s[3] for c in range(3)]
        store(ys[sky], xs[sky], sky_rgb)
        st["sky_hit"] += int(hit.sum())
        st["sky_in_disc"] += int((~hit & inside).sum())
        st["sky_outside_disc"] += int((~hit & ~inside).sum())
        if detail is not None:
            detail.update(sky_hit=hit, sky_in_disc=~hit & inside, sky_nV=nVs, sky_rgb=sky_rgb, sky_uv=(su, sv))
    st["lit_nol_positive"] += int((lit & (NoL > 0)).sum())
    st["lit_nol_zero"] += int((lit & ~(NoL > 0)).sum())
    # E. aerial perspective (evaluated for the lit pixels; the others are not stored from here)
    aerial_c = [np.zeros(len(ys), np.float32) for _ in range(3)]
    spec_sky = [np.zeros(len(ys), np.float32) for _ in range(3)]
    diff_sky = [np.zeros(len(ys), np.float32) for _ in range(3)]
    if lit.any():
        rel = tuple(((world[c] - cam[c]) * F(0.01))[lit] for c in range(3))
        for c, plane in enumerate(aerial_perspective(A, K, aerial, u[lit], v[lit], rel, st)):
            aerial_c[c][lit] = plane
        # F, G. sky ambient
        t = F(1.0) - roughness
        refl = normalize(tuple(lerp(N[c], R[c], t) for c in range(3)))
        spec = cube_sample(cube, tuple(c[lit] for c in refl))
        diff = cube_sample(cube, tuple(c[lit] for c in N))
        for c in range(3):
            spec_sky[c][lit] = (spec[c] * spec[3]) * hd
            diff_sky[c][lit] = (diff[c] * diff[3]) * hd
    # H. surface, ambient
    F0 = [F(0.04) + (alb[c] - F(0.04)) * metallic for c in range(3)]
    alpha = np.fmax(roughness * roughness, PM.MIN_ALPHA)
    alpha2 = alpha * alpha
    ABx, ABy = PM.ggx_directional_albedo(NoV, alpha)
    Ess = saturate(ABx + ABy)
    ec = [F(1.0) + (F0[c] * (F(1.0) - Ess)) / np.fmax(Ess, F(1e-4)) for c in range(3)]
    S = dict(N=N, V=V, albedo=alb, F0=F0, ec=ec, metallic=metallic, NoV=NoV, alpha2=alpha2)
    spec_occlusion = saturate((pow_rule(NoV + occlusion, exp2_rule(F(-16.0) * roughness - F(1.0))) - F(1.0)) + occlusion)
    indirect = []
    for c in range(3):
        kS = F0[c] * ABx + ABy
        kD = (F(1.0) - metallic) * (F(1.0) - kS)
        ibl_diffuse = ((kD * diff_sky[c]) * alb[c]) * PM.FD_LAMBERT
        ibl_specular = (kS * spec_sky[c]) * spec_occlusion
        indirect.append(ibl_diffuse * occlusion + ibl_specular)
    # I. lights
    total = [np.zeros(len(ys), np.float32) for _ in range(3)]
    n_lights = 0 if lights is None else (len(np.asarray(lights).reshape(-1).view(np.uint8)) // 64 if light_count is None else int(light_count))
    if n_lights:
        lt = PM.unpack_lights(lights, n_lights)
        n_lit = int(lit.sum())
        for i in range(n_lights):
            kind = int(lt["kind"][i])
            if kind not in (PM.KIND_POINT, PM.KIND_SPOT):
                st["light_kind_skipped"] += n_lit
                continue
            pos = lt["position"][i]
            lv = (pos[0] - world[0], pos[1] - world[1], pos[2] - world[2])
            dist = np.sqrt(dot(lv, lv))
            Ll = (lv[0] / dist, lv[1] / dist, lv[2] / dist)
            att = PM.attenuate_point(dist, lt["range"][i])
            if kind == PM.KIND_SPOT:
                sd = normalize(tuple(lt["direction"][i]))
                cos_angle = dot((-Ll[0], -Ll[1], -Ll[2]), sd)
                att = att * PM.smoothstep(PM.cos_reduced_rule(lt["outer_cone_angle"][i])[0], PM.cos_reduced_rule(lt["inner_cone_angle"][i])[0], cos_angle)
            intensity = lt["intensity"][i]
            out_att = (att <= 0) | bool(intensity <= 0)
            NdotL = saturate(dot(N, Ll))
            out_ndl = ~out_att & (NdotL <= 0)
            shaded = ~out_att & ~out_ndl
            st["light_attenuation_out"] += int((out_att & lit).sum())
            st["light_ndotl_out"] += int((out_ndl & lit).sum())
            st["light_shaded"] += int((shaded & lit).sum())
            diffuse, specular = PM.brdf(S, Ll)
            for c in range(3):
                radiance = (lt["color"][i][c] * att) * intensity
                total[c] = np.where(shaded, total[c] + ((diffuse[c] + specular[c]) * radiance) * NdotL, total[c])
    # J. sun term
    horizon = saturate(F(1.0) + F(1.3) * dot(R, smooth))
    horizon = horizon * horizon
    diffuse, specular = PM.brdf(S, L)
    surface = [np.where(NoL > 0, (((diffuse[c] + specular[c] * horizon) * direct[c]) * NoL) * visibility, F(0.0)) for c in range(3)]
    # K. store
    rgb = [((((surface[c] + total[c]) + indirect[c]) + emission[c]) + aerial_c[c])[lit] for c in range(3)]
    store(ys[lit], xs[lit], rgb)
    if detail is not None:
        detail.update(ys=ys, xs=xs, lit=lit, sky=sky, world=world, V=V, N=N, NoL=NoL, indirect=indirect, aerial=aerial_c, direct=direct, sun_transmittance=sun_t,
                      surface=surface, total=total, emission=emission, lit_rgb=rgb)
    return out, st
