"""Checker of oxc_decode_visbuffer_textured: steps 9 - 14 of include/oxcull.h restated in numpy -- the texcoords, the rescaled gradients, the
tangent frame, SampleGrad by the stated rule and the outputs -- on top of visbuffer_decode_model, whose fetch chain, barycentrics and
factor-only images it joins.  Binary32 in the header's order; the arithmetic of steps 10 and 12 runs in the dtype of its operands, so
tests/test_textured_decode_model.py evaluates the same lines in binary64.  Written from the header, not from the kernel.

An image is a dict(width, height, format, levels = [uint8 [h_k, w_k, 4 or 2]]) or None / levels = [] for an absent record; a sampler is
(filter, address, mip_filter)."""
from __future__ import annotations

import numpy as np

import visbuffer_decode_model as VD
from pixel_rules import (axis_clamp, cross, cvt_i32_sat, dot, log2_f64, mul_mp, pack_ufloat, pack_unorm4x8, sign, srgb_decode, srgb_unorm_encode,
                         unorm8, vec3_to_oct)

F = np.float32
UNORM, SRGB, RG8 = 0, 1, 2
KINDS = ("albedo", "normal", "emissive", "metallic_roughness", "occlusion")
TWO_COMPONENT, FLIP_Y = 1 << 5, 1 << 6
DEFAULT_SAMPLER = (1, 0, 1)
COUNTER_NAMES = VD.COUNTER_NAMES + tuple("sampled_" + k for k in KINDS) + ("level_taps", "jacobian_zero", "uniform_waves", "per_lane_waves")


# ---- step 10 ------------------------------------------------------------------------------------------------------------------------------------
@np.errstate(all="ignore")
def partials(world_pos, pv, u, v, W: int, H: int):
    """compute_partial_derivatives (visbuffer_decode.slang:45-83) in the dtype of its operands: world_pos [N, 3, 3], pv [16], u / v [N] ->
    (lambda [N, 3], ddx'' [N, 3], ddy'' [N, 3])."""
    t = world_pos.dtype.type
    one = t(1.0)
    clip = np.stack([mul_mp(pv, world_pos[:, k]) for k in range(3)], axis=1)
    inv_w = one / clip[..., 3]
    nx, ny = clip[..., 0] * inv_w, clip[..., 1] * inv_w
    inv_det = one / ((nx[:, 2] - nx[:, 1]) * (ny[:, 0] - ny[:, 1]) - (ny[:, 2] - ny[:, 1]) * (nx[:, 0] - nx[:, 1]))
    ddx = [((ny[:, 1] - ny[:, 2]) * inv_det) * inv_w[:, 0], ((ny[:, 2] - ny[:, 0]) * inv_det) * inv_w[:, 1], ((ny[:, 0] - ny[:, 1]) * inv_det) * inv_w[:, 2]]
    ddy = [((nx[:, 2] - nx[:, 1]) * inv_det) * inv_w[:, 0], ((nx[:, 0] - nx[:, 2]) * inv_det) * inv_w[:, 1], ((nx[:, 1] - nx[:, 0]) * inv_det) * inv_w[:, 2]]
    ddx_sum, ddy_sum = (ddx[0] + ddx[1]) + ddx[2], (ddy[0] + ddy[1]) + ddy[2]
    dvx, dvy = u - nx[:, 0], v - ny[:, 0]
    interp_inv_w = (inv_w[:, 0] + dvx * ddx_sum) + dvy * ddy_sum
    interp_w = one / interp_inv_w
    lam = [interp_w * ((inv_w[:, 0] + dvx * ddx[0]) + dvy * ddy[0]), interp_w * (dvx * ddx[1] + dvy * ddy[1]), interp_w * (dvx * ddx[2] + dvy * ddy[2])]
    sx, sy = t(2.0) / t(W), -(t(2.0) / t(H))
    rx, ry = [d * sx for d in ddx], [d * sy for d in ddy]
    interp_ddx_w, interp_ddy_w = one / (interp_inv_w + ddx_sum * sx), one / (interp_inv_w + ddy_sum * sy)
    bx = [interp_ddx_w * (lam[c] * interp_inv_w + rx[c]) - lam[c] for c in range(3)]
    by = [interp_ddy_w * (lam[c] * interp_inv_w + ry[c]) - lam[c] for c in range(3)]
    return np.stack(lam, axis=-1), np.stack(bx, axis=-1), np.stack(by, axis=-1)


def weigh(w, corners):
    """mul(vec, mat): (w.x * c_0 + w.y * c_1) + w.z * c_2 per component; w [N, 3], corners [N, 3, C] -> [N, C]."""
    return (w[:, 0, None] * corners[:, 0] + w[:, 1, None] * corners[:, 1]) + w[:, 2, None] * corners[:, 2]


@np.errstate(all="ignore")
def uv_gradient(lam, bx, by, texcoords, uv_size, uv_offset):
    """gradient_of and the material's scale (visbuffer_decode.slang:32-39, 119-122): texcoords [N, 3, 2] -> (uv, uv_ddx, uv_ddy), each [N, 2]."""
    return weigh(lam, texcoords) * uv_size + uv_offset, weigh(bx, texcoords) * uv_size, weigh(by, texcoords) * uv_size


# ---- step 12 ------------------------------------------------------------------------------------------------------------------------------------
def decode_level(level, fmt: int, dtype=np.float32):
    """uint8 [h, w, 4 or 2] -> [h, w, 4] in `dtype`: decode first, then filter.  binary64: the real sRGB curve."""
    b = np.asarray(level, dtype=np.uint8)
    out = np.empty(b.shape[:2] + (4,), dtype=dtype)
    if dtype == np.float32:
        unorm, curve = b.astype(np.float32) / F(255.0), srgb_decode
    else:
        unorm = b.astype(np.float64) / 255.0
        curve = lambda x: np.where(x / 255.0 <= 0.04045, x / 255.0 / 12.92, ((x / 255.0 + 0.055) / 1.055) ** 2.4)  # noqa: E731
    if fmt == RG8:
        out[..., :2], out[..., 2], out[..., 3] = unorm[..., :2], 0.0, 1.0
    else:
        out[..., :3] = curve(b[..., :3].astype(np.uint32)) if fmt == SRGB else unorm[..., :3]
        out[..., 3] = unorm[..., 3]
    return out


@np.errstate(all="ignore")
def level_of_detail(gx, gy, width: int, height: int, levels: int):
    """lambda of step 12 in the dtype of the gradients: binary32 takes the closed-form log2, binary64 the real one."""
    t = gx.dtype.type
    mxx, mxy, myx, myy = gx[:, 0] * t(width), gx[:, 1] * t(height), gy[:, 0] * t(width), gy[:, 1] * t(height)
    rho = np.fmax(np.sqrt(mxx * mxx + mxy * mxy), np.sqrt(myx * myx + myy * myy))
    lam = log2_f64(rho).astype(np.float32) if gx.dtype == np.float32 else np.log2(np.where(rho > 0, rho, 0.0))
    lam = np.where(np.isnan(lam), t(0.0), lam)
    return np.fmin(np.fmax(lam, t(0.0)), t(levels - 1)).astype(gx.dtype)


@np.errstate(all="ignore")
def axis_repeat(p, n: int):
    """wrap_axis of oxcull_pixel_device.hpp, the repeat axis oxc_apply_tonemap's taps use: (i0, i1, f) of the manual bilinear at the normalised
    coordinate p of a side of n texels, g = p * n - 0.5, i0 = floor_mod(the saturating conversion of floor(g), n), i1 = i0 + 1 wrapped to
    0, f = g - floor(g); both indices in [0, n - 1] for every bit pattern of p.  tests/test_textured_decode_model.py holds it to
    tonemap_model.bilinear_repeat bit for bit."""
    g = (p * F(n) - F(0.5)).astype(np.float32)
    fl = np.floor(g)
    i0 = np.mod(cvt_i32_sat(fl), n)
    return i0, np.where(i0 + 1 == n, 0, i0 + 1), (g - fl).astype(np.float32)


@np.errstate(all="ignore")
def axis(p, n: int, linear: bool, clamp: bool):
    """One axis of a level tap: (i0, i1, f)."""
    if linear:
        if p.dtype == np.float32:
            return axis_clamp(p, n) if clamp else axis_repeat(p, n)
        g = p * float(n) - 0.5  # the binary64 transcription of the same two axes
        fl = np.floor(g)
        i = cvt_i32_sat(fl)
        return (np.clip(i, 0, n - 1), np.clip(i + 1, 0, n - 1), g - fl) if clamp else (np.mod(i, n), np.mod(np.mod(i, n) + 1, n), g - fl)
    i = cvt_i32_sat(np.floor(p * p.dtype.type(n)))
    i = np.clip(i, 0, n - 1) if clamp else np.mod(i, n)
    return i, i, np.zeros(p.shape, dtype=p.dtype)


@np.errstate(all="ignore")
def level_tap(plane, uv, linear: bool, clamp: bool):
    """plane [h, w, 4] decoded, uv [N, 2] -> [N, 4]: the four texels in the bloom's order, lerp(lerp(t00, t10, fx), lerp(t01, t11, fx), fy)."""
    h, w = plane.shape[:2]
    x0, x1, fx = axis(uv[:, 0], w, linear, clamp)
    y0, y1, fy = axis(uv[:, 1], h, linear, clamp)
    if not linear:
        return plane[y0, x0]
    lerp = lambda a, b, t: a + (b - a) * t[:, None]  # noqa: E731
    return lerp(lerp(plane[y0, x0], plane[y0, x1], fx), lerp(plane[y1, x0], plane[y1, x1], fx), fy)


@np.errstate(all="ignore")
def sample_grad(image, sampler, uv, gx, gy, stats=None):
    """SampleGrad of a present image -> [N, 4] in the dtype of uv."""
    filt, address, mip = (int(v) != 0 for v in sampler)
    levels = min(len(image["levels"]), 15)
    dtype = uv.dtype.type
    planes = [decode_level(l, image["format"], dtype) for l in image["levels"][:levels]]
    lam = level_of_detail(gx, gy, image["width"], image["height"], levels)
    if stats is not None:
        stats["lambda"] = lam
    out = np.empty((len(uv), 4), dtype=uv.dtype)
    if mip:
        fl = np.floor(lam)
        lo = fl.astype(np.int64)
        hi = np.minimum(lo + 1, levels - 1)
        t = (lam - fl)[:, None]
        for a in np.unique(lo):
            for b in np.unique(hi[lo == a]):
                m = (lo == a) & (hi == b)
                ta, tb = level_tap(planes[a], uv[m], filt, address), level_tap(planes[b], uv[m], filt, address)
                out[m] = ta + (tb - ta) * t[m]
    else:
        lvl = np.minimum(np.floor(lam + dtype(0.5)).astype(np.int64), levels - 1)
        for a in np.unique(lvl):
            out[lvl == a] = level_tap(planes[a], uv[lvl == a], filt, address)
    return out


def present(image) -> bool:
    return (image is not None and len(image.get("levels", ())) > 0 and image["format"] <= 2 and 1 <= image["width"] <= 16384 and 1 <= image["height"] <= 16384)


# ---- step 11 ------------------------------------------------------------------------------------------------------------------------------------
@np.errstate(all="ignore")
def tangent_frame(bx, by, world_pos, camera_position, N, gx, gy):
    """(T, B, jacobian_sign): bx / by [N, 3], world_pos [N, 3, 3], N a 3-tuple of [N], gx / gy [N, 2]."""
    cam = np.asarray(camera_position, dtype=np.float32)
    r = world_pos - cam[None, None, :]
    pdx, pdy = weigh(bx, r), weigh(by, r)
    pdx, pdy = tuple(pdx[:, c] for c in range(3)), tuple(pdy[:, c] for c in range(3))
    dx, dy = dot(pdx, N), dot(pdy, N)
    sx, sy = tuple(pdx[c] - dx * N[c] for c in range(3)), tuple(pdy[c] - dy * N[c] for c in range(3))
    js = sign(gx[:, 0] * gy[:, 1] - gx[:, 1] * gy[:, 0])
    T = [js * (gy[:, 1] * sx[c] - gx[:, 1] * sy[c]) for c in range(3)]
    ln = np.sqrt((T[0] * T[0] + T[1] * T[1]) + T[2] * T[2])
    nz = js != 0
    T = tuple(np.where(nz, T[c] / ln, T[c]).astype(np.float32) for c in range(3))
    w = js * sign(dot(pdy, cross(N, pdx)))
    c = cross(N, T)
    return T, tuple((-w) * c[k] for k in range(3)), js


# ---- the whole call -----------------------------------------------------------------------------------------------------------------------------
def fetch_texcoords(scene, meshlet_instances, f, texels) -> np.ndarray:
    """Mesh::decode_texcoord for the valid texels of VD.fetch: float32 [n, 3, 2]; a null texture_coords decodes (0, 0)."""
    valid = f["valid"]
    inst = (np.asarray(texels, dtype=np.uint32) >> np.uint32(8)).astype(np.int64)[valid]
    recs = np.asarray(meshlet_instances).reshape(-1, 2).astype(np.int64)[inst]
    mesh_index = np.asarray(scene.mesh_instances).reshape(-1, 5).astype(np.int64)[recs[:, 0], 0]
    ptr = np.asarray(scene.meshes).reshape(-1, 8)[mesh_index, 2]
    out = np.zeros((len(inst), 3, 2), dtype=np.float32)
    has = ptr != 0
    if has.any():
        halves = np.ascontiguousarray(np.asarray(scene.texcoords)).view(np.uint16).reshape(-1, 2)
        out[has] = VD.dequantize_half_flush(halves[((ptr[has] - scene.texcoords.data_ptr()) // 4)[:, None] + f["vertex_indices"][valid][has]])
    return out


def wave_paths(H: int, W: int, ys, xs, material_index):
    """(uniform, per-lane): the 8 x 8 tiles with a decoded pixel whose decoded pixels name one material index, and the others."""
    tile = (ys // 8) * ((W + 7) // 8) + xs // 8
    uniform = per_lane = 0
    for t in np.unique(tile):
        if len(np.unique(material_index[tile == t])) == 1:
            uniform += 1
        else:
            per_lane += 1
    return uniform, per_lane


@np.errstate(all="ignore")
def decode(scene, meshlet_instances, vis, depth, projection_view, materials=None, material_count: int = 0, meshlet_instance_count: int = None, clear: bool = True,
           init: dict = None, stats: dict = None, *, camera_position=(0.0, 0.0, 0.0), images=(), samplers=()) -> dict:
    """The four images of oxc_decode_visbuffer_textured; `stats` as VD.decode fills it, plus the per-pixel uv, gradients and samples."""
    st = {}
    img = VD.decode(scene, meshlet_instances, vis, depth, projection_view, materials, material_count, meshlet_instance_count, clear, init, st)
    st.update({"sampled_" + k: 0 for k in KINDS}, level_taps=0, jacobian_zero=0, uniform_waves=0, per_lane_waves=0)
    if st["decoded"]:
        H, W = np.asarray(vis).shape
        ys, xs, t, f = st["ys"], st["xs"], st["triangle_slot"], st["fetched"]
        st["uniform_waves"], st["per_lane_waves"] = wave_paths(H, W, ys, xs, f["material_index"][f["valid"]][t])
        pv = np.asarray(projection_view, dtype=np.float32)
        u, v = VD.pixel_ndc(xs, ys, W, H)
        world_pos = f["world_pos"][t]
        lam, bx, by = partials(world_pos, pv, u, v, W, H)
        assert np.array_equal(lam.view(np.uint32), st["lam"].view(np.uint32))  # steps 1 - 4 are shared
        mli = np.asarray(meshlet_instances).reshape(-1, 2)
        tc = fetch_texcoords(scene, mli, f, _fetched_texels(vis, depth, mli, meshlet_instance_count))[t]
        mat = f["material_halves"][t]
        word = lambda k: mat[:, 2 * k].astype(np.uint32) | (mat[:, 2 * k + 1].astype(np.uint32) << np.uint32(16))  # noqa: E731
        flags, sampler_index = word(5), word(6)
        m = VD.dequantize_half_flush(mat)
        uv, gx, gy = uv_gradient(lam, bx, by, tc, m[:, 24:26], m[:, 26:28])
        st.update(uv=uv, uv_ddx=gx, uv_ddy=gy, ddx=bx, ddy=by)
        n = len(t)
        sampled = np.ones((5, n, 4), dtype=np.float32)
        has = np.zeros((5, n), dtype=bool)
        lod = np.full((5, n), np.nan, dtype=np.float32)  # lambda of step 12 per image kind; NaN where the kind is not sampled
        smp = np.array([samplers[i] if i < len(samplers) else DEFAULT_SAMPLER for i in sampler_index.tolist()], dtype=np.int64).reshape(n, -1)[:, :3] != 0
        for kind in range(5):
            index = word(7 + kind).astype(np.int64)
            flagged = ((flags >> np.uint32(kind)) & np.uint32(1)) != 0
            for i in np.unique(index[flagged]):
                if i >= len(images) or not present(images[i]):
                    continue
                for s in np.unique(smp[flagged & (index == i)], axis=0):
                    sel = flagged & (index == i) & (smp == s).all(axis=-1)
                    one = {}
                    sampled[kind][sel] = sample_grad(images[i], s, uv[sel], gx[sel], gy[sel], one)
                    lod[kind][sel] = one["lambda"]
                    has[kind] |= sel
                    st["level_taps"] += int(sel.sum()) * (2 if s[2] else 1)
            st["sampled_" + KINDS[kind]] = int(has[kind].sum())
        st.update(has=has, sampled=sampled, lod=lod)
        # step 14
        a = np.where(has[0][:, None], m[:, 0:4] * sampled[0], m[:, 0:4])
        albedo = (unorm8(srgb_unorm_encode(a[:, 0])) | (unorm8(srgb_unorm_encode(a[:, 1])) << np.uint32(8)) | (unorm8(srgb_unorm_encode(a[:, 2])) << np.uint32(16))
                  | (unorm8(a[:, 3]) << np.uint32(24)))
        e = np.where(has[2][:, None], m[:, 4:7] * sampled[2][:, :3], m[:, 4:7])
        emissive = pack_ufloat(e[:, 0], 6) | (pack_ufloat(e[:, 1], 6) << np.uint32(11)) | (pack_ufloat(e[:, 2], 5) << np.uint32(22))
        metallic = np.where(has[3], m[:, 8] * sampled[3][:, 2], m[:, 8])
        roughness = np.where(has[3], m[:, 7] * sampled[3][:, 1], m[:, 7])
        occlusion = np.where(has[4], sampled[4][:, 0], F(1.0)).astype(np.float32)
        img["albedo"][ys, xs], img["emissive"][ys, xs] = albedo, emissive
        img["mro"][ys, xs] = pack_unorm4x8(metallic, roughness, occlusion, np.zeros_like(occlusion))
        k = np.flatnonzero(has[1])
        if len(k):
            # world_normal once more, as VD.decode's step 5 has it
            Nm = VD.normal_matrix(f["world"])
            nn = f["normals"]
            wn = np.stack([(Nm[:, None, r, 0] * nn[..., 0] + Nm[:, None, r, 1] * nn[..., 1]) + Nm[:, None, r, 2] * nn[..., 2] for r in range(3)], axis=-1)[t[k]]
            L = lam[k]
            vec = [(L[:, 0] * wn[:, 0, c] + L[:, 1] * wn[:, 1, c]) + L[:, 2] * wn[:, 2, c] for c in range(3)]
            ln = np.sqrt((vec[0] * vec[0] + vec[1] * vec[1]) + vec[2] * vec[2])
            N = (vec[0] / ln, vec[1] / ln, vec[2] / ln)
            T, B, js = tangent_frame(bx[k], by[k], world_pos[k], camera_position, N, gx[k], gy[k])
            st["jacobian_zero"] = int((js == 0).sum())
            s = sampled[1][k, :3] * F(2.0) - F(1.0)
            sx, sy, sz = s[:, 0], s[:, 1], s[:, 2]
            sy = np.where((flags[k] & FLIP_Y) != 0, -sy, sy)
            two = np.sqrt(np.fmin(np.fmax(F(1.0) - (sx * sx + sy * sy), F(0.0)), F(1.0)))
            sz = np.where((flags[k] & TWO_COMPONENT) != 0, two, sz)
            nv = [(sx * T[c] + sy * B[c]) + sz * N[c] for c in range(3)]
            ln = np.sqrt((nv[0] * nv[0] + nv[1] * nv[1]) + nv[2] * nv[2])
            ex, ey = vec3_to_oct((nv[0] / ln, nv[1] / ln, nv[2] / ln))
            img["normal"][ys[k], xs[k], 0], img["normal"][ys[k], xs[k], 1] = VD.normal_half(ex), VD.normal_half(ey)
            st.update(tangent=T, bitangent=B, jacobian_sign=js, normal_pixels=k)
    if stats is not None:
        stats.update(st)
    return img


def _fetched_texels(vis, depth, mli, meshlet_instance_count):
    """The distinct non-empty texels in VD.decode's order (step 1 of the header)."""
    vis = np.ascontiguousarray(np.asarray(vis)).view(np.uint32)
    count = len(mli) if meshlet_instance_count is None else int(meshlet_instance_count)
    inst = vis >> np.uint32(8)
    empty = (vis == np.uint32(0xFFFFFFFF)) | (inst == VD.TERRAIN_INSTANCE_ID) | (np.ascontiguousarray(depth, dtype=np.float32).view(np.uint32) == 0) | (inst >= count)
    return np.unique(vis[~empty])


def counters(stats) -> dict:
    """The device's counters (oxc_debug_visbuffer_decode_textured_stats) from the checker's stats."""
    return {k: int(stats[k]) for k in COUNTER_NAMES}
