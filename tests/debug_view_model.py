"""Checker of oxc_apply_debug_view: the views of passes/debug_view.slang and passes/rmvsm_debug.slang restated in numpy binary32, vectorised
over pixels, by the rules of include/oxcull.h (steps V1 - V4 and R1 - R5).  The numeric rules come from pixel_rules; the resolve's set-up
(texel length, clipmap index, the clipmap records, the page wrap) from vsm_resolve_model, which this checker joins as
pbr_atmosphere_model joins the checkers it builds on."""
from __future__ import annotations

import numpy as np

import vsm_resolve_model as RM
from pixel_rules import _u32, channel_half, exp2_rule, f32a, from_half_bits, length, log2_rule, oct_to_vec3, saturate, srgb_decode, unpack_b10g11r11, unproject

F = np.float32
(TRIANGLES, MESHLETS, OVERDRAW, MATERIALS, MESH_INSTANCES, MESH_LODS, ALBEDO, NORMAL, EMISSIVE, METALLIC, ROUGHNESS, BAKED_OCCLUSION, GTAO, GEOMETRIC_NORMAL,
 RMVSM) = range(1, 16)
MAIN_VIEWS = tuple(range(TRIANGLES, RMVSM))
ID_VIEWS = (TRIANGLES, MESHLETS, MATERIALS, MESH_INSTANCES, MESH_LODS)
RECORD_VIEWS = (MATERIALS, MESH_INSTANCES, MESH_LODS)
NAMES = {TRIANGLES: "triangles", MESHLETS: "meshlets", OVERDRAW: "overdraw", MATERIALS: "materials", MESH_INSTANCES: "mesh_instances", MESH_LODS: "mesh_lods",
         ALBEDO: "albedo", NORMAL: "normal", EMISSIVE: "emissive", METALLIC: "metallic", ROUGHNESS: "roughness", BAKED_OCCLUSION: "baked_occlusion", GTAO: "gtao",
         GEOMETRIC_NORMAL: "geometric_normal", RMVSM: "rmvsm"}
EMPTY = 0xFFFFFFFF
HALF_ONE = 0x3C00
TAU = F(6.283185307179586)
SIXTH = F(1.0471975512)
VISIBLE, DIRTY, BACKED = 1, 2, 4
INFERNO = tuple(tuple(F(c) for c in row) for row in (
    (0.0002189403691192265, 0.001651004631001012, -0.01948089843709184),
    (0.1065134194856116, 0.5639564367884091, 3.932712388889277),
    (11.60249308247187, -3.972853965665698, -15.9423941062914),
    (-41.70399613139459, 17.43639888205313, 44.35414519872813),
    (77.162935699427, -33.40235894210092, -81.80730925738993),
    (-71.31942824499214, 32.62606426397723, 73.20951985803202),
    (25.13112622477341, -12.24266895238567, -23.07032500287172)))
SOBEL_X = (1, 0, -1, 2, 0, -2, 1, 0, -1)
SOBEL_Y = (1, 2, 1, 0, 0, 0, -1, -2, -1)
SAMPLE_OFFSET = ((-1, 1), (0, 1), (1, 1), (-1, 0), (0, 0), (1, 0), (-1, -1), (0, -1), (1, -1))


# ---- the shared rules -----------------------------------------------------------------------------------------------------------------------
def hash_u32(a) -> np.ndarray:
    """debug_view.slang:31-39, modulo 2^32."""
    M = np.uint64(0xFFFFFFFF)
    a = np.atleast_1d(np.asarray(a)).astype(np.uint64) & M
    a = ((a + np.uint64(0x7ed55d16)) + (a << np.uint64(12))) & M
    a = (a ^ np.uint64(0xc761c23c)) ^ (a >> np.uint64(19))
    a = ((a + np.uint64(0x165667b1)) + (a << np.uint64(5))) & M
    a = ((a + np.uint64(0xd3a2646c)) & M) ^ ((a << np.uint64(9)) & M)
    a = ((a + np.uint64(0xfd7046c5)) + (a << np.uint64(3))) & M
    a = (a ^ np.uint64(0xb55a4f09)) ^ (a >> np.uint64(16))
    return a.astype(np.uint32)


def hash_colour(a):
    h = hash_u32(a)
    return tuple(((h >> np.uint32(s)) & np.uint32(255)).astype(np.float32) / F(255.0) for s in (0, 8, 16))


@np.errstate(all="ignore")
def hsv_to_rgb(hue):
    """hsv_to_rgb((hue, 1.0, 0.5)), debug_view.slang:25-29: fmodf is exact, a NaN k gives 0.5 - 0.5 * 1.0."""
    q = f32a(hue) / SIXTH
    out = []
    for n in (F(5.0), F(3.0), F(1.0)):
        k = np.fmod(n + q, F(6.0)).astype(np.float32)
        out.append(F(0.5) - (F(0.5) * F(1.0)) * np.fmax(F(0.0), np.fmin(k, np.fmin(F(4.0) - k, F(1.0)))))
    return tuple(out)


def inferno(t):
    t = saturate(t)
    out = []
    for ch in range(3):
        c = [row[ch] for row in INFERNO]
        out.append(c[0] + t * (c[1] + t * (c[2] + t * (c[3] + t * (c[4] + t * (c[5] + t * c[6]))))))
    return tuple(out)


@np.errstate(all="ignore")
def density(vis, depth) -> np.ndarray:
    """V4's s of every texel: log2(depth + 1.0) * 10.0, NaN where the tap adds nothing (a ~0u texel).  The rule never gives a NaN itself."""
    s = (log2_rule(f32a(depth).reshape(-1) + F(1.0)) * F(10.0)).astype(np.float32).reshape(np.shape(depth))
    return np.where(_u32(vis) == EMPTY, F(np.nan), s).astype(np.float32)


@np.errstate(all="ignore")
def outline(vis, depth) -> np.ndarray:
    """V4: float32 [H, W], the taps in the order of sample_offset, a tap outside the image adding nothing."""
    H, W = np.shape(depth)
    tile = np.full((H + 2, W + 2), np.nan, dtype=np.float32)
    tile[1:-1, 1:-1] = density(vis, depth)
    gx, gy = np.zeros((H, W), np.float32), np.zeros((H, W), np.float32)
    for (dx, dy), wx, wy in zip(SAMPLE_OFFSET, SOBEL_X, SOBEL_Y):
        s = tile[1 + dy:1 + dy + H, 1 + dx:1 + dx + W]
        on = ~np.isnan(s)
        gx = np.where(on, gx + F(wx) * s, gx)
        gy = np.where(on, gy + F(wy) * s, gy)
    return np.fmax(np.abs(gx), np.abs(gy)).astype(np.float32)


def records(texel, meshlet_instance_count, meshlet_instances, mesh_instances, meshes):
    """V3: (material_index, mesh_index, lod_index, lod_count) behind every texel, zeros beyond the count."""
    inst = (np.asarray(texel).astype(np.int64) >> 8)
    ok = inst < int(meshlet_instance_count)
    zero = np.zeros(inst.shape, np.int64)
    if not ok.any():
        return zero, zero, zero, zero
    mli = _u32(meshlet_instances).reshape(-1, 2).astype(np.int64)
    mi = _u32(mesh_instances).reshape(-1, 5).astype(np.int64)
    lod_counts = _u32(meshes).reshape(-1, 16)[:, 7].astype(np.int64)
    rec = mi[mli[np.where(ok, inst, 0), 0]]
    pick = lambda v: np.where(ok, v, 0)  # noqa: E731
    return pick(rec[:, 2]), pick(rec[:, 0]), pick(rec[:, 1]), pick(lod_counts[rec[:, 0]])


@np.errstate(all="ignore")
def colour(view, texel, pix, *, heatmap_scale=0.0, meshlet_instance_count=0, overdraw=None, albedo=None, normal=None, emissive=None, mr_occlusion=None, ao=None,
           meshlet_instances=None, mesh_instances=None, meshes=None):
    """V2 / V3 for the covered pixels: `texel` their visbuffer texels, `pix` = (ys, xs)."""
    texel = np.asarray(texel).astype(np.uint32)
    if view == TRIANGLES:
        return hash_colour(texel & np.uint32(0xFF))
    if view == MESHLETS:
        return hash_colour(texel >> np.uint32(8))
    if view in RECORD_VIEWS:
        material, mesh, lod, lod_count = records(texel, meshlet_instance_count, meshlet_instances, mesh_instances, meshes)
        if view == MATERIALS:
            return hash_colour(material)
        if view == MESH_INSTANCES:
            return hash_colour(mesh)
        divisor = ((lod_count + 1) & 0xFFFFFFFF).astype(np.uint32).astype(np.float32)
        return hsv_to_rgb((lod.astype(np.uint32).astype(np.float32) / divisor) * TAU)
    if view == OVERDRAW:
        draw_scale = np.fmin(np.fmax(F(heatmap_scale), F(0.0)), F(100.0)) / F(100.0)
        count = _u32(overdraw)[pix].astype(np.float32)
        return inferno(F(1.0) - exp2_rule((-count) * draw_scale))
    if view == ALBEDO:
        w = _u32(albedo)[pix]
        return tuple(srgb_decode((w >> np.uint32(s)) & np.uint32(0xFF)) for s in (0, 8, 16))
    if view in (NORMAL, GEOMETRIC_NORMAL):
        h = np.ascontiguousarray(np.asarray(normal)).view(np.uint16).reshape(np.shape(normal)[0], np.shape(normal)[1], 4)[pix]
        k = 0 if view == NORMAL else 2
        n = oct_to_vec3(from_half_bits(h[:, k]), from_half_bits(h[:, k + 1]))
        return tuple(c * F(0.5) + F(0.5) for c in n)
    if view == EMISSIVE:
        return unpack_b10g11r11(_u32(emissive)[pix])
    if view == GTAO:
        v = from_half_bits(np.ascontiguousarray(np.asarray(ao)).view(np.uint16)[pix])
        return v, v, v
    v = ((_u32(mr_occlusion)[pix] >> np.uint32(8 * (view - METALLIC))) & np.uint32(0xFF)).astype(np.float32) / F(255.0)
    return v, v, v


@np.errstate(all="ignore")
def debug_view(view, vis, depth, *, clear=True, init=None, stats=None, **inputs) -> np.ndarray:
    """One oxc_apply_debug_view call of a main view: uint16 [H, W, 4].  `init` is the image before the call (what a discarded pixel keeps
    without `clear`).  `stats` receives `outline` (float32 [H, W]) and `covered` (bool [H, W])."""
    assert view in MAIN_VIEWS
    vis = _u32(vis)
    H, W = vis.shape
    depth = f32a(depth).reshape(H, W)
    out = np.zeros((H, W, 4), np.uint16) if init is None else np.ascontiguousarray(np.asarray(init)).view(np.uint16).reshape(H, W, 4).copy()
    covered = vis != EMPTY
    if clear:
        out[~covered] = (0, 0, 0, HALF_ONE)
    ol = outline(vis, depth)
    pix = np.nonzero(covered)
    if pix[0].size:
        rgb = colour(view, vis[pix], pix, **inputs)
        k = F(1.0) - ol[pix]
        for ch in range(3):
            out[pix[0], pix[1], ch] = channel_half(saturate(f32a(rgb[ch]) * k))
        out[pix[0], pix[1], 3] = HALF_ONE
    if stats is not None:
        stats.update(outline=ol, covered=covered)
    return out


# ---- the RMVSM view -------------------------------------------------------------------------------------------------------------------------
SKY, BORDER, PAGE_BACKED, PAGE_DIRTY, PAGE_VISIBLE, NOT_BACKED_VISIBLE = 1, 2, 4, 8, 16, 32


@np.errstate(all="ignore")
def rmvsm(depth, table, clipmaps, inv_pv, resolution, *, page_size=128, page_table_size=64, physical_page_table_size=8192, clipmap_count=10,
          first_clipmap_width=10.0, bias=-1.5, virtual_extent=8192.0, stats=None) -> np.ndarray:
    """One oxc_apply_debug_view call of the RMVSM view: uint16 [H, W, 4].  `stats` receives `classes` (uint8 [H, W]: SKY, or BORDER, or the
    PAGE_* bits of the entry, with NOT_BACKED_VISIBLE), `in_page` (int64 [H, W, 2], -1 at sky pixels), `clipmap` (the selected index, -1 at sky
    pixels) and `nan_uv` (a component of clip_uv is a NaN)."""
    depth = f32a(depth)
    H, W = depth.shape
    ps, n = int(page_size), int(page_table_size)
    S = RM.Shape(table, clipmaps, np.zeros((0, 0), np.float32), page_size=ps, page_table_size=n, physical_page_table_size=0, clipmap_count=clipmap_count)
    out = np.full((H, W, 4), HALF_ONE, np.uint16)
    classes = np.full((H, W), SKY, np.uint8)
    in_page = np.full((H, W, 2), -1, np.int64)
    clipmap, nan_uv = np.full((H, W), -1, np.int64), np.zeros((H, W), bool)
    ys, xs = np.nonzero(depth != F(0.0))  # (a NaN depth is not sky)
    if xs.size:
        inv_pv, resolution, d = f32a(inv_pv), f32a(resolution), depth[ys, xs]
        # R2: oxc_resolve_shadowmap step 2
        u = (xs.astype(np.float32) + F(0.5)) / F(W)
        v = (ys.astype(np.float32) + F(0.5)) / F(H)
        world = unproject(inv_pv, u, v, d)
        o = (F(1.0) / resolution) * F(0.5)
        lft = unproject(inv_pv, u + -o[0], v + o[1], d)
        rgt = unproject(inv_pv, u + o[0], v + o[1], d)
        tl = RM.texel_length(n, first_clipmap_width, virtual_extent)
        c = RM.clipmap_index(length((lft[0] - rgt[0], lft[1] - rgt[1], lft[2] - rgt[2])) / tl, bias, clipmap_count)
        m = S.mats[c]
        hx, hy, hw = RM._row(m, 0, world), RM._row(m, 1, world), RM._row(m, 3, world)
        su, sv = (hx / hw + F(1.0)) * F(0.5), (hy / hw + F(1.0)) * F(0.5)
        # R3
        inside = (su >= 0) & (su <= 1) & (sv >= 0) & (sv <= 1)
        su0, sv0 = np.where(inside, su, F(0)), np.where(inside, sv, F(0))
        fphys = F(physical_page_table_size)
        tx = np.where(inside, np.floor(su0 * fphys).astype(np.int64) % ps, ps - 1)
        ty = np.where(inside, np.floor(sv0 * fphys).astype(np.int64) % ps, ps - 1)
        border = (tx < 2) | (ty < 2) | (tx > ps - 2) | (ty > ps - 2)
        # R4
        rgb = hsv_to_rgb((c.astype(np.uint32).astype(np.float32) / F(clipmap_count + 1)) * TAU)
        # R5
        vx, vy = np.floor(su0 * F(n)).astype(np.int64), np.floor(sv0 * F(n)).astype(np.int64)
        in_table = (vx >= 0) & (vx <= n - 1) & (vy >= 0) & (vy <= n - 1)
        wx, wy = RM.wrap(np.clip(vx, 0, n - 1), S.offs[c, 0], n), RM.wrap(np.clip(vy, 0, n - 1), S.offs[c, 1], n)
        e = np.where(in_table, S.table[c, wy, wx].astype(np.int64), 0)
        backed, dirty, visible = (e & BACKED) != 0, (e & DIRTY) != 0, (e & VISIBLE) != 0
        red = ~backed & visible
        page = [np.where(red, True, backed), np.where(red, False, dirty), np.where(red, False, visible)]
        for ch in range(3):
            out[ys, xs, ch] = np.where(border, channel_half(rgb[ch]), np.where(page[ch], HALF_ONE, 0)).astype(np.uint16)
        cls = backed * PAGE_BACKED + dirty * PAGE_DIRTY + visible * PAGE_VISIBLE + red * NOT_BACKED_VISIBLE
        classes[ys, xs] = np.where(border, BORDER, cls).astype(np.uint8)
        in_page[ys, xs, 0], in_page[ys, xs, 1] = tx, ty
        clipmap[ys, xs], nan_uv[ys, xs] = c, np.isnan(su) | np.isnan(sv)
    if stats is not None:
        stats.update(classes=classes, in_page=in_page, clipmap=clipmap, nan_uv=nan_uv)
    return out
