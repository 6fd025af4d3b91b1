"""Checker of oxc_decode_visbuffer: the geometry and material-factor half of passes/visbuffer_decode.slang (RendererInstance::decode_visbuffer,
Passes/DrawGeometry.cpp:192-274) restated in numpy from the rules include/oxcull.h states -- binary32 in the Slang's evaluation order, no
contraction, IEEE division and square root, the ambient occlusion's closed-form pow.  The fetch chain runs once per distinct texel, the
arithmetic once per pixel.  Written from the header, not from the kernel.  Returns the four images and fills `stats`."""
from __future__ import annotations

import numpy as np

import vsm_draw_model as DM
from pixel_rules import _u32, cross, mul_mp, pack_ufloat, pack_unorm4x8, srgb_unorm_encode, to_half_bits, unorm8, vec3_to_oct

F = np.float32
TERRAIN_INSTANCE_ID = 0xFFFFFE
HALF_NAN = 0x7E00
MATERIAL_BYTES = 56
IMAGES = ("albedo", "normal", "emissive", "mro")
COUNTER_NAMES = ("decoded", "empty", "zero_vertex_index", "default_material")


def dequantize_half_flush(h) -> np.ndarray:
    """com::dequantize_half with the flush spelled out, as the kernel must (its FP16 denormal mode keeps denormals): an exponent field of 0
    gives the sign alone."""
    h = np.asarray(h).astype(np.uint16)
    sign = ((h.astype(np.uint32) & np.uint32(0x8000)) << np.uint32(16)).view(np.float32)
    return np.where((h & 0x7C00) == 0, sign, h.view(np.float16).astype(np.float32)).astype(np.float32)


def decode_mesh_normal(packed) -> np.ndarray:
    """Mesh::decode_mesh_normal (scene.slang:486-489): uint32 [...] -> float32 [..., 3]."""
    p = np.asarray(packed, dtype=np.uint32)
    return np.stack([((p >> np.uint32(s)) & np.uint32(1023)).astype(np.float32) / F(511.0) - F(1.0) for s in (20, 10, 0)], axis=-1)


def normal_half(x) -> np.ndarray:
    """binary16 bits, round to nearest even, denormals kept, every NaN 0x7E00."""
    x = np.asarray(x, dtype=np.float32)
    return np.where(np.isnan(x), np.uint16(HALF_NAN), to_half_bits(x)).astype(np.uint16)


def normal_matrix(world) -> np.ndarray:
    """TransformWorld::normal_matrix (scene.slang:292-299): world float [..., 16] column-major -> [..., 3, 3] with N[..., r, c]: column c is
    cross(basis[c + 1], basis[c + 2]), basis[j] = column j of world's upper 3 x 3."""
    b = [(world[..., 4 * j + 0], world[..., 4 * j + 1], world[..., 4 * j + 2]) for j in range(3)]
    cols = [cross(b[1], b[2]), cross(b[2], b[0]), cross(b[0], b[1])]
    return np.stack([np.stack([cols[c][r] for c in range(3)], axis=-1) for r in range(3)], axis=-2)


@np.errstate(all="ignore")
def barycentrics(world_pos, pv, u, v):
    """compute_partial_derivatives up to lambda (visbuffer_decode.slang:45-73) in the dtype of its operands: world_pos [N, 3, 3], pv [16],
    u / v [N] -> (lambda [N, 3], clip [N, 3, 4])."""
    one = world_pos.dtype.type(1.0)
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
    lam = np.stack([interp_w * ((inv_w[:, 0] + dvx * ddx[0]) + dvy * ddy[0]), interp_w * (dvx * ddx[1] + dvy * ddy[1]),
                    interp_w * (dvx * ddx[2] + dvy * ddy[2])], axis=-1)
    return lam, clip


def pixel_ndc(xs, ys, W: int, H: int, dtype=np.float32):
    t = dtype
    return ((xs.astype(t) + t(0.5)) / t(W)) * t(2.0) - t(1.0), ((ys.astype(t) + t(0.5)) / t(H)) * t(2.0) - t(1.0)


def fetch(scene, meshlet_instances, texels, materials, material_count: int) -> dict:
    """The fetch chain of visbuffer_decode.slang:95-110 for distinct texels whose meshlet instance is in range.  `scene` is a CPU Scene: its
    Mesh and MeshLOD records hold the addresses of its own arrays.  Returns per texel: valid (no vertex index beyond vertex_count - 1), the
    vertex indices, and for the valid ones local / world positions, decoded normals, the world matrix, the material's halves."""
    texels = np.asarray(texels, dtype=np.uint32)
    inst, tri = (texels >> np.uint32(8)).astype(np.int64), (texels & np.uint32(0xFF)).astype(np.int64)
    recs = np.asarray(meshlet_instances).reshape(-1, 2).astype(np.int64)[inst]
    mi = np.asarray(scene.mesh_instances).reshape(-1, 5).astype(np.int64)[recs[:, 0]]
    meshes = np.asarray(scene.meshes).reshape(-1, 8)
    mesh = meshes[mi[:, 0]]
    vertex_count = _u32(np.asarray(scene.meshes)).reshape(-1, 16)[mi[:, 0], 6].astype(np.int64)
    lod = np.asarray(scene.lods).reshape(-1, 8)[(mesh[:, 4] - scene.lods.data_ptr()) // 64 + mi[:, 1]]
    ml = _u32(np.asarray(scene.meshlets)).reshape(-1, 4).astype(np.int64)[(lod[:, 1] - scene.meshlets.data_ptr()) // 16 + recs[:, 1]]
    micro = np.asarray(scene.micro).reshape(-1).view(np.uint8)
    vidx = _u32(scene.vidx).reshape(-1)
    vi = np.stack([vidx[(lod[:, 4] - scene.vidx.data_ptr()) // 4 + ml[:, 0] + micro[lod[:, 3] - scene.micro.data_ptr() + ml[:, 1] + tri * 3 + k].astype(np.int64)]
                   for k in range(3)], axis=-1).astype(np.int64)
    last = (vertex_count - 1) & 0xFFFFFFFF  # unsigned: wraps for vertex_count == 0
    valid = (vi <= last[:, None]).all(axis=-1)
    out = dict(valid=valid, vertex_indices=vi, material_index=mi[:, 2], triangle=tri)
    v = np.flatnonzero(valid)
    pairs = np.stack([np.repeat(inst[v], 3), (tri[v, None] * 3 + np.arange(3)).reshape(-1)], axis=-1).astype(np.uint32).reshape(-1)
    out["world_pos"] = DM.fetch_world(scene, meshlet_instances, pairs, wide=2)
    q = _u32(scene.positions).view(np.uint16).reshape(-1, 4)[((mesh[v, 0] - scene.positions.data_ptr()) // 8)[:, None] + vi[v]]
    out["local_pos"] = DM.dequantize_half(q[..., :3])
    normals = np.zeros((len(v), 3, 3), dtype=np.float32)
    has = mesh[v, 1] != 0  # a null vertex_normals decodes (0, 0, 0)
    if has.any():
        packed = _u32(scene.normals).reshape(-1)[((mesh[v, 1][has] - scene.normals.data_ptr()) // 4)[:, None] + vi[v][has]]
        normals[has] = decode_mesh_normal(packed)
    out["normals"] = normals
    out["world"] = np.asarray(scene.transforms, dtype=np.float32).reshape(-1, 16)[mi[v, 3]]
    mat = np.zeros((len(v), MATERIAL_BYTES // 2), dtype=np.uint16)
    inside = mi[v, 2] < int(material_count)
    if inside.any():
        mat[inside] = np.ascontiguousarray(np.asarray(materials)).view(np.uint16).reshape(-1, MATERIAL_BYTES // 2)[mi[v, 2][inside]]
    out["material_halves"], out["default_material"] = mat, ~inside
    return out


@np.errstate(all="ignore")
def decode(scene, meshlet_instances, vis, depth, projection_view, materials=None, material_count: int = 0, meshlet_instance_count: int = None,
           clear: bool = True, init: dict = None, stats: dict = None) -> dict:
    """vis uint32 / int32 [H, W], depth float32 [H, W] -> {"albedo": uint32 [H, W], "normal": uint16 [H, W, 4], "emissive": uint32 [H, W],
    "mro": uint32 [H, W]}.  `init`: what the images hold before the call (they matter with clear = False; zeros otherwise)."""
    vis, depth = _u32(vis), np.ascontiguousarray(depth, dtype=np.float32)
    H, W = vis.shape
    mli = np.asarray(meshlet_instances).reshape(-1, 2)
    count = len(mli) if meshlet_instance_count is None else int(meshlet_instance_count)
    pv = np.asarray(projection_view, dtype=np.float32)
    img = {"albedo": np.zeros((H, W), np.uint32), "normal": np.zeros((H, W, 4), np.uint16), "emissive": np.zeros((H, W), np.uint32), "mro": np.zeros((H, W), np.uint32)}
    if init is not None:
        img = {k: np.array(init[k], dtype=img[k].dtype).reshape(img[k].shape) for k in IMAGES}

    # 1. empty pixels, the first cause that holds
    inst = vis >> np.uint32(8)
    causes = [("empty_clear_value", vis == np.uint32(0xFFFFFFFF)), ("empty_terrain", inst == TERRAIN_INSTANCE_ID),
              ("empty_depth_zero", depth.view(np.uint32) == 0), ("empty_instance_range", inst >= count)]
    empty = np.zeros((H, W), dtype=bool)
    st = {}
    for name, hit in causes:
        st[name] = int((hit & ~empty).sum())
        empty |= hit
    if clear:
        for k in IMAGES:
            img[k][empty] = 0

    # 2. the fetch chain, once per distinct texel
    ys, xs = np.nonzero(~empty)
    texels, inverse = np.unique(vis[ys, xs], return_inverse=True)
    st.update(empty=int(empty.sum()), decoded=0, zero_vertex_index=0, default_material=0, distinct_triangles=0, distinct_materials=0,
              written=~empty | bool(clear))  # the pixels the call stores to
    if len(texels):
        f = fetch(scene, mli, texels, materials, material_count)
        bad = ~f["valid"][inverse]
        for k in IMAGES:
            img[k][ys[bad], xs[bad]] = 0
        st["zero_vertex_index"] = int(bad.sum())
        slot = np.cumsum(f["valid"]) - 1  # row of a valid texel in the per-triangle arrays
        ys, xs, t = ys[~bad], xs[~bad], slot[inverse[~bad]]
        st["decoded"] = len(t)
        st["distinct_triangles"] = int(len(np.unique(t)))
        st["default_material"] = int(f["default_material"][t].sum())
        st["distinct_materials"] = int(len(np.unique(f["material_index"][f["valid"]][t])))
        if len(t):
            # 4. barycentrics
            u, v = pixel_ndc(xs, ys, W, H)
            lam, clip = barycentrics(f["world_pos"][t], pv, u, v)
            # 5. normal
            N = normal_matrix(f["world"])
            n = f["normals"]
            wn = np.stack([(N[:, None, r, 0] * n[..., 0] + N[:, None, r, 1] * n[..., 1]) + N[:, None, r, 2] * n[..., 2] for r in range(3)], axis=-1)[t]  # [N, corner, 3]
            vec = [(lam[:, 0] * wn[:, 0, c] + lam[:, 1] * wn[:, 1, c]) + lam[:, 2] * wn[:, 2, c] for c in range(3)]
            ln = np.sqrt((vec[0] * vec[0] + vec[1] * vec[1]) + vec[2] * vec[2])
            world_normal = (vec[0] / ln, vec[1] / ln, vec[2] / ln)
            ex, ey = vec3_to_oct(world_normal)
            hx, hy = normal_half(ex), normal_half(ey)
            img["normal"][ys, xs] = np.stack([hx, hy, hx, hy], axis=-1)
            # 6. - 8. the material factors, per distinct triangle
            m = dequantize_half_flush(f["material_halves"][:, :9])
            albedo = (unorm8(srgb_unorm_encode(m[:, 0])) | (unorm8(srgb_unorm_encode(m[:, 1])) << np.uint32(8)) | (unorm8(srgb_unorm_encode(m[:, 2])) << np.uint32(16))
                      | (unorm8(m[:, 3]) << np.uint32(24)))
            emissive = pack_ufloat(m[:, 4], 6) | (pack_ufloat(m[:, 5], 6) << np.uint32(11)) | (pack_ufloat(m[:, 6], 5) << np.uint32(22))
            mro = pack_unorm4x8(m[:, 8], m[:, 7], np.ones_like(m[:, 7]), np.zeros_like(m[:, 7]))
            img["albedo"][ys, xs], img["emissive"][ys, xs], img["mro"][ys, xs] = albedo[t], emissive[t], mro[t]
            st.update(ys=ys, xs=xs, triangle_slot=t, lam=lam, clip=clip, fetched=f)
    if stats is not None:
        stats.update(st)
    return img


def counters(stats) -> dict:
    """The device's counters (oxc_debug_visbuffer_decode_stats) from the checker's stats."""
    return {k: int(stats[k]) for k in COUNTER_NAMES}
