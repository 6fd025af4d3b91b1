"""oxc_draw_terrain beside the passes around it: after and before oxc_draw_visbuffer on one context and one image (the shared raster scratch
allocated by either draw), and the frame with ground from bake to lit image on the device with no texel made on the CPU."""
import ctypes as C
import dataclasses

import numpy as np
import pytest
import torch

import terrain_decode_frames as DF
import terrain_draw_frames as FR
import terrain_draw_model as TM
from oxylus_amd import lib as L

pytestmark = pytest.mark.gpu
rep = dataclasses.replace
W, H = 96, 64


def _u64(t) -> np.ndarray:
    return t.cpu().numpy().view(np.uint64).copy()


def _draw_context(f, visdepth, depth=None, vis=None, clear=False):
    from oxylus_amd.renderer import ImageAttachment, TerrainDrawContext

    t = lambda a, view: torch.from_numpy(np.ascontiguousarray(a).view(view).copy()).cuda()  # noqa: E731
    return TerrainDrawContext(visdepth, [float(x) for x in f.cam.projection_view], f.cam.position, f.cam.near_clip, f.cam.projection_scale, DF.renderer_terrain(f.T),
                              (f.heightmap.shape[1], f.heightmap.shape[0]), t(f.heightmap, np.int16), t(f.visible, np.int32), t(f.draw_cmd, np.int32), clear,
                              None if depth is None else ImageAttachment.depth(depth), vis)


def _mesh_frame(r):
    from scenes import main_scene
    from test_gpu_visbuffer_decode import draw

    cpu, _ = main_scene()
    gpu, vis_t, depth_t, main, visdepth = draw(r, cpu, W, H)
    return cpu, gpu, vis_t, depth_t, main, visdepth


def test_after_the_mesh_draw_with_exact_depth_ties(renderer):
    """The mesh frame drawn first by oxc_draw_visbuffer, then the terrain into the same image without clear.  At every third mesh pixel the
    depth half is replaced by the terrain's own depth bits (the mesh vis stays): an exact tie, which the terrain wins; elsewhere the
    nearer of the two.  The raster stats read the shared header after either draw."""
    r = renderer
    _, _, _, _, _, visdepth = _mesh_frame(r)
    mesh_stats = r.debug_raster_stats()
    assert set(mesh_stats) == {"big", "clipped", "tiles", "overflowed_segments"}
    f = FR.frame((W, H), (3, 2), "ground", target_edge_pixels=4.0, clear=False)
    alone = FR.want(rep(f, clear=True))["visdepth"]
    assert (alone != 0).all()
    image = _u64(visdepth)
    ys, xs = np.mgrid[0:H, 0:W]
    tie = (image != 0) & ((ys * W + xs) % 3 == 0)
    assert tie.sum() > 50
    image[tie] = (alone[tie] & np.uint64(0xFFFFFFFF00000000)) | (image[tie] & np.uint64(0xFFFFFFFF))
    visdepth.copy_(torch.from_numpy(image.view(np.int64)).cuda())
    f = rep(f, before=image)
    counts = {}
    want = FR.want(f, counts)
    r.draw_terrain_for_visbuffer(_draw_context(f, visdepth))
    got = _u64(visdepth)
    assert (got == want["visdepth"]).all()
    assert ((got[tie] & np.uint64(0xFFFFFFFF)) == TM.VIS).all()
    mesh_kept = (image != 0) & ~tie & ((got & np.uint64(0xFFFFFFFF)) != TM.VIS)
    assert mesh_kept.any() and (got[mesh_kept] == image[mesh_kept]).all()
    s = r.debug_terrain_draw_stats()
    assert {k: s[k] for k in TM.STATS} == {k: counts[k] for k in TM.STATS}
    assert r.debug_raster_stats()["clipped"] == 0  # the terrain's counters sit beside the raster's in the header and do not leak into them


def test_a_fresh_context_terrain_first_then_the_mesh_draw(renderer):
    """On a context of its own the terrain call is the one that allocates the raster scratch; the mesh draw follows on the same image without
    clear.  The image is the session context's mesh image with the terrain over it."""
    from oxylus_amd.renderer import CullGeometryContext, PreparedFrame, RendererInstance

    cpu, _, _, _, _, mesh_visdepth = _mesh_frame(renderer)
    mesh = _u64(mesh_visdepth)
    f = FR.frame((W, H), (3, 2), "oblique", target_edge_pixels=2.0)
    r2 = RendererInstance(0)
    try:
        visdepth = torch.full((H, W), -1, dtype=torch.int64, device="cuda")
        r2.draw_terrain_for_visbuffer(_draw_context(f, visdepth, clear=True))
        counts = {}
        want_terrain = FR.want(f, counts)["visdepth"]
        s = r2.debug_terrain_draw_stats()
        assert {k: s[k] for k in TM.STATS} == {k: counts[k] for k in TM.STATS}
        assert (_u64(visdepth) == want_terrain).all()
        gpu = cpu.to("cuda")
        r2.reserve(gpu.n_mesh_instances, gpu.n_meshlet_instances)
        r2.prepared_frame = PreparedFrame.create(gpu)
        main = CullGeometryContext(init_cull_meshes=False, cull_flags=L.CULL_TEST_ALL, cull_camera=gpu.cull_camera())
        r2.seed_meshlet_instances(main, gpu.n_meshlet_instances)
        r2.cull_geometry(main)
        r2.draw_visbuffer(main, cpu.camera["projection_view"], W, H, visdepth, clear=False)
        torch.cuda.synchronize()
        assert (_u64(visdepth) == np.maximum(want_terrain, mesh)).all()
        assert (np.maximum(want_terrain, mesh) != want_terrain).any() and (np.maximum(want_terrain, mesh) != mesh).any()
    finally:
        r2.close()


class _WithCommand:
    """A TerrainDrawContext whose draw_cmd_buffer is the callee-owned command of oxc_cull_terrain."""

    def __init__(self, base, command: L.Buffer):
        self.base, self.command = base, command

    def c(self):
        c = self.base.c()
        c.draw_cmd_buffer = self.command
        return c


def test_the_frame_with_ground_from_bake_to_lit_image_in_one_graph(renderer, oracle_lib):
    """oxc_generate_terrain_maps -> oxc_cull_terrain -> oxc_draw_terrain -> oxc_decode_visbuffer(clear) -> oxc_decode_terrain -> oxc_apply_pbr,
    captured in one graph and replayed twice, against the checkers chained.  The mesh pixels are main_scene drawn by oxc_draw_visbuffer into
    the image before; the draw reads the heightmap the bake wrote, the list and the command the cull wrote, and resolves the depth and vis the
    decodes read: no texel is made on the CPU."""
    import gpu_passes as GP
    import oracle
    import terrain_decode_model as TD
    import terrain_maps_frames as TF
    from gpu_passes import same
    from oxylus_amd.renderer import PBRContext, TerrainDecodeContext, TerrainDrawContext, ImageAttachment
    from pixel_rules import unpack_b10g11r11

    r = renderer
    cpu, gpu, vis_t, depth_t, _, visdepth = _mesh_frame(r)
    frame_of_scene = r.prepared_frame
    mesh_image = _u64(visdepth)
    res, pc, G, D, images, maps_want, _ = TF.engine_48x40()
    T = FR.terrain(pc, target_edge_pixels=2.0, layers=(0, 1, 2, TD.INVALID_LAYER))
    pv, ipv = DF.camera(W, H)
    cam = FR.camera("down", W, H)
    assert cam.projection_view.tobytes() == pv.tobytes()

    gs = TF.guards(images)
    maps_ctx = TF.context(G, D, res, pc, gs)
    # the cull: TestFrustum alone keeps the mask's patches that are inside the frustum; two patches are masked out
    total = pc[0] * pc[1]
    mask_bits = ((1 << total) - 1) & ~((1 << 4) | (1 << 7))
    mask_cpu = torch.tensor([mask_bits], dtype=torch.int64).to(torch.int32)
    mask_gpu = mask_cpu.clone().cuda()
    cull_cam = L.CullCamera()
    for i in range(16):
        cull_cam.projection_view[i] = float(pv[i])
    for i in range(3):
        cull_cam.position[i] = cam.position[i]
    cull_cam.near_clip = cam.near_clip
    cull_cam.resolution[0], cull_cam.resolution[1] = float(W), float(H)
    cull_cam.acceptable_lod_error = 2.0
    visible_t = torch.full((total,), -1, dtype=torch.int32, device="cuda")
    mm_t = gs["patch_minmax"].tensor
    tc = L.TerrainContext()
    tc.struct_size = C.sizeof(L.TerrainContext)
    tc.cull_flags = L.CULL_TEST_FRUSTUM
    tc.cull_camera = cull_cam
    tc.world_min[0], tc.world_min[1] = T.world_min
    tc.world_size[0], tc.world_size[1] = T.world_size
    tc.patch_count[0], tc.patch_count[1] = pc
    tc.base_height, tc.height_scale = T.base_height, T.height_scale
    mm = L.Image()
    mm.dptr, mm.width, mm.height, mm.levels = mm_t.data_ptr(), pc[0], pc[1], 1
    tc.patch_minmax_attachment = mm
    tc.visible_patches_buffer = L.Buffer(C.c_void_p(visible_t.data_ptr()), total * 4)
    tc.patch_visibility_mask_buffer = L.Buffer(C.c_void_p(mask_gpu.data_ptr()), 4)
    lib = L.load()

    def cull(stream=None):
        r._check(lib.oxc_cull_terrain(r._ctx, C.byref(tc), r._stream(stream)))

    r.generate_terrain_maps(maps_ctx)
    cull()  # the callee-owned command exists from here on
    command = L.Buffer(tc.draw_cmd_buffer.dptr, tc.draw_cmd_buffer.bytes)
    assert command.dptr and command.bytes >= 16
    base = TerrainDrawContext(visdepth, [float(x) for x in pv], cam.position, cam.near_clip, cam.projection_scale, DF.renderer_terrain(T), res, maps_ctx.heightmap, visible_t,
                              visible_t[:4], False, ImageAttachment.depth(depth_t), vis_t)
    draw_ctx = _WithCommand(base, command)
    dctx = GP.decode_context(gpu, vis_t, depth_t, cpu.camera["projection_view"])
    tctx = TerrainDecodeContext.over(dctx, maps_ctx, ipv, DF.renderer_terrain(T), None)
    ones = torch.ones((H, W), dtype=torch.float32, device="cuda")
    pctx = PBRContext.create(depth_t, dctx.albedo_attachment, dctx.normal_attachment, dctx.emissive_attachment, dctx.metallic_roughness_occlusion_attachment,
                             ones.to(torch.float16).view(torch.int16), ones, None, L.SCENE_HAS_DIRECTIONAL_LIGHT | L.SCENE_HAS_SKY, ipv, (0.0, DF.CAMERA_HEIGHT, 0.0),
                             (0.3, 0.8, 0.5), 3.0, sky_solid_color=(0.25, 0.5, 1.0, 1.0), sky_ambient_color=(0.1, 0.15, 0.2))
    outputs = (gs["heightmap"].tensor, gs["normalmap"].tensor, gs["splatmap"].tensor, gs["patch_minmax"].tensor, visible_t, vis_t, depth_t, dctx.albedo_attachment,
               dctx.normal_attachment, dctx.emissive_attachment, dctx.metallic_roughness_occlusion_attachment, pctx.final_attachment)

    def chain(stream=None):
        r.generate_terrain_maps(maps_ctx, stream=stream)
        cull(stream)
        r.draw_terrain_for_visbuffer(draw_ctx, stream=stream)
        r.prepared_frame = frame_of_scene
        r.decode_visbuffer(dctx, stream=stream)
        r.decode_terrain(tctx, stream=stream)
        r.apply_pbr(pctx, stream=stream)

    # the checkers chained
    visible_want = oracle.cull_terrain(list(T.world_min), list(T.world_size), pc, T.base_height, T.height_scale, torch.from_numpy(maps_want["patch_minmax"].copy()), cull_cam,
                                       L.CULL_TEST_FRUSTUM, None, mask_cpu)
    assert 0 < visible_want.numel() < total
    counts = {}
    image_want = TM.draw(T, maps_want["heightmap"], cam, visible_want.numpy(), [4, visible_want.numel(), 0, 0], W, H, image=mesh_image, clear=False, counts=counts)
    depth_want, vis_want = TM.resolve(image_want)
    ground = vis_want == TM.VIS
    assert 0.1 < ground.mean() < 0.95 and ((vis_want != TM.VIS) & (depth_want != 0)).mean() > 0.05  # both terrain and mesh pixels
    mesh_want = None

    def check(label):
        nonlocal mesh_want
        torch.cuda.synchronize()
        same(TF.got_of(gs, images), maps_want, f"{label}: maps")
        assert visible_t.cpu()[:visible_want.numel()].tolist() == visible_want.tolist(), f"{label}: visible patches"
        assert (_u64(visdepth) == image_want).all(), f"{label}: depth|vis image"
        same(vis_t.cpu().numpy().view(np.uint32), vis_want, f"{label}: vis")
        same(depth_t.cpu().numpy(), depth_want, f"{label}: depth")
        if mesh_want is None:
            mesh_want = GP.decode_want_of(dctx, cpu)
        gbuffer_want = TD.decode(T, vis_want, depth_want, ipv, maps_want["normalmap"], maps_want["splatmap"], gpu.materials.cpu().numpy(), dctx.material_count, None, mesh_want)
        same(GP.decode_got_of(dctx), gbuffer_want, f"{label}: G-buffer")
        final = GP.pbr_got_of(pctx)
        same(final, GP.pbr_want_of(pctx), f"{label}: lit image")
        lit = np.stack(unpack_b10g11r11(final[ground]), axis=-1)
        assert np.isfinite(lit).all() and (lit.sum(-1) > 0).all(), f"{label}: {int((lit.sum(-1) <= 0).sum())} terrain pixels are black"

    def poison():
        for t in outputs:
            t.fill_(-5)

    chain()
    check("first eager run")
    s = r.debug_terrain_draw_stats()
    assert {k: s[k] for k in TM.STATS} == {k: counts[k] for k in TM.STATS}
    stream = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        chain(stream)
    for replay in range(2):
        poison()
        graph.replay()
        check(f"replay {replay}")
    for g in gs.values():
        g.check("chain")
