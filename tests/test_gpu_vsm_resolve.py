"""oxc_resolve_shadowmap on the GPU: the resolved image byte-identical to tests/vsm_resolve_model.py, every pixel -- the compute-only frame
depth -> page table -> HPB -> shadow cull -> shadow draw -> resolve at the reference's shape and at a second one, a frame after
invalidation, an allocation-failure frame, an all-sky image, non-finite texels, graph capture of the whole shadow path, and invalid
arguments."""
import numpy as np
import pytest
import torch

import vsm_draw_model as DM
import vsm_resolve_model as RM

pytestmark = pytest.mark.gpu

LIGHT = np.array([0.35, 0.8, 0.5]) / np.linalg.norm([0.35, 0.8, 0.5])  # towards the light: above and behind the camera's right shoulder
MAX_SHADOW_DIST = 500.0
Z_LENGTH = 4000.0  # four times the clipmaps' depth range (the reference: max_shadow_dist * 2): a four times wider light, penumbrae of several texels
REFERENCE = dict(page_size=128, page_table_size=64, physical_page_table_size=8192, clipmap_count=10)


def occluder_scene(seed):
    """A floor at y = -2 below a camera at the origin that looks down -z, and 40 horizontal quads of 2..6 units floating 2..12 units above
    it: lit floor, umbra, penumbra bands and sky in one view.  Every surface is drawn with both windings (the main view culls back
    faces).  Integer coordinates: exact in the mesh's binary16 positions."""
    rng = np.random.default_rng(seed)
    tris = []

    def quad(x0, x1, z0, z1, y):
        a, b, c, d = (x0, y, z0), (x1, y, z0), (x1, y, z1), (x0, y, z1)
        tris.extend([[a, b, c], [a, c, d], [a, c, b], [a, d, c]])

    quad(-24, 24, -4, -64, -2)
    for _ in range(40):
        cx, cz, y = int(rng.integers(-14, 15)), int(rng.integers(-40, -7)), int(rng.integers(0, 11))
        w, d = int(rng.integers(1, 4)), int(rng.integers(1, 4))
        quad(cx - w, cx + w, cz - d, cz + d, y)
    return DM.flat_scene([[tuple(float(v) for v in p) for p in t] for t in tris])[0]


class Frame:
    """The compute-only shadow frame of tests/test_gpu_vsm_draw.py with the resolve at its end.  `evict`: before the resolve a third of
    the page-table entries, chosen by (7 x + 13 y + layer) % 3 == 0, lose their Backed bit, as pages evicted since the draw.  In a frame
    straight from the update every pixel's own page is backed and the fallback clipmaps are hardly ever asked; with evicted pages the
    taps near a clipmap boundary are served by the neighbouring clipmaps and the others miss."""

    def __init__(self, r, W, H, shape=REFERENCE, seed=61, evict=False, first_clipmap_width=10.0):
        from oxylus_amd import lib as L
        from oxylus_amd.renderer import CullGeometryContext, ImageAttachment, PreparedFrame, ShadowResolveContext, VirtualShadowmapContext, VsmDrawContext
        from oxylus_amd.synth import normals_from_depth, pack_clipmaps, virtual_shadow_matrices

        self.r, self.W, self.H, self.shape, self.L, self.evict = r, W, H, shape, L, evict
        self.fcw = first_clipmap_width
        count, n = shape["clipmap_count"], shape["page_table_size"]
        cpu = occluder_scene(seed)
        self.gpu = gpu = cpu.to("cuda")
        r.reserve(gpu.n_mesh_instances, gpu.n_meshlet_instances)
        r.prepared_frame = PreparedFrame.create(gpu)
        main = CullGeometryContext(init_cull_meshes=False, cull_flags=L.CULL_TEST_ALL, cull_camera=gpu.cull_camera())
        r.seed_meshlet_instances(main, gpu.n_meshlet_instances)
        r.cull_geometry(main)
        pv = [float(x) for x in cpu.camera["projection_view"]]
        visdepth = torch.empty((H, W), dtype=torch.int64, device="cuda")
        self.depth = torch.zeros((H, W), dtype=torch.float32, device="cuda")
        r.draw_visbuffer(main, pv, W, H, visdepth, clear=True, depth=ImageAttachment.depth(self.depth))
        torch.cuda.synchronize()
        self.inv = np.linalg.inv(np.asarray(pv, np.float64).reshape(4, 4).T).T.reshape(-1).astype(np.float32)
        mats, offs, zn = virtual_shadow_matrices(list(cpu.camera["position"]), LIGHT, MAX_SHADOW_DIST, first_clipmap_width, count, page_table_size=n)
        self.clip = pack_clipmaps(mats, offs, zn)
        self.vctx = VirtualShadowmapContext.create(self.depth, self.inv, (W, H), self.clip, with_physical=True, first_clipmap_width=first_clipmap_width,
                                                   virtual_extent=float(n * shape["page_size"]), **shape)
        cam = gpu.cull_camera()
        for i in range(16):
            cam.projection_view[i] = float(mats[count - 1][i])
        for i in range(3):
            cam.position[i] = float(-LIGHT[i])
        cam.near_clip = zn
        self.sframe = PreparedFrame.create(gpu, expand=False)
        self.sctx = CullGeometryContext(use_hpb=True, init_cull_meshes=True, cull_flags=L.CULL_TEST_FRUSTUM, cull_camera=cam, hpb_attachment=self.vctx.hpb_attachment,
                                        vsm_clipmaps_buffer=self.vctx.vsm_clipmaps_buffer, vsm_clipmap_dirty_flags_buffer=self.vctx.vsm_clipmap_dirty_flags_buffer,
                                        vsm_clipmap_count=count)
        self.dctx = VsmDrawContext.create(self.vctx, self.sctx)
        self.normal = normals_from_depth(self.depth, self.inv, cpu.camera["position"])
        self.rctx = ShadowResolveContext.create(self.vctx, self.normal, LIGHT, Z_LENGTH)
        c, y, x = np.mgrid[0:count, 0:n, 0:n]
        self.keep = torch.from_numpy(np.where((7 * x + 13 * y + c) % 3 == 0, ~np.int32(4), np.int32(-1)).astype(np.int32)).cuda()

    def shadow_path(self, stream=None):
        r = self.r
        r.update_virtual_shadowmap(self.vctx, stream=stream)
        r.prepared_frame = self.sframe
        r.cull_geometry(self.sctx, stream=stream)
        r.draw_physical_pages(self.dctx, stream=stream)
        if self.evict:
            self.vctx.virtual_page_table &= self.keep
        r.resolve_shadowmap(self.rctx, stream=stream)

    def got(self):
        torch.cuda.synchronize()
        return self.rctx.resolved_shadows_attachment.data.view(self.H, self.W).cpu().numpy().copy()

    def want(self, stats=None):
        phys = self.shape["physical_page_table_size"]
        return RM.resolve(self.rctx.depth_attachment.data.view(self.H, self.W).cpu().numpy(), self.rctx.normal_attachment.cpu().numpy(),
                          self.vctx.virtual_page_table.cpu().numpy(), self.clip.numpy(), self.vctx.physical_page_image.data.view(phys, phys).cpu().numpy(),
                          self.inv, (self.W, self.H), LIGHT, Z_LENGTH, first_clipmap_width=self.fcw, bias=self.vctx.clipmap_selection_bias,
                          virtual_extent=self.vctx.virtual_extent, stats=stats, **self.shape)

    def check(self, stats=None):
        got, want = self.got(), self.want(stats)
        bad = int((got.view(np.uint32) != want.view(np.uint32)).sum())
        assert bad == 0, f"{bad} of {got.size} pixels differ"
        return got


def _outcomes(st):
    oc = st["outcome"]
    return {name: int((oc == k).sum()) for name, k in (("sky", RM.SKY), ("hard", RM.HARD), ("no_blocker", RM.NO_BLOCKER), ("all_blockers", RM.ALL_BLOCKERS))}


def test_frame_at_the_reference_shape(renderer):
    """768 x 768, page 128, table 64, physical 8192, 10 clipmaps, a third of the pages evicted before the resolve.  The fixture is not
    degenerate: asserted through the checker, each of sky / hard-shadow / "no blocker" / "all blockers" / PCF ratio strictly inside (0, 1)
    holds at least 1000 pixels and each fallback clipmap serves at least 1000 taps.  Counts reached (first tried with the checker alone
    on the CPU models' frame, then on the device's): sky 267 518, hard 58 624, no blocker 32 398, all blockers 36 570, PCF inside (0, 1)
    2 289; 10 414 106 taps, 1 542 836 missed, 311 095 served by base - 1, 810 523 by base + 1.  The device's own counters agree with the checker's."""
    f = Frame(renderer, 768, 768, evict=True)
    L = f.L
    renderer.debug_set_tuning(L.TUNE_VSM_RESOLVE_STATS, 1)
    try:
        f.shadow_path()
        st = {}
        got = f.check(st)
        dev = renderer.debug_vsm_resolve_stats()
    finally:
        renderer.debug_set_tuning(L.TUNE_VSM_RESOLVE_STATS, 0)
    counts = _outcomes(st)
    counts["pcf_inside"] = int(((st["outcome"] == RM.PCF) & (got > 0.0) & (got < 1.0)).sum())
    print("outcomes", counts, "taps", st["taps"], "misses", st["misses"], "fallback_minus", st["fallback_minus"], "fallback_plus", st["fallback_plus"])
    print("device", dev)
    for name, v in counts.items():
        assert v >= 1000, (name, counts)
    assert st["fallback_minus"] >= 1000 and st["fallback_plus"] >= 1000, st
    assert dev == {"non_sky_pixels": got.size - counts["sky"], "taps": st["taps"], "misses": st["misses"], "fallback_minus": st["fallback_minus"],
                   "fallback_plus": st["fallback_plus"], "hard": counts["hard"], "no_blocker": counts["no_blocker"], "all_blockers": counts["all_blockers"]}
    f.r.resolve_shadowmap(f.rctx)  # the plain instantiation writes the same image
    f.check()


def test_second_shape_odd_resolution(renderer):
    shape = dict(page_size=64, page_table_size=32, physical_page_table_size=4096, clipmap_count=6)  # V = 2048 != physical
    f = Frame(renderer, 1277, 719, shape=shape, seed=62, first_clipmap_width=12.0)
    f.shadow_path()
    got = f.check()
    assert ((got > 0) & (got < 1)).any() and (got == 0).any() and (got == 1).any()


def test_frame_after_invalidation(renderer):
    f = Frame(renderer, 384, 384, seed=63)
    f.shadow_path()
    f.check()
    ids = torch.zeros(1, dtype=torch.int32, device="cuda")  # the scene's one mesh instance
    v, s = f.vctx, f.gpu
    v.dirty_mesh_instance_indices = ids
    v.mesh_instances_buffer, v.meshes_buffer = s.mesh_instances, s.meshes
    v.transforms_world_buffer = v.transforms_previous_buffer = s.transforms
    f.shadow_path()
    assert int(v.counters_buffer.cpu()[1]) > 0  # pages were invalidated, requested again and redrawn
    f.check()


def test_allocation_failure_frame(renderer):
    """64 physical pages for a frame that asks for more: the pages that got none stay Visible and unbacked, and their taps miss."""
    shape = dict(page_size=128, page_table_size=64, physical_page_table_size=1024, clipmap_count=10)
    f = Frame(renderer, 384, 384, shape=shape, seed=64)
    f.shadow_path()
    st = {}
    f.check(st)
    assert int(f.vctx.counters_buffer.cpu()[4]) > 0 and st["misses"] > 0


def test_all_sky_and_non_finite_texels(renderer):
    f = Frame(renderer, 256, 256, seed=65)
    f.shadow_path()
    f.check()
    # non-finite depth and normal texels: the device and the checker agree on every NaN rule
    ys, xs = np.nonzero(f.depth.cpu().numpy() != 0)
    assert len(xs) > 100
    d, nrm = f.depth, f.normal
    for k, value in enumerate((float("nan"), float("inf"), -float("inf"), -0.0, 1e-30, 3e38)):
        d[int(ys[k * 7]), int(xs[k * 7])] = value
    for k, bits in enumerate((0x7E00, 0x7C00, -1024, 0x0001, -32768)):  # NaN, +inf, -inf, a denormal, -0.0 halves
        nrm[int(ys[50 + k * 5]), int(xs[50 + k * 5]), 2] = bits
        nrm[int(ys[80 + k * 5]), int(xs[80 + k * 5]), 3] = bits
    f.r.resolve_shadowmap(f.rctx)
    f.check()
    d.zero_()
    f.rctx.resolved_shadows_attachment.data.fill_(-5.0)
    f.r.resolve_shadowmap(f.rctx)
    assert (f.got() == 1.0).all()


def test_shadow_path_is_capturable_into_a_graph(renderer):
    f = Frame(renderer, 320, 320, seed=66)
    f.shadow_path()  # eager; every scratch grows here
    eager = f.check()
    assert ((eager > 0) & (eager < 1)).any()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        f.shadow_path(stream=s)
    f.vctx.virtual_page_table.zero_()
    f.vctx.physical_page_image.data.zero_()
    for _ in range(2):  # the first replay is the first frame again, the second a steady one: the same shadow term
        f.rctx.resolved_shadows_attachment.data.fill_(-5.0)
        torch.cuda.synchronize()
        g.replay()
        assert np.array_equal(f.got().view(np.uint32), eager.view(np.uint32))
    f.check()


def test_invalid_arguments(renderer):
    from oxylus_amd import lib as L
    from oxylus_amd.renderer import ImageAttachment

    f = Frame(renderer, 128, 128, seed=67)
    f.shadow_path()
    torch.cuda.synchronize()
    ctx = f.rctx

    def bad(**kw):
        saved = {k: getattr(ctx, k) for k in kw}
        for k, v in kw.items():
            setattr(ctx, k, v)
        with pytest.raises(L.OxcError) as e:
            renderer.resolve_shadowmap(ctx)
        assert e.value.status == L.OXC_INVALID_ARG
        for k, v in saved.items():
            setattr(ctx, k, v)

    bad(page_size=8)
    bad(page_size=24)
    bad(page_table_size=12)
    bad(page_table_size=264)
    bad(clipmap_count=0)
    bad(clipmap_count=17)
    bad(physical_page_table_size=64)                         # not a multiple of the page, and not the image's extent
    bad(page_size=16, physical_page_table_size=8192)         # 512 x 512 physical pages: beyond 16 address bits
    bad(physical_page_table_size=4096)                       # the image is 8192 square
    bad(resolved_shadows_attachment=ImageAttachment.depth(torch.zeros((128, 64), dtype=torch.float32, device="cuda")))
    bad(normal_attachment=torch.zeros((64, 128, 4), dtype=torch.int16, device="cuda"))
    bad(virtual_page_table=torch.zeros((9, 64, 64), dtype=torch.int32, device="cuda"))
    bad(vsm_clipmaps_buffer=torch.zeros(9 * 76, dtype=torch.uint8, device="cuda"))
    c = ctx.c()
    c.struct_size = 4
    assert renderer._lib.oxc_resolve_shadowmap(renderer._ctx, c, renderer._stream(None)) == L.OXC_INVALID_ARG
    renderer.resolve_shadowmap(ctx)  # and the context still resolves
    f.check()
