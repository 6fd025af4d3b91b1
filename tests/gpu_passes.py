"""The GPU-side plumbing the tests share: tensors between poisoned guard bands, the context / got_of / want_of / check of every per-pixel
pass under the pass's own name, one `same`, the shadow `Frame` and the 192 x 192 `DrawnFrame` of the library's own passes.  Imports torch
but touches no device until a helper is called; scenes, cameras and constants come from tests/scenes.py."""
import numpy as np
import torch

import ambient_occlusion_model as AM
import contact_shadows_model as CM
import eye_adaptation_model as EM
import pbr_apply_model as PM
import visbuffer_decode_model as VD
import vsm_resolve_model as RM
from pbr_apply_model import HAS_CONTACT_SHADOWS, HAS_DIRECTIONAL_LIGHT, HAS_SKY
from scenes import (AO_MAIN, CAMERA, CS_SUN, INV_PV, LIGHT, MAX_SHADOW_DIST, PBR_SUN, REFERENCE, SKY, SUN_INTENSITY, Z_LENGTH, camera_of, identity_camera, main_scene,
                    occluder_scene)

FILL_F32 = 0xC0A00000  # -5.0f: no pass writes a negative value
FILL_U32 = 0xFFFFFFFB  # -5, as the existing tests pre-fill; compared against the checker's image before it is trusted
FILL_U16 = 0xFFFB      # -5: a NaN half
DEVICE = "cuda"


def _signed(bits: int, size: int) -> int:
    return bits - (1 << (8 * size)) if bits >> (8 * size - 1) else bits


class Guard:
    """A tensor as a contiguous window in the middle of a larger 1-D buffer.  The band before it and the band after it hold `poison` and
    are each at least `row` + 64 elements long; the window starts at a multiple of `align` bytes that is not a multiple of 2 * `align`
    (the least the ABI demands).  `data` (numpy, same element size) fills an input window, `fill` pre-fills an output window with a pattern
    the pass does not write there."""

    def __init__(self, name, shape, dtype, row, poison, align, data=None, fill=None):
        size = torch.empty((), dtype=dtype).element_size()
        store, view = (torch.int16, np.int16) if size == 2 else (torch.int32, np.int32)
        per = align // size
        band = -(-(row + 64) // per) * per
        band += per if (band // per) % 2 == 0 else 0
        n = int(np.prod(shape))
        self.name, self.poison, self.fill, self.size, self.lo, self.hi = name, poison, fill, size, band, band + n
        self.buf = torch.full((band + n + band,), _signed(poison, size), dtype=store, device=DEVICE)
        window = self.buf[band:band + n]
        if data is not None:
            window.copy_(torch.from_numpy(np.ascontiguousarray(data).view(view).reshape(-1).copy()))
        else:
            window.fill_(_signed(fill, size))
        self.tensor = window.view(dtype).view(shape)
        assert self.tensor.data_ptr() % align == 0 and self.tensor.is_contiguous()

    def refill(self):
        self.buf[self.lo:self.hi].fill_(_signed(self.fill, self.size))

    def bits(self):
        """(band before, window, band after) as unsigned bit patterns."""
        a = self.buf.cpu().numpy().view(np.uint16 if self.size == 2 else np.uint32)
        return a[:self.lo], a[self.lo:self.hi], a[self.hi:]

    def check(self, label, want=None):
        """Both bands bit-identical to the poison (a NaN poison equals itself: patterns are compared, not values).  With `want`, the
        checker's image: no element of it equals the pre-fill pattern, so a window equal to `want` was overwritten everywhere."""
        before, _, after = self.bits()
        for side, band, base in (("before", before, -len(before)), ("after", after, self.hi - self.lo)):
            bad = np.flatnonzero(band != self.poison)
            assert bad.size == 0, (f"{label}: {self.name}: {bad.size} elements of the band {side} the image changed, the first at element "
                                   f"{int(bad[0]) + base} relative to the window's start (value 0x{int(band[bad[0]]):X})")
        if want is not None:
            assert not (np.ascontiguousarray(want).view(before.dtype) == self.fill).any(), f"{label}: {self.name}: the checker's image holds the pre-fill pattern"


def words_tensor(words) -> torch.Tensor:
    return torch.from_numpy(np.asarray(words, dtype=np.uint32).view(np.float32).copy()).cuda()


def lights_tensor(lights):
    from oxylus_amd.synth import pack_lights

    return pack_lights(lights).cuda() if lights else None


def upload(inp: dict) -> dict:
    """The numpy images of scenes.synthetic_inputs() as CUDA tensors in the dtypes the renderer takes."""
    t = lambda a, view: torch.from_numpy(np.ascontiguousarray(a).view(view).copy()).cuda()  # noqa: E731
    return dict(depth=t(inp["depth"], np.float32), albedo=t(inp["albedo"], np.int32), normal=t(inp["normal"], np.int16), emissive=t(inp["emissive"], np.int32),
                mro=t(inp["mro"], np.int32), ao=t(inp["ao"], np.int16), resolved=t(inp["resolved"], np.float32), contact=t(inp["contact"], np.float32))


def same(got, want, label=""):
    """got == want, bit for bit: two arrays (floats by their bit patterns), or dicts / lists / tuples of them, compared entry by entry."""
    at = f"{label}: " if label and not label.endswith(": ") else label
    if isinstance(got, dict):
        for k in got:
            same(got[k], want[k], f"{at}{k}")
        return
    if isinstance(got, (list, tuple)):
        assert len(got) == len(want), f"{at}{len(got)} entries != {len(want)}"
        for k, (g, w) in enumerate(zip(got, want)):
            same(g, w, f"{at}{k}")
        return
    bits = lambda a: a.view(f"u{a.dtype.itemsize}") if a.dtype.kind == "f" else a  # noqa: E731
    g, w = bits(np.asarray(got)), bits(np.asarray(want))
    assert g.shape == w.shape, f"{at}shape {g.shape} != {w.shape}"
    bad = np.argwhere(g != w)
    assert len(bad) == 0, (f"{at}{len(bad)} of {g.size} elements differ, the first at {bad[0].tolist()}: 0x{int(g[tuple(bad[0])]):X} != "
                           f"0x{int(w[tuple(bad[0])]):X}")


# ---- the main view's depth -------------------------------------------------------------------------------------------------------------------------
def drawn_depth(r, W, H, seed):
    """The main view's depth of scenes.occluder_scene, drawn by oxc_draw_visbuffer (the first steps of its Frame)."""
    from oxylus_amd import lib as L
    from oxylus_amd.renderer import CullGeometryContext, ImageAttachment, PreparedFrame

    cpu = occluder_scene(seed)
    gpu = cpu.to("cuda")
    r.reserve(gpu.n_mesh_instances, gpu.n_meshlet_instances)
    r.prepared_frame = PreparedFrame.create(gpu)
    main = CullGeometryContext(init_cull_meshes=False, cull_flags=L.CULL_TEST_ALL, cull_camera=gpu.cull_camera())
    r.seed_meshlet_instances(main, gpu.n_meshlet_instances)
    r.cull_geometry(main)
    pv = [float(x) for x in cpu.camera["projection_view"]]
    visdepth = torch.empty((H, W), dtype=torch.int64, device="cuda")
    depth = torch.zeros((H, W), dtype=torch.float32, device="cuda")
    r.draw_visbuffer(main, pv, W, H, visdepth, clear=True, depth=ImageAttachment.depth(depth))
    torch.cuda.synchronize()
    return cpu, depth


# ---- contact shadows -------------------------------------------------------------------------------------------------------------------------------
def contact_context(depth, camera, sun=CS_SUN, **kw):
    from oxylus_amd.renderer import ContactShadowsContext

    inv, view, proj, near = camera
    return ContactShadowsContext.create(depth, inv, view, proj, near, sun, **kw)


def contact_got_of(ctx):
    torch.cuda.synchronize()
    a = ctx.contact_shadows_attachment
    return a.data.view(a.height, a.width).cpu().numpy().copy()


def contact_want_of(ctx, stats=None):
    d = ctx.depth_attachment
    return CM.contact_shadows(d.data.view(d.height, d.width).cpu().numpy(), ctx.inv_projection_view, ctx.view, ctx.projection, ctx.near_clip, ctx.sun_dir,
                              ctx.steps, ctx.thickness, ctx.shadow_length, stats=stats)


def contact_check(ctx, stats=None):
    got, want = contact_got_of(ctx), contact_want_of(ctx, stats)
    bad = int((got.view(np.uint32) != want.view(np.uint32)).sum())
    assert bad == 0, f"{bad} of {got.size} pixels differ"
    return got


# ---- ambient occlusion -----------------------------------------------------------------------------------------------------------------------------
def hilbert_gpu():
    from oxylus_amd.synth import hilbert_noise_lut

    return hilbert_noise_lut().cuda()


def ao_context(depth, normal, view, proj, far, **kw):
    from oxylus_amd.renderer import AmbientOcclusionContext

    return AmbientOcclusionContext.create(depth, normal, hilbert_gpu(), view, proj, far, **kw)


def ao_got_of(ctx) -> dict:
    torch.cuda.synchronize()
    u16 = lambda t: t.cpu().numpy().view(np.uint16).copy()  # noqa: E731
    return {"levels": [ctx.prefiltered_depth.level(k).cpu().numpy().copy() for k in range(5)],
            "depth_differences": ctx.depth_differences.cpu().numpy().view(np.uint32).copy(), "noisy_occlusion": u16(ctx.noisy_occlusion),
            "ambient_occlusion": u16(ctx.ambient_occlusion_attachment)}


def ao_want_of(ctx, stats=None) -> dict:
    d = ctx.depth_attachment
    return AM.generate(d.data.view(d.height, d.width).cpu().numpy(), ctx.normal_attachment.cpu().numpy(), ctx.hilbert_noise.cpu().numpy().view(np.uint16),
                       ctx.view, ctx.projection, ctx.resolution, ctx.far_clip, ctx.thickness, ctx.slice_count, ctx.samples_per_slice_side,
                       ctx.effect_radius, ctx.noise_index, ctx.final_power, stats=stats)


def ao_check(ctx, stats=None) -> dict:
    got = ao_got_of(ctx)
    same(got, ao_want_of(ctx, stats))
    return got


# ---- visbuffer decode ------------------------------------------------------------------------------------------------------------------------------
def decode_context(gpu, vis, depth, pv, **kw):
    from oxylus_amd.renderer import VisbufferDecodeContext

    return VisbufferDecodeContext.create(vis, depth, pv, gpu.n_meshlet_instances, gpu.materials, **kw)


def decode_got_of(ctx) -> dict:
    torch.cuda.synchronize()
    u32 = lambda t: t.cpu().numpy().view(np.uint32).copy()  # noqa: E731
    return {"albedo": u32(ctx.albedo_attachment), "normal": ctx.normal_attachment.cpu().numpy().view(np.uint16).copy(), "emissive": u32(ctx.emissive_attachment),
            "mro": u32(ctx.metallic_roughness_occlusion_attachment)}


def decode_want_of(ctx, cpu, stats=None, init=None) -> dict:
    d = ctx.depth_attachment
    m = ctx.materials_buffer
    return VD.decode(cpu, cpu.meshlet_instances, ctx.visbuffer_attachment.cpu().numpy(), d.data.view(d.height, d.width).cpu().numpy(), ctx.projection_view,
                     None if m is None else m.cpu().numpy(), ctx.material_count, ctx.meshlet_instance_count, clear=ctx.clear, init=init, stats=stats)


def decode_check(ctx, cpu, stats=None, init=None, label=""):
    got = decode_got_of(ctx)
    same(got, decode_want_of(ctx, cpu, stats, init), label)
    return got


# ---- apply_pbr -------------------------------------------------------------------------------------------------------------------------------------
ALL_FLAGS = HAS_DIRECTIONAL_LIGHT | HAS_CONTACT_SHADOWS | HAS_SKY


def pbr_context(dev: dict, flags: int, lights=None, **kw):
    from oxylus_amd.renderer import PBRContext

    kw = {**dict(inv_projection_view=INV_PV, camera_position=CAMERA, sun_dir=PBR_SUN, sun_intensity=SUN_INTENSITY, **SKY), **kw}
    return PBRContext.create(dev["depth"], dev["albedo"], dev["normal"], dev["emissive"], dev["mro"], dev["ao"], dev["resolved"], dev["contact"], flags,
                             lights=lights, **kw)


def pbr_got_of(ctx) -> np.ndarray:
    torch.cuda.synchronize()
    a = ctx.final_attachment.cpu().numpy()
    return a.view(np.uint16 if a.dtype == np.int16 else np.uint32).copy()


def pbr_want_of(ctx, stats=None) -> np.ndarray:
    d = ctx.depth_attachment
    img = lambda a: None if a is None else a.data.view(d.height, d.width).cpu().numpy()  # noqa: E731
    lights = None if ctx.lights_buffer is None else ctx.lights_buffer.cpu().numpy()
    return PM.apply_pbr(img(d), ctx.albedo_attachment.cpu().numpy(), ctx.normal_attachment.cpu().numpy(), ctx.emissive_attachment.cpu().numpy(),
                        ctx.metallic_roughness_occlusion_attachment.cpu().numpy(), ctx.ambient_occlusion_attachment.cpu().numpy(),
                        img(ctx.resolved_shadows_attachment) if ctx.scene_flags & HAS_DIRECTIONAL_LIGHT else None,
                        img(ctx.contact_shadows_attachment) if ctx.scene_flags & HAS_CONTACT_SHADOWS else None, ctx.scene_flags, ctx.inv_projection_view,
                        ctx.camera_position, ctx.sun_dir, ctx.sun_intensity, lights, ctx.light_count, ctx.base_ambient_color, ctx.sky_solid_color,
                        ctx.sky_ambient_color, ctx.sky_has_texture, stats=stats)


# ---- eye adaptation --------------------------------------------------------------------------------------------------------------------------------
ONE_ONE = np.array([0x3F800000, 0x3F800000], dtype=np.uint32)
EYE_DEFAULTS = dict(min_exposure=-6.0, max_exposure=18.0, ev100_bias=1.0)
EYE_COMPONENT = dict(min_exposure=-11.5, max_exposure=18.0, ev100_bias=1.0)


def eye_context(image_t, exposure_t, time_coeff=1.0, settings=EYE_DEFAULTS):
    from oxylus_amd.renderer import EyeAdaptationContext

    ctx = EyeAdaptationContext.create(image_t, exposure_t, time_coeff=time_coeff, **settings)
    ctx.histogram_buffer.fill_(-5)
    return ctx


def eye_want_of(ctx, exposure_words):
    image = ctx.final_attachment.cpu().numpy()
    return EM.apply_eye_adaptation(image, ctx.source_format, exposure_words, ctx.min_exposure, ctx.max_exposure, ctx.ev100_bias, ctx.time_coeff)


# ---- the shadow frame ------------------------------------------------------------------------------------------------------------------------------
class Frame:
    """The compute-only shadow frame of tests/test_gpu_vsm_draw.py with the resolve at its end.  `evict`: before the resolve a third of
    the page-table entries, chosen by (7 x + 13 y + layer) % 3 == 0, lose their Backed bit, as pages evicted since the draw.  In a frame
    straight from the update every pixel's own page is backed and the fallback clipmaps are hardly ever asked; with evicted pages the
    taps near a clipmap boundary are served by the neighbouring clipmaps and the others miss.  `scene`: the CPU scene drawn,
    occluder_scene(seed) by default."""

    def __init__(self, r, W, H, shape=REFERENCE, seed=61, evict=False, first_clipmap_width=10.0, scene=None):
        from oxylus_amd import lib as L
        from oxylus_amd.renderer import CullGeometryContext, ImageAttachment, PreparedFrame, ShadowResolveContext, VirtualShadowmapContext, VsmDrawContext
        from oxylus_amd.synth import normals_from_depth, pack_clipmaps, virtual_shadow_matrices

        self.r, self.W, self.H, self.shape, self.L, self.evict = r, W, H, shape, L, evict
        self.fcw = first_clipmap_width
        count, n = shape["clipmap_count"], shape["page_table_size"]
        cpu = occluder_scene(seed) if scene is None else scene
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


# ---- the drawn frame -------------------------------------------------------------------------------------------------------------------------------
class DrawnFrame:
    """The 192 x 192 frame of scenes.main_scene(66): draw -> decode -> resolve -> contact shadows -> ambient occlusion,
    every context kept, `passes(stream)` runs the five producers."""

    def __init__(self, renderer):
        from oxylus_amd import lib as L
        from oxylus_amd.renderer import CullGeometryContext, ImageAttachment, PreparedFrame

        self.r, self.W, self.H = renderer, 192, 192
        W, H = self.W, self.H
        self.cpu = cpu = main_scene(66)[0]
        self.f = f = Frame(renderer, W, H, seed=66, scene=cpu)
        f.shadow_path()  # eager; every scratch grows here
        gpu = f.gpu
        self.frame = PreparedFrame.create(gpu)
        renderer.prepared_frame = self.frame
        self.main = CullGeometryContext(init_cull_meshes=False, cull_flags=L.CULL_TEST_ALL, cull_camera=gpu.cull_camera())
        renderer.seed_meshlet_instances(self.main, gpu.n_meshlet_instances)
        renderer.cull_geometry(self.main)
        self.pv = cpu.camera["projection_view"]
        self.visdepth = torch.empty((H, W), dtype=torch.int64, device="cuda")
        self.vis = torch.zeros((H, W), dtype=torch.int32, device="cuda")
        self.dctx = decode_context(gpu, self.vis, f.depth, self.pv)
        f.rctx.normal_attachment = self.dctx.normal_attachment
        self.cctx = contact_context(f.depth, identity_camera(gpu), steps=8, thickness=0.3, shadow_length=0.3)
        _, view, proj, far = camera_of(gpu)
        self.actx = ao_context(f.depth, self.dctx.normal_attachment, view, proj, far, **AO_MAIN)
        self.sun = tuple(float(v) for v in LIGHT)
        self.depth_image = ImageAttachment.depth(f.depth)

    def passes(self, stream=None):
        r, f = self.r, self.f
        r.prepared_frame = self.frame
        r.draw_visbuffer(self.main, self.pv, self.W, self.H, self.visdepth, clear=True, depth=self.depth_image, visbuffer=self.vis, stream=stream)
        r.decode_visbuffer(self.dctx, stream=stream)
        r.resolve_shadowmap(f.rctx, stream=stream)
        r.contact_shadows(self.cctx, stream=stream)
        r.generate_ambient_occlusion(self.actx, stream=stream)

    def pbr(self, flags, lights):
        from oxylus_amd.renderer import PBRContext

        d, f = self.dctx, self.f
        return PBRContext.create(f.depth, d.albedo_attachment, d.normal_attachment, d.emissive_attachment, d.metallic_roughness_occlusion_attachment,
                                 self.actx.ambient_occlusion_attachment, f.rctx.resolved_shadows_attachment, self.cctx.contact_shadows_attachment, flags,
                                 f.inv, self.cpu.camera["position"], self.sun, 3.0, lights=lights, sky_solid_color=(0.25, 0.5, 1.0, 1.0),
                                 sky_ambient_color=(0.1, 0.15, 0.2))

    def four_lights(self, shift=0.0):
        """A point light with a cutoff that leaves part of the frame at win == 0, a point light with range == 0, a spot light whose cone edge
        crosses the frame, and a record of kind Directional -- placed from the world positions the checker finds behind the lit pixels."""
        st = {}
        pbr_want_of(self.pbr(ALL_FLAGS, None), st)
        lit = st["lit"] & (self.f.depth.cpu().numpy()[st["ys"], st["xs"]] != 0)
        world = np.stack([w[lit] for w in st["world"]], axis=-1).astype(np.float64)
        cam = np.asarray(self.cpu.camera["position"], dtype=np.float64)
        centre = np.median(world, axis=0)
        near = centre + 0.25 * (cam - centre) + shift
        reach = float(np.median(np.linalg.norm(world - near, axis=-1)))
        to_centre = centre - cam
        return [dict(kind=1, position=tuple(near), range=reach, color=(1.0, 0.8, 0.6), intensity=40.0),
                dict(kind=1, position=tuple(cam + 0.1 + shift), range=0.0, color=(0.2, 0.4, 1.0), intensity=15.0),
                dict(kind=2, position=tuple(cam + shift), direction=tuple(to_centre), inner_cone_angle=0.06, outer_cone_angle=0.14, range=0.0, color=(1.0, 1.0, 1.0),
                     intensity=60.0),
                dict(kind=0, position=tuple(centre), range=0.0, color=(9.0, 9.0, 9.0), intensity=1000.0)]
