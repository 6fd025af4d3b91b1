"""Host-side mirror of the reference's RendererInstance over the C ABI: the passes of a frame from the cull to the anti-aliased,
tonemapped image, and the producers around them.

Same names and field meaning as Oxylus/include/Render/RendererInstance.hpp.  The module holds the image types (ImageAttachment,
HpbAttachment, BloomPyramid), PreparedFrame, one dataclass per oxc_*_context of include/oxcull.h (CullGeometryContext, the virtual
shadowmap's three, the per-pixel passes', the post-process passes', the two sky contexts) and `RendererInstance`, whose methods are the
entry points.  Buffers are torch CUDA tensors (device memory + streams only; all compute is in liboxcull.so).  The compiled C++ shim with
the same surface is oxylus_amd/host/RendererInstance.hpp; this Python twin exists because the test runner and bench driver are Python.

Marshalling (_marshal.py): a context's `.c()` fills its L.<Structure> by walking the structure's `_fields_`.  A C field takes the
dataclass field of the same name, converted by the C type (tensor -> oxc_buffer, image -> its own .c(), sequence -> array, bool / int ->
u32, number -> float); the class states only the exceptions, `_derived` (C field -> another attribute's path, or a function of the context)
and `_leave` (padding and what the library writes back).  A C field that none of the three accounts for is a TypeError when the class is
created.
"""
from __future__ import annotations

import ctypes as C
import math
import struct
from dataclasses import dataclass, field
from typing import Optional

import torch

from . import lib as L
from ._marshal import Marshalled, _buf
from .synth import Scene, hiz_layout


@dataclass
class ImageAttachment:
    """Linear R32F mip chain (stand-in for vuk::ImageAttachment)."""
    data: torch.Tensor  # float32 1-D
    width: int
    height: int
    levels: int
    level_offset: list  # bytes

    @staticmethod
    def hiz(width: int, height: int, device, levels: Optional[int] = None) -> "ImageAttachment":
        levels, offs, total = hiz_layout(width, height, levels)
        # vuk::clear_image(hiz, DepthZero), RendererInstance.cpp:588
        return ImageAttachment(torch.zeros(total // 4, dtype=torch.float32, device=device), width, height, levels, offs)

    @staticmethod
    def depth(t: torch.Tensor) -> "ImageAttachment":
        assert t.dtype == torch.float32 and t.dim() == 2 and t.is_contiguous()
        return ImageAttachment(t.view(-1), t.shape[1], t.shape[0], 1, [0])

    def level(self, k: int) -> torch.Tensor:
        w, h = max(1, self.width >> k), max(1, self.height >> k)
        o = self.level_offset[k] // 4
        return self.data[o:o + w * h].view(h, w)

    def c(self) -> L.Image:
        im = L.Image()
        im.dptr = self.data.data_ptr()
        im.width, im.height, im.levels = self.width, self.height, self.levels
        for k, o in enumerate(self.level_offset):
            im.level_offset[k] = o
        return im


@dataclass
class HpbAttachment:
    """R8UI Texture2DArray with mips (VSM hierarchical page buffer), linear layout."""
    data: torch.Tensor  # uint8 1-D
    width: int
    height: int
    layers: int
    levels: int
    level_offset: list  # bytes

    @staticmethod
    def create(width: int, height: int, layers: int, levels: int, device) -> "HpbAttachment":
        offs, off = [], 0
        for k in range(levels):
            offs.append(off)
            off += layers * max(1, width >> k) * max(1, height >> k)
            off = (off + 255) // 256 * 256
        return HpbAttachment(torch.zeros(off, dtype=torch.uint8, device=device), width, height, layers, levels, offs)

    def level(self, k: int) -> torch.Tensor:
        w, h = max(1, self.width >> k), max(1, self.height >> k)
        o = self.level_offset[k]
        return self.data[o:o + self.layers * w * h].view(self.layers, h, w)

    def build_mips(self):
        """Any-bit pyramid from level 0 (what rmvsm_downsample_hpb produces: a texel is set if
        any of its 2x2 children is)."""
        for k in range(1, self.levels):
            p = self.level(k - 1)
            w, h = max(1, self.width >> k), max(1, self.height >> k)
            self.level(k).copy_(p.view(self.layers, h, 2, w, 2).amax(dim=(2, 4)) if p.shape[1] >= 2 and p.shape[2] >= 2 else p.amax(dim=(1, 2), keepdim=True))

    def c(self) -> L.ImageArrayU8:
        im = L.ImageArrayU8()
        im.dptr = self.data.data_ptr()
        im.width, im.height, im.layers, im.levels = self.width, self.height, self.layers, self.levels
        for k, o in enumerate(self.level_offset):
            im.level_offset[k] = o
        return im


@dataclass
class PreparedFrame(Marshalled):
    """The PreparedFrame buffers of the cull path (RendererInstance.hpp:143-169), sized as in
    RendererInstance::update (RendererInstance.cpp:1640-1732)."""
    _ctype = L.PreparedFrame
    _derived = {"mesh_instance_count": "scene.n_mesh_instances", "meshes_buffer": "scene.meshes", "transforms_world_buffer": "scene.transforms",
                "mesh_instances_buffer": "scene.mesh_instances"}
    scene: Scene
    max_meshlet_instance_count: int
    meshlet_instances_buffer: torch.Tensor
    visible_meshlet_instances_indices_buffer: torch.Tensor
    meshlet_instance_visibility_mask_buffer: torch.Tensor
    reordered_indices_buffer: Optional[torch.Tensor]

    @staticmethod
    def create(scene: Scene, with_triangles: bool = True, expand: bool = True, max_tris: int = 64, index_words: int = 1) -> "PreparedFrame":
        """max_tris = 128 for wide_triangle_index != 0; index_words = 2 for wide_triangle_index = 2 ({id, corner} pairs, 8 bytes per index)."""
        dev = scene.device
        n = scene.n_meshlet_instances
        mli = scene.meshlet_instances.clone() if expand else torch.zeros((n, 2), dtype=torch.int32, device=dev)
        vis_idx = torch.zeros(max(n, 1), dtype=torch.int32, device=dev)
        # zero-filled on (re)upload of the instances, RendererInstance.cpp:1651-1665
        mask = torch.zeros(max((n + 31) // 32, 1), dtype=torch.int32, device=dev)
        reordered = torch.zeros(max(n, 1) * max_tris * 3 * index_words, dtype=torch.int32, device=dev) if with_triangles else None
        return PreparedFrame(scene, n, mli, vis_idx, mask, reordered)


@dataclass
class CullGeometryContext(Marshalled):
    """RendererInstance.hpp:171-197.  `.c()` fills and returns the persistent `_c`: the library writes the call's output buffers into it, and
    read_counters, draw_visbuffer and VsmDrawContext read them there."""
    _ctype = L.CullGeometryContext
    _leave = ("_reserved1", "visibility_buffer", "cull_meshlets_cmd_buffer", "cull_triangles_cmd_buffer", "draw_geometry_cmd_buffer")
    use_hiz: bool = False
    use_hpb: bool = False
    init_cull_meshes: bool = False
    cull_flags: int = L.CULL_TEST_ALL
    cull_camera: Optional[L.CullCamera] = None
    hiz_attachment: Optional[ImageAttachment] = None
    hpb_attachment: Optional[HpbAttachment] = None
    vsm_clipmaps_buffer: Optional[torch.Tensor] = None            # uint8 [V*76] GPU::VirtualClipmap records
    vsm_clipmap_dirty_flags_buffer: Optional[torch.Tensor] = None  # int32 [V]
    vsm_clipmap_count: int = 0
    wide_triangle_index: int = 0  # extension: 1 / True = (id << 9) | (3t+k), meshlets of up to 128 triangles, <= 2^23 ids; 2 = {id, corner} pairs, no id limit
    small_triangle_cull: bool = False  # extension (north star): also drop triangles whose screen bbox covers no pixel centre
    async_triangles: bool = False  # extension (scheduling only): the triangle stage runs on the context's own stream; RendererInstance.join_triangles
    share_pass_tests: bool = False  # extension (caching only): the late HiZ call of a frame reuses the early call's frustum + cone results (include/oxcull.h)
    unordered_output: int = 0  # extension (order only): 0 ascending lists, 1 the reference's atomic slot allocation where it is faster (include/oxcull.h)
    implicit_meshlet_instances: bool = False  # extension (multi-view batch only): the MeshletInstance list stays implicit, runs in meshlet_instance_runs_buffer
    meshlet_instance_runs_buffer: Optional[torch.Tensor] = None  # int32 [M, 2] {first, count} per mesh instance (out)
    stages: int = 0
    _c: L.CullGeometryContext = field(default_factory=L.CullGeometryContext)

    def c(self) -> L.CullGeometryContext:
        return self._fill(self._c)


@dataclass
class VirtualShadowmapContext(Marshalled):
    """oxc_vsm_update_context: the page-management part of RendererInstance::draw_virtual_shadowmap (Shadowmaps.cpp:143-421).
    Sizes default to the reference's configuration (RendererInstance.hpp:262-267); `create` allocates the outputs."""
    _ctype = L.VsmUpdateContext
    _derived = {"depth_extent": lambda s: (s.depth_attachment.width, s.depth_attachment.height),
                "dirty_mesh_instance_count": lambda s: 0 if s.dirty_mesh_instance_indices is None else s.dirty_mesh_instance_indices.numel()}
    virtual_page_table: torch.Tensor              # int32 [clipmap_count, n, n], persistent across frames
    vsm_clipmaps_buffer: torch.Tensor             # uint8 [clipmap_count * 76] GPU::VirtualClipmap records
    depth_attachment: ImageAttachment             # R32F, levels = 1: the main view's reversed-Z depth
    inv_projection_view: list                     # Camera::inv_projection_view, 16 floats column-major
    resolution: tuple                             # Camera::resolution
    vsm_clipmap_dirty_flags_buffer: torch.Tensor  # int32 [clipmap_count] out
    dirty_physical_pages_buffer: torch.Tensor     # int32 [min(pages, physical pages), 2] out
    clear_cmd_buffer: torch.Tensor                # int32 [3] out: VkDispatchIndirectCommand
    counters_buffer: torch.Tensor                 # int32 [8] out
    page_size: int = 128
    page_table_size: int = 64
    physical_page_table_size: int = 8192
    clipmap_count: int = 10
    first_clipmap_width: float = 10.0
    clipmap_selection_bias: float = -1.5
    virtual_extent: float = 8192.0
    sun_moved: bool = False
    dirty_mesh_instance_indices: Optional[torch.Tensor] = None  # int32 [k]; with the four scene buffers below (read when k > 0)
    mesh_instances_buffer: Optional[torch.Tensor] = None
    meshes_buffer: Optional[torch.Tensor] = None
    transforms_world_buffer: Optional[torch.Tensor] = None
    transforms_previous_buffer: Optional[torch.Tensor] = None   # float32 [M, 16] GPU::TransformPrevious
    hpb_attachment: Optional[HpbAttachment] = None              # optional out
    physical_page_image: Optional[ImageAttachment] = None       # optional out

    @staticmethod
    def create(depth: torch.Tensor, inv_projection_view, resolution, clipmaps: torch.Tensor, page_size: int = 128, page_table_size: int = 64,
               physical_page_table_size: int = 8192, clipmap_count: int = 10, with_hpb: bool = True, with_physical: bool = False,
               **kw) -> "VirtualShadowmapContext":
        dev = depth.device
        n, layers = page_table_size, clipmap_count
        phys_pages = (physical_page_table_size // page_size) ** 2
        hpb = None
        if with_hpb:
            hpb = HpbAttachment.create(n, n, layers, min(max(n.bit_length(), 1), 13), dev)
        phys = None
        if with_physical:
            phys = ImageAttachment.depth(torch.zeros((physical_page_table_size, physical_page_table_size), dtype=torch.float32, device=dev))
        return VirtualShadowmapContext(
            virtual_page_table=torch.zeros((layers, n, n), dtype=torch.int32, device=dev), vsm_clipmaps_buffer=torch.as_tensor(clipmaps).to(dev),
            depth_attachment=ImageAttachment.depth(depth), inv_projection_view=[float(x) for x in inv_projection_view],
            resolution=(float(resolution[0]), float(resolution[1])),
            vsm_clipmap_dirty_flags_buffer=torch.zeros(layers, dtype=torch.int32, device=dev),
            dirty_physical_pages_buffer=torch.zeros((max(min(layers * n * n, phys_pages), 1), 2), dtype=torch.int32, device=dev),
            clear_cmd_buffer=torch.zeros(3, dtype=torch.int32, device=dev), counters_buffer=torch.zeros(8, dtype=torch.int32, device=dev),
            page_size=page_size, page_table_size=n, physical_page_table_size=physical_page_table_size, clipmap_count=layers,
            hpb_attachment=hpb, physical_page_image=phys, **kw)


def _vsm_draw_cmd(s: "VsmDrawContext") -> L.Buffer:
    if s.draw_cmd is not None:
        return _buf(s.draw_cmd)
    return s.cull._c.draw_geometry_cmd_buffer if s.cull is not None else _buf(None)


@dataclass
class VsmDrawContext(Marshalled):
    """oxc_vsm_draw_context: the shadow draw of RendererInstance::draw_virtual_shadowmap (Shadowmaps.cpp:466-754).  `create` takes the shape and
    the page buffers from a VirtualShadowmapContext and the triangle list from the shadow CullGeometryContext (its draw_geometry_cmd_buffer,
    read when the draw is enqueued)."""
    _ctype = L.VsmDrawContext
    _derived = {"draw_geometry_cmd_buffer": _vsm_draw_cmd}
    virtual_page_table: torch.Tensor              # int32 [clipmap_count, n, n]
    vsm_clipmaps_buffer: torch.Tensor             # uint8 [clipmap_count * 76] GPU::VirtualClipmap records
    vsm_clipmap_dirty_flags_buffer: torch.Tensor  # int32 [clipmap_count]
    physical_page_image: ImageAttachment          # R32F, physical_page_table_size square (in/out)
    page_size: int = 128
    page_table_size: int = 64
    physical_page_table_size: int = 8192
    clipmap_count: int = 10
    wide_triangle_index: int = 0
    cull: Optional[CullGeometryContext] = None    # the use_hpb cull whose triangles are drawn
    draw_cmd: Optional[torch.Tensor] = None       # int32 [5] VkDrawIndexedIndirectCommand: replaces the cull's own command
    draw_commands_buffer: Optional[torch.Tensor] = None  # optional out: int32 [clipmap_count, 5]
    draw_count_buffer: Optional[torch.Tensor] = None     # optional out: int32 [1]
    draw_clipmaps_buffer: Optional[torch.Tensor] = None  # optional out: int32 [clipmap_count]

    @staticmethod
    def create(vsm: VirtualShadowmapContext, cull: Optional[CullGeometryContext] = None, physical_page_image: Optional[ImageAttachment] = None,
               with_commands: bool = False) -> "VsmDrawContext":
        img = physical_page_image if physical_page_image is not None else vsm.physical_page_image
        assert img is not None, "the draw needs a physical_page_image"
        k, dev = vsm.clipmap_count, vsm.virtual_page_table.device
        cmds = dict(draw_commands_buffer=torch.zeros((k, 5), dtype=torch.int32, device=dev), draw_count_buffer=torch.zeros(1, dtype=torch.int32, device=dev),
                    draw_clipmaps_buffer=torch.zeros(k, dtype=torch.int32, device=dev)) if with_commands else {}
        return VsmDrawContext(vsm.virtual_page_table, vsm.vsm_clipmaps_buffer, vsm.vsm_clipmap_dirty_flags_buffer, img, page_size=vsm.page_size,
                              page_table_size=vsm.page_table_size, physical_page_table_size=vsm.physical_page_table_size, clipmap_count=k,
                              wide_triangle_index=int(cull.wide_triangle_index) if cull is not None else 0, cull=cull, **cmds)


@dataclass
class ShadowResolveContext(Marshalled):
    """oxc_shadow_resolve_context: RendererInstance::resolve_shadowmap (Shadowmaps.cpp:756-822).  `create` takes the shape, the camera and the
    page buffers from a VirtualShadowmapContext and allocates the output."""
    _ctype = L.ShadowResolveContext
    depth_attachment: ImageAttachment             # R32F, levels = 1: the main view's reversed-Z depth
    normal_attachment: torch.Tensor               # int16 [H, W, 4]: R16G16B16A16Sfloat bits, .ba = the octahedral world normal
    vsm_clipmaps_buffer: torch.Tensor             # uint8 [clipmap_count * 76]
    virtual_page_table: torch.Tensor              # int32 [clipmap_count, n, n]
    physical_page_image: ImageAttachment          # R32F, physical_page_table_size square
    resolved_shadows_attachment: ImageAttachment  # R32F out, the extent of the depth image
    inv_projection_view: list
    resolution: tuple
    directional_light_dir: tuple
    z_length: float                               # max_shadow_dist * 2
    page_size: int = 128
    page_table_size: int = 64
    physical_page_table_size: int = 8192
    clipmap_count: int = 10
    first_clipmap_width: float = 10.0
    clipmap_selection_bias: float = -1.5
    virtual_extent: float = 8192.0

    @staticmethod
    def create(vsm: VirtualShadowmapContext, normal: torch.Tensor, light_dir, z_length: float,
               physical_page_image: Optional[ImageAttachment] = None) -> "ShadowResolveContext":
        img = physical_page_image if physical_page_image is not None else vsm.physical_page_image
        assert img is not None, "the resolve needs a physical_page_image"
        d = vsm.depth_attachment
        assert normal.dtype == torch.int16 and tuple(normal.shape) == (d.height, d.width, 4) and normal.is_contiguous()
        out = ImageAttachment.depth(torch.zeros((d.height, d.width), dtype=torch.float32, device=d.data.device))
        return ShadowResolveContext(d, normal, vsm.vsm_clipmaps_buffer, vsm.virtual_page_table, img, out, list(vsm.inv_projection_view), tuple(vsm.resolution),
                                    tuple(float(x) for x in light_dir), float(z_length), page_size=vsm.page_size, page_table_size=vsm.page_table_size,
                                    physical_page_table_size=vsm.physical_page_table_size, clipmap_count=vsm.clipmap_count,
                                    first_clipmap_width=vsm.first_clipmap_width, clipmap_selection_bias=vsm.clipmap_selection_bias,
                                    virtual_extent=vsm.virtual_extent)


@dataclass
class ContactShadowsContext(Marshalled):
    """oxc_contact_shadows_context: the contact_shadows pass of RendererInstance::render (RendererInstance.cpp:990-1020).  `create` takes the
    depth image and the camera and allocates the output; steps / thickness / shadow_length default to the engine's (RendererCVar.cpp:30-34)."""
    _ctype = L.ContactShadowsContext
    depth_attachment: ImageAttachment            # R32F, levels = 1: the main view's reversed-Z depth
    contact_shadows_attachment: ImageAttachment  # R32F out, the extent of the depth image
    inv_projection_view: list                    # column-major float[16], as view and projection
    view: list
    projection: list
    near_clip: float
    sun_dir: tuple                               # towards the sun; the pass normalises it
    steps: int = 8
    thickness: float = 0.1
    shadow_length: float = 0.01

    @staticmethod
    def create(depth, inv_projection_view, view, projection, near_clip: float, sun_dir, steps: int = 8, thickness: float = 0.1,
               shadow_length: float = 0.01) -> "ContactShadowsContext":
        d = depth if isinstance(depth, ImageAttachment) else ImageAttachment.depth(depth)
        out = ImageAttachment.depth(torch.zeros((d.height, d.width), dtype=torch.float32, device=d.data.device))
        return ContactShadowsContext(d, out, [float(x) for x in inv_projection_view], [float(x) for x in view], [float(x) for x in projection],
                                     float(near_clip), tuple(float(x) for x in sun_dir), int(steps), float(thickness), float(shadow_length))


@dataclass
class AmbientOcclusionContext(Marshalled):
    """oxc_ambient_occlusion_context: RendererInstance::generate_ambient_occlusion (Passes/PBR.cpp:179-311).  `create` takes the depth image,
    the normal image, the Hilbert table and the camera and allocates the three intermediates and the output; the settings default to
    GPU::VBGTAOSettings' (SceneGPU.hpp:286-293)."""
    _ctype = L.AmbientOcclusionContext
    depth_attachment: ImageAttachment         # R32F, levels = 1: the main view's reversed-Z depth
    normal_attachment: torch.Tensor           # int16 / uint16 [H, W, 4]
    hilbert_noise: torch.Tensor               # int16 / uint16 [64, 64]
    prefiltered_depth: ImageAttachment        # R32F out, 5 levels
    depth_differences: torch.Tensor           # int32 [H, W] out: the packed edges
    noisy_occlusion: torch.Tensor             # int16 [H, W] out: binary16 bits
    ambient_occlusion_attachment: torch.Tensor  # int16 [H, W] out: binary16 bits
    view: list                                # column-major float[16], as projection
    projection: list
    resolution: tuple
    far_clip: float
    thickness: float = 0.25
    slice_count: int = 3
    samples_per_slice_side: int = 3
    effect_radius: float = 0.5
    noise_index: int = 0
    final_power: float = 2.2

    @staticmethod
    def create(depth, normal, hilbert_noise, view, projection, far_clip: float, resolution=None, thickness: float = 0.25, slice_count: int = 3,
               samples_per_slice_side: int = 3, effect_radius: float = 0.5, noise_index: int = 0, final_power: float = 2.2) -> "AmbientOcclusionContext":
        d = depth if isinstance(depth, ImageAttachment) else ImageAttachment.depth(depth)
        dev = d.data.device
        pre = ImageAttachment.hiz(d.width, d.height, dev, levels=5)
        z16 = lambda: torch.zeros((d.height, d.width), dtype=torch.int16, device=dev)  # noqa: E731
        res = (float(d.width), float(d.height)) if resolution is None else (float(resolution[0]), float(resolution[1]))
        return AmbientOcclusionContext(d, normal, hilbert_noise, pre, torch.zeros((d.height, d.width), dtype=torch.int32, device=dev), z16(), z16(),
                                       [float(x) for x in view], [float(x) for x in projection], res, float(far_clip), float(thickness),
                                       int(slice_count), int(samples_per_slice_side), float(effect_radius), int(noise_index), float(final_power))


@dataclass
class PBRContext(Marshalled):
    """oxc_pbr_context: the no-atmosphere branch of RendererInstance::apply_pbr (Passes/PBR.cpp:313-534, pbr_apply_no_atmos).  `create` takes
    the depth image, the four G-buffer images of decode_visbuffer, the ambient occlusion and the two shadow terms as their producers wrote
    them, the camera, the sun, the lights (synth.pack_lights) and the Sky record, and allocates the output: int32 [H, W] (B10G11R11), or
    int16 [H, W, 4] (R16G16B16A16 Sfloat) with L.SCENE_TRANSPARENT_BACKGROUND.  An image whose flag is clear may be None."""
    _ctype = L.PbrContext
    _derived = {"width": "depth_attachment.width", "height": "depth_attachment.height"}
    depth_attachment: ImageAttachment             # R32F, levels = 1
    albedo_attachment: torch.Tensor               # int32 [H, W]: R8G8B8A8 sRGB
    normal_attachment: torch.Tensor               # int16 [H, W, 4]: .rg mapped, .ba smooth
    emissive_attachment: torch.Tensor             # int32 [H, W]: B10G11R11 UfloatPack32
    metallic_roughness_occlusion_attachment: torch.Tensor  # int32 [H, W]: R8G8B8A8 Unorm
    ambient_occlusion_attachment: torch.Tensor    # int16 [H, W]: binary16 bits
    resolved_shadows_attachment: Optional[ImageAttachment]  # R32F, read with HasDirectionalLight
    contact_shadows_attachment: Optional[ImageAttachment]   # R32F, read with HasContactShadows
    final_attachment: torch.Tensor                # out
    scene_flags: int
    inv_projection_view: list                     # column-major float[16]
    camera_position: tuple
    sun_dir: tuple                                # L, used as given
    sun_intensity: float
    lights_buffer: Optional[torch.Tensor] = None  # uint8 [light_count * 64] GPU::Light records
    light_count: int = 0
    base_ambient_color: tuple = (0.03, 0.03, 0.03)
    sky_solid_color: tuple = (0.0, 0.0, 0.0, 1.0)
    sky_ambient_color: tuple = (0.0, 0.0, 0.0)
    sky_has_texture: bool = False

    @staticmethod
    def create(depth, albedo, normal, emissive, metallic_roughness_occlusion, ambient_occlusion, resolved_shadows, contact_shadows, scene_flags: int,
               inv_projection_view, camera_position, sun_dir, sun_intensity: float, lights: Optional[torch.Tensor] = None,
               base_ambient_color=(0.03, 0.03, 0.03), sky_solid_color=(0.0, 0.0, 0.0, 1.0), sky_ambient_color=(0.0, 0.0, 0.0),
               sky_has_texture: bool = False) -> "PBRContext":
        d = depth if isinstance(depth, ImageAttachment) else ImageAttachment.depth(depth)
        img = lambda t: t if t is None or isinstance(t, ImageAttachment) else ImageAttachment.depth(t)  # noqa: E731
        dev = d.data.device
        if int(scene_flags) & L.SCENE_TRANSPARENT_BACKGROUND:
            out = torch.zeros((d.height, d.width, 4), dtype=torch.int16, device=dev)
        else:
            out = torch.zeros((d.height, d.width), dtype=torch.int32, device=dev)
        count = 0 if lights is None else lights.numel() * lights.element_size() // 64
        return PBRContext(d, albedo, normal, emissive, metallic_roughness_occlusion, ambient_occlusion, img(resolved_shadows), img(contact_shadows), out,
                          int(scene_flags), [float(x) for x in inv_projection_view], tuple(float(x) for x in camera_position),
                          tuple(float(x) for x in sun_dir), float(sun_intensity), lights, count, tuple(float(x) for x in base_ambient_color),
                          tuple(float(x) for x in sky_solid_color), tuple(float(x) for x in sky_ambient_color), bool(sky_has_texture))


def exposure_buffer(device="cuda") -> torch.Tensor:
    """A fresh GPU::HistogramLuminance {adapted_luminance, exposure} = {1.0, 1.0}, as RendererInstance.cpp:1778-1784 fills it: float32 [2].
    The caller keeps it between frames; apply_eye_adaptation reads and rewrites it."""
    return torch.ones(2, dtype=torch.float32, device=device)


def eye_adaptation_time_coeff(adaptation_speed: float, delta_time: float) -> float:
    """1 - exp(-adaptation_speed * delta_time) in binary32 (PostProcess.cpp:63) with this host's exp: outside the parity claim.  The exponential is
    Python's binary64 `exp` rounded to binary32 once, the C++ shim's is the platform's `expf`: for the same inputs the two may differ in the last
    bit.  Both pass their result on as `time_coeff`, and the rule starts behind it."""
    f32 = lambda x: struct.unpack("<f", struct.pack("<f", x))[0]  # noqa: E731
    return f32(1.0 - f32(math.exp(f32(-f32(adaptation_speed) * f32(delta_time)))))


@dataclass
class EyeAdaptationContext(Marshalled):
    """oxc_eye_adaptation_context: RendererInstance::apply_eye_adaptation (Passes/PostProcess.cpp:7-77).  `create` takes the image apply_pbr
    wrote -- int32 [H, W] (B10G11R11) or int16 [H, W, 4] (R16G16B16A16 Sfloat); the format follows from the shape --, the persistent
    exposure buffer (exposure_buffer()) and the GPU::HistogramLuminanceInfo settings, and allocates the histogram: int32 [256]."""
    _ctype = L.EyeAdaptationContext
    _derived = {"time_coeff": lambda s, delta_time: float(s.time_coeff) if s.time_coeff is not None
                else eye_adaptation_time_coeff(s.adaptation_speed, delta_time)}
    final_attachment: torch.Tensor   # in
    histogram_buffer: torch.Tensor   # out: int32 [256], this frame's counts
    exposure_buffer: torch.Tensor    # in/out: float32 [2]
    width: int
    height: int
    source_format: int
    min_exposure: float = -6.0
    max_exposure: float = 18.0
    adaptation_speed: float = 1.1
    ev100_bias: float = 1.0
    time_coeff: Optional[float] = None  # set: passed on as given; None: from adaptation_speed and the call's delta_time

    @staticmethod
    def create(final_attachment: torch.Tensor, exposure: torch.Tensor, min_exposure: float = -6.0, max_exposure: float = 18.0,
               adaptation_speed: float = 1.1, ev100_bias: float = 1.0, time_coeff: Optional[float] = None) -> "EyeAdaptationContext":
        fmt = L.EYE_SOURCE_R16G16B16A16 if final_attachment.dim() == 3 else L.EYE_SOURCE_B10G11R11
        hist = torch.zeros(256, dtype=torch.int32, device=final_attachment.device)
        return EyeAdaptationContext(final_attachment, hist, exposure, int(final_attachment.shape[1]), int(final_attachment.shape[0]), fmt,
                                    float(min_exposure), float(max_exposure), float(adaptation_speed), float(ev100_bias), time_coeff)

    def c(self, delta_time: float = 0.0) -> L.EyeAdaptationContext:
        return self._fill(L.EyeAdaptationContext(), delta_time)


def bloom_layout(width: int, height: int, source_format: int = L.EYE_SOURCE_B10G11R11, gap_texels: int = 0):
    """The shape of oxc_apply_bloom's two pyramids for a width x height source: (w2, h2, L, level_offset, total_bytes) with
    (w2, h2) = (width // 2, height // 2), L = floor(log2(max(w2, h2))) + 1 and level k, max(1, w2 >> k) x max(1, h2 >> k) texels of 4
    (B10G11R11) or 8 (R16G16B16A16 Sfloat) bytes, at level_offset[k] in one buffer, the levels one behind the other with `gap_texels`
    unused texels before each.  (Texture::calculate_mip_count and RendererInstance.cpp:509-510.)"""
    w2, h2 = width // 2, height // 2
    levels = max(w2, h2, 1).bit_length()
    texel = 8 if source_format == L.EYE_SOURCE_R16G16B16A16 else 4
    offsets, at = [], 0
    for k in range(levels):
        at += gap_texels * texel
        offsets.append(at)
        at += max(1, w2 >> k) * max(1, h2 >> k) * texel
    return w2, h2, levels, offsets, at + gap_texels * texel


@dataclass
class BloomPyramid:
    """oxc_image_pyramid: a mip pyramid of B10G11R11 (int32 buffer) or R16G16B16A16 Sfloat (int16 buffer) texels in one 1-D tensor."""
    data: torch.Tensor
    width: int
    height: int
    levels: int
    level_offset: list  # bytes
    source_format: int

    @staticmethod
    def create(width: int, height: int, source_format: int, device="cuda") -> "BloomPyramid":
        """The pyramid of a width x height SOURCE image: level 0 is width // 2 x height // 2."""
        w2, h2, levels, offsets, total = bloom_layout(width, height, source_format)
        dtype, size = (torch.int16, 2) if source_format == L.EYE_SOURCE_R16G16B16A16 else (torch.int32, 4)
        return BloomPyramid(torch.zeros(total // size, dtype=dtype, device=device), w2, h2, levels, offsets, source_format)

    def level(self, k: int) -> torch.Tensor:
        """Level k as a view: int32 [h, w] or int16 [h, w, 4]."""
        w, h = max(1, self.width >> k), max(1, self.height >> k)
        per = 4 if self.source_format == L.EYE_SOURCE_R16G16B16A16 else 1
        first = self.level_offset[k] // self.data.element_size()
        flat = self.data[first:first + w * h * per]
        return flat.view(h, w, 4) if per == 4 else flat.view(h, w)

    def c(self) -> L.ImagePyramid:
        im = L.ImagePyramid()
        im.dptr = self.data.data_ptr() if self.data is not None else None
        im.width, im.height, im.levels = int(self.width), int(self.height), int(self.levels)
        for k, o in enumerate(self.level_offset[:13]):
            im.level_offset[k] = int(o)
        im.bytes = self.data.numel() * self.data.element_size() if self.data is not None else 0
        return im


@dataclass
class BloomContext(Marshalled):
    """oxc_bloom_context: RendererInstance::apply_bloom (Passes/PostProcess.cpp:79-203).  `create` takes the image apply_pbr wrote -- int32
    [H, W] (B10G11R11) or int16 [H, W, 4] (R16G16B16A16 Sfloat); the format follows from the shape --, the scene flags (only
    L.SCENE_HAS_EYE_ADAPTATION is read) and the exposure buffer apply_eye_adaptation left behind, and allocates the two pyramids.
    bloom_intensity is what apply_bloom hands to the tonemap: TonemapContext.create reads it from here; oxc_apply_bloom does not."""
    _ctype = L.BloomContext
    _leave = ("_pad",)
    final_attachment: torch.Tensor                # in
    exposure_buffer: Optional[torch.Tensor]       # in with SCENE_HAS_EYE_ADAPTATION: float32 [2]
    bloom_downsampled_attachment: BloomPyramid    # out
    bloom_upsampled_attachment: BloomPyramid      # out: level 0 is the bloom the tonemap reads
    width: int
    height: int
    source_format: int
    scene_flags: int = 0
    threshold: float = 1.0        # the pp.bloom_* defaults, RendererCVar.cpp:44-48
    soft_threshold: float = 0.125
    clamp_value: float = 4.0
    radius: float = 0.75
    bloom_intensity: float = 0.1

    @staticmethod
    def create(final_attachment: torch.Tensor, scene_flags: int = 0, exposure: Optional[torch.Tensor] = None, threshold: float = 1.0,
               soft_threshold: float = 0.125, clamp_value: float = 4.0, radius: float = 0.75, bloom_intensity: float = 0.1) -> "BloomContext":
        fmt = L.EYE_SOURCE_R16G16B16A16 if final_attachment.dim() == 3 else L.EYE_SOURCE_B10G11R11
        H, W = int(final_attachment.shape[0]), int(final_attachment.shape[1])
        dev = final_attachment.device
        return BloomContext(final_attachment, exposure, BloomPyramid.create(W, H, fmt, dev), BloomPyramid.create(W, H, fmt, dev), W, H, fmt, int(scene_flags),
                            float(threshold), float(soft_threshold), float(clamp_value), float(radius), float(bloom_intensity))


@dataclass
class TonemapContext(Marshalled):
    """oxc_tonemap_context: RendererInstance::apply_tonemap (Passes/PostProcess.cpp:205-247).  `create` takes the image apply_pbr wrote -- int32
    [H, W] (B10G11R11) or int16 [H, W, 4] (R16G16B16A16 Sfloat); the format follows from the shape --, the scene flags, the tone curve, the
    exposure buffer apply_eye_adaptation left behind and the BloomContext apply_bloom ran on (its upsample pyramid and its bloom_intensity),
    and allocates the 8-bit destination, int32 [H, W].  The six GPU::PostProcessSettings fields carry the engine's defaults."""
    _ctype = L.TonemapContext
    final_attachment: torch.Tensor                            # in
    exposure_buffer: Optional[torch.Tensor]                   # in with SCENE_HAS_EYE_ADAPTATION: float32 [2]
    bloom_upsampled_attachment: Optional[BloomPyramid]        # in with SCENE_HAS_BLOOM: only level 0 is read
    dst_attachment: torch.Tensor                              # out: int32 [H, W]
    width: int
    height: int
    source_format: int
    output_format: int = L.TONEMAP_OUT_R8G8B8A8_SRGB
    scene_flags: int = 0
    tonemap_type: int = L.TONEMAP_ACES
    exposure: float = 1.0                                     # SceneGPU.hpp:295-302
    chromatic_aberration_amount: float = 0.5
    vignette_amount: float = 0.5
    film_grain_scale: float = 1.0
    film_grain_amount: float = 0.5
    film_grain_seed: int = 0
    bloom_intensity: float = 0.1

    @staticmethod
    def create(final_attachment: torch.Tensor, scene_flags: int = 0, tonemap_type: int = L.TONEMAP_ACES, exposure_buffer: Optional[torch.Tensor] = None,
               bloom: Optional[BloomContext] = None, output_format: int = L.TONEMAP_OUT_R8G8B8A8_SRGB, **settings) -> "TonemapContext":
        fmt = L.EYE_SOURCE_R16G16B16A16 if final_attachment.dim() == 3 else L.EYE_SOURCE_B10G11R11
        H, W = int(final_attachment.shape[0]), int(final_attachment.shape[1])
        dst = torch.zeros((H, W), dtype=torch.int32, device=final_attachment.device)
        if bloom is not None:
            settings.setdefault("bloom_intensity", bloom.bloom_intensity)
        return TonemapContext(final_attachment, exposure_buffer, bloom.bloom_upsampled_attachment if bloom is not None else None, dst, W, H, fmt,
                              int(output_format), int(scene_flags), int(tonemap_type), **settings)


@dataclass
class FxaaContext(Marshalled):
    """oxc_fxaa_context: the `fxaa` pass (RendererInstance.cpp:1225-1255, passes/fxaa/fxaa.slang).  `create` takes the image apply_pbr wrote --
    int32 [H, W] (B10G11R11) or int16 [H, W, 4] (R16G16B16A16 Sfloat); the format follows from the shape -- and allocates fxaa_attachment,
    a second image of the same shape."""
    _ctype = L.FxaaContext
    final_attachment: torch.Tensor  # in
    fxaa_attachment: torch.Tensor   # out
    width: int
    height: int
    source_format: int

    @staticmethod
    def create(final_attachment: torch.Tensor) -> "FxaaContext":
        fmt = L.EYE_SOURCE_R16G16B16A16 if final_attachment.dim() == 3 else L.EYE_SOURCE_B10G11R11
        H, W = int(final_attachment.shape[0]), int(final_attachment.shape[1])
        return FxaaContext(final_attachment, torch.zeros_like(final_attachment), W, H, fmt)


@dataclass
class Atmosphere(Marshalled):
    """GPU::Atmosphere (SceneGPU.hpp:158-181).  The defaults are the record's own; `engine()` is what RendererInstance.cpp:1445-1455 makes of the
    AtmosphereComponent's defaults (the scattering and absorption coefficients times 1e-3f in binary32) with the engine's four LUT extents."""
    _ctype = L.Atmosphere
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

    @staticmethod
    def engine(**overrides) -> "Atmosphere":
        f32 = lambda x: struct.unpack("f", struct.pack("f", x))[0]  # noqa: E731
        s = lambda v: tuple(f32(f32(x) * f32(1e-3)) for x in v)  # noqa: E731  (the binary32 product the engine forms: exact in binary64, rounded once)
        a = Atmosphere(rayleigh_scatter=s((5.802, 13.558, 33.100)), mie_scatter=s((3.996, 3.996, 3.996)), mie_extinction=s((4.44,))[0],
                       ozone_absorption=s((0.650, 1.881, 0.085)))
        for k, v in overrides.items():
            setattr(a, k, v)
        return a


def _lut(size, device) -> torch.Tensor:
    return torch.zeros(tuple(int(n) for n in size) + (4,), dtype=torch.int16, device=device)


@dataclass
class SkyLutContext(Marshalled):
    """oxc_sky_lut_context: the constructor-time pair of the reference (RendererInstance.cpp:136-251).  `create` takes the Atmosphere record and
    the caller's 64 hemisphere directions (float32 [64, 3]) and allocates the two LUTs, int16 [H, W, 4] of binary16 bits."""
    _ctype = L.SkyLutContext
    _leave = ("_pad",)
    atmosphere: Atmosphere
    hemisphere_directions: torch.Tensor  # in: float32 [64, 3]
    sky_transmittance_lut: torch.Tensor  # out
    sky_multiscatter_lut: torch.Tensor   # out

    @staticmethod
    def create(atmosphere: Atmosphere, hemisphere_directions: torch.Tensor) -> "SkyLutContext":
        dev = hemisphere_directions.device
        t, m = atmosphere.transmittance_lut_size, atmosphere.multiscattering_lut_size
        return SkyLutContext(atmosphere, hemisphere_directions, _lut((t[1], t[0]), dev), _lut((m[1], m[0]), dev))


@dataclass
class AtmosphereContext(Marshalled):
    """oxc_atmosphere_context: RendererInstance::draw_atmosphere (Passes/PBR.cpp:9-141) without its sky_ibl pass; the reference's
    sky_cubemap_attachment belongs to SkyIblContext, which is made from this one.  `create` lays out the four buffers from an Atmosphere; generate_sky_luts fills the first two through
    `sky_luts(hemisphere_directions)`."""
    _ctype = L.AtmosphereContext
    _derived = {"sky_transmittance_lut": "sky_transmittance_lut_attachment", "sky_multiscatter_lut": "sky_multiscatter_lut_attachment",
                "sky_view_lut": "sky_view_lut_attachment", "sky_aerial_perspective_lut": "sky_aerial_perspective_lut_attachment"}
    _leave = ("_pad", "_pad1")
    atmosphere: Atmosphere
    sky_transmittance_lut_attachment: torch.Tensor       # in
    sky_multiscatter_lut_attachment: torch.Tensor        # in
    sky_view_lut_attachment: torch.Tensor                # out: int16 [H, W, 4]
    sky_aerial_perspective_lut_attachment: torch.Tensor  # out: int16 [D, H, W, 4]
    sun_dir: tuple = (0.0, 1.0, 0.0)
    sun_intensity: float = 10.0
    camera_position: tuple = (0.0, 0.0, 0.0)
    camera_inv_projection_view: tuple = (1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0)

    @staticmethod
    def create(atmosphere: Atmosphere, device="cuda", **settings) -> "AtmosphereContext":
        t, m, v, a = (atmosphere.transmittance_lut_size, atmosphere.multiscattering_lut_size, atmosphere.sky_view_lut_size,
                      atmosphere.aerial_perspective_lut_size)
        return AtmosphereContext(atmosphere, _lut((t[1], t[0]), device), _lut((m[1], m[0]), device), _lut((v[1], v[0]), device),
                                 _lut((a[2], a[1], a[0]), device), **settings)

    def sky_luts(self, hemisphere_directions: torch.Tensor) -> SkyLutContext:
        return SkyLutContext(self.atmosphere, hemisphere_directions, self.sky_transmittance_lut_attachment, self.sky_multiscatter_lut_attachment)


@dataclass
class SkyIblContext(Marshalled):
    """oxc_sky_ibl_context: the sky_ibl pass of RendererInstance::draw_atmosphere (Passes/PBR.cpp:52-94).  `create` takes the AtmosphereContext
    whose sky-view and transmittance LUTs it reads -- the tensors are shared, with its record, sun and camera -- and allocates the zeroed cube,
    int16 [6, cube_size, cube_size, 4]; the cube is its own history, so one context is kept across frames and only `frame_index` moves."""
    _ctype = L.SkyIblContext
    _derived = {"sky_view_lut": "sky_view_lut_attachment", "sky_transmittance_lut": "sky_transmittance_lut_attachment", "sky_cubemap": "sky_cubemap_attachment"}
    _leave = ("_pad",)
    atmosphere: Atmosphere
    sky_view_lut_attachment: torch.Tensor           # in
    sky_transmittance_lut_attachment: torch.Tensor  # in
    sky_cubemap_attachment: torch.Tensor            # in and out
    cube_size: int = 32
    sun_dir: tuple = (0.0, 1.0, 0.0)
    sun_intensity: float = 10.0
    camera_position: tuple = (0.0, 0.0, 0.0)
    sun_ambient_strength: float = 0.15
    frame_index: int = 0

    @staticmethod
    def create(context: AtmosphereContext, cube_size: int = 32, **settings) -> "SkyIblContext":
        view = context.sky_view_lut_attachment
        for name in ("sun_dir", "sun_intensity", "camera_position"):
            settings.setdefault(name, getattr(context, name))
        return SkyIblContext(context.atmosphere, view, context.sky_transmittance_lut_attachment, _lut((6, cube_size, cube_size), view.device),
                             int(cube_size), **settings)


@dataclass
class PBRAtmosphereContext(Marshalled):
    """oxc_pbr_atmosphere_context: the atmosphere branch of RendererInstance::apply_pbr (Passes/PBR.cpp:318-434, pbr_apply).  `create` takes the
    G-buffer, the shadow terms, the lights and the flags from a PBRContext, the record, the transmittance, sky-view and aerial LUTs, the sun and
    the camera from the AtmosphereContext they were drawn with, and the cube and its size from the SkyIblContext -- every tensor is shared --
    and allocates the output in the format the flags pick.  The Sky record and base_ambient_color of the PBRContext are not read."""
    _ctype = L.PbrAtmosphereContext
    _derived = {"width": "depth_attachment.width", "height": "depth_attachment.height", "sky_transmittance_lut": "sky_transmittance_lut_attachment",
                "sky_view_lut": "sky_view_lut_attachment", "sky_aerial_perspective_lut": "sky_aerial_perspective_lut_attachment",
                "sky_cubemap": "sky_cubemap_attachment"}
    _leave = ("_pad",)
    depth_attachment: ImageAttachment
    albedo_attachment: torch.Tensor
    normal_attachment: torch.Tensor
    emissive_attachment: torch.Tensor
    metallic_roughness_occlusion_attachment: torch.Tensor
    ambient_occlusion_attachment: torch.Tensor
    resolved_shadows_attachment: Optional[ImageAttachment]  # R32F, read with HasDirectionalLight
    contact_shadows_attachment: Optional[ImageAttachment]   # R32F, read with HasContactShadows
    final_attachment: torch.Tensor                          # out
    scene_flags: int
    inv_projection_view: list
    camera_position: tuple
    sun_dir: tuple
    sun_intensity: float
    atmosphere: Atmosphere
    sky_transmittance_lut_attachment: torch.Tensor          # in: int16 [H, W, 4]
    sky_view_lut_attachment: torch.Tensor                   # in: int16 [H, W, 4]
    sky_aerial_perspective_lut_attachment: torch.Tensor     # in: int16 [D, H, W, 4]
    sky_cubemap_attachment: torch.Tensor                    # in: int16 [6, cube_size, cube_size, 4]
    cube_size: int = 32
    lights_buffer: Optional[torch.Tensor] = None
    light_count: int = 0

    @staticmethod
    def create(pbr_context: PBRContext, atmosphere_context: AtmosphereContext, sky_ibl_context: SkyIblContext, **settings) -> "PBRAtmosphereContext":
        p, a, i = pbr_context, atmosphere_context, sky_ibl_context
        values = dict(scene_flags=p.scene_flags, inv_projection_view=list(a.camera_inv_projection_view), camera_position=tuple(a.camera_position),
                      sun_dir=tuple(a.sun_dir), sun_intensity=float(a.sun_intensity), atmosphere=a.atmosphere, cube_size=int(i.cube_size),
                      lights_buffer=p.lights_buffer, light_count=p.light_count)
        values.update(settings)
        d = p.depth_attachment
        if int(values["scene_flags"]) & L.SCENE_TRANSPARENT_BACKGROUND:
            out = torch.zeros((d.height, d.width, 4), dtype=torch.int16, device=d.data.device)
        else:
            out = torch.zeros((d.height, d.width), dtype=torch.int32, device=d.data.device)
        return PBRAtmosphereContext(d, p.albedo_attachment, p.normal_attachment, p.emissive_attachment, p.metallic_roughness_occlusion_attachment,
                                    p.ambient_occlusion_attachment, p.resolved_shadows_attachment, p.contact_shadows_attachment, out,
                                    sky_transmittance_lut_attachment=a.sky_transmittance_lut_attachment, sky_view_lut_attachment=a.sky_view_lut_attachment,
                                    sky_aerial_perspective_lut_attachment=a.sky_aerial_perspective_lut_attachment,
                                    sky_cubemap_attachment=i.sky_cubemap_attachment, **values)


@dataclass
class TerrainErosion(Marshalled):
    """GPU::TerrainErosion (SceneGPU.hpp:358-372) with the record's own defaults."""
    _ctype = L.TerrainErosion
    scale: float = 0.15
    strength: float = 0.22
    gully_weight: float = 0.5
    detail: float = 1.5
    rounding: tuple = (0.1, 0.0, 0.1, 2.0)
    onset: tuple = (1.25, 1.25, 2.8, 1.5)
    assumed_slope: tuple = (0.7, 1.0)
    cell_scale: float = 0.7
    gain: float = 0.5
    lacunarity: float = 2.0
    normalization: float = 0.5
    octaves: int = 5
    seed: int = 0


@dataclass
class TerrainGenerate(Marshalled):
    """GPU::TerrainGenerate (SceneGPU.hpp:374-384) with the record's own defaults; `resolution` is filled by the context."""
    _ctype = L.TerrainGenerate
    erosion: TerrainErosion = field(default_factory=TerrainErosion)
    resolution: tuple = (0, 0)
    height_offset: tuple = (-0.65, 0.0)
    domain_size: float = 2.0
    height_frequency: float = 3.0
    height_amplitude: float = 0.125
    height_lacunarity: float = 2.0
    height_gain: float = 0.1
    height_octaves: int = 3


@dataclass
class TerrainDerive(Marshalled):
    """GPU::TerrainDerive (SceneGPU.hpp:386-395) with the record's own defaults; the first three are what Terrain::bake fills."""
    _ctype = L.TerrainDerive
    resolution: tuple = (0, 0)
    texel_world_size: tuple = (0.0, 0.0)
    height_range: float = 0.0
    slope_rock_begin: float = 0.55
    slope_rock_end: float = 0.8
    altitude_snow_begin: float = 0.7
    altitude_snow_end: float = 0.85
    ridge_drainage_scale: float = 1.0


def _patch_minmax_image(self) -> L.Image:
    im = L.Image()
    t = self.patch_minmax
    if t is not None:
        im.dptr, im.width, im.height, im.levels = t.data_ptr(), int(t.shape[1]), int(t.shape[0]), 1
    return im


@dataclass
class TerrainMapsContext(Marshalled):
    """oxc_terrain_maps_context: the three passes of Terrain::bake (Scene/Terrain.cpp:406-461) and of the brush's regional re-bake
    (Passes/Terrain.cpp:134-156).  `create` allocates the five outputs and zeroed edit images for a Terrain of `resolution`, `patch_count`,
    `world_size` and `height_range`, and fills the settings' resolution, texel_world_size and height_range as bake does; the dispatch is the
    whole map.  `patch_minmax` is float32 [patch_count.y, patch_count.x, 2], what RendererInstance.cull_terrain takes.  `region`: int32 [4]
    on the device {texel_origin.xy, patch_origin.xy}, or None for zero origins."""
    _ctype = L.TerrainMapsContext
    _derived = {"patch_minmax": _patch_minmax_image}
    generate: TerrainGenerate
    derive: TerrainDerive
    resolution: tuple
    patch_count: tuple
    dispatch_texels: tuple
    dispatch_patches: tuple
    heightmap: Optional[torch.Tensor]     # int16 [H, W]: R16 Unorm
    ridgemap: Optional[torch.Tensor]      # int16 [H, W]: binary16 bits
    normalmap: Optional[torch.Tensor]     # int16 [H, W, 2]: binary16 bits
    splatmap: Optional[torch.Tensor]      # int32 [H, W]: R8G8B8A8 Unorm
    height_edit: Optional[torch.Tensor]   # float32 [H, W]
    splat_edit: Optional[torch.Tensor]    # int32 [H, W]
    patch_minmax: Optional[torch.Tensor]  # float32 [py, px, 2]
    region: Optional[torch.Tensor] = None
    stages: int = L.TERRAIN_ALL

    @staticmethod
    def create(resolution=(2048, 2048), patch_count=(64, 64), world_size=(1024.0, 1024.0), height_range=(0.0, 400.0),
               generate: Optional[TerrainGenerate] = None, derive: Optional[TerrainDerive] = None, device="cuda", **settings) -> "TerrainMapsContext":
        import dataclasses

        f32 = lambda x: struct.unpack("f", struct.pack("f", x))[0]  # noqa: E731
        W, H = int(resolution[0]), int(resolution[1])
        g = dataclasses.replace(generate or TerrainGenerate(), resolution=(W, H))
        tws = tuple(f32(f32(world_size[k]) / f32(float(resolution[k]))) for k in range(2))  # Terrain::texel_world_size, binary32
        d = dataclasses.replace(derive or TerrainDerive(), resolution=(W, H), texel_world_size=tws, height_range=f32(f32(height_range[1]) - f32(height_range[0])))
        z = lambda shape, dtype: torch.zeros(shape, dtype=dtype, device=device)  # noqa: E731
        return TerrainMapsContext(g, d, (W, H), tuple(int(v) for v in patch_count), (W, H), tuple(int(v) for v in patch_count), z((H, W), torch.int16),
                                  z((H, W), torch.int16), z((H, W, 2), torch.int16), z((H, W), torch.int32), z((H, W), torch.float32), z((H, W), torch.int32),
                                  z((int(patch_count[1]), int(patch_count[0]), 2), torch.float32), **settings)


@dataclass
class TerrainBrushParams(Marshalled):
    """GPU::TerrainBrushParams (scene.slang:606-621), field for field.  `engine` forms them from a Terrain's and its brush's values the way
    RendererInstance::apply_terrain_brush does (Passes/Terrain.cpp:42-67), in binary32."""
    _ctype = L.TerrainBrushParams
    ray_origin: tuple = (0.0, 0.0, 0.0)
    radius_texels: float = 0.0
    ray_direction: tuple = (0.0, -1.0, 0.0)
    strength: float = 0.0
    resolution: tuple = (0, 0)
    world_min: tuple = (0.0, 0.0)
    world_size: tuple = (0.0, 0.0)
    inv_world_size: tuple = (0.0, 0.0)
    patch_count: tuple = (0, 0)
    base_height: float = 0.0
    height_scale: float = 0.0
    falloff: float = 1.0
    flatten_height: float = 0.0
    mode: int = L.TERRAIN_BRUSH_RAISE
    layer: int = 0

    @staticmethod
    def engine(resolution, patch_count, ray_origin, ray_direction, world_size=(1024.0, 1024.0), height_range=(0.0, 400.0), radius_world: float = 32.0,
               mode: int = L.TERRAIN_BRUSH_RAISE, layer: int = 0, falloff: float = 1.0, height_rate: float = 4.0, blend_rate: float = 3.0,
               flatten_height_world: float = 0.0, invert: bool = False, delta_time: float = 1.0 / 60.0, world_origin=(0.0, 0.0, 0.0)) -> "TerrainBrushParams":
        import numpy as np

        F = np.float32
        ws, res = [F(v) for v in world_size], [F(float(v)) for v in resolution]
        texel = [ws[k] / res[k] for k in range(2)]  # Terrain::texel_world_size
        base, scale = F(world_origin[1]) + F(height_range[0]), F(height_range[1]) - F(height_range[0])
        height_scale = max(scale, F(1e-3))
        dt = min(max(F(delta_time), F(0.0)), F(1.0) / F(30.0))
        displaces = mode in (L.TERRAIN_BRUSH_RAISE, L.TERRAIN_BRUSH_NOISE)
        strength = F(height_rate) * dt / height_scale if displaces else min(max(F(blend_rate) * dt, F(0.0)), F(1.0))
        flatten = min(max((F(flatten_height_world) - base) / height_scale, F(0.0)), F(1.0))
        return TerrainBrushParams(tuple(ray_origin), float(F(radius_world) / max(texel[0], texel[1])), tuple(ray_direction), float(-strength if invert else strength),
                                  tuple(int(v) for v in resolution), tuple(float(F(world_origin[2 * k]) - ws[k] * F(0.5)) for k in range(2)), tuple(float(w) for w in ws),
                                  tuple(float(F(1.0) / w) for w in ws), tuple(int(v) for v in patch_count), float(base), float(scale), float(falloff),
                                  float(flatten), int(mode), int(layer))


@dataclass
class TerrainBrushContext(Marshalled):
    """oxc_terrain_brush_context: the brush's ray trace and its stroke into the edit images (Passes/Terrain.cpp:35-132).  `hit` int32 [4]
    ({f32 world_position[3], u32 valid}) and `region` int32 [4] on the device; `region` is what TerrainMapsContext.region takes.  `over` binds a
    TerrainMapsContext's heightmap and edit images and allocates the two records."""
    _ctype = L.TerrainBrushContext
    params: TerrainBrushParams
    heightmap: Optional[torch.Tensor]    # int16 [H, W]: R16 Unorm
    height_edit: Optional[torch.Tensor]  # float32 [H, W]
    splat_edit: Optional[torch.Tensor]   # int32 [H, W]
    hit: Optional[torch.Tensor]          # int32 [4]
    region: Optional[torch.Tensor]       # int32 [4]
    stages: int = L.TERRAIN_BRUSH_ALL

    @staticmethod
    def over(maps: TerrainMapsContext, params: TerrainBrushParams, **settings) -> "TerrainBrushContext":
        z = lambda: torch.zeros((4,), dtype=torch.int32, device=maps.heightmap.device)  # noqa: E731
        return TerrainBrushContext(params, maps.heightmap, maps.height_edit, maps.splat_edit, z(), z() if maps.region is None else maps.region, **settings)


@dataclass
class TerrainData(Marshalled):
    """GPU::TerrainData (scene.slang:634-647), field for field, with the record's own defaults (SceneGPU.hpp:440-453).  `of` forms it for a
    Terrain centred on the origin, in binary32."""
    _ctype = L.TerrainData
    world_min: tuple = (0.0, 0.0)
    world_size: tuple = (0.0, 0.0)
    inv_world_size: tuple = (0.0, 0.0)
    patch_count: tuple = (0, 0)
    base_height: float = 0.0
    height_scale: float = 0.0
    target_edge_pixels: float = 16.0
    max_tessellation: float = 64.0
    layer_tiling: float = 8.0
    triplanar_begin: float = 0.5
    layer_material_indices: tuple = (L.TERRAIN_INVALID_LAYER_MATERIAL,) * 4
    brush_radius: float = 0.0

    @staticmethod
    def of(world_size=(1024.0, 1024.0), patch_count=(64, 64), height_range=(0.0, 400.0), **settings) -> "TerrainData":
        import numpy as np

        F = np.float32
        ws = [F(v) for v in world_size]
        return TerrainData(tuple(float(-w * F(0.5)) for w in ws), tuple(float(w) for w in ws), tuple(float(F(1.0) / w) for w in ws),
                           tuple(int(v) for v in patch_count), float(F(height_range[0])), float(F(height_range[1]) - F(height_range[0])), **settings)


@dataclass
class TerrainDecodeContext(Marshalled):
    """oxc_terrain_decode_context: RendererInstance::decode_terrain (Passes/Terrain.cpp:279-360), the geometry and material-factor half of
    terrain_decode.slang.  The four attachments are the ones a VisbufferDecodeContext wrote; only their terrain pixels are written.  `over`
    binds a VisbufferDecodeContext's images, a TerrainMapsContext's normal and splat maps and a TerrainBrushContext's hit record."""
    _ctype = L.TerrainDecodeContext
    _derived = {"width": "depth_attachment.width", "height": "depth_attachment.height"}
    visbuffer_attachment: Optional[torch.Tensor]  # int32 [H, W]
    depth_attachment: ImageAttachment             # R32F, levels = 1
    inv_projection_view: list                     # column-major float[16]
    terrain: TerrainData
    map_resolution: tuple
    normalmap: Optional[torch.Tensor]             # int16 [h, w, 2]: R16G16 Sfloat bits
    splatmap: Optional[torch.Tensor]              # int32 [h, w]: R8G8B8A8 Unorm
    materials_buffer: Optional[torch.Tensor]      # uint8 [material_count * 56]
    material_count: int
    brush_hit: Optional[torch.Tensor]             # int32 [4]: oxc_terrain_brush_hit; may be None unless terrain.brush_radius > 0
    albedo_attachment: Optional[torch.Tensor]
    normal_attachment: Optional[torch.Tensor]
    emissive_attachment: Optional[torch.Tensor]
    metallic_roughness_occlusion_attachment: Optional[torch.Tensor]

    @staticmethod
    def over(decode: "VisbufferDecodeContext", maps: TerrainMapsContext, inv_projection_view, terrain: TerrainData, brush_hit: Optional[torch.Tensor] = None) -> "TerrainDecodeContext":
        h, w = maps.splatmap.shape[:2]
        return TerrainDecodeContext(decode.visbuffer_attachment, decode.depth_attachment, [float(x) for x in inv_projection_view], terrain, (int(w), int(h)),
                                    maps.normalmap, maps.splatmap, decode.materials_buffer, decode.material_count, brush_hit, decode.albedo_attachment,
                                    decode.normal_attachment, decode.emissive_attachment, decode.metallic_roughness_occlusion_attachment)


def terrain_projection_scale(resolution_y: float, fov_degrees: float) -> float:
    """The engine's projection_scale of terrain_visbuffer.slang:36, resolution.y * 0.5 / tan(radians(fov) * 0.5), evaluated in binary64 and
    rounded to binary32 once: the value oxc_terrain_draw_context.projection_scale takes as given (include/oxcull.h, step T2)."""
    import math

    import numpy as np

    return float(np.float32(float(resolution_y) * 0.5 / math.tan(math.radians(float(fov_degrees)) * 0.5)))


@dataclass
class TerrainDrawContext(Marshalled):
    """oxc_terrain_draw_context: RendererInstance::draw_terrain_for_visbuffer (Passes/Terrain.cpp:218-277, terrain_visbuffer.slang), the
    tessellated patches of a terrain cull into the depth|vis image a draw_visbuffer call writes.  The patch list and the indirect command
    are read on the device; `projection_scale` is taken as given (`terrain_projection_scale`)."""
    _ctype = L.TerrainDrawContext
    _derived = {"width": lambda self: self.visdepth_buffer.shape[1], "height": lambda self: self.visdepth_buffer.shape[0]}
    visdepth_buffer: Optional[torch.Tensor]          # int64 [H, W]: depth bits << 32 | vis, in/out
    projection_view: list                            # column-major float[16]
    camera_position: tuple
    near_clip: float
    projection_scale: float
    terrain: TerrainData
    map_resolution: tuple
    heightmap: Optional[torch.Tensor]                # int16 [h, w]: R16 Unorm
    visible_patches_buffer: Optional[torch.Tensor]   # int32 [n]: patch indices
    draw_cmd_buffer: Optional[torch.Tensor]          # int32 [4]: VkDrawIndirectCommand
    clear: bool = False
    depth_attachment: Optional[ImageAttachment] = None
    visbuffer_attachment: Optional[torch.Tensor] = None


@dataclass
class DebugViewContext(Marshalled):
    """oxc_debug_view_context: RendererInstance::apply_debug_view (Passes/Debug.cpp:9-153), the views of debug_view.slang and rmvsm_debug.slang.
    Only what `debug_view` reads has to be given (include/oxcull.h, oxc_apply_debug_view); the rest may stay None.  `over` binds the images of
    a VisbufferDecodeContext, `vsm` the shape, camera and page buffers of a ShadowResolveContext; both allocate the output when none is
    given.  The frame's record buffers (Materials, MeshInstances, MeshLods) come from the renderer's prepared_frame."""
    _ctype = L.DebugViewContext
    _derived = {"width": "depth_attachment.width", "height": "depth_attachment.height"}
    debug_view: int
    depth_attachment: ImageAttachment                       # R32F, levels = 1
    debug_attachment: Optional[torch.Tensor]                # int16 [H, W, 4] out: R16G16B16A16 Sfloat bits
    visbuffer_attachment: Optional[torch.Tensor] = None     # int32 [H, W]
    clear: bool = True
    heatmap_scale: float = 10.0
    meshlet_instance_count: int = 0
    overdraw_attachment: Optional[torch.Tensor] = None      # int32 [H, W]: R32 Uint
    albedo_attachment: Optional[torch.Tensor] = None
    normal_attachment: Optional[torch.Tensor] = None
    emissive_attachment: Optional[torch.Tensor] = None
    metallic_roughness_occlusion_attachment: Optional[torch.Tensor] = None
    ambient_occlusion_attachment: Optional[torch.Tensor] = None  # int16 [H, W]: binary16 bits
    vsm_clipmaps_buffer: Optional[torch.Tensor] = None
    virtual_page_table: Optional[torch.Tensor] = None
    inv_projection_view: tuple = (0.0,) * 16
    resolution: tuple = (0.0, 0.0)
    page_size: int = 0
    page_table_size: int = 0
    physical_page_table_size: int = 0
    clipmap_count: int = 0
    first_clipmap_width: float = 0.0
    clipmap_selection_bias: float = 0.0
    virtual_extent: float = 0.0

    @staticmethod
    def _output(d: ImageAttachment) -> torch.Tensor:
        return torch.zeros((d.height, d.width, 4), dtype=torch.int16, device=d.data.device)

    @staticmethod
    def over(debug_view: int, decode: "VisbufferDecodeContext", ambient_occlusion: Optional[torch.Tensor] = None, overdraw: Optional[torch.Tensor] = None,
             debug_attachment: Optional[torch.Tensor] = None, **settings) -> "DebugViewContext":
        d = decode.depth_attachment
        return DebugViewContext(int(debug_view), d, DebugViewContext._output(d) if debug_attachment is None else debug_attachment,
                                visbuffer_attachment=decode.visbuffer_attachment, meshlet_instance_count=decode.meshlet_instance_count,
                                overdraw_attachment=overdraw, albedo_attachment=decode.albedo_attachment, normal_attachment=decode.normal_attachment,
                                emissive_attachment=decode.emissive_attachment,
                                metallic_roughness_occlusion_attachment=decode.metallic_roughness_occlusion_attachment,
                                ambient_occlusion_attachment=ambient_occlusion, **settings)

    @staticmethod
    def vsm(resolve: "ShadowResolveContext", debug_attachment: Optional[torch.Tensor] = None) -> "DebugViewContext":
        d = resolve.depth_attachment
        return DebugViewContext(L.DEBUG_VIEW_RMVSM, d, DebugViewContext._output(d) if debug_attachment is None else debug_attachment,
                                vsm_clipmaps_buffer=resolve.vsm_clipmaps_buffer, virtual_page_table=resolve.virtual_page_table,
                                inv_projection_view=tuple(resolve.inv_projection_view), resolution=tuple(resolve.resolution), page_size=resolve.page_size,
                                page_table_size=resolve.page_table_size, physical_page_table_size=resolve.physical_page_table_size,
                                clipmap_count=resolve.clipmap_count, first_clipmap_width=resolve.first_clipmap_width,
                                clipmap_selection_bias=resolve.clipmap_selection_bias, virtual_extent=resolve.virtual_extent)


@dataclass
class PickingContext(Marshalled):
    """oxc_pick_context: the editor's `mouse_picking` stage (ViewportPanel.cpp:1439-1497, editor/mouse_picking.slang): the transform index
    behind visbuffer texel `picking_texel`, one u32 into `transform_id`.  The record buffers come from the renderer's prepared_frame."""
    _ctype = L.PickContext
    _derived = {"x": lambda self: int(self.picking_texel[0]), "y": lambda self: int(self.picking_texel[1])}
    visbuffer_attachment: torch.Tensor      # int32 [H, W]
    width: int
    height: int
    picking_texel: tuple
    terrain_transform_index: int
    meshlet_instance_count: int
    transform_id: torch.Tensor              # int32 [1] out

    @staticmethod
    def over(visbuffer: torch.Tensor, picking_texel, terrain_transform_index: int, meshlet_instance_count: int, transform_id: Optional[torch.Tensor] = None) -> "PickingContext":
        out = torch.zeros(1, dtype=torch.int32, device=visbuffer.device) if transform_id is None else transform_id
        return PickingContext(visbuffer, visbuffer.shape[1], visbuffer.shape[0], tuple(picking_texel), terrain_transform_index, meshlet_instance_count, out)


@dataclass
class HighlightContext(Marshalled):
    """oxc_highlight_context: the editor's highlight_mask_stage and highlight_composite_stage (ViewportPanel.cpp:1166-1345; editor/
    highlight_mask.slang, highlight_dilate_horizontal.slang, highlight_composite.slang).  `stages` selects the mask (after the visbuffer is
    drawn), the composite (after the tonemap) or both; only what they read has to be given (include/oxcull.h, oxc_apply_highlight).
    `transform_indices` is the selection, `mask_bits` the one-bit-per-pixel silhouette mask the two stages share."""
    _ctype = L.HighlightContext
    _derived = {"selected_count": lambda self: 0 if self.transform_indices is None else self.transform_indices.numel()}
    stages: int
    width: int
    height: int
    mask_bits: Optional[torch.Tensor]                    # int64 [H, ceil(W / 64)]
    visbuffer_attachment: Optional[torch.Tensor] = None  # int32 [H, W]
    transform_indices: Optional[torch.Tensor] = None     # int32 [selected_count]
    terrain_transform_index: int = 0xFFFFFFFF
    meshlet_instance_count: int = 0
    mask_attachment: Optional[torch.Tensor] = None       # uint8 [H, W] out: the engine's R8 image, optional
    depth_attachment: Optional[ImageAttachment] = None   # R32F, levels = 1
    color_attachment: Optional[torch.Tensor] = None      # int32 [H, W]: what apply_tonemap wrote
    dst_attachment: Optional[torch.Tensor] = None        # int32 [H, W] out
    color_format: int = 0                                # the tonemap's output_format
    outline_color: tuple = (1.0, 0.53, 0.0, 1.0)
    dilate_radius: int = 8
    outline_width: int = 5
    occluded_mode: int = 2

    @staticmethod
    def mask_words(width: int, height: int, device="cuda") -> torch.Tensor:
        return torch.zeros((height, (width + 63) // 64), dtype=torch.int64, device=device)

    @staticmethod
    def over(visbuffer: torch.Tensor, transform_indices, meshlet_instance_count: int, depth: ImageAttachment, color: torch.Tensor, color_format: int = 0,
             **settings) -> "HighlightContext":
        """Both stages over a drawn visbuffer and a tonemapped image; allocates mask_bits and dst_attachment."""
        H, W = visbuffer.shape
        return HighlightContext(L.HIGHLIGHT_ALL, W, H, HighlightContext.mask_words(W, H, visbuffer.device), visbuffer_attachment=visbuffer,
                                transform_indices=transform_indices, meshlet_instance_count=meshlet_instance_count, depth_attachment=depth, color_attachment=color,
                                dst_attachment=torch.zeros_like(color), color_format=color_format, **settings)


def pack_sprite(render_flags: int, position_y: float, transform_id: int, material_id: int, distance: float) -> tuple:
    """RenderQueue2D::add (SceneGPU.hpp:532-545) through oxc_pack_sprite: the three words of one GPU::SpriteGPUData.  Host only."""
    out = L.Sprite()
    st = L.load().oxc_pack_sprite(int(render_flags), float(position_y), int(transform_id), int(material_id), float(distance), C.byref(out))
    if st != L.OXC_OK:
        raise L.OxcError(st, "oxc_pack_sprite")
    return out.material_id16_ypos16, out.flags16_distance16, out.transform_id


def sort_sprites(sprites):
    """RenderQueue2D::sort (SceneGPU.hpp:547) through oxc_sort_sprites: `sprites`, a C-contiguous numpy uint32 [n, 3] array, sorted in place --
    descending by distance bits, then by the y key of the SORT_Y sprites; stable.  Host only.  Returns the array."""
    assert sprites.dtype.name == "uint32" and sprites.ndim == 2 and sprites.shape[1] == 3 and sprites.flags.c_contiguous
    st = L.load().oxc_sort_sprites(sprites.ctypes.data_as(C.POINTER(L.Sprite)), sprites.shape[0])
    if st != L.OXC_OK:
        raise L.OxcError(st, "oxc_sort_sprites")
    return sprites


@dataclass
class SpriteContext(Marshalled):
    """oxc_sprite_context: the 2D block of the frame (RendererInstance.cpp:1080-1223; passes/2d_forward_vis.slang, passes/2d_forward.slang)
    over one DrawBatch2D.  `stages` selects the vis pass, the colour pass or both; `final_attachment` is the image apply_pbr wrote -- int32
    [H, W] (B10G11R11) or int16 [H, W, 4] (R16G16B16A16 Sfloat); `depth_attachment` is tested and written (include/oxcull.h, S1 - S7)."""
    _ctype = L.SpriteContext
    stages: int
    width: int
    height: int
    projection_view: tuple
    sprites_buffer: Optional[torch.Tensor]               # int32 [n, 3]: GPU::SpriteGPUData
    sprite_count: int
    transform_count: int
    depth_attachment: Optional[ImageAttachment]          # R32F, levels = 1, in/out
    materials_buffer: Optional[torch.Tensor] = None      # uint8 [material_count * 56]
    material_count: int = 0
    visbuffer_2d: Optional[torch.Tensor] = None          # int32 [H, W] out (vis)
    final_attachment: Optional[torch.Tensor] = None      # in/out (colour)
    source_format: int = 0
    first_sprite: int = 0
    clear: bool = True

    @staticmethod
    def create(sprites: torch.Tensor, materials: torch.Tensor, transform_count: int, projection_view, depth: ImageAttachment, final_attachment: torch.Tensor,
               stages: int = L.SPRITES_ALL, first_sprite: int = 0, sprite_count: Optional[int] = None, clear: bool = True) -> "SpriteContext":
        """Both stages over the depth and the lit image of a frame; allocates visbuffer_2d.  The format follows from the image's shape."""
        fmt = L.EYE_SOURCE_R16G16B16A16 if final_attachment.dim() == 3 else L.EYE_SOURCE_B10G11R11
        count = sprites.shape[0] - first_sprite if sprite_count is None else sprite_count
        vis = torch.full((depth.height, depth.width), -1, dtype=torch.int32, device=sprites.device)
        return SpriteContext(stages, depth.width, depth.height, tuple(float(v) for v in projection_view), sprites, count, transform_count, depth, materials,
                             materials.numel() * materials.element_size() // 56, vis, final_attachment, fmt, first_sprite, clear)


@dataclass
class SpritePickContext(Marshalled):
    """oxc_sprite_pick_context: the editor's mouse_picking_2d stage: texel `picking_texel` of `visbuffer_2d`, one u32 into `transform_id`."""
    _ctype = L.SpritePickContext
    _derived = {"x": lambda self: int(self.picking_texel[0]), "y": lambda self: int(self.picking_texel[1])}
    visbuffer_2d: torch.Tensor   # int32 [H, W]
    width: int
    height: int
    picking_texel: tuple
    transform_id: torch.Tensor   # int32 [1] out

    @staticmethod
    def over(visbuffer_2d: torch.Tensor, picking_texel, transform_id: Optional[torch.Tensor] = None) -> "SpritePickContext":
        out = torch.zeros(1, dtype=torch.int32, device=visbuffer_2d.device) if transform_id is None else transform_id
        return SpritePickContext(visbuffer_2d, visbuffer_2d.shape[1], visbuffer_2d.shape[0], tuple(picking_texel), out)


@dataclass
class VisbufferDecodeContext(Marshalled):
    """oxc_decode_context: RendererInstance::decode_visbuffer (Passes/DrawGeometry.cpp:192-274), the geometry and material-factor half of
    visbuffer_decode.slang.  `create` takes the visbuffer and the depth as oxc_draw_visbuffer resolved them, the matrix they were drawn with and
    the materials, and allocates the four G-buffer images; the scene buffers come from the renderer's prepared_frame."""
    _ctype = L.DecodeContext
    _derived = {"width": "depth_attachment.width", "height": "depth_attachment.height"}
    visbuffer_attachment: torch.Tensor            # int32 [H, W]
    depth_attachment: ImageAttachment             # R32F, levels = 1
    projection_view: list                         # column-major float[16]
    meshlet_instance_count: int
    materials_buffer: Optional[torch.Tensor]      # uint8 [material_count * 56] GPU::Material records (synth.pack_materials)
    material_count: int
    albedo_attachment: torch.Tensor               # int32 [H, W] out: R8G8B8A8 sRGB
    normal_attachment: torch.Tensor               # int16 [H, W, 4] out: R16G16B16A16 Sfloat bits, what the resolve and the ambient occlusion read
    emissive_attachment: torch.Tensor             # int32 [H, W] out: B10G11R11 UfloatPack32
    metallic_roughness_occlusion_attachment: torch.Tensor  # int32 [H, W] out: R8G8B8A8 Unorm
    clear: bool = True

    @staticmethod
    def create(visbuffer: torch.Tensor, depth, projection_view, meshlet_instance_count: int, materials: Optional[torch.Tensor] = None,
               clear: bool = True) -> "VisbufferDecodeContext":
        d = depth if isinstance(depth, ImageAttachment) else ImageAttachment.depth(depth)
        dev = d.data.device
        assert visbuffer.dtype == torch.int32 and tuple(visbuffer.shape) == (d.height, d.width) and visbuffer.is_contiguous()
        z32 = lambda: torch.zeros((d.height, d.width), dtype=torch.int32, device=dev)  # noqa: E731
        count = 0 if materials is None else materials.numel() * materials.element_size() // 56
        return VisbufferDecodeContext(visbuffer, d, [float(x) for x in projection_view], int(meshlet_instance_count), materials, count, z32(),
                                      torch.zeros((d.height, d.width, 4), dtype=torch.int16, device=dev), z32(), z32(), bool(clear))


# the five SamplingMode presets of Renderer.cpp:64-70 as oxc_material_sampler records {filter, address, mip_filter}; anisotropy is not sampled
SAMPLER_PRESETS = {"LinearRepeated": (1, 0, 1), "LinearClamped": (1, 1, 1), "NearestRepeated": (0, 0, 0), "NearestClamped": (0, 1, 0),
                   "LinearRepeatedAnisotropy": (1, 0, 1)}
_TEXEL_BYTES = {L.IMAGE_R8G8B8A8_UNORM: 4, L.IMAGE_R8G8B8A8_SRGB: 4, L.IMAGE_R8G8_UNORM: 2}


def pack_material_images(images, device="cuda") -> tuple:
    """`images`: [(levels, format)] with `levels` a list of uint8 arrays [h_k, w_k, 4] (or [h_k, w_k, 2] for IMAGE_R8G8_UNORM), level k of
    max(1, w >> k) x max(1, h >> k) texels -> (records uint8 [n * 144] on `device`, the texel tensors the records point into).  Each image
    is one allocation, its levels one behind the other, each 4-byte aligned.  Keep the second value alive while the records are used."""
    import numpy as np

    records, keep = (L.MaterialImage * max(1, len(images)))(), []
    for i, (levels, fmt) in enumerate(images):
        per = _TEXEL_BYTES[int(fmt)]
        h0, w0 = levels[0].shape[:2]
        blob, offsets = bytearray(), []
        for k, lvl in enumerate(levels):
            a = np.ascontiguousarray(lvl, dtype=np.uint8)
            assert a.shape == (max(1, h0 >> k), max(1, w0 >> k), per), (i, k, a.shape)
            offsets.append(len(blob))
            blob += a.tobytes() + bytes(-a.size % 4)
        t = torch.frombuffer(bytearray(blob), dtype=torch.uint8).to(device)
        keep.append(t)
        rec = records[i]
        rec.dptr, rec.width, rec.height, rec.levels, rec.format = t.data_ptr(), w0, h0, len(levels), int(fmt)
        rec.level_offset[:len(offsets)] = offsets
    raw = torch.frombuffer(bytearray(bytes(records)), dtype=torch.uint8)  # at least one record long: an empty table is an empty slice of it
    return raw[:144 * len(images)].to(device), keep


def pack_material_samplers(samplers, device="cuda") -> torch.Tensor:
    """[(filter, address, mip_filter)] or names of SAMPLER_PRESETS -> int32 [n, 4] oxc_material_sampler records on `device`."""
    rows = [list(SAMPLER_PRESETS[s] if isinstance(s, str) else s) + [0] for s in samplers]
    return torch.tensor(rows, dtype=torch.int32).reshape(-1, 4).to(device)


@dataclass
class MaterialImagesContext(Marshalled):
    """oxc_material_images: the image and sampler tables oxc_decode_visbuffer_textured samples through (the engine's global_images and
    global_samplers) and the camera position its tangent frame reads.  `images_buffer` holds oxc_material_image records
    (pack_material_images), `samplers_buffer` oxc_material_sampler records (pack_material_samplers); either may be None with its count 0."""
    _ctype = L.MaterialImages
    camera_position: tuple
    images_buffer: Optional[torch.Tensor] = None    # uint8 [image_count * 144]
    samplers_buffer: Optional[torch.Tensor] = None  # int32 [sampler_count, 4]
    image_count: int = 0
    sampler_count: int = 0

    @staticmethod
    def create(camera_position, images_buffer=None, samplers_buffer=None) -> "MaterialImagesContext":
        n = lambda t, size: 0 if t is None else t.numel() * t.element_size() // size  # noqa: E731
        return MaterialImagesContext(tuple(float(v) for v in camera_position), images_buffer, samplers_buffer, n(images_buffer, 144), n(samplers_buffer, 16))


@dataclass
class MainGeometryContext(Marshalled):
    """The fields generate_hiz uses (RendererInstance.hpp:199-216)."""
    _ctype = L.MainGeometryContext
    _leave = ("_pad",)
    depth_attachment: ImageAttachment
    hiz_attachment: ImageAttachment


# the oxc_debug_*_stats read-backs: RendererInstance.debug_<key>_stats -> (symbol, the u32 counters in the library's order)
_STATS = {
    "raster": ("oxc_debug_raster_stats", ("big", "clipped", "tiles", "overflowed_segments")),
    "terrain_draw": ("oxc_debug_terrain_draw_stats", ("patches_drawn", "patches_discarded", "patches_skipped", "triangles", "set_up", "clipped", "big", "fragments")),
    "visbuffer_decode": ("oxc_debug_visbuffer_decode_stats", ("decoded", "empty", "zero_vertex_index", "default_material")),
    "visbuffer_decode_textured": ("oxc_debug_visbuffer_decode_textured_stats", ("decoded", "empty", "zero_vertex_index", "default_material", "sampled_albedo",
                                                                                "sampled_normal", "sampled_emissive", "sampled_metallic_roughness",
                                                                                "sampled_occlusion", "level_taps", "jacobian_zero", "uniform_waves",
                                                                                "per_lane_waves")),
    "vsm_draw": ("oxc_debug_vsm_draw_stats", ("pairs", "fragments", "big_pairs", "big_pairs_overflowed", "tiles", "tiles_overflowed", "clipped_pairs",
                                              "clipped_pairs_overflowed")),
    "vsm_resolve": ("oxc_debug_vsm_resolve_stats", ("non_sky_pixels", "taps", "misses", "fallback_minus", "fallback_plus", "hard", "no_blocker",
                                                    "all_blockers")),
    "contact_shadows": ("oxc_debug_contact_shadows_stats", ("non_sky_pixels", "taps", "miss", "hit_zero", "hit_partial", "hit_one", "rejected", "n_lower",
                                                            "n_between", "n_upper", "end_clip", "start_moved")),
    "ambient_occlusion": ("oxc_debug_ambient_occlusion_stats", ("non_sky_pixels", "samples", "mip0", "mip1", "mip2", "mip3", "mip4", "fractional",
                                                                "result_one", "result_partial", "result_zero", "zero_width", "sign_minus", "sign_zero",
                                                                "sign_plus")),
    "pbr_apply": ("oxc_debug_pbr_apply_stats", ("transparent_empty", "sky", "fallthrough_empty", "lit_nol_positive", "lit_nol_zero", "light_kind_skipped",
                                                "light_attenuation_out", "light_ndotl_out", "light_shaded")),
    "fxaa": ("oxc_debug_fxaa_stats", ("early_out", "searched", "search_taps", "ran_all_steps")),
}


class RendererInstance:
    """Owns one oxc_ctx on one device."""

    def __init__(self, device_index: int = 0, lib_path: str = None):
        self._lib = L.load(lib_path)
        if not torch.cuda.is_available():
            raise RuntimeError("oxylus_amd.RendererInstance needs a GPU: the cull path has no CPU fallback")
        self.device_index = device_index
        self._ctx = C.c_void_p()
        st = self._lib.oxc_create(device_index, C.byref(self._ctx))
        if st != L.OXC_OK:
            raise L.OxcError(st, "oxc_create failed")
        self.prepared_frame: Optional[PreparedFrame] = None

    def close(self):
        if self._ctx:
            self._lib.oxc_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, st: int):
        if st != L.OXC_OK:
            raise L.OxcError(st, self._lib.oxc_last_error(self._ctx).decode())

    @staticmethod
    def _stream(stream) -> C.c_void_p:
        s = stream if stream is not None else torch.cuda.current_stream()
        return C.c_void_p(s.cuda_stream)

    def reserve(self, max_mesh_instances: int, max_meshlet_instances: int):
        self._check(self._lib.oxc_reserve(self._ctx, max_mesh_instances, max_meshlet_instances))

    def _call(self, symbol: str, context, stream, *, frame=False, c=None):
        """One pass over its context: oxc_<pass>(ctx, [prepared frame,] context, stream).  `frame`: True passes the prepared frame, which
        must exist; "optional" passes it when there is one and NULL otherwise.  The context stays referenced in `_keep`, so its tensors
        outlive the launches the call enqueued."""
        args = [self._ctx]
        if frame:
            assert frame == "optional" or self.prepared_frame is not None
            args.append(C.byref(self.prepared_frame.c()) if self.prepared_frame is not None else None)
        args.append(C.byref(context.c() if c is None else c))
        self._keep = context
        self._check(getattr(self._lib, symbol)(*args, self._stream(stream)))

    def generate_hiz(self, context: MainGeometryContext, stream=None):
        self._check(self._lib.oxc_generate_hiz(self._ctx, C.byref(context.c()), self._stream(stream)))

    def cull_geometry(self, context: CullGeometryContext, stream=None):
        assert self.prepared_frame is not None
        f = self.prepared_frame.c()
        self._check(self._lib.oxc_cull_geometry(self._ctx, C.byref(f), C.byref(context.c()), self._stream(stream)))

    def join_triangles(self, stream=None):
        """`stream` waits for every triangle stage still in flight on the context's own stream (async_triangles)."""
        self._check(self._lib.oxc_join_triangles(self._ctx, self._stream(stream)))

    def cull_geometry_batch(self, frames, contexts, stream=None):
        """Batched cull of independent (PreparedFrame, CullGeometryContext) pairs (oxc_cull_geometry_batch).
        The contexts' output buffers are updated like cull_geometry does."""
        n = len(frames)
        assert n == len(contexts) and n > 0
        cf = (L.PreparedFrame * n)(*[f.c() for f in frames])
        cc = (L.CullGeometryContext * n)(*[c.c() for c in contexts])
        self._check(self._lib.oxc_cull_geometry_batch(self._ctx, n, cf, cc, self._stream(stream)))
        for i, c in enumerate(contexts):
            for name in ("visibility_buffer", "cull_meshlets_cmd_buffer", "cull_triangles_cmd_buffer", "draw_geometry_cmd_buffer"):
                setattr(c._c, name, getattr(cc[i], name))

    def seed_meshlet_instances(self, context: CullGeometryContext, total: int, stream=None):
        self._check(self._lib.oxc_seed_meshlet_instances(self._ctx, C.byref(context.c()), total, self._stream(stream)))

    def read_counters(self, context: CullGeometryContext, stream=None) -> L.Counters:
        out = L.Counters()
        self._check(self._lib.oxc_read_counters(self._ctx, C.byref(context._c), C.byref(out), self._stream(stream)))
        return out

    def stream_read_probe(self, t: torch.Tensor, stream=None):
        self._check(self._lib.oxc_stream_read_probe(self._ctx, C.c_void_p(t.data_ptr()), t.numel() * t.element_size(), self._stream(stream)))

    def debug_decode_bounds(self, bounds: torch.Tensor) -> torch.Tensor:
        n = bounds.shape[0]
        out = torch.empty((n, 10), dtype=torch.float32, device=bounds.device)
        self._check(self._lib.oxc_debug_decode_bounds(self._ctx, C.c_void_p(bounds.data_ptr()), n, C.c_void_p(out.data_ptr()), self._stream(None)))
        return out

    def build_meshlet_bounds(self, positions: torch.Tensor, meshlets: torch.Tensor, vidx: torch.Tensor, micro: torch.Tensor,
                             quantize_positions: bool = True, stream=None):
        """SURVEY 8(f)-1, AssetManager_GLTF.cpp:573-578,683-744: positions f32 [V,3], meshlets i32 [M,4] (GPU::Meshlet),
        vidx i32, micro u8 -> (MeshletBounds as i16 [M,8], mesh bounds f32 [6] = center xyz + extent xyz, u16x4 positions as i16 [V,4])."""
        dev = positions.device
        V, M = positions.shape[0], meshlets.shape[0]
        bounds = torch.empty((M, 8), dtype=torch.int16, device=dev)
        mesh6 = torch.empty(6, dtype=torch.float32, device=dev)
        qpos = torch.empty((V, 4), dtype=torch.int16, device=dev) if quantize_positions else None

        def buf(t):
            return L.Buffer(C.c_void_p(t.data_ptr()), t.numel() * t.element_size()) if t is not None and t.numel() else L.Buffer(None, 0)

        d = L.MeshletBoundsDesc()
        d.struct_size = C.sizeof(L.MeshletBoundsDesc)
        d.vertex_count, d.meshlet_count = V, M
        d.positions, d.meshlets = buf(positions), buf(meshlets)
        d.indirect_vertex_indices, d.local_triangle_indices = buf(vidx), buf(micro)
        d.meshlet_bounds, d.mesh_bounds, d.quantized_positions = buf(bounds), buf(mesh6), buf(qpos)
        self._keep = (positions, meshlets, vidx, micro)
        self._check(self._lib.oxc_build_meshlet_bounds(self._ctx, C.byref(d), self._stream(stream)))
        return bounds, mesh6, qpos

    def quantize_vertex_streams(self, positions: torch.Tensor = None, normals: torch.Tensor = None, texcoords: torch.Tensor = None, stream=None):
        """AssetManager_GLTF.cpp:570-588: f32 [V,3] positions -> i16 [V,4] (u16x4 halfs), f32 [V,3] normals -> i32 [V] (10:10:10),
        f32 [V,2] texcoords -> i16 [V,2]; absent streams come back as None."""
        given = [t for t in (positions, normals, texcoords) if t is not None]
        if not given:
            return None, None, None
        dev, V = given[0].device, given[0].shape[0]
        qpos = torch.empty((V, 4), dtype=torch.int16, device=dev) if positions is not None else None
        qnrm = torch.empty(V, dtype=torch.int32, device=dev) if normals is not None else None
        quv = torch.empty((V, 2), dtype=torch.int16, device=dev) if texcoords is not None else None

        def buf(t):
            return L.Buffer(C.c_void_p(t.data_ptr()), t.numel() * t.element_size()) if t is not None and t.numel() else L.Buffer(None, 0)

        d = L.VertexStreamsDesc()
        d.struct_size, d.vertex_count = C.sizeof(L.VertexStreamsDesc), V
        d.positions, d.normals, d.texcoords = buf(positions), buf(normals), buf(texcoords)
        d.quantized_positions, d.quantized_normals, d.quantized_texcoords = buf(qpos), buf(qnrm), buf(quv)
        self._keep = (positions, normals, texcoords)
        self._check(self._lib.oxc_quantize_vertex_streams(self._ctx, C.byref(d), self._stream(stream)))
        return qpos, qnrm, quv

    def generate_hpb(self, page_table: torch.Tensor, hpb: "HpbAttachment", stream=None):
        """SURVEY 8(f)-3, Shadowmaps.cpp:331-366: page_table int32 [layers, h, w] -> every level of `hpb`."""
        im = hpb.c()
        self._keep = (page_table, hpb)
        self._check(self._lib.oxc_generate_hpb(self._ctx, L.Buffer(C.c_void_p(page_table.data_ptr()), page_table.numel() * 4), C.byref(im), self._stream(stream)))

    def update_virtual_shadowmap(self, context: VirtualShadowmapContext, stream=None):
        """Shadowmaps.cpp:143-421: sun_moved clear, reset, invalidate, mark, free, free list, allocate, HPB, mark dirty, clear dirty
        pages (include/oxcull.h, oxc_update_virtual_shadowmap)."""
        self._call("oxc_update_virtual_shadowmap", context, stream)

    def cull_terrain(self, cull_flags: int, cull_camera, world_min, world_size, patch_count, base_height: float, height_scale: float,
                     patch_minmax: torch.Tensor, mask: torch.Tensor, hiz: "ImageAttachment" = None, stream=None):
        """SURVEY 8(f)-4, Terrain.cpp:159-216 + terrain_cull.slang: patch_minmax f32 [py, px, 2], mask int32 [ceil(total/32)] (in/out).
        Returns (visible_patches int32 [count], count)."""
        pcx, pcy = int(patch_count[0]), int(patch_count[1])
        total = pcx * pcy
        visible = torch.full((max(total, 1),), -1, dtype=torch.int32, device=patch_minmax.device)
        c = L.TerrainContext()
        c.struct_size = C.sizeof(L.TerrainContext)
        c.cull_flags = cull_flags
        c.cull_camera = cull_camera
        c.world_min[0], c.world_min[1] = float(world_min[0]), float(world_min[1])
        c.world_size[0], c.world_size[1] = float(world_size[0]), float(world_size[1])
        c.patch_count[0], c.patch_count[1] = pcx, pcy
        c.base_height, c.height_scale = float(base_height), float(height_scale)
        mm = L.Image()
        mm.dptr, mm.width, mm.height, mm.levels = patch_minmax.data_ptr(), pcx, pcy, 1
        c.patch_minmax_attachment = mm
        if hiz is not None:
            c.hiz_attachment = hiz.c()
        c.visible_patches_buffer = L.Buffer(C.c_void_p(visible.data_ptr()), visible.numel() * 4)
        c.patch_visibility_mask_buffer = L.Buffer(C.c_void_p(mask.data_ptr()), mask.numel() * 4)
        self._keep = (patch_minmax, mask, visible, hiz)
        self._check(self._lib.oxc_cull_terrain(self._ctx, C.byref(c), self._stream(stream)))
        host = (C.c_uint32 * 4)()
        self._check(self._lib.oxc_debug_read_u32(self._ctx, c.draw_cmd_buffer.dptr, 4, C.cast(host, C.c_void_p), self._stream(stream)))
        cmd_host = list(host)
        return visible[: cmd_host[1]].clone(), cmd_host

    def draw_visbuffer(self, context: CullGeometryContext, projection_view, width: int, height: int, visdepth: torch.Tensor, clear: bool,
                       depth: "ImageAttachment" = None, visbuffer: torch.Tensor = None, stream=None, draw_cmd: torch.Tensor = None):
        """SURVEY 8(f)-2, DrawGeometry.cpp:104-190: rasterise the triangles the last cull_geometry(context) emitted into
        `visdepth` (int64 [h, w]: depth bits << 32 | vis); optional resolves into `depth` (ImageAttachment, levels = 1) and
        `visbuffer` (int32 [h, w]).  `draw_cmd` (int32 [5], VkDrawIndexedIndirectCommand) replaces the context's own command:
        draw a caller-written `reordered_indices_buffer`."""
        assert self.prepared_frame is not None
        f = self.prepared_frame.c()
        d = L.DrawContext()
        d.struct_size = C.sizeof(L.DrawContext)
        d.wide_triangle_index = int(context.wide_triangle_index)
        d.clear = 1 if clear else 0
        d.width, d.height = width, height
        for i in range(16):
            d.projection_view[i] = float(projection_view[i])
        d.draw_geometry_cmd_buffer = context._c.draw_geometry_cmd_buffer if draw_cmd is None else L.Buffer(C.c_void_p(draw_cmd.data_ptr()), draw_cmd.numel() * 4)
        d.visdepth_buffer = L.Buffer(C.c_void_p(visdepth.data_ptr()), visdepth.numel() * 8)
        if depth is not None:
            d.depth_attachment = depth.c()
        if visbuffer is not None:
            d.visbuffer_attachment = L.Buffer(C.c_void_p(visbuffer.data_ptr()), visbuffer.numel() * 4)
        self._keep = (visdepth, depth, visbuffer, draw_cmd)
        self._check(self._lib.oxc_draw_visbuffer(self._ctx, C.byref(f), C.byref(d), self._stream(stream)))

    def decode_visbuffer(self, context: VisbufferDecodeContext, stream=None):
        """Passes/DrawGeometry.cpp:192-274 (visbuffer_decode): per pixel the triangle behind the visbuffer texel, its perspective-correct
        barycentrics, the interpolated vertex normal and the material factors, into the four G-buffer images of `context`
        (include/oxcull.h, oxc_decode_visbuffer)."""
        self._call("oxc_decode_visbuffer", context, stream, frame=True)

    def decode_visbuffer_textured(self, context: VisbufferDecodeContext, images: "MaterialImagesContext", stream=None):
        """The whole of visbuffer_decode.slang: decode_visbuffer with the five material images sampled through `images` -- texcoords,
        gradients, the tangent frame, SampleGrad by the stated rule, the normal map (include/oxcull.h, oxc_decode_visbuffer_textured).  One
        launch; with no image flag set the outputs are decode_visbuffer's."""
        assert self.prepared_frame is not None
        self._keep = (context, images)
        self._check(self._lib.oxc_decode_visbuffer_textured(self._ctx, C.byref(self.prepared_frame.c()), C.byref(context.c()), C.byref(images.c()),
                                                            self._stream(stream)))

    def debug_visbuffer_decode_textured_stats(self, stream=None) -> dict:
        """What the last decode_visbuffer_textured did, after debug_set_tuning(L.TUNE_VISBUFFER_DECODE_TEXTURED_STATS, 1) (measurement hook;
        synchronises)."""
        return self._read_stats("visbuffer_decode_textured", stream)

    def debug_visbuffer_decode_stats(self, stream=None) -> dict:
        """What the last decode_visbuffer did, after debug_set_tuning(L.TUNE_VISBUFFER_DECODE_STATS, 1) (measurement hook; synchronises)."""
        return self._read_stats("visbuffer_decode", stream)

    def draw_physical_pages(self, context: VsmDrawContext, stream=None):
        """Shadowmaps.cpp:466-754 (rmvsm_build_draw_commands + rmvsm_draw_physical_pages): rasterise the shadow cull's triangles once per
        dirty clipmap into the dirty physical pages of `context.physical_page_image` (include/oxcull.h, oxc_draw_physical_pages)."""
        self._call("oxc_draw_physical_pages", context, stream, frame=True)

    def resolve_shadowmap(self, context: ShadowResolveContext, stream=None):
        """Shadowmaps.cpp:756-822 (resolve_shadowmaps): the PCSS light-visibility value of every pixel from the page table and the physical
        pages into `context.resolved_shadows_attachment` (include/oxcull.h, oxc_resolve_shadowmap)."""
        self._call("oxc_resolve_shadowmap", context, stream)

    def apply_pbr(self, context: PBRContext, stream=None):
        """Passes/PBR.cpp:313-534, the no-atmosphere branch (pbr_apply_no_atmos): per pixel the G-buffer, the ambient occlusion, the two shadow
        terms, the sun and the point / spot lights become the lit HDR colour in `context.final_attachment` (include/oxcull.h, oxc_apply_pbr).
        L.SCENE_HAS_ATMOSPHERE in the flags is refused: that branch is apply_pbr_atmosphere."""
        self._call("oxc_apply_pbr", context, stream)

    def apply_pbr_atmosphere(self, context: PBRAtmosphereContext, stream=None):
        """Passes/PBR.cpp:318-434, the atmosphere branch (pbr_apply): apply_pbr's G-buffer, shadow terms and lights under the sun's colour from
        the transmittance LUT, the sky cube as the ambient term, aerial perspective on lit pixels, and the sky-view LUT with the sun disc on
        empty ones, one launch (include/oxcull.h, oxc_apply_pbr_atmosphere).  After generate_sky_luts, draw_atmosphere and generate_sky_ibl."""
        self._call("oxc_apply_pbr_atmosphere", context, stream)

    def apply_eye_adaptation(self, context: EyeAdaptationContext, delta_time: float = 0.0, stream=None):
        """Passes/PostProcess.cpp:7-77: the 256-bin log-luminance histogram of `context.final_attachment` into `context.histogram_buffer` and
        the adapted luminance and exposure it gives into `context.exposure_buffer` (include/oxcull.h, oxc_apply_eye_adaptation).  time_coeff
        is `context.time_coeff` where set, else 1 - exp(-adaptation_speed * delta_time)."""
        self._call("oxc_apply_eye_adaptation", context, stream, c=context.c(delta_time))

    def apply_bloom(self, context: BloomContext, stream=None):
        """Passes/PostProcess.cpp:79-203: the thresholded half-resolution image and its downsample pyramid into
        `context.bloom_downsampled_attachment`, the upsample pyramid into `context.bloom_upsampled_attachment` (include/oxcull.h,
        oxc_apply_bloom).  The exposure is the second word of `context.exposure_buffer` with L.SCENE_HAS_EYE_ADAPTATION, else 1."""
        self._call("oxc_apply_bloom", context, stream)

    def apply_tonemap(self, context: TonemapContext, stream=None):
        """Passes/PostProcess.cpp:205-247: exposure, bloom composite, tone curve, lens effects and the 8-bit store of `context.final_attachment`
        into `context.dst_attachment`, one launch (include/oxcull.h, oxc_apply_tonemap)."""
        self._call("oxc_apply_tonemap", context, stream)

    def apply_fxaa(self, context: FxaaContext, scene_flags: int = L.SCENE_HAS_FXAA, stream=None) -> torch.Tensor:
        """RendererInstance.cpp:1225-1255: with L.SCENE_HAS_FXAA in `scene_flags`, edge anti-aliasing of `context.final_attachment` into
        `context.fxaa_attachment`, one launch (include/oxcull.h, oxc_apply_fxaa); without it nothing runs.  Returns the image the eye
        adaptation, the bloom and the tonemap read: fxaa_attachment when the pass ran, final_attachment otherwise, as the reference hands it on."""
        if not int(scene_flags) & L.SCENE_HAS_FXAA:
            return context.final_attachment
        self._call("oxc_apply_fxaa", context, stream)
        return context.fxaa_attachment

    def generate_sky_luts(self, context: SkyLutContext, stream=None) -> None:
        """RendererInstance.cpp:136-251, the pair the reference builds in its constructor: sky_transmittance_lut, then sky_multiscatter_lut from
        it, two launches (include/oxcull.h, oxc_generate_sky_luts).  Called again whenever the Atmosphere record changes."""
        self._call("oxc_generate_sky_luts", context, stream)

    def draw_atmosphere(self, context: AtmosphereContext, stream=None) -> None:
        """Passes/PBR.cpp:9-141 without the sky_ibl pass: sky_view_lut and sky_aerial_perspective_lut from the two LUTs of generate_sky_luts, the
        sun and the camera, two launches (include/oxcull.h, oxc_draw_atmosphere)."""
        self._call("oxc_draw_atmosphere", context, stream)

    def generate_sky_ibl(self, context: SkyIblContext, stream=None) -> None:
        """Passes/PBR.cpp:52-94, the sky_ibl pass of draw_atmosphere: 64 samples of sky_view_lut per cube texel, blended into the texel's own
        history, one launch (include/oxcull.h, oxc_generate_sky_ibl).  After draw_atmosphere; `context.frame_index` is the caller's to advance."""
        self._call("oxc_generate_sky_ibl", context, stream)

    def apply_terrain_brush(self, context: TerrainBrushContext, stream=None) -> None:
        """Passes/Terrain.cpp:35-132 (terrain_brush_trace, terrain_brush_apply): the stages of context.stages in the order trace, apply
        (include/oxcull.h, oxc_apply_terrain_brush).  `context.region` is the record generate_terrain_maps reads for the regional re-bake."""
        self._call("oxc_apply_terrain_brush", context, stream)

    def decode_terrain(self, context: TerrainDecodeContext, stream=None) -> None:
        """Passes/Terrain.cpp:279-360 (terrain_decode): the four G-buffer images at the terrain pixels, one launch (include/oxcull.h,
        oxc_decode_terrain).  After decode_visbuffer on the same attachments; every other pixel keeps its bytes."""
        self._call("oxc_decode_terrain", context, stream)

    def draw_terrain_for_visbuffer(self, context: TerrainDrawContext, stream=None) -> None:
        """Passes/Terrain.cpp:218-277 (terrain_visbuffer): the visible patches, tessellated by the stated rules T1 - T7, into
        `context.visdepth_buffer` (include/oxcull.h, oxc_draw_terrain).  After draw_visbuffer on the same image, without `clear`."""
        self._call("oxc_draw_terrain", context, stream)

    def debug_terrain_draw_stats(self, stream=None) -> dict:
        """What the last draw_terrain_for_visbuffer did with its patches and triangles (test hook; synchronises); `fragments` only after
        debug_set_tuning(L.TUNE_TERRAIN_DRAW_STATS, 1)."""
        return self._read_stats("terrain_draw", stream)

    def apply_debug_view(self, context: DebugViewContext, stream=None) -> None:
        """Passes/Debug.cpp:9-153 (debug_view, rmvsm_debug): the picture of `context.debug_view` into `context.debug_attachment`, one launch
        (include/oxcull.h, oxc_apply_debug_view).  The prepared frame is passed when there is one; only the Materials, MeshInstances and
        MeshLods views read it."""
        self._call("oxc_apply_debug_view", context, stream, frame="optional")

    def pick_transform(self, context: PickingContext, stream=None) -> None:
        """ViewportPanel.cpp:1439-1497 (mouse_picking): the transform index behind `context.picking_texel` into `context.transform_id`, one
        launch (include/oxcull.h, oxc_pick_transform)."""
        self._call("oxc_pick_transform", context, stream, frame=True)

    def apply_highlight(self, context: HighlightContext, stream=None) -> None:
        """ViewportPanel.cpp:1166-1345 (highlight_mask_stage, highlight_composite_stage): the stages of `context.stages`, one launch each
        (include/oxcull.h, oxc_apply_highlight).  The prepared frame is passed when there is one; only the mask stage needs it."""
        self._call("oxc_apply_highlight", context, stream, frame="optional")

    def draw_sprites(self, context: "SpriteContext", stream=None) -> None:
        """RendererInstance.cpp:1080-1223 (2d_forward_vis_pass, 2d_forward_pass): the stages of `context.stages` over one batch of sprites,
        between apply_pbr and apply_fxaa (include/oxcull.h, oxc_draw_sprites).  The world matrices come from the prepared frame."""
        self._call("oxc_draw_sprites", context, stream, frame=True)

    def pick_sprite(self, context: "SpritePickContext", stream=None) -> None:
        """editor/mouse_picking_2d.slang: texel `context.picking_texel` of visbuffer_2d into `context.transform_id`."""
        self._call("oxc_pick_sprite", context, stream)

    pack_sprite = staticmethod(lambda *a, **k: pack_sprite(*a, **k))
    sort_sprites = staticmethod(lambda *a, **k: sort_sprites(*a, **k))

    def generate_terrain_maps(self, context: TerrainMapsContext, stream=None) -> None:
        """Scene/Terrain.cpp:406-461 and Passes/Terrain.cpp:134-156 (terrain_generate, terrain_derive, terrain_minmax): the stages of
        `context.stages` in that order, one launch each: heightmap and ridgemap, normalmap and splatmap, patch_minmax (include/oxcull.h,
        oxc_generate_terrain_maps).  `context.patch_minmax` is what cull_terrain reads."""
        self._call("oxc_generate_terrain_maps", context, stream)

    def debug_fxaa_stats(self, stream=None) -> dict:
        """What the last apply_fxaa did, after debug_set_tuning(L.TUNE_FXAA_STATS, 1) (measurement hook; synchronises)."""
        return self._read_stats("fxaa", stream)

    def debug_pbr_apply_stats(self, stream=None) -> dict:
        """What the last apply_pbr did, after debug_set_tuning(L.TUNE_PBR_APPLY_STATS, 1) (measurement hook; synchronises)."""
        return self._read_stats("pbr_apply", stream)

    def _read_stats(self, key: str, stream) -> dict:
        """One of the oxc_debug_*_stats read-backs (_STATS): its u32 counters under their names."""
        symbol, names = _STATS[key]
        out = (C.c_uint32 * len(names))()
        self._check(getattr(self._lib, symbol)(self._ctx, C.cast(out, C.c_void_p), self._stream(stream)))
        return {k: int(v) for k, v in zip(names, out)}

    def debug_vsm_resolve_stats(self, stream=None) -> dict:
        """What the last resolve_shadowmap did, after debug_set_tuning(L.TUNE_VSM_RESOLVE_STATS, 1) (measurement hook; synchronises)."""
        return self._read_stats("vsm_resolve", stream)

    def contact_shadows(self, context: ContactShadowsContext, stream=None):
        """RendererInstance.cpp:990-1020 (contact_shadows): per pixel a short ray towards the sun marched through the depth image, the
        shadow term into `context.contact_shadows_attachment` (include/oxcull.h, oxc_contact_shadows)."""
        self._call("oxc_contact_shadows", context, stream)

    def debug_contact_shadows_stats(self, stream=None) -> dict:
        """What the last contact_shadows did, after debug_set_tuning(L.TUNE_CONTACT_SHADOWS_STATS, 1) (measurement hook; synchronises)."""
        return self._read_stats("contact_shadows", stream)

    def generate_ambient_occlusion(self, context: AmbientOcclusionContext, stream=None):
        """Passes/PBR.cpp:179-311 (vbgtao_prefilter, vbgtao_main, vbgtao_denoise): the ambient occlusion term pbr_apply reads, into
        `context.ambient_occlusion_attachment` as binary16 (include/oxcull.h, oxc_generate_ambient_occlusion)."""
        self._call("oxc_generate_ambient_occlusion", context, stream)

    def debug_ambient_occlusion_stats(self, stream=None) -> dict:
        """What the last generate_ambient_occlusion did, after debug_set_tuning(L.TUNE_AMBIENT_OCCLUSION_STATS, 1) (measurement hook;
        synchronises)."""
        return self._read_stats("ambient_occlusion", stream)

    def debug_vsm_draw_stats(self, stream=None) -> dict:
        """What the last draw_physical_pages did (measurement hook; synchronises).  `pairs` / `fragments` are counted only with
        debug_set_tuning(L.TUNE_VSM_DRAW_STATS, 1)."""
        return self._read_stats("vsm_draw", stream)

    def debug_raster_stats(self, stream=None) -> dict:
        """What the last draw_visbuffer did with its triangles (test hook; synchronises)."""
        return self._read_stats("raster", stream)

    def debug_set_tuning(self, knob: int, value: int):
        """Harness knobs (L.TUNE_*): async stage grid caps, the raster queues' capacity (before the first draw), the bounds producer's grid cap and chunk."""
        self._check(self._lib.oxc_debug_set_tuning(self._ctx, knob, value))

    def debug_count_occlusion_candidates(self, counters):
        """Measurement aid (include/oxcull.h): `counters` = int32 CUDA tensor of 256 * 64 zeros (or None to switch it off); the HiZ calls that follow
        run the counting instantiations of their meshlet test, which add the candidates that reach test_occlusion to it (sum = the count)."""
        self._check(self._lib.oxc_debug_count_occlusion_candidates(self._ctx, C.c_void_p(counters.data_ptr()) if counters is not None else None))

    def debug_shared_tests_mode(self) -> int:
        """What share_pass_tests did in the last cull_geometry call: 0 tested on its own, 1 early call that published, 2 late call that reused,
        3 late call that reused and needed no prepare kernel."""
        return int(self._lib.oxc_debug_shared_tests_mode(self._ctx))

    def debug_tri_loads_mode(self) -> int:
        """1 = the last call's triangle kernels used nt loads, 2 = plain loads (shared geometry), 0 = no triangle stage ran."""
        return int(self._lib.oxc_debug_tri_loads_mode(self._ctx))

    def debug_project_aabb(self, mvp16, near_clip: float, boxes6: torch.Tensor) -> torch.Tensor:
        """boxes6 f32 [n, 6] = {center.xyz, extent.xyz} -> f32 [n, 7] = {min.u, min.v, min.z, max.u, max.v, max.z, valid}."""
        n = boxes6.shape[0]
        out = torch.empty((n, 7), dtype=torch.float32, device=boxes6.device)
        m = (C.c_float * 16)(*[float(v) for v in mvp16])
        self._check(self._lib.oxc_debug_project_aabb(self._ctx, m, float(near_clip), C.c_void_p(boxes6.data_ptr()), n, C.c_void_p(out.data_ptr()), self._stream(None)))
        return out

    # ---- multi-GPU exchange through the C ABI (RCCL): SURVEY 8e ----
    def comm_unique_id(self) -> bytes:
        buf = C.create_string_buffer(128)
        self._check(self._lib.oxc_comm_unique_id(self._ctx, buf))
        return buf.raw

    def comm_init(self, unique_id: bytes, rank: int, world: int):
        assert len(unique_id) == 128
        self._check(self._lib.oxc_comm_init(self._ctx, C.c_char_p(unique_id), rank, world))
        self._comm_world = world

    def comm_destroy(self):
        self._check(self._lib.oxc_comm_destroy(self._ctx))

    def pack_counters(self, context: CullGeometryContext, counts4: torch.Tensor, stream=None):
        """{emitted, early, late, index_count} of the context's last call -> counts4 (int32 [4], device), on the stream."""
        self._check(self._lib.oxc_pack_counters(self._ctx, C.byref(context._c), C.c_void_p(counts4.data_ptr()), self._stream(stream)))

    def exchange_counts(self, counts4: torch.Tensor, stream=None) -> torch.Tensor:
        """counts4: int32 [4] on the device -> int32 [world, 4] (all-gather on the stream)."""
        out = torch.empty((self._comm_world, 4), dtype=torch.int32, device=counts4.device)
        self._keep = (counts4, out)
        self._check(self._lib.oxc_exchange_counts(self._ctx, C.c_void_p(counts4.data_ptr()), C.c_void_p(out.data_ptr()), self._stream(stream)))
        return out

    def broadcast_hiz(self, hiz: "ImageAttachment", root: int, stream=None, first_level: int = 0):
        """Every level (first_level = 0) or only the top of the pyramid, levels >= first_level (the rest is built locally)."""
        im = hiz.c()
        if first_level:
            self._check(self._lib.oxc_broadcast_hiz_levels(self._ctx, C.byref(im), first_level, hiz.data.numel() * 4, root, self._stream(stream)))
        else:
            self._check(self._lib.oxc_broadcast_hiz(self._ctx, C.byref(im), hiz.data.numel() * 4, root, self._stream(stream)))

    def profile_begin(self):
        self._check(self._lib.oxc_profile_begin(self._ctx))

    def profile_end(self) -> dict:
        kt = L.KernelTimes()
        self._check(self._lib.oxc_profile_end(self._ctx, C.byref(kt)))
        out = {"empty_pair_ms": kt.empty_pair_ms, "kernels": {}}
        for i, name in enumerate(L.KERNEL_NAMES):
            if kt.launches[i]:
                out["kernels"][name] = {"launches": int(kt.launches[i]), "total_ms": float(kt.total_ms[i])}
        return out
