"""ctypes binding of liboxcull.so (the C ABI in include/oxcull.h).

The product path has no CPU fallback: if the HIP library is missing or fails to load this
module raises, it never routes to oracle/.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "liboxcull.so")
CSRC_DIR = os.path.join(_HERE, "csrc")

OXC_OK, OXC_INVALID_ARG, OXC_HIP_ERROR, OXC_RCCL_ERROR, OXC_OUT_OF_MEMORY = range(5)
ABI_VERSION = 5  # OXC_ABI_VERSION of include/oxcull.h

CULL_TEST_FRUSTUM = 1
CULL_SELECT_LOD = 2
CULL_TEST_OCCLUSION = 4
CULL_LATE_PASS = 8
CULL_TEST_ALL = 7

STAGE_MESHES = 1
STAGE_MESHLETS = 2
STAGE_TRIANGLES = 4
STAGE_ALL = 7

TUNE_ASYNC_MTEST_BLOCKS_PER_CU, TUNE_ASYNC_TRI_BLOCKS_PER_CU, TUNE_RASTER_BIG_CAPACITY, TUNE_TRI_BLOCKS_PER_CU, TUNE_MV_EXPAND_ASYNC, TUNE_TRI_LOADS = 0, 1, 2, 3, 5, 7  # oxc_debug_set_tuning knobs
TUNE_VSM_DRAW_STATS, TUNE_VSM_DRAW_CAPACITY, TUNE_VSM_RESOLVE_STATS, TUNE_CONTACT_SHADOWS_STATS, TUNE_AMBIENT_OCCLUSION_STATS = 8, 9, 10, 11, 12
TUNE_VISBUFFER_DECODE_STATS = 13
TUNE_PBR_APPLY_STATS = 14
TUNE_EYE_ADAPTATION_GRID = 15
TUNE_BLOOM_TAIL_LEVEL = 16
TUNE_FXAA_STATS = 17
TUNE_RASTER_GRID = 18
TUNE_VSM_DRAW_GRID = 19
TUNE_BOUNDS_GRID = 20
TUNE_BOUNDS_CHUNK = 21
TUNE_TERRAIN_DRAW_GRID = 22
TUNE_TERRAIN_DRAW_STATS = 23
TUNE_VISBUFFER_DECODE_TEXTURED_STATS = 24

# GPU::SceneFlags bits oxc_apply_pbr reads (scene.slang:242-256)
SCENE_HAS_DIRECTIONAL_LIGHT, SCENE_HAS_ATMOSPHERE, SCENE_HAS_CONTACT_SHADOWS, SCENE_HAS_SKY, SCENE_TRANSPARENT_BACKGROUND = 1 << 0, 1 << 1, 1 << 9, 1 << 10, 1 << 11
SCENE_HAS_EYE_ADAPTATION = 1 << 2  # RendererInstance.cpp:1278; oxc_apply_eye_adaptation does not read it, oxc_bloom_context.scene_flags does
EYE_SOURCE_B10G11R11, EYE_SOURCE_R16G16B16A16 = 0, 1  # oxc_eye_adaptation_context.source_format, oxc_bloom_context.source_format
SCENE_HAS_BLOOM = 1 << 3  # RendererInstance.cpp:1282; oxc_apply_bloom does not read it, oxc_tonemap_context.scene_flags does
SCENE_HAS_FILM_GRAIN, SCENE_HAS_CHROMATIC_ABERRATION, SCENE_HAS_VIGNETTE = 1 << 6, 1 << 7, 1 << 8  # SceneGPU.hpp:258-266; oxc_tonemap_context.scene_flags
SCENE_HAS_FXAA = 1 << 4  # SceneGPU.hpp:259; oxc_apply_fxaa does not read it: RendererInstance.apply_fxaa decides by it which image the later passes read
TONEMAP_NONE, TONEMAP_ACES, TONEMAP_AGX, TONEMAP_GT7 = 0, 1, 2, 3  # GPU::TonemapType, oxc_tonemap_context.tonemap_type
TONEMAP_OUT_R8G8B8A8_SRGB, TONEMAP_OUT_B8G8R8A8_SRGB, TONEMAP_OUT_R8G8B8A8_UNORM = 0, 1, 2  # oxc_tonemap_context.output_format
# oxc_material_image.format; oxc_material_sampler.filter / .mip_filter and .address (oxc_decode_visbuffer_textured)
IMAGE_R8G8B8A8_UNORM, IMAGE_R8G8B8A8_SRGB, IMAGE_R8G8_UNORM = 0, 1, 2
FILTER_NEAREST, FILTER_LINEAR = 0, 1
ADDRESS_REPEAT, ADDRESS_CLAMP_TO_EDGE = 0, 1
# GPU::MaterialFlag (scene.slang:34-49): the bits oxc_decode_visbuffer_textured reads
(MATERIAL_HAS_ALBEDO_IMAGE, MATERIAL_HAS_NORMAL_IMAGE, MATERIAL_HAS_EMISSIVE_IMAGE, MATERIAL_HAS_METALLIC_ROUGHNESS_IMAGE, MATERIAL_HAS_OCCLUSION_IMAGE,
 MATERIAL_NORMAL_TWO_COMPONENT, MATERIAL_NORMAL_FLIP_Y) = (1 << k for k in range(7))
LIGHT_KIND_DIRECTIONAL, LIGHT_KIND_POINT, LIGHT_KIND_SPOT = 0, 1, 2  # GPU::LightKind
TERRAIN_GENERATE, TERRAIN_DERIVE, TERRAIN_MINMAX, TERRAIN_ALL = 1, 2, 4, 7  # oxc_terrain_maps_context.stages
TERRAIN_BRUSH_TRACE, TERRAIN_BRUSH_APPLY, TERRAIN_BRUSH_ALL = 1, 2, 3  # oxc_terrain_brush_context.stages
TERRAIN_INVALID_LAYER_MATERIAL = 0xFFFFFFFF  # scene.slang:632
HIGHLIGHT_MASK, HIGHLIGHT_COMPOSITE, HIGHLIGHT_ALL = 1, 2, 3  # oxc_highlight_context.stages
SPRITES_VIS, SPRITES_COLOR, SPRITES_ALL = 1, 2, 3  # oxc_sprite_context.stages
SPRITE_SORT_Y, SPRITE_FLIP_X = 1, 2  # GPU::RenderFlags2D, the low half of oxc_sprite.flags16_distance16
# GPU::DebugView (scene.slang:10-26; RMVSM from SceneGPU.hpp:44), oxc_debug_view_context.debug_view
(DEBUG_VIEW_TRIANGLES, DEBUG_VIEW_MESHLETS, DEBUG_VIEW_OVERDRAW, DEBUG_VIEW_MATERIALS, DEBUG_VIEW_MESH_INSTANCES, DEBUG_VIEW_MESH_LODS, DEBUG_VIEW_ALBEDO,
 DEBUG_VIEW_NORMAL, DEBUG_VIEW_EMISSIVE, DEBUG_VIEW_METALLIC, DEBUG_VIEW_ROUGHNESS, DEBUG_VIEW_BAKED_OCCLUSION, DEBUG_VIEW_GTAO, DEBUG_VIEW_GEOMETRIC_NORMAL,
 DEBUG_VIEW_RMVSM) = range(1, 16)
TERRAIN_BRUSH_RAISE, TERRAIN_BRUSH_SMOOTH, TERRAIN_BRUSH_FLATTEN, TERRAIN_BRUSH_NOISE, TERRAIN_BRUSH_PAINT_LAYER = 0, 1, 2, 3, 4  # GPU::TerrainBrushMode


class Buffer(C.Structure):
    _c_name_ = "oxc_buffer"
    _fields_ = [("dptr", C.c_void_p), ("bytes", C.c_uint64)]


class Image(C.Structure):
    _c_name_ = "oxc_image"
    _fields_ = [
        ("dptr", C.c_void_p),
        ("width", C.c_uint32),
        ("height", C.c_uint32),
        ("levels", C.c_uint32),
        ("_pad", C.c_uint32),
        ("level_offset", C.c_uint64 * 13),
    ]


class ImageArrayU8(C.Structure):
    _c_name_ = "oxc_image_array_u8"
    _fields_ = [
        ("dptr", C.c_void_p),
        ("width", C.c_uint32),
        ("height", C.c_uint32),
        ("layers", C.c_uint32),
        ("levels", C.c_uint32),
        ("level_offset", C.c_uint64 * 13),
    ]


class VirtualClipmap(C.Structure):
    _c_name_ = "oxc_virtual_clipmap"
    _fields_ = [("projection_view_mat", C.c_float * 16), ("page_offset", C.c_int32 * 2), ("z_near", C.c_float)]


class CullCamera(C.Structure):
    _c_name_ = "oxc_cull_camera"
    _fields_ = [
        ("projection_view", C.c_float * 16),
        ("position", C.c_float * 3),
        ("acceptable_lod_error", C.c_float),
        ("resolution", C.c_float * 2),
        ("near_clip", C.c_float),
        ("mesh_instance_count", C.c_uint32),
    ]


class PreparedFrame(C.Structure):
    _c_name_ = "oxc_prepared_frame"
    _fields_ = [
        ("mesh_instance_count", C.c_uint32),
        ("max_meshlet_instance_count", C.c_uint32),
        ("meshes_buffer", Buffer),
        ("transforms_world_buffer", Buffer),
        ("mesh_instances_buffer", Buffer),
        ("meshlet_instances_buffer", Buffer),
        ("visible_meshlet_instances_indices_buffer", Buffer),
        ("meshlet_instance_visibility_mask_buffer", Buffer),
        ("reordered_indices_buffer", Buffer),
    ]


class CullGeometryContext(C.Structure):
    _c_name_ = "oxc_cull_geometry_context"
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("use_hiz", C.c_uint32),
        ("use_hpb", C.c_uint32),
        ("init_cull_meshes", C.c_uint32),
        ("cull_flags", C.c_uint32),
        ("stages", C.c_uint32),
        ("cull_camera", CullCamera),
        ("hiz_attachment", Image),
        ("hpb_attachment", ImageArrayU8),
        ("vsm_clipmaps_buffer", Buffer),
        ("vsm_clipmap_dirty_flags_buffer", Buffer),
        ("vsm_clipmap_count", C.c_uint32),
        ("wide_triangle_index", C.c_uint32),
        ("small_triangle_cull", C.c_uint32),
        ("async_triangles", C.c_uint32),
        ("share_pass_tests", C.c_uint32),
        ("unordered_output", C.c_uint32),
        ("implicit_meshlet_instances", C.c_uint32),
        ("_reserved1", C.c_uint32),
        ("visibility_buffer", Buffer),
        ("cull_meshlets_cmd_buffer", Buffer),
        ("cull_triangles_cmd_buffer", Buffer),
        ("draw_geometry_cmd_buffer", Buffer),
        ("meshlet_instance_runs_buffer", Buffer),
    ]


class MainGeometryContext(C.Structure):
    _c_name_ = "oxc_main_geometry_context"
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("_pad", C.c_uint32),
        ("depth_attachment", Image),
        ("hiz_attachment", Image),
    ]


class Counters(C.Structure):
    _c_name_ = "oxc_counters"
    _fields_ = [
        ("total_visible_meshlet_instances", C.c_uint32),
        ("early_visible_meshlet_instances", C.c_uint32),
        ("late_visible_meshlet_instances", C.c_uint32),
        ("cull_meshlets_cmd_x", C.c_uint32),
        ("cull_triangles_cmd_x", C.c_uint32),
        ("draw_index_count", C.c_uint32),
    ]


class MeshletBoundsDesc(C.Structure):
    _c_name_ = "oxc_meshlet_bounds_desc"
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("vertex_count", C.c_uint32),
        ("meshlet_count", C.c_uint32),
        ("_pad", C.c_uint32),
        ("positions", Buffer),
        ("meshlets", Buffer),
        ("indirect_vertex_indices", Buffer),
        ("local_triangle_indices", Buffer),
        ("meshlet_bounds", Buffer),
        ("mesh_bounds", Buffer),
        ("quantized_positions", Buffer),
    ]


class VertexStreamsDesc(C.Structure):
    _c_name_ = "oxc_vertex_streams_desc"
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("vertex_count", C.c_uint32),
        ("positions", Buffer),
        ("normals", Buffer),
        ("texcoords", Buffer),
        ("quantized_positions", Buffer),
        ("quantized_normals", Buffer),
        ("quantized_texcoords", Buffer),
    ]


MESH_MAX_LODS = 8


class MeshLodCounts(C.Structure):
    _c_name_ = "oxc_mesh_lod_counts"
    _fields_ = [
        ("indices_count", C.c_uint32),
        ("meshlet_count", C.c_uint32),
        ("local_triangle_indices_count", C.c_uint32),
        ("indirect_vertex_indices_count", C.c_uint32),
        ("error", C.c_float),
    ]


class MeshBlobDesc(C.Structure):
    _c_name_ = "oxc_mesh_blob_desc"
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("vertex_count", C.c_uint32),
        ("has_texture_coords", C.c_uint32),
        ("lod_count", C.c_uint32),
        ("lods", MeshLodCounts * MESH_MAX_LODS),
    ]


class MeshLodOffsets(C.Structure):
    _c_name_ = "oxc_mesh_lod_offsets"
    _fields_ = [(n, C.c_uint64) for n in ("indices", "meshlets", "meshlet_bounds", "local_triangle_indices", "indirect_vertex_indices")]


class MeshBlobLayout(C.Structure):
    _c_name_ = "oxc_mesh_blob_layout"
    _fields_ = [
        ("size", C.c_uint64),
        ("lod_metadata_offset", C.c_uint64),
        ("vertex_positions", C.c_uint64),
        ("vertex_normals", C.c_uint64),
        ("texture_coords", C.c_uint64),
        ("lods", MeshLodOffsets * MESH_MAX_LODS),
    ]


class TerrainContext(C.Structure):
    _c_name_ = "oxc_terrain_context"
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("cull_flags", C.c_uint32),
        ("cull_camera", CullCamera),
        ("world_min", C.c_float * 2),
        ("world_size", C.c_float * 2),
        ("patch_count", C.c_uint32 * 2),
        ("base_height", C.c_float),
        ("height_scale", C.c_float),
        ("patch_minmax_attachment", Image),
        ("hiz_attachment", Image),
        ("visible_patches_buffer", Buffer),
        ("patch_visibility_mask_buffer", Buffer),
        ("draw_cmd_buffer", Buffer),
    ]


class DrawContext(C.Structure):
    _c_name_ = "oxc_draw_context"
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("wide_triangle_index", C.c_uint32),
        ("clear", C.c_uint32),
        ("width", C.c_uint32),
        ("height", C.c_uint32),
        ("_pad", C.c_uint32),
        ("projection_view", C.c_float * 16),
        ("draw_geometry_cmd_buffer", Buffer),
        ("visdepth_buffer", Buffer),
        ("depth_attachment", Image),
        ("visbuffer_attachment", Buffer),
    ]


class VsmUpdateContext(C.Structure):
    _c_name_ = "oxc_vsm_update_context"
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("sun_moved", C.c_uint32),
        ("page_size", C.c_int32),
        ("page_table_size", C.c_int32),
        ("physical_page_table_size", C.c_int32),
        ("clipmap_count", C.c_int32),
        ("depth_extent", C.c_int32 * 2),
        ("first_clipmap_width", C.c_float),
        ("clipmap_selection_bias", C.c_float),
        ("virtual_extent", C.c_float),
        ("dirty_mesh_instance_count", C.c_uint32),
        ("inv_projection_view", C.c_float * 16),
        ("resolution", C.c_float * 2),
        ("virtual_page_table", Buffer),
        ("vsm_clipmaps_buffer", Buffer),
        ("depth_attachment", Image),
        ("dirty_mesh_instance_indices", Buffer),
        ("mesh_instances_buffer", Buffer),
        ("meshes_buffer", Buffer),
        ("transforms_world_buffer", Buffer),
        ("transforms_previous_buffer", Buffer),
        ("vsm_clipmap_dirty_flags_buffer", Buffer),
        ("dirty_physical_pages_buffer", Buffer),
        ("clear_cmd_buffer", Buffer),
        ("counters_buffer", Buffer),
        ("hpb_attachment", ImageArrayU8),
        ("physical_page_image", Image),
    ]


class VsmDrawContext(C.Structure):
    _c_name_ = "oxc_vsm_draw_context"
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("wide_triangle_index", C.c_uint32),
        ("page_size", C.c_int32),
        ("page_table_size", C.c_int32),
        ("physical_page_table_size", C.c_int32),
        ("clipmap_count", C.c_int32),
        ("draw_geometry_cmd_buffer", Buffer),
        ("virtual_page_table", Buffer),
        ("vsm_clipmaps_buffer", Buffer),
        ("vsm_clipmap_dirty_flags_buffer", Buffer),
        ("physical_page_image", Image),
        ("draw_commands_buffer", Buffer),
        ("draw_count_buffer", Buffer),
        ("draw_clipmaps_buffer", Buffer),
    ]


class ShadowResolveContext(C.Structure):
    _c_name_ = "oxc_shadow_resolve_context"
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("page_size", C.c_int32),
        ("page_table_size", C.c_int32),
        ("physical_page_table_size", C.c_int32),
        ("clipmap_count", C.c_int32),
        ("first_clipmap_width", C.c_float),
        ("clipmap_selection_bias", C.c_float),
        ("virtual_extent", C.c_float),
        ("z_length", C.c_float),
        ("directional_light_dir", C.c_float * 3),
        ("inv_projection_view", C.c_float * 16),
        ("resolution", C.c_float * 2),
        ("depth_attachment", Image),
        ("normal_attachment", Buffer),
        ("vsm_clipmaps_buffer", Buffer),
        ("virtual_page_table", Buffer),
        ("physical_page_image", Image),
        ("resolved_shadows_attachment", Image),
    ]


class ContactShadowsContext(C.Structure):
    _c_name_ = "oxc_contact_shadows_context"
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("inv_projection_view", C.c_float * 16),
        ("view", C.c_float * 16),
        ("projection", C.c_float * 16),
        ("near_clip", C.c_float),
        ("sun_dir", C.c_float * 3),
        ("steps", C.c_uint32),
        ("thickness", C.c_float),
        ("shadow_length", C.c_float),
        ("depth_attachment", Image),
        ("contact_shadows_attachment", Image),
    ]


class AmbientOcclusionContext(C.Structure):
    _c_name_ = "oxc_ambient_occlusion_context"
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("view", C.c_float * 16),
        ("projection", C.c_float * 16),
        ("resolution", C.c_float * 2),
        ("far_clip", C.c_float),
        ("thickness", C.c_float),
        ("slice_count", C.c_uint32),
        ("samples_per_slice_side", C.c_uint32),
        ("effect_radius", C.c_float),
        ("noise_index", C.c_uint32),
        ("final_power", C.c_float),
        ("depth_attachment", Image),
        ("normal_attachment", Buffer),
        ("hilbert_noise", Buffer),
        ("prefiltered_depth", Image),
        ("depth_differences", Buffer),
        ("noisy_occlusion", Buffer),
        ("ambient_occlusion_attachment", Buffer),
    ]


class DecodeContext(C.Structure):
    _c_name_ = "oxc_decode_context"
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("width", C.c_uint32),
        ("height", C.c_uint32),
        ("clear", C.c_uint32),
        ("meshlet_instance_count", C.c_uint32),
        ("material_count", C.c_uint32),
        ("projection_view", C.c_float * 16),
        ("visbuffer_attachment", Buffer),
        ("depth_attachment", Image),
        ("materials_buffer", Buffer),
        ("albedo_attachment", Buffer),
        ("normal_attachment", Buffer),
        ("emissive_attachment", Buffer),
        ("metallic_roughness_occlusion_attachment", Buffer),
    ]


class MaterialImage(C.Structure):
    _c_name_ = "oxc_material_image"
    _fields_ = [
        ("dptr", C.c_uint64),
        ("width", C.c_uint32),
        ("height", C.c_uint32),
        ("levels", C.c_uint32),
        ("format", C.c_uint32),
        ("level_offset", C.c_uint64 * 15),
    ]


class MaterialSampler(C.Structure):
    _c_name_ = "oxc_material_sampler"
    _fields_ = [
        ("filter", C.c_uint32),
        ("address", C.c_uint32),
        ("mip_filter", C.c_uint32),
        ("_pad", C.c_uint32),
    ]


class MaterialImages(C.Structure):
    _c_name_ = "oxc_material_images"
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("camera_position", C.c_float * 3),
        ("image_count", C.c_uint32),
        ("sampler_count", C.c_uint32),
        ("images_buffer", Buffer),
        ("samplers_buffer", Buffer),
    ]


class PbrContext(C.Structure):
    _c_name_ = "oxc_pbr_context"
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("width", C.c_uint32),
        ("height", C.c_uint32),
        ("scene_flags", C.c_uint32),
        ("light_count", C.c_uint32),
        ("sky_has_texture", C.c_uint32),
        ("inv_projection_view", C.c_float * 16),
        ("camera_position", C.c_float * 3),
        ("sun_dir", C.c_float * 3),
        ("sun_intensity", C.c_float),
        ("base_ambient_color", C.c_float * 3),
        ("sky_solid_color", C.c_float * 4),
        ("sky_ambient_color", C.c_float * 3),
        ("depth_attachment", Image),
        ("albedo_attachment", Buffer),
        ("normal_attachment", Buffer),
        ("emissive_attachment", Buffer),
        ("metallic_roughness_occlusion_attachment", Buffer),
        ("ambient_occlusion_attachment", Buffer),
        ("resolved_shadows_attachment", Image),
        ("contact_shadows_attachment", Image),
        ("lights_buffer", Buffer),
        ("final_attachment", Buffer),
    ]


class EyeAdaptationContext(C.Structure):
    _c_name_ = "oxc_eye_adaptation_context"
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("width", C.c_uint32),
        ("height", C.c_uint32),
        ("source_format", C.c_uint32),
        ("min_exposure", C.c_float),
        ("max_exposure", C.c_float),
        ("ev100_bias", C.c_float),
        ("time_coeff", C.c_float),
        ("final_attachment", Buffer),
        ("histogram_buffer", Buffer),
        ("exposure_buffer", Buffer),
    ]


class ImagePyramid(C.Structure):
    _c_name_ = "oxc_image_pyramid"
    """oxc_image_pyramid (include/oxcull.h): oxc_image's fields, then the allocation's size."""
    _fields_ = [
        ("dptr", C.c_void_p),
        ("width", C.c_uint32),
        ("height", C.c_uint32),
        ("levels", C.c_uint32),
        ("_pad", C.c_uint32),
        ("level_offset", C.c_uint64 * 13),
        ("bytes", C.c_uint64),
    ]


class BloomContext(C.Structure):
    _c_name_ = "oxc_bloom_context"
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("width", C.c_uint32),
        ("height", C.c_uint32),
        ("source_format", C.c_uint32),
        ("scene_flags", C.c_uint32),
        ("threshold", C.c_float),
        ("soft_threshold", C.c_float),
        ("clamp_value", C.c_float),
        ("radius", C.c_float),
        ("_pad", C.c_uint32),
        ("final_attachment", Buffer),
        ("exposure_buffer", Buffer),
        ("bloom_downsampled_attachment", ImagePyramid),
        ("bloom_upsampled_attachment", ImagePyramid),
    ]


class TonemapContext(C.Structure):
    _c_name_ = "oxc_tonemap_context"
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("width", C.c_uint32),
        ("height", C.c_uint32),
        ("source_format", C.c_uint32),
        ("output_format", C.c_uint32),
        ("scene_flags", C.c_uint32),
        ("tonemap_type", C.c_uint32),
        ("exposure", C.c_float),
        ("chromatic_aberration_amount", C.c_float),
        ("vignette_amount", C.c_float),
        ("film_grain_scale", C.c_float),
        ("film_grain_amount", C.c_float),
        ("film_grain_seed", C.c_uint32),
        ("bloom_intensity", C.c_float),
        ("final_attachment", Buffer),
        ("bloom_upsampled_attachment", ImagePyramid),
        ("exposure_buffer", Buffer),
        ("dst_attachment", Buffer),
    ]


class FxaaContext(C.Structure):
    _c_name_ = "oxc_fxaa_context"
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("width", C.c_uint32),
        ("height", C.c_uint32),
        ("source_format", C.c_uint32),
        ("final_attachment", Buffer),
        ("fxaa_attachment", Buffer),
    ]


class Atmosphere(C.Structure):
    _c_name_ = "oxc_atmosphere"
    """oxc_atmosphere: the byte layout of GPU::Atmosphere (SceneGPU.hpp:158-181), 136 bytes; the defaults are the record's own."""
    _fields_ = [
        ("rayleigh_scatter", C.c_float * 3),
        ("rayleigh_density", C.c_float),
        ("mie_scatter", C.c_float * 3),
        ("mie_density", C.c_float),
        ("mie_extinction", C.c_float),
        ("mie_asymmetry", C.c_float),
        ("ozone_absorption", C.c_float * 3),
        ("ozone_height", C.c_float),
        ("ozone_thickness", C.c_float),
        ("terrain_albedo", C.c_float * 3),
        ("planet_radius", C.c_float),
        ("atmos_radius", C.c_float),
        ("aerial_perspective_start_km", C.c_float),
        ("aerial_perspective_exposure", C.c_float),
        ("transmittance_lut_size", C.c_uint32 * 3),
        ("sky_view_lut_size", C.c_uint32 * 3),
        ("multiscattering_lut_size", C.c_uint32 * 3),
        ("aerial_perspective_lut_size", C.c_uint32 * 3),
    ]


class SkyLutContext(C.Structure):
    _c_name_ = "oxc_sky_lut_context"
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("_pad", C.c_uint32),
        ("atmosphere", Atmosphere),
        ("hemisphere_directions", Buffer),
        ("sky_transmittance_lut", Buffer),
        ("sky_multiscatter_lut", Buffer),
    ]


class AtmosphereContext(C.Structure):
    _c_name_ = "oxc_atmosphere_context"
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("_pad", C.c_uint32),
        ("atmosphere", Atmosphere),
        ("sun_dir", C.c_float * 3),
        ("sun_intensity", C.c_float),
        ("camera_position", C.c_float * 3),
        ("_pad1", C.c_float),
        ("camera_inv_projection_view", C.c_float * 16),
        ("sky_transmittance_lut", Buffer),
        ("sky_multiscatter_lut", Buffer),
        ("sky_view_lut", Buffer),
        ("sky_aerial_perspective_lut", Buffer),
    ]


class SkyIblContext(C.Structure):
    _c_name_ = "oxc_sky_ibl_context"
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("_pad", C.c_uint32),
        ("atmosphere", Atmosphere),
        ("sun_dir", C.c_float * 3),
        ("sun_intensity", C.c_float),
        ("camera_position", C.c_float * 3),
        ("sun_ambient_strength", C.c_float),
        ("frame_index", C.c_uint32),
        ("cube_size", C.c_uint32),
        ("sky_view_lut", Buffer),
        ("sky_transmittance_lut", Buffer),
        ("sky_cubemap", Buffer),
    ]


class PbrAtmosphereContext(C.Structure):
    _c_name_ = "oxc_pbr_atmosphere_context"
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("width", C.c_uint32),
        ("height", C.c_uint32),
        ("scene_flags", C.c_uint32),
        ("light_count", C.c_uint32),
        ("inv_projection_view", C.c_float * 16),
        ("camera_position", C.c_float * 3),
        ("sun_dir", C.c_float * 3),
        ("sun_intensity", C.c_float),
        ("atmosphere", Atmosphere),
        ("cube_size", C.c_uint32),
        ("_pad", C.c_uint32),
        ("depth_attachment", Image),
        ("albedo_attachment", Buffer),
        ("normal_attachment", Buffer),
        ("emissive_attachment", Buffer),
        ("metallic_roughness_occlusion_attachment", Buffer),
        ("ambient_occlusion_attachment", Buffer),
        ("resolved_shadows_attachment", Image),
        ("contact_shadows_attachment", Image),
        ("lights_buffer", Buffer),
        ("sky_transmittance_lut", Buffer),
        ("sky_view_lut", Buffer),
        ("sky_aerial_perspective_lut", Buffer),
        ("sky_cubemap", Buffer),
        ("final_attachment", Buffer),
    ]


class TerrainErosion(C.Structure):
    _c_name_ = "oxc_terrain_erosion"
    _fields_ = [
        ("scale", C.c_float),
        ("strength", C.c_float),
        ("gully_weight", C.c_float),
        ("detail", C.c_float),
        ("rounding", C.c_float * 4),
        ("onset", C.c_float * 4),
        ("assumed_slope", C.c_float * 2),
        ("cell_scale", C.c_float),
        ("gain", C.c_float),
        ("lacunarity", C.c_float),
        ("normalization", C.c_float),
        ("octaves", C.c_uint32),
        ("seed", C.c_uint32),
    ]


class TerrainGenerate(C.Structure):
    _c_name_ = "oxc_terrain_generate"
    _fields_ = [
        ("erosion", TerrainErosion),
        ("resolution", C.c_uint32 * 2),
        ("height_offset", C.c_float * 2),
        ("domain_size", C.c_float),
        ("height_frequency", C.c_float),
        ("height_amplitude", C.c_float),
        ("height_lacunarity", C.c_float),
        ("height_gain", C.c_float),
        ("height_octaves", C.c_uint32),
    ]


class TerrainDerive(C.Structure):
    _c_name_ = "oxc_terrain_derive"
    _fields_ = [
        ("resolution", C.c_uint32 * 2),
        ("texel_world_size", C.c_float * 2),
        ("height_range", C.c_float),
        ("slope_rock_begin", C.c_float),
        ("slope_rock_end", C.c_float),
        ("altitude_snow_begin", C.c_float),
        ("altitude_snow_end", C.c_float),
        ("ridge_drainage_scale", C.c_float),
    ]


class TerrainMapsContext(C.Structure):
    _c_name_ = "oxc_terrain_maps_context"
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("stages", C.c_uint32),
        ("generate", TerrainGenerate),
        ("derive", TerrainDerive),
        ("resolution", C.c_uint32 * 2),
        ("patch_count", C.c_uint32 * 2),
        ("dispatch_texels", C.c_uint32 * 2),
        ("dispatch_patches", C.c_uint32 * 2),
        ("region", Buffer),
        ("heightmap", Buffer),
        ("ridgemap", Buffer),
        ("normalmap", Buffer),
        ("splatmap", Buffer),
        ("height_edit", Buffer),
        ("splat_edit", Buffer),
        ("patch_minmax", Image),
    ]


class TerrainBrushParams(C.Structure):
    _c_name_ = "oxc_terrain_brush_params"
    _fields_ = [
        ("ray_origin", C.c_float * 3),
        ("radius_texels", C.c_float),
        ("ray_direction", C.c_float * 3),
        ("strength", C.c_float),
        ("resolution", C.c_uint32 * 2),
        ("world_min", C.c_float * 2),
        ("world_size", C.c_float * 2),
        ("inv_world_size", C.c_float * 2),
        ("patch_count", C.c_uint32 * 2),
        ("base_height", C.c_float),
        ("height_scale", C.c_float),
        ("falloff", C.c_float),
        ("flatten_height", C.c_float),
        ("mode", C.c_uint32),
        ("layer", C.c_uint32),
    ]


class TerrainBrushHit(C.Structure):
    _c_name_ = "oxc_terrain_brush_hit"
    _fields_ = [("world_position", C.c_float * 3), ("valid", C.c_uint32)]


class TerrainRegion(C.Structure):
    _c_name_ = "oxc_terrain_region"
    _fields_ = [("texel_origin", C.c_uint32 * 2), ("patch_origin", C.c_uint32 * 2)]


class TerrainBrushContext(C.Structure):
    _c_name_ = "oxc_terrain_brush_context"
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("stages", C.c_uint32),
        ("params", TerrainBrushParams),
        ("heightmap", Buffer),
        ("height_edit", Buffer),
        ("splat_edit", Buffer),
        ("hit", Buffer),
        ("region", Buffer),
    ]


class TerrainData(C.Structure):
    _c_name_ = "oxc_terrain_data"
    _fields_ = [
        ("world_min", C.c_float * 2),
        ("world_size", C.c_float * 2),
        ("inv_world_size", C.c_float * 2),
        ("patch_count", C.c_uint32 * 2),
        ("base_height", C.c_float),
        ("height_scale", C.c_float),
        ("target_edge_pixels", C.c_float),
        ("max_tessellation", C.c_float),
        ("layer_tiling", C.c_float),
        ("triplanar_begin", C.c_float),
        ("layer_material_indices", C.c_uint32 * 4),
        ("brush_radius", C.c_float),
    ]


class TerrainDecodeContext(C.Structure):
    _c_name_ = "oxc_terrain_decode_context"
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("width", C.c_uint32),
        ("height", C.c_uint32),
        ("inv_projection_view", C.c_float * 16),
        ("terrain", TerrainData),
        ("map_resolution", C.c_uint32 * 2),
        ("material_count", C.c_uint32),
        ("visbuffer_attachment", Buffer),
        ("depth_attachment", Image),
        ("normalmap", Buffer),
        ("splatmap", Buffer),
        ("materials_buffer", Buffer),
        ("brush_hit", Buffer),
        ("albedo_attachment", Buffer),
        ("normal_attachment", Buffer),
        ("emissive_attachment", Buffer),
        ("metallic_roughness_occlusion_attachment", Buffer),
    ]


class TerrainDrawContext(C.Structure):
    _c_name_ = "oxc_terrain_draw_context"
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("clear", C.c_uint32),
        ("width", C.c_uint32),
        ("height", C.c_uint32),
        ("projection_view", C.c_float * 16),
        ("camera_position", C.c_float * 3),
        ("near_clip", C.c_float),
        ("projection_scale", C.c_float),
        ("terrain", TerrainData),
        ("map_resolution", C.c_uint32 * 2),
        ("heightmap", Buffer),
        ("visible_patches_buffer", Buffer),
        ("draw_cmd_buffer", Buffer),
        ("visdepth_buffer", Buffer),
        ("depth_attachment", Image),
        ("visbuffer_attachment", Buffer),
    ]


class DebugViewContext(C.Structure):
    _c_name_ = "oxc_debug_view_context"
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("width", C.c_uint32),
        ("height", C.c_uint32),
        ("debug_view", C.c_uint32),
        ("clear", C.c_uint32),
        ("heatmap_scale", C.c_float),
        ("meshlet_instance_count", C.c_uint32),
        ("page_size", C.c_int32),
        ("page_table_size", C.c_int32),
        ("physical_page_table_size", C.c_int32),
        ("clipmap_count", C.c_int32),
        ("first_clipmap_width", C.c_float),
        ("clipmap_selection_bias", C.c_float),
        ("virtual_extent", C.c_float),
        ("inv_projection_view", C.c_float * 16),
        ("resolution", C.c_float * 2),
        ("visbuffer_attachment", Buffer),
        ("depth_attachment", Image),
        ("overdraw_attachment", Buffer),
        ("albedo_attachment", Buffer),
        ("normal_attachment", Buffer),
        ("emissive_attachment", Buffer),
        ("metallic_roughness_occlusion_attachment", Buffer),
        ("ambient_occlusion_attachment", Buffer),
        ("vsm_clipmaps_buffer", Buffer),
        ("virtual_page_table", Buffer),
        ("debug_attachment", Buffer),
    ]


class PickContext(C.Structure):
    _c_name_ = "oxc_pick_context"
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("width", C.c_uint32),
        ("height", C.c_uint32),
        ("x", C.c_uint32),
        ("y", C.c_uint32),
        ("terrain_transform_index", C.c_uint32),
        ("meshlet_instance_count", C.c_uint32),
        ("visbuffer_attachment", Buffer),
        ("transform_id", Buffer),
    ]


class HighlightContext(C.Structure):
    _c_name_ = "oxc_highlight_context"
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("stages", C.c_uint32),
        ("width", C.c_uint32),
        ("height", C.c_uint32),
        ("color_format", C.c_uint32),
        ("terrain_transform_index", C.c_uint32),
        ("meshlet_instance_count", C.c_uint32),
        ("selected_count", C.c_uint32),
        ("outline_color", C.c_float * 4),
        ("dilate_radius", C.c_int32),
        ("outline_width", C.c_int32),
        ("occluded_mode", C.c_int32),
        ("visbuffer_attachment", Buffer),
        ("transform_indices", Buffer),
        ("mask_bits", Buffer),
        ("mask_attachment", Buffer),
        ("depth_attachment", Image),
        ("color_attachment", Buffer),
        ("dst_attachment", Buffer),
    ]


class Sprite(C.Structure):
    _c_name_ = "oxc_sprite"
    _fields_ = [("material_id16_ypos16", C.c_uint32), ("flags16_distance16", C.c_uint32), ("transform_id", C.c_uint32)]


class SpriteContext(C.Structure):
    _c_name_ = "oxc_sprite_context"
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("stages", C.c_uint32),
        ("width", C.c_uint32),
        ("height", C.c_uint32),
        ("clear", C.c_uint32),
        ("source_format", C.c_uint32),
        ("first_sprite", C.c_uint32),
        ("sprite_count", C.c_uint32),
        ("material_count", C.c_uint32),
        ("transform_count", C.c_uint32),
        ("projection_view", C.c_float * 16),
        ("sprites_buffer", Buffer),
        ("materials_buffer", Buffer),
        ("depth_attachment", Image),
        ("visbuffer_2d", Buffer),
        ("final_attachment", Buffer),
    ]


class SpritePickContext(C.Structure):
    _c_name_ = "oxc_sprite_pick_context"
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("width", C.c_uint32),
        ("height", C.c_uint32),
        ("x", C.c_uint32),
        ("y", C.c_uint32),
        ("visbuffer_2d", Buffer),
        ("transform_id", Buffer),
    ]


class MeshBuildDesc(C.Structure):
    _c_name_ = "oxc_mesh_build_desc"
    _fields_ = [("struct_size", C.c_uint32), ("vertex_count", C.c_uint32), ("index_count", C.c_uint32), ("max_lods", C.c_uint32), ("max_vertices", C.c_uint32),
                ("max_triangles", C.c_uint32), ("positions", C.c_void_p), ("normals", C.c_void_p), ("indices", C.c_void_p)]


class MeshLodView(C.Structure):
    _c_name_ = "oxc_mesh_lod_view"
    _fields_ = [("indices", C.c_void_p), ("meshlets", C.c_void_p), ("indirect_vertex_indices", C.c_void_p), ("local_triangle_indices", C.c_void_p),
                ("indices_count", C.c_uint32), ("meshlet_count", C.c_uint32), ("indirect_vertex_indices_count", C.c_uint32),
                ("local_triangle_indices_count", C.c_uint32), ("error", C.c_float), ("_pad", C.c_uint32)]


class KernelTimes(C.Structure):
    _c_name_ = "oxc_kernel_times"
    _fields_ = [("total_ms", C.c_double * 16), ("launches", C.c_uint32 * 16), ("empty_pair_ms", C.c_double)]


_vp, _u32, _u64, _P, _status = C.c_void_p, C.c_uint32, C.c_uint64, C.POINTER, C.c_int  # every entry point but five returns an oxc_status
_stats = (_status, [_vp, _vp, _vp])  # the oxc_debug_*_stats read-backs: (ctx, u32 counters out, stream)

# every symbol include/oxcull.h and include/oxcull_debug.h declare: symbol -> (restype, argtypes); load() applies it
PROTOTYPES = {
    "oxc_abi_version": (_u32, []),
    "oxc_create": (_status, [C.c_int, _P(_vp)]),
    "oxc_destroy": (None, [_vp]),
    "oxc_last_error": (C.c_char_p, [_vp]),
    "oxc_reserve": (_status, [_vp, _u32, _u32]),
    "oxc_generate_hiz": (_status, [_vp, _P(MainGeometryContext), _vp]),
    "oxc_cull_geometry": (_status, [_vp, _P(PreparedFrame), _P(CullGeometryContext), _vp]),
    "oxc_cull_geometry_batch": (_status, [_vp, _u32, _P(PreparedFrame), _P(CullGeometryContext), _vp]),
    "oxc_join_triangles": (_status, [_vp, _vp]),
    "oxc_seed_meshlet_instances": (_status, [_vp, _P(CullGeometryContext), _u32, _vp]),
    "oxc_read_counters": (_status, [_vp, _P(CullGeometryContext), _P(Counters), _vp]),
    "oxc_stream_read_probe": (_status, [_vp, _vp, _u64, _vp]),
    "oxc_debug_decode_bounds": (_status, [_vp, _vp, _u32, _vp, _vp]),
    "oxc_debug_raster_stats": _stats,
    "oxc_debug_terrain_draw_stats": _stats,
    "oxc_profile_begin": (_status, [_vp]),
    "oxc_profile_end": (_status, [_vp, _P(KernelTimes)]),
    "oxc_build_meshlet_bounds": (_status, [_vp, _P(MeshletBoundsDesc), _vp]),
    "oxc_quantize_vertex_streams": (_status, [_vp, _P(VertexStreamsDesc), _vp]),
    "oxc_mesh_blob_layout_of": (_status, [_P(MeshBlobDesc), _P(MeshBlobLayout)]),
    "oxc_mesh_blob_finalize": (_status, [_P(MeshBlobDesc), _P(MeshBlobLayout), _u64, _vp, _u64, _P(C.c_float * 6), _vp]),
    "oxc_mesh_build_create": (_status, [_P(MeshBuildDesc), _P(_vp)]),
    "oxc_mesh_build_lod_count": (_u32, [_vp]),
    "oxc_mesh_build_lod": (_status, [_vp, _u32, _P(MeshLodView)]),
    "oxc_mesh_build_destroy": (None, [_vp]),
    "oxc_mesh_vertex_fetch_remap": (_status, [_vp, _u64, _u32, _vp, _vp]),
    "oxc_generate_hpb": (_status, [_vp, Buffer, _P(ImageArrayU8), _vp]),
    "oxc_update_virtual_shadowmap": (_status, [_vp, _P(VsmUpdateContext), _vp]),
    "oxc_cull_terrain": (_status, [_vp, _P(TerrainContext), _vp]),
    "oxc_draw_visbuffer": (_status, [_vp, _P(PreparedFrame), _P(DrawContext), _vp]),
    "oxc_decode_visbuffer": (_status, [_vp, _P(PreparedFrame), _P(DecodeContext), _vp]),
    "oxc_debug_visbuffer_decode_stats": _stats,
    "oxc_decode_visbuffer_textured": (_status, [_vp, _P(PreparedFrame), _P(DecodeContext), _P(MaterialImages), _vp]),
    "oxc_debug_visbuffer_decode_textured_stats": _stats,
    "oxc_apply_pbr": (_status, [_vp, _P(PbrContext), _vp]),
    "oxc_debug_pbr_apply_stats": _stats,
    "oxc_apply_eye_adaptation": (_status, [_vp, _P(EyeAdaptationContext), _vp]),
    "oxc_apply_bloom": (_status, [_vp, _P(BloomContext), _vp]),
    "oxc_apply_tonemap": (_status, [_vp, _P(TonemapContext), _vp]),
    "oxc_apply_fxaa": (_status, [_vp, _P(FxaaContext), _vp]),
    "oxc_debug_fxaa_stats": _stats,
    "oxc_generate_sky_luts": (_status, [_vp, _P(SkyLutContext), _vp]),
    "oxc_draw_atmosphere": (_status, [_vp, _P(AtmosphereContext), _vp]),
    "oxc_generate_sky_ibl": (_status, [_vp, _P(SkyIblContext), _vp]),
    "oxc_apply_pbr_atmosphere": (_status, [_vp, _P(PbrAtmosphereContext), _vp]),
    "oxc_generate_terrain_maps": (_status, [_vp, _P(TerrainMapsContext), _vp]),
    "oxc_apply_terrain_brush": (_status, [_vp, _P(TerrainBrushContext), _vp]),
    "oxc_decode_terrain": (_status, [_vp, _P(TerrainDecodeContext), _vp]),
    "oxc_draw_terrain": (_status, [_vp, _P(TerrainDrawContext), _vp]),
    "oxc_apply_debug_view": (_status, [_vp, _P(PreparedFrame), _P(DebugViewContext), _vp]),
    "oxc_pick_transform": (_status, [_vp, _P(PreparedFrame), _P(PickContext), _vp]),
    "oxc_apply_highlight": (_status, [_vp, _P(PreparedFrame), _P(HighlightContext), _vp]),
    "oxc_pack_sprite": (_status, [_u32, C.c_float, _u32, _u32, C.c_float, _P(Sprite)]),
    "oxc_sort_sprites": (_status, [_P(Sprite), _u64]),
    "oxc_draw_sprites": (_status, [_vp, _P(PreparedFrame), _P(SpriteContext), _vp]),
    "oxc_pick_sprite": (_status, [_vp, _P(SpritePickContext), _vp]),
    "oxc_draw_physical_pages": (_status, [_vp, _P(PreparedFrame), _P(VsmDrawContext), _vp]),
    "oxc_debug_vsm_draw_stats": _stats,
    "oxc_resolve_shadowmap": (_status, [_vp, _P(ShadowResolveContext), _vp]),
    "oxc_debug_vsm_resolve_stats": _stats,
    "oxc_contact_shadows": (_status, [_vp, _P(ContactShadowsContext), _vp]),
    "oxc_debug_contact_shadows_stats": _stats,
    "oxc_generate_ambient_occlusion": (_status, [_vp, _P(AmbientOcclusionContext), _vp]),
    "oxc_debug_ambient_occlusion_stats": _stats,
    "oxc_comm_unique_id": (_status, [_vp, _vp]),
    "oxc_comm_init": (_status, [_vp, _vp, _u32, _u32]),
    "oxc_comm_destroy": (_status, [_vp]),
    "oxc_pack_counters": (_status, [_vp, _P(CullGeometryContext), _vp, _vp]),
    "oxc_pack_counters_batch": (_status, [_vp, _u32, _P(CullGeometryContext), _vp, _vp]),
    "oxc_exchange_counts": (_status, [_vp, _vp, _vp, _vp]),
    "oxc_broadcast_hiz": (_status, [_vp, _P(Image), _u64, _u32, _vp]),
    "oxc_broadcast_hiz_levels": (_status, [_vp, _P(Image), _u32, _u64, _u32, _vp]),
    "oxc_debug_read_u32": (_status, [_vp, _vp, _u32, _vp, _vp]),
    "oxc_debug_shared_tests_mode": (_u32, [_vp]),
    "oxc_debug_tri_loads_mode": (_u32, [_vp]),
    "oxc_debug_set_tuning": (_status, [_vp, _u32, _u32]),
    "oxc_debug_count_occlusion_candidates": (_status, [_vp, _vp]),
    "oxc_debug_project_aabb": (_status, [_vp, _P(C.c_float), C.c_float, _vp, _u32, _vp, _vp]),
}
EXPORTS = list(PROTOTYPES)


def build(force: bool = False) -> str:
    """Compile liboxcull.so for gfx950 with hipcc (cross-compiles without a GPU)."""
    if force:
        subprocess.check_call(["make", "-C", CSRC_DIR, "clean"], stdout=subprocess.DEVNULL)
    subprocess.check_call(["make", "-C", CSRC_DIR], stdout=subprocess.DEVNULL)
    return LIB_PATH


_libs = {}


def load(path: str = None) -> C.CDLL:
    """liboxcull.so with prototypes.  `path`: another build of the same library (tools/kbench.py compares kernel
    variants built with different -D flags in one process)."""
    path = os.path.abspath(path or os.environ.get("OXC_LIB_PATH") or LIB_PATH)  # OXC_LIB_PATH: an experiment build (tools/build_variants.sh)
    if path in _libs:
        return _libs[path]
    if not os.path.exists(path):
        raise RuntimeError(
            f"{path} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(there is no CPU fallback for the cull path)"
        )
    lib = C.CDLL(path)
    lib.oxc_abi_version.restype = C.c_uint32
    if lib.oxc_abi_version() != ABI_VERSION:
        raise RuntimeError(f"{path}: ABI version {lib.oxc_abi_version()} != {ABI_VERSION} (stale build: run __graft_entry__.build())")
    for name, (restype, argtypes) in PROTOTYPES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    _libs[path] = lib
    return lib


# OXC_K_* (include/oxcull.h); the *_late entries are the LatePass instantiations, timed apart
KERNEL_NAMES = ["prepare_instances", "cull_meshes_scan", "cull_meshes_expand", "cull_meshlets_test", "cull_meshlets_emit",
                "cull_triangles_test", "cull_triangles_emit", "hiz", "cull_meshlets_test_late", "cull_meshlets_emit_late",
                "cull_triangles_test_late", "cull_triangles_emit_late", "draw_visbuffer", "build_meshlet_bounds",
                "multiview_setup", "vsm_update"]


class OxcError(RuntimeError):
    def __init__(self, status: int, msg: str):
        super().__init__(f"oxcull status {status}: {msg}")
        self.status = status
