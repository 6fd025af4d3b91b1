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

# GPU::SceneFlags bits oxc_apply_pbr reads (scene.slang:242-256)
SCENE_HAS_DIRECTIONAL_LIGHT, SCENE_HAS_ATMOSPHERE, SCENE_HAS_CONTACT_SHADOWS, SCENE_HAS_SKY, SCENE_TRANSPARENT_BACKGROUND = 1 << 0, 1 << 1, 1 << 9, 1 << 10, 1 << 11
SCENE_HAS_EYE_ADAPTATION = 1 << 2  # RendererInstance.cpp:1278; oxc_apply_eye_adaptation does not read it, oxc_bloom_context.scene_flags does
EYE_SOURCE_B10G11R11, EYE_SOURCE_R16G16B16A16 = 0, 1  # oxc_eye_adaptation_context.source_format, oxc_bloom_context.source_format
SCENE_HAS_BLOOM = 1 << 3  # RendererInstance.cpp:1282; oxc_apply_bloom does not read it, oxc_tonemap_context.scene_flags does
SCENE_HAS_FILM_GRAIN, SCENE_HAS_CHROMATIC_ABERRATION, SCENE_HAS_VIGNETTE = 1 << 6, 1 << 7, 1 << 8  # SceneGPU.hpp:258-266; oxc_tonemap_context.scene_flags
SCENE_HAS_FXAA = 1 << 4  # SceneGPU.hpp:259; oxc_apply_fxaa does not read it: RendererInstance.apply_fxaa decides by it which image the later passes read
TONEMAP_NONE, TONEMAP_ACES, TONEMAP_AGX, TONEMAP_GT7 = 0, 1, 2, 3  # GPU::TonemapType, oxc_tonemap_context.tonemap_type
TONEMAP_OUT_R8G8B8A8_SRGB, TONEMAP_OUT_B8G8R8A8_SRGB, TONEMAP_OUT_R8G8B8A8_UNORM = 0, 1, 2  # oxc_tonemap_context.output_format
LIGHT_KIND_DIRECTIONAL, LIGHT_KIND_POINT, LIGHT_KIND_SPOT = 0, 1, 2  # GPU::LightKind


class Buffer(C.Structure):
    _fields_ = [("dptr", C.c_void_p), ("bytes", C.c_uint64)]


class Image(C.Structure):
    _fields_ = [
        ("dptr", C.c_void_p),
        ("width", C.c_uint32),
        ("height", C.c_uint32),
        ("levels", C.c_uint32),
        ("_pad", C.c_uint32),
        ("level_offset", C.c_uint64 * 13),
    ]


class ImageArrayU8(C.Structure):
    _fields_ = [
        ("dptr", C.c_void_p),
        ("width", C.c_uint32),
        ("height", C.c_uint32),
        ("layers", C.c_uint32),
        ("levels", C.c_uint32),
        ("level_offset", C.c_uint64 * 13),
    ]


class VirtualClipmap(C.Structure):
    _fields_ = [("projection_view_mat", C.c_float * 16), ("page_offset", C.c_int32 * 2), ("z_near", C.c_float)]


class CullCamera(C.Structure):
    _fields_ = [
        ("projection_view", C.c_float * 16),
        ("position", C.c_float * 3),
        ("acceptable_lod_error", C.c_float),
        ("resolution", C.c_float * 2),
        ("near_clip", C.c_float),
        ("mesh_instance_count", C.c_uint32),
    ]


class PreparedFrame(C.Structure):
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
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("_pad", C.c_uint32),
        ("depth_attachment", Image),
        ("hiz_attachment", Image),
    ]


class Counters(C.Structure):
    _fields_ = [
        ("total_visible_meshlet_instances", C.c_uint32),
        ("early_visible_meshlet_instances", C.c_uint32),
        ("late_visible_meshlet_instances", C.c_uint32),
        ("cull_meshlets_cmd_x", C.c_uint32),
        ("cull_triangles_cmd_x", C.c_uint32),
        ("draw_index_count", C.c_uint32),
    ]


class MeshletBoundsDesc(C.Structure):
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
    _fields_ = [
        ("indices_count", C.c_uint32),
        ("meshlet_count", C.c_uint32),
        ("local_triangle_indices_count", C.c_uint32),
        ("indirect_vertex_indices_count", C.c_uint32),
        ("error", C.c_float),
    ]


class MeshBlobDesc(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("vertex_count", C.c_uint32),
        ("has_texture_coords", C.c_uint32),
        ("lod_count", C.c_uint32),
        ("lods", MeshLodCounts * MESH_MAX_LODS),
    ]


class MeshLodOffsets(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("indices", "meshlets", "meshlet_bounds", "local_triangle_indices", "indirect_vertex_indices")]


class MeshBlobLayout(C.Structure):
    _fields_ = [
        ("size", C.c_uint64),
        ("lod_metadata_offset", C.c_uint64),
        ("vertex_positions", C.c_uint64),
        ("vertex_normals", C.c_uint64),
        ("texture_coords", C.c_uint64),
        ("lods", MeshLodOffsets * MESH_MAX_LODS),
    ]


class TerrainContext(C.Structure):
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
    """oxc_vsm_update_context (include/oxcull.h)."""
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
    """oxc_vsm_draw_context (include/oxcull.h)."""
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
    """oxc_shadow_resolve_context (include/oxcull.h)."""
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
    """oxc_contact_shadows_context (include/oxcull.h)."""
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
    """oxc_ambient_occlusion_context (include/oxcull.h)."""
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
    """oxc_decode_context (include/oxcull.h)."""
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


class PbrContext(C.Structure):
    """oxc_pbr_context (include/oxcull.h)."""
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
    """oxc_eye_adaptation_context (include/oxcull.h)."""
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
    """oxc_bloom_context (include/oxcull.h)."""
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
    """oxc_tonemap_context (include/oxcull.h)."""
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
    """oxc_fxaa_context (include/oxcull.h)."""
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("width", C.c_uint32),
        ("height", C.c_uint32),
        ("source_format", C.c_uint32),
        ("final_attachment", Buffer),
        ("fxaa_attachment", Buffer),
    ]


class Atmosphere(C.Structure):
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
    """oxc_sky_lut_context (include/oxcull.h)."""
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("_pad", C.c_uint32),
        ("atmosphere", Atmosphere),
        ("hemisphere_directions", Buffer),
        ("sky_transmittance_lut", Buffer),
        ("sky_multiscatter_lut", Buffer),
    ]


class AtmosphereContext(C.Structure):
    """oxc_atmosphere_context (include/oxcull.h)."""
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


# every symbol include/oxcull.h declares
EXPORTS = [
    "oxc_abi_version",
    "oxc_create",
    "oxc_destroy",
    "oxc_last_error",
    "oxc_reserve",
    "oxc_generate_hiz",
    "oxc_cull_geometry",
    "oxc_cull_geometry_batch",
    "oxc_join_triangles",
    "oxc_seed_meshlet_instances",
    "oxc_read_counters",
    "oxc_stream_read_probe",
    "oxc_debug_decode_bounds",
    "oxc_debug_raster_stats",
    "oxc_profile_begin",
    "oxc_profile_end",
    "oxc_build_meshlet_bounds",
    "oxc_quantize_vertex_streams",
    "oxc_mesh_blob_layout_of",
    "oxc_mesh_blob_finalize",
    "oxc_mesh_build_create",
    "oxc_mesh_build_lod_count",
    "oxc_mesh_build_lod",
    "oxc_mesh_build_destroy",
    "oxc_mesh_vertex_fetch_remap",
    "oxc_generate_hpb",
    "oxc_update_virtual_shadowmap",
    "oxc_cull_terrain",
    "oxc_draw_visbuffer",
    "oxc_decode_visbuffer",
    "oxc_debug_visbuffer_decode_stats",
    "oxc_apply_pbr",
    "oxc_debug_pbr_apply_stats",
    "oxc_apply_eye_adaptation",
    "oxc_apply_bloom",
    "oxc_apply_tonemap",
    "oxc_apply_fxaa",
    "oxc_debug_fxaa_stats",
    "oxc_generate_sky_luts",
    "oxc_draw_atmosphere",
    "oxc_draw_physical_pages",
    "oxc_debug_vsm_draw_stats",
    "oxc_resolve_shadowmap",
    "oxc_debug_vsm_resolve_stats",
    "oxc_contact_shadows",
    "oxc_debug_contact_shadows_stats",
    "oxc_generate_ambient_occlusion",
    "oxc_debug_ambient_occlusion_stats",
    "oxc_comm_unique_id",
    "oxc_comm_init",
    "oxc_comm_destroy",
    "oxc_pack_counters",
    "oxc_pack_counters_batch",
    "oxc_exchange_counts",
    "oxc_broadcast_hiz",
    "oxc_broadcast_hiz_levels",
    "oxc_debug_read_u32",
    "oxc_debug_shared_tests_mode",
    "oxc_debug_tri_loads_mode",
    "oxc_debug_set_tuning",
    "oxc_debug_count_occlusion_candidates",
    "oxc_debug_project_aabb",
]


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
    vp = C.c_void_p
    lib.oxc_abi_version.restype = C.c_uint32
    lib.oxc_create.argtypes = [C.c_int, C.POINTER(vp)]
    lib.oxc_destroy.argtypes = [vp]
    lib.oxc_destroy.restype = None
    lib.oxc_last_error.argtypes = [vp]
    lib.oxc_last_error.restype = C.c_char_p
    lib.oxc_reserve.argtypes = [vp, C.c_uint32, C.c_uint32]
    lib.oxc_generate_hiz.argtypes = [vp, C.POINTER(MainGeometryContext), vp]
    lib.oxc_cull_geometry.argtypes = [vp, C.POINTER(PreparedFrame), C.POINTER(CullGeometryContext), vp]
    lib.oxc_cull_geometry_batch.argtypes = [vp, C.c_uint32, C.POINTER(PreparedFrame), C.POINTER(CullGeometryContext), vp]
    lib.oxc_join_triangles.argtypes = [vp, vp]
    lib.oxc_seed_meshlet_instances.argtypes = [vp, C.POINTER(CullGeometryContext), C.c_uint32, vp]
    lib.oxc_read_counters.argtypes = [vp, C.POINTER(CullGeometryContext), C.POINTER(Counters), vp]
    lib.oxc_stream_read_probe.argtypes = [vp, vp, C.c_uint64, vp]
    lib.oxc_debug_decode_bounds.argtypes = [vp, vp, C.c_uint32, vp, vp]
    lib.oxc_profile_begin.argtypes = [vp]
    lib.oxc_profile_end.argtypes = [vp, C.POINTER(KernelTimes)]
    lib.oxc_build_meshlet_bounds.argtypes = [vp, C.POINTER(MeshletBoundsDesc), vp]
    lib.oxc_quantize_vertex_streams.argtypes = [vp, C.POINTER(VertexStreamsDesc), vp]
    lib.oxc_mesh_blob_layout_of.argtypes = [C.POINTER(MeshBlobDesc), C.POINTER(MeshBlobLayout)]
    lib.oxc_mesh_blob_finalize.argtypes = [C.POINTER(MeshBlobDesc), C.POINTER(MeshBlobLayout), C.c_uint64, vp, C.c_uint64, C.POINTER(C.c_float * 6), vp]
    lib.oxc_mesh_build_create.argtypes = [C.POINTER(MeshBuildDesc), C.POINTER(vp)]
    lib.oxc_mesh_build_lod_count.argtypes = [vp]
    lib.oxc_mesh_build_lod_count.restype = C.c_uint32
    lib.oxc_mesh_build_lod.argtypes = [vp, C.c_uint32, C.POINTER(MeshLodView)]
    lib.oxc_mesh_build_destroy.argtypes = [vp]
    lib.oxc_mesh_build_destroy.restype = None
    lib.oxc_mesh_vertex_fetch_remap.argtypes = [vp, C.c_uint64, C.c_uint32, vp, vp]
    lib.oxc_generate_hpb.argtypes = [vp, Buffer, C.POINTER(ImageArrayU8), vp]
    lib.oxc_update_virtual_shadowmap.argtypes = [vp, C.POINTER(VsmUpdateContext), vp]
    lib.oxc_cull_terrain.argtypes = [vp, C.POINTER(TerrainContext), vp]
    lib.oxc_debug_read_u32.argtypes = [vp, vp, C.c_uint32, vp, vp]
    lib.oxc_debug_shared_tests_mode.argtypes = [vp]
    lib.oxc_debug_shared_tests_mode.restype = C.c_uint32
    lib.oxc_debug_tri_loads_mode.argtypes = [vp]
    lib.oxc_debug_tri_loads_mode.restype = C.c_uint32
    lib.oxc_debug_raster_stats.argtypes = [vp, vp, vp]
    lib.oxc_debug_set_tuning.argtypes = [vp, C.c_uint32, C.c_uint32]
    lib.oxc_debug_count_occlusion_candidates.argtypes = [vp, vp]
    lib.oxc_comm_unique_id.argtypes = [vp, vp]
    lib.oxc_comm_init.argtypes = [vp, vp, C.c_uint32, C.c_uint32]
    lib.oxc_comm_destroy.argtypes = [vp]
    lib.oxc_pack_counters.argtypes = [vp, C.POINTER(CullGeometryContext), vp, vp]
    lib.oxc_pack_counters_batch.argtypes = [vp, C.c_uint32, C.POINTER(CullGeometryContext), vp, vp]
    lib.oxc_exchange_counts.argtypes = [vp, vp, vp, vp]
    lib.oxc_broadcast_hiz.argtypes = [vp, C.POINTER(Image), C.c_uint64, C.c_uint32, vp]
    lib.oxc_broadcast_hiz_levels.argtypes = [vp, C.POINTER(Image), C.c_uint32, C.c_uint64, C.c_uint32, vp]
    lib.oxc_debug_project_aabb.argtypes = [vp, C.POINTER(C.c_float), C.c_float, vp, C.c_uint32, vp, vp]
    lib.oxc_draw_visbuffer.argtypes = [vp, C.POINTER(PreparedFrame), C.POINTER(DrawContext), vp]
    lib.oxc_decode_visbuffer.argtypes = [vp, C.POINTER(PreparedFrame), C.POINTER(DecodeContext), vp]
    lib.oxc_debug_visbuffer_decode_stats.argtypes = [vp, vp, vp]
    lib.oxc_apply_pbr.argtypes = [vp, C.POINTER(PbrContext), vp]
    lib.oxc_debug_pbr_apply_stats.argtypes = [vp, vp, vp]
    lib.oxc_apply_eye_adaptation.argtypes = [vp, C.POINTER(EyeAdaptationContext), vp]
    lib.oxc_apply_bloom.argtypes = [vp, C.POINTER(BloomContext), vp]
    lib.oxc_apply_tonemap.argtypes = [vp, C.POINTER(TonemapContext), vp]
    lib.oxc_apply_fxaa.argtypes = [vp, C.POINTER(FxaaContext), vp]
    lib.oxc_debug_fxaa_stats.argtypes = [vp, vp, vp]
    lib.oxc_generate_sky_luts.argtypes = [vp, C.POINTER(SkyLutContext), vp]
    lib.oxc_draw_atmosphere.argtypes = [vp, C.POINTER(AtmosphereContext), vp]
    lib.oxc_draw_physical_pages.argtypes = [vp, C.POINTER(PreparedFrame), C.POINTER(VsmDrawContext), vp]
    lib.oxc_debug_vsm_draw_stats.argtypes = [vp, vp, vp]
    lib.oxc_resolve_shadowmap.argtypes = [vp, C.POINTER(ShadowResolveContext), vp]
    lib.oxc_debug_vsm_resolve_stats.argtypes = [vp, vp, vp]
    lib.oxc_contact_shadows.argtypes = [vp, C.POINTER(ContactShadowsContext), vp]
    lib.oxc_debug_contact_shadows_stats.argtypes = [vp, vp, vp]
    lib.oxc_generate_ambient_occlusion.argtypes = [vp, C.POINTER(AmbientOcclusionContext), vp]
    lib.oxc_debug_ambient_occlusion_stats.argtypes = [vp, vp, vp]
    for name in EXPORTS:
        if name not in ("oxc_abi_version", "oxc_destroy", "oxc_last_error", "oxc_mesh_build_lod_count", "oxc_mesh_build_destroy"):
            getattr(lib, name).restype = C.c_int
    _libs[path] = lib
    return lib


class MeshBuildDesc(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("vertex_count", C.c_uint32), ("index_count", C.c_uint32), ("max_lods", C.c_uint32), ("max_vertices", C.c_uint32),
                ("max_triangles", C.c_uint32), ("positions", C.c_void_p), ("normals", C.c_void_p), ("indices", C.c_void_p)]


class MeshLodView(C.Structure):
    _fields_ = [("indices", C.c_void_p), ("meshlets", C.c_void_p), ("indirect_vertex_indices", C.c_void_p), ("local_triangle_indices", C.c_void_p),
                ("indices_count", C.c_uint32), ("meshlet_count", C.c_uint32), ("indirect_vertex_indices_count", C.c_uint32),
                ("local_triangle_indices_count", C.c_uint32), ("error", C.c_float), ("_pad", C.c_uint32)]


class KernelTimes(C.Structure):
    _fields_ = [("total_ms", C.c_double * 16), ("launches", C.c_uint32 * 16), ("empty_pair_ms", C.c_double)]


# OXC_K_* (include/oxcull.h); the *_late entries are the LatePass instantiations, timed apart
KERNEL_NAMES = ["prepare_instances", "cull_meshes_scan", "cull_meshes_expand", "cull_meshlets_test", "cull_meshlets_emit",
                "cull_triangles_test", "cull_triangles_emit", "hiz", "cull_meshlets_test_late", "cull_meshlets_emit_late",
                "cull_triangles_test_late", "cull_triangles_emit_late", "draw_visbuffer", "build_meshlet_bounds",
                "multiview_setup", "vsm_update"]


class OxcError(RuntimeError):
    def __init__(self, status: int, msg: str):
        super().__init__(f"oxcull status {status}: {msg}")
        self.status = status
