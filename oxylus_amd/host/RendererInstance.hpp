// RendererInstance.hpp -- C++ drop-in shim over the C ABI (include/oxcull.h).
//
// Keeps the reference's names and field meaning for the cull path so that the engine-side
// code of RendererInstance::render (Oxylus/src/Render/RendererInstance.cpp:793-884) compiles
// against it with `vuk::Value<vuk::Buffer>` replaced by `ox::amd::Buffer` (device pointer +
// size) and `vuk::Value<vuk::ImageAttachment>` by `ox::amd::ImageAttachment` (linear mip
// chain).  Mirrors:
//   GPU::CullFlag / GPU::CullCamera           Oxylus/include/Scene/SceneGPU.hpp:222-229,345-353
//   PreparedFrame                             Oxylus/include/Render/RendererInstance.hpp:143-169
//   CullGeometryContext / MainGeometryContext Oxylus/include/Render/RendererInstance.hpp:171-216
//   RendererInstance::generate_hiz / cull_geometry            ...RendererInstance.hpp:397-398
// Error behaviour: the reference's entry points return void and abort through OX_CHECK_* on
// programmer errors (Oxylus/include/Utils/Log.hpp:38-47); the shim throws std::runtime_error
// carrying oxc_last_error() instead of aborting.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <utility>

#include "oxcull.h"

namespace ox::amd {

namespace GPU {
enum struct CullFlag : uint32_t {
  None = 0,
  TestFrustum = 1 << 0,
  SelectLOD = 1 << 1,
  TestOcclusion = 1 << 2,
  LatePass = 1 << 3,
  TestAll = TestFrustum | SelectLOD | TestOcclusion,
};
constexpr CullFlag operator|(CullFlag a, CullFlag b) { return static_cast<CullFlag>(static_cast<uint32_t>(a) | static_cast<uint32_t>(b)); }
constexpr CullFlag& operator|=(CullFlag& a, CullFlag b) { return a = a | b; }
constexpr bool operator&(CullFlag a, CullFlag b) { return (static_cast<uint32_t>(a) & static_cast<uint32_t>(b)) != 0; }

using CullCamera = oxc_cull_camera;  // same 96-byte layout as GPU::CullCamera
static_assert(sizeof(CullCamera) == 96, "GPU::CullCamera is a 96-byte push constant");
}  // namespace GPU

using Buffer = oxc_buffer;             // stands in for vuk::Value<vuk::Buffer>
using ImageAttachment = oxc_image;     // stands in for vuk::Value<vuk::ImageAttachment> (R32F / D32F)
using ImageArrayAttachment = oxc_image_array_u8;  // the R8UI mip-mapped array `hpb_attachment`

struct PreparedFrame {
  uint32_t mesh_instance_count = 0;
  uint32_t max_meshlet_instance_count = 0;
  bool use_mesh_shaders = false;  // the mesh-shader path needs graphics hardware: must stay false
  Buffer transforms_world_buffer = {};
  Buffer meshes_buffer = {};
  Buffer mesh_instances_buffer = {};
  Buffer meshlet_instances_buffer = {};
  Buffer visible_meshlet_instances_indices_buffer = {};
  Buffer meshlet_instance_visibility_mask_buffer = {};
  Buffer reordered_indices_buffer = {};
  Buffer materials_buffer = {};  // GPU::Material[], read by decode_visbuffer
  Buffer lights_buffer = {};     // GPU::Light[], 64 bytes each, read by apply_pbr
  Buffer exposure_buffer = {};   // GPU::HistogramLuminance {adapted_luminance, exposure}, 8 bytes, kept between frames; the caller fills it with 1.0f once (RendererInstance.cpp:1778-1784)
};

struct CullGeometryContext {
  bool use_hiz = false;
  bool use_hpb = false;
  bool init_cull_meshes = false;
  GPU::CullFlag cull_flags = GPU::CullFlag::TestAll;
  GPU::CullCamera cull_camera = {};
  Buffer vsm_clipmaps_buffer = {};
  Buffer vsm_clipmap_dirty_flags_buffer = {};
  uint32_t vsm_clipmap_count = 0;
  ImageAttachment hiz_attachment = {};
  ImageArrayAttachment hpb_attachment = {};
  Buffer visibility_buffer = {};
  Buffer cull_meshlets_cmd_buffer = {};
  Buffer draw_geometry_cmd_buffer = {};
  // not in the reference struct (it is a local there, CullGeometry.cpp:125-127): the indirect
  // dispatch command of cull_triangles, exposed so callers can read the visible-meshlet count
  Buffer cull_triangles_cmd_buffer = {};
  // extension: 1 = wide packed index for meshlets of up to 128 triangles (<= 2^23 ids), 2 = {id, corner} pairs (no id limit)
  uint32_t wide_triangle_index = 0;
  bool small_triangle_cull = false;  // extension named by the north star; default OFF = reference behaviour
  // extension (scheduling only): cull_triangles of this call runs on the backend's own stream beside what the caller enqueues next
  // (the next cull_geometry's meshlet stage, generate_hiz); join_triangles() before anything of the caller's reads the index list
  bool async_triangles = false;
  // extension (caching only): set on both HiZ calls of a frame (early, then LatePass with the same camera and buffers), the late call
  // takes the frustum + cone results from the early one instead of testing again -- the caller vouches that no input of those tests
  // was written in between (include/oxcull.h: share_pass_tests)
  bool share_pass_tests = false;
  // extension (order only): 0 = ascending lists; 1 / 2 = the reference's own atomic slot allocation, aggregated per block / wave step
  // (one launch per stage instead of test + ordered emit; include/oxcull.h: unordered_output)
  uint32_t unordered_output = 0;
  // extension (oxc_cull_geometry_batch's multi-view path only): cull_meshes leaves the MeshletInstance list implicit and writes
  // {first, count} per mesh instance here instead (include/oxcull.h: implicit_meshlet_instances)
  bool implicit_meshlet_instances = false;
  Buffer meshlet_instance_runs_buffer = {};
};

struct MainGeometryContext {
  GPU::CullFlag cull_flags = GPU::CullFlag::TestAll;
  GPU::CullCamera cull_camera = {};
  ImageAttachment depth_attachment = {};
  ImageAttachment hiz_attachment = {};
  Buffer visbuffer_attachment = {};  // R32_UINT image as a linear buffer of width * height u32 (the reference: vuk::ImageAttachment)
  Buffer draw_geometry_cmd_buffer = {};
  Buffer visibility_buffer = {};
  // not in the reference struct: the compute rasteriser's packed depth|vis image (u64 per pixel) that persists between the early
  // and the late draw of a frame, whether this draw starts from a cleared image (the early one), and the wide-index extension
  Buffer visdepth_buffer = {};
  bool clear = true;
  uint32_t wide_triangle_index = 0;
  // decode_visbuffer's outputs, linear buffers of width * height texels in the reference's formats (RendererInstance.cpp:700-737):
  // R8G8B8A8 sRGB, R16G16B16A16 Sfloat, B10G11R11 UfloatPack32, R8G8B8A8 Unorm
  Buffer albedo_attachment = {};
  Buffer normal_attachment = {};
  Buffer emissive_attachment = {};
  Buffer metallic_roughness_occlusion_attachment = {};
};

// What resolve_shadowmap reads and writes (Passes/Shadowmaps.cpp:756-822): the GPU::VSMContext and GPU::Camera fields, the main view's depth
// and normal images, the clipmaps, the page table, the physical pages, and the R32F resolved_shadows_attachment.
using ShadowResolveContext = oxc_shadow_resolve_context;

// What the contact_shadows pass reads and writes (RendererInstance.cpp:990-1020, passes/contact_shadows.slang): the GPU::Camera fields, the
// push constants (sun_dir, steps, thickness, shadow_length), the main view's depth and the R32F contact_shadows_attachment.
using ContactShadowsContext = oxc_contact_shadows_context;

// What generate_ambient_occlusion reads and writes (Passes/PBR.cpp:179-311): the GPU::Camera fields, GPU::VBGTAOSettings, the main view's depth,
// the normal image, the Hilbert index table, the three caller-owned intermediates and the R16F ambient_occlusion_attachment.
using AmbientOcclusionContext = oxc_ambient_occlusion_context;

// What apply_pbr reads (RendererInstance.hpp:310-325 of the reference, without bindless_set): the depth, the four G-buffer images of
// decode_visbuffer as linear buffers, the ambient occlusion, the two R32F shadow terms and, for the atmosphere branch, the four sky images
// generate_sky_luts, draw_atmosphere and generate_sky_ibl wrote (the AtmosphereContext's buffers; unread without HasAtmosphere).
struct PBRContext {
  Buffer sky_transmittance_lut_attachment = {};
  Buffer sky_aerial_perspective_lut_attachment = {};
  Buffer sky_view_lut_attachment = {};
  Buffer sky_cubemap_attachment = {};
  ImageAttachment depth_attachment = {};
  Buffer albedo_attachment = {};
  Buffer normal_attachment = {};
  Buffer emissive_attachment = {};
  Buffer metallic_roughness_occlusion_attachment = {};
  Buffer ambient_occlusion_attachment = {};
  ImageAttachment contact_shadows_attachment = {};
  ImageAttachment resolved_shadows_attachment = {};
};

// What the post passes share (RendererInstance.hpp:344-351 of the reference, the members apply_eye_adaptation reads): final_attachment is the
// linear buffer apply_pbr wrote, in the format gpu_scene_flags' TransparentBackground picks.
struct Extent3D {
  uint32_t width = 0, height = 0, depth = 1;
};
// A mip pyramid of the final attachment's format in one allocation (oxc_image_pyramid): the stand-in for the two bloom images.
using ImagePyramid = oxc_image_pyramid;
// RendererInstance.hpp:327-342 of the reference: the debug view's settings and attachments under the reference's names.  debug_view is
// GPU::DebugView as OXC_DEBUG_VIEW_* (0 = None).  What the reference takes from the instance for the RMVSM view -- the VSM shape constants,
// first_clipmap_width, clipmap_selection_bias and the camera -- is carried in `vsm` (its depth, normal, physical-page and output fields are
// not read), and `debug_attachment`, which the reference declares inside the pass, is caller-owned.
struct DebugContext {
  float overdraw_heatmap_scale = 0.0f;
  uint32_t debug_view = 0;
  Buffer vsm_clipmaps_buffer = {};
  Buffer visbuffer_attachment = {};
  ImageAttachment depth_attachment = {};
  Buffer overdraw_attachment = {};
  Buffer albedo_attachment = {};
  Buffer normal_attachment = {};
  Buffer emissive_attachment = {};
  Buffer metallic_roughness_occlusion_attachment = {};
  Buffer ambient_occlusion_attachment = {};
  Buffer vsm_page_table_attachment = {};
  ShadowResolveContext vsm = {};
  Buffer debug_attachment = {};
};

// The editor's selection path (OxylusEditor/src/Panels/ViewportPanel.cpp:1166-1556).  The reference keeps these values in lambda captures and
// push-constant blocks; the names are its own.  HighlightContext: highlight_mask_stage's transform_indices and terrain_transform_index, the
// shared `silhouette_mask` (here one bit per pixel, mask_bits, with the R8 image optional), and highlight_composite_stage's push constants
// and attachments; outlined_composite, which the reference declares inside the pass, is caller-owned.
struct HighlightContext {
  Buffer transform_indices = {};  // u32 per selected transform
  uint32_t terrain_transform_index = ~0u;
  Buffer visbuffer_attachment = {};
  Buffer silhouette_mask_bits = {};  // u64 [height][ceil(width / 64)]
  Buffer silhouette_mask = {};       // optional: the R8 image
  ImageAttachment depth_attachment = {};
  float outline_color[4] = {1.0f, 0.53f, 0.0f, 1.0f};
  int32_t dilate_radius = 8;
  int32_t outline_width = 5;
  int32_t occluded_mode = 2;  // OccludeMode::AlwaysVisible
  Buffer outlined_composite = {};
};
// mouse_picking_stages: the texel under the cursor and the u32 the pass writes
struct PickingContext {
  uint32_t picking_texel[2] = {0, 0};
  uint32_t terrain_transform_index = ~0u;
  Buffer visbuffer_attachment = {};
  Buffer transform_id = {};
};

// The 2D block of the render function (RendererInstance.cpp:1080-1223): what `2d_forward_vis_pass` and `2d_forward_pass` capture and bind.  The
// sprites are one DrawBatch2D of the render queue's GPU::SpriteGPUData (oxc_pack_sprite and oxc_sort_sprites fill and sort the queue on the
// host); the world matrices are prepared_frame.transforms_world_buffer, the materials prepared_frame.materials_buffer.
struct SpriteContext {
  Buffer sprites_buffer = {};       // the render queue's vertex buffer
  uint32_t batch_offset = 0;        // DrawBatch2D::offset
  uint32_t batch_count = 0;         // DrawBatch2D::count
  float projection_view[16] = {};   // camera_buffer->projection_view
  Buffer visbuffer_attachment_2d = {};
};
// mouse_picking_2d: the texel under the cursor and the u32 the pass writes
struct SpritePickingContext {
  uint32_t picking_texel[2] = {0, 0};
  Buffer visbuffer_attachment_2d = {};
  Buffer transform_id = {};
};

struct PostProcessContext {
  float delta_time = 0.0f;
  Extent3D extent = {};
  Buffer final_attachment = {};
  ImagePyramid bloom_upsampled_attachment = {};  // extent / 2, Texture::calculate_mip_count levels (RendererInstance.cpp:1257-1267); written by apply_bloom
  float bloom_intensity = 0.0f;                  // set by apply_bloom, read by apply_tonemap
  Buffer dst_attachment = {};                    // the 8-bit image apply_tonemap writes, one u32 per pixel
  Buffer fxaa_attachment = {};                   // the image apply_fxaa writes with HasFXAA: final_attachment's extent and format
};

// RendererInstance.hpp:294-300 of the reference: the four sky LUTs, linear u16x4 buffers of the extents the Atmosphere record names, and the
// sky cubemap, u16x4 [6][32][32], which the owner zeroes once (the reference clears it in its constructor).
struct AtmosphereContext {
  Buffer sky_transmittance_lut_attachment = {};
  Buffer sky_multiscatter_lut_attachment = {};
  Buffer sky_view_lut_attachment = {};
  Buffer sky_aerial_perspective_lut_attachment = {};
  Buffer sky_cubemap_attachment = {};
};

// The five pp.bloom_* cvars apply_bloom reads, with the engine's defaults (RendererCVar.cpp:44-48)
struct BloomCVars {
  float threshold = 1.0f;
  float soft_threshold = 0.125f;
  float radius = 0.75f;
  float intensity = 0.1f;
  float clamp = 4.0f;
};

namespace GPU {
// SceneGPU.hpp:295-302
struct PostProcessSettings {
  float exposure = 1.0f;
  float chromatic_aberration_amount = 0.5f;
  float vignette_amount = 0.5f;
  float film_grain_scale = 1.0f;
  float film_grain_amount = 0.5f;
  uint32_t film_grain_seed = 0;
};
// SceneGPU.hpp:304-309
enum struct TonemapType : uint32_t {
  None = 0,
  ACES,
  AgX,
  GT7,
};
// SceneGPU.hpp:278-284
struct HistogramLuminanceInfo {
  float min_exposure = -6.0f;
  float max_exposure = 18.0f;
  float adaptation_speed = 1.1f;
  float ev100_bias = 1.0f;
};
// scene.slang:236-240
struct Sky {
  float solid_color[4] = {0.0f, 0.0f, 0.0f, 1.0f};
  float ambient_color[3] = {0.0f, 0.0f, 0.0f};
  uint32_t has_texture = 0;
};
// scene.slang:264-268
struct DirectionalLight {
  float color[3] = {1.0f, 1.0f, 1.0f};
  float intensity = 0.0f;
  float direction[3] = {0.0f, 1.0f, 0.0f};
};
// the GPU::Camera fields apply_pbr reads
struct Camera {
  float inv_projection_view[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  float position[3] = {0.0f, 0.0f, 0.0f};
};
}  // namespace GPU

class RendererInstance {
public:
  explicit RendererInstance(int device = 0, void* hip_stream = nullptr) : stream_(hip_stream) {
    if (oxc_create(device, &ctx_) != OXC_OK) throw std::runtime_error("oxc_create failed");
  }
  ~RendererInstance() { oxc_destroy(ctx_); }
  RendererInstance(const RendererInstance&) = delete;
  RendererInstance& operator=(const RendererInstance&) = delete;

  PreparedFrame prepared_frame = {};
  // what apply_pbr takes from the instance in the reference: gpu_scene_flags (the specialisation constant), directional_light (sun_dir,
  // sun_intensity), sky_data (the Sky record) and the camera buffer's contents
  uint32_t gpu_scene_flags = 0;  // GPU::SceneFlags, OXC_SCENE_*
  GPU::DirectionalLight directional_light = {};
  GPU::Sky sky_data = {};
  GPU::Camera camera = {};
  oxc_atmosphere atmosphere = {};                   // prepared_frame.atmosphere_buffer's contents: read by generate_sky_luts and draw_atmosphere
  Buffer hemisphere_directions = {};                // 64 x float3, the caller's table (the reference embeds its own in the shader)
  GPU::HistogramLuminanceInfo eye_adaptation = {};  // read by apply_eye_adaptation
  GPU::PostProcessSettings post_proces_settings = {};  // read by apply_tonemap (the reference spells it so: RendererInstance.hpp)
  GPU::TonemapType tonemap_type = GPU::TonemapType::AgX;
  Buffer histogram_bin_indices_buffer = {};         // u32[256]: the reference's transient buffer, here caller-owned; this frame's counts after the call

  void set_stream(void* hip_stream) { stream_ = hip_stream; }

  // Oxylus/src/Render/Passes/CullGeometry.cpp:10-59
  auto generate_hiz(MainGeometryContext& context) -> void {
    oxc_main_geometry_context c = {};
    c.struct_size = sizeof c;
    c.depth_attachment = context.depth_attachment;
    c.hiz_attachment = context.hiz_attachment;
    check(oxc_generate_hiz(ctx_, &c, stream_));
  }

  // Oxylus/src/Render/Passes/CullGeometry.cpp:61-404
  auto cull_geometry(CullGeometryContext& context) -> void {
    if (prepared_frame.use_mesh_shaders) throw std::runtime_error("cull_geometry: the mesh-shader path is not available on the compute-only backend");
    oxc_prepared_frame f = {};
    f.mesh_instance_count = prepared_frame.mesh_instance_count;
    f.max_meshlet_instance_count = prepared_frame.max_meshlet_instance_count;
    f.meshes_buffer = prepared_frame.meshes_buffer;
    f.transforms_world_buffer = prepared_frame.transforms_world_buffer;
    f.mesh_instances_buffer = prepared_frame.mesh_instances_buffer;
    f.meshlet_instances_buffer = prepared_frame.meshlet_instances_buffer;
    f.visible_meshlet_instances_indices_buffer = prepared_frame.visible_meshlet_instances_indices_buffer;
    f.meshlet_instance_visibility_mask_buffer = prepared_frame.meshlet_instance_visibility_mask_buffer;
    f.reordered_indices_buffer = prepared_frame.reordered_indices_buffer;
    oxc_cull_geometry_context c = {};
    c.struct_size = sizeof c;
    c.use_hiz = context.use_hiz;
    c.use_hpb = context.use_hpb;
    c.init_cull_meshes = context.init_cull_meshes;
    c.cull_flags = static_cast<uint32_t>(context.cull_flags);
    c.cull_camera = context.cull_camera;
    c.hiz_attachment = context.hiz_attachment;
    c.hpb_attachment = context.hpb_attachment;
    c.vsm_clipmaps_buffer = context.vsm_clipmaps_buffer;
    c.vsm_clipmap_dirty_flags_buffer = context.vsm_clipmap_dirty_flags_buffer;
    c.vsm_clipmap_count = context.vsm_clipmap_count;
    c.wide_triangle_index = context.wide_triangle_index;
    c.small_triangle_cull = context.small_triangle_cull;
    c.async_triangles = context.async_triangles;
    c.share_pass_tests = context.share_pass_tests;
    c.unordered_output = context.unordered_output;
    c.implicit_meshlet_instances = context.implicit_meshlet_instances;
    c.meshlet_instance_runs_buffer = context.meshlet_instance_runs_buffer;
    c.visibility_buffer = context.visibility_buffer;
    c.cull_meshlets_cmd_buffer = context.cull_meshlets_cmd_buffer;
    check(oxc_cull_geometry(ctx_, &f, &c, stream_));
    context.visibility_buffer = c.visibility_buffer;
    context.cull_meshlets_cmd_buffer = c.cull_meshlets_cmd_buffer;
    context.cull_triangles_cmd_buffer = c.cull_triangles_cmd_buffer;
    context.draw_geometry_cmd_buffer = c.draw_geometry_cmd_buffer;
  }

  // The stream waits for every cull_triangles stage still in flight (async_triangles); draw_for_visbuffer joins by itself.
  auto join_triangles() -> void { check(oxc_join_triangles(ctx_, stream_)); }

  // Oxylus/src/Render/Passes/DrawGeometry.cpp:104-190 for the compute-only backend: the triangles of context.draw_geometry_cmd_buffer
  // (prepared_frame.reordered_indices_buffer, as vs_main decodes them) into depth_attachment / visbuffer_attachment, with
  // context.cull_camera.projection_view as Camera::projection_view.  Rules: include/oxcull.h, oxc_draw_visbuffer.
  auto draw_for_visbuffer(MainGeometryContext& context) -> void {
    if (prepared_frame.use_mesh_shaders) throw std::runtime_error("draw_for_visbuffer: the mesh-shader path is not available on the compute-only backend");
    oxc_prepared_frame f = {};
    f.mesh_instance_count = prepared_frame.mesh_instance_count;
    f.max_meshlet_instance_count = prepared_frame.max_meshlet_instance_count;
    f.meshes_buffer = prepared_frame.meshes_buffer;
    f.transforms_world_buffer = prepared_frame.transforms_world_buffer;
    f.mesh_instances_buffer = prepared_frame.mesh_instances_buffer;
    f.meshlet_instances_buffer = prepared_frame.meshlet_instances_buffer;
    f.visible_meshlet_instances_indices_buffer = prepared_frame.visible_meshlet_instances_indices_buffer;
    f.meshlet_instance_visibility_mask_buffer = prepared_frame.meshlet_instance_visibility_mask_buffer;
    f.reordered_indices_buffer = prepared_frame.reordered_indices_buffer;
    oxc_draw_context d = {};
    d.struct_size = sizeof d;
    d.wide_triangle_index = context.wide_triangle_index;
    d.clear = context.clear;
    d.width = context.depth_attachment.width;
    d.height = context.depth_attachment.height;
    for (int i = 0; i < 16; i++) d.projection_view[i] = context.cull_camera.projection_view[i];
    d.draw_geometry_cmd_buffer = context.draw_geometry_cmd_buffer;
    d.visdepth_buffer = context.visdepth_buffer;
    d.depth_attachment = context.depth_attachment;
    d.visbuffer_attachment = context.visbuffer_attachment;
    check(oxc_draw_visbuffer(ctx_, &f, &d, stream_));
  }

  // Oxylus/src/Render/Passes/DrawGeometry.cpp:192-274, the full-screen pass after the draw (RendererInstance.cpp:924): the four G-buffer
  // images from visbuffer_attachment / depth_attachment, with context.cull_camera.projection_view as Camera::projection_view and
  // prepared_frame.materials_buffer.  Without tables: material factors only, no texture sampling (oxc_decode_visbuffer).  With the image
  // and sampler tables -- what the engine binds as global_images and global_samplers -- the whole shader: the five material images through
  // SampleGrad by the stated rule, the normal map, with context.cull_camera.position as Camera::position (oxc_decode_visbuffer_textured).
  // Rules: include/oxcull.h.
  auto decode_visbuffer(MainGeometryContext& context, Buffer images = {}, Buffer samplers = {}) -> void {
    oxc_prepared_frame f = {};
    f.mesh_instance_count = prepared_frame.mesh_instance_count;
    f.max_meshlet_instance_count = prepared_frame.max_meshlet_instance_count;
    f.meshes_buffer = prepared_frame.meshes_buffer;
    f.transforms_world_buffer = prepared_frame.transforms_world_buffer;
    f.mesh_instances_buffer = prepared_frame.mesh_instances_buffer;
    f.meshlet_instances_buffer = prepared_frame.meshlet_instances_buffer;
    oxc_decode_context d = {};
    d.struct_size = sizeof d;
    d.width = context.depth_attachment.width;
    d.height = context.depth_attachment.height;
    d.clear = 1;  // the engine clears the four images to black before the pass
    d.meshlet_instance_count = static_cast<uint32_t>(prepared_frame.meshlet_instances_buffer.bytes / 8u);
    d.material_count = static_cast<uint32_t>(prepared_frame.materials_buffer.bytes / 56u);
    for (int i = 0; i < 16; i++) d.projection_view[i] = context.cull_camera.projection_view[i];
    d.visbuffer_attachment = context.visbuffer_attachment;
    d.depth_attachment = context.depth_attachment;
    d.materials_buffer = prepared_frame.materials_buffer;
    d.albedo_attachment = context.albedo_attachment;
    d.normal_attachment = context.normal_attachment;
    d.emissive_attachment = context.emissive_attachment;
    d.metallic_roughness_occlusion_attachment = context.metallic_roughness_occlusion_attachment;
    if (!images.dptr && !samplers.dptr) {
      check(oxc_decode_visbuffer(ctx_, &f, &d, stream_));
      return;
    }
    oxc_material_images m = {};
    m.struct_size = sizeof m;
    for (int i = 0; i < 3; i++) m.camera_position[i] = context.cull_camera.position[i];
    m.image_count = static_cast<uint32_t>(images.bytes / sizeof(oxc_material_image));
    m.sampler_count = static_cast<uint32_t>(samplers.bytes / sizeof(oxc_material_sampler));
    m.images_buffer = images;
    m.samplers_buffer = samplers;
    check(oxc_decode_visbuffer_textured(ctx_, &f, &d, &m, stream_));
  }

  // Oxylus/src/Render/Passes/Terrain.cpp:159-216 (the reference's TerrainContext carries the Terrain object; here its GPU-side fields)
  auto cull_terrain(oxc_terrain_context& context) -> void {
    context.struct_size = sizeof context;
    check(oxc_cull_terrain(ctx_, &context, stream_));
  }

  // Producers around the cull path: the downsample_hpb_pass of draw_virtual_shadowmap
  // (Passes/Shadowmaps.cpp:331-366) and the per-meshlet bounds loop of the asset import
  // (Asset/AssetManager_GLTF.cpp:573-578,683-744).
  auto generate_hpb(oxc_buffer virtual_page_table, const oxc_image_array_u8& hpb_attachment) -> void {
    check(oxc_generate_hpb(ctx_, virtual_page_table, &hpb_attachment, stream_));
  }
  // the page-management passes of draw_virtual_shadowmap (Passes/Shadowmaps.cpp:143-421): mark, allocate and invalidate pages
  auto update_virtual_shadowmap(const oxc_vsm_update_context& context) -> void {
    check(oxc_update_virtual_shadowmap(ctx_, &context, stream_));
  }
  // the shadow draw of draw_virtual_shadowmap (Passes/Shadowmaps.cpp:466-754: rmvsm_build_draw_commands + rmvsm_draw_physical_pages) for
  // the compute-only backend: the triangles of the use_hpb cull (context.draw_geometry_cmd_buffer) into the dirty physical pages.
  // Rules: include/oxcull.h, oxc_draw_physical_pages.
  auto draw_physical_pages(oxc_vsm_draw_context context) -> void {
    if (prepared_frame.use_mesh_shaders) throw std::runtime_error("draw_physical_pages: the mesh-shader path is not available on the compute-only backend");
    oxc_prepared_frame f = {};
    f.mesh_instance_count = prepared_frame.mesh_instance_count;
    f.max_meshlet_instance_count = prepared_frame.max_meshlet_instance_count;
    f.meshes_buffer = prepared_frame.meshes_buffer;
    f.transforms_world_buffer = prepared_frame.transforms_world_buffer;
    f.mesh_instances_buffer = prepared_frame.mesh_instances_buffer;
    f.meshlet_instances_buffer = prepared_frame.meshlet_instances_buffer;
    f.visible_meshlet_instances_indices_buffer = prepared_frame.visible_meshlet_instances_indices_buffer;
    f.meshlet_instance_visibility_mask_buffer = prepared_frame.meshlet_instance_visibility_mask_buffer;
    f.reordered_indices_buffer = prepared_frame.reordered_indices_buffer;
    context.struct_size = sizeof context;
    check(oxc_draw_physical_pages(ctx_, &f, &context, stream_));
  }
  // RendererInstance::resolve_shadowmap (Passes/Shadowmaps.cpp:756-822, pipeline resolve_shadowmaps): the PCSS light-visibility value of
  // every pixel from the page table and the physical pages, directly after the shadow draw (RendererInstance.cpp:974-985).
  // Rules: include/oxcull.h, oxc_resolve_shadowmap.
  auto resolve_shadowmap(ShadowResolveContext context) -> void {
    context.struct_size = sizeof context;
    check(oxc_resolve_shadowmap(ctx_, &context, stream_));
  }
  // The contact_shadows pass, inline in RendererInstance::render (RendererInstance.cpp:990-1020, directly after resolve_shadowmap); the
  // shim gives it a name.  pbr_apply multiplies its output with resolve_shadowmap's.  Rules: include/oxcull.h, oxc_contact_shadows.
  auto contact_shadows(ContactShadowsContext context) -> void {
    context.struct_size = sizeof context;
    check(oxc_contact_shadows(ctx_, &context, stream_));
  }
  // RendererInstance::generate_ambient_occlusion (Passes/PBR.cpp:179-311), the call after the contact shadows (RendererInstance.cpp:1040-1055):
  // vbgtao_prefilter, vbgtao_main and vbgtao_denoise.  Rules: include/oxcull.h, oxc_generate_ambient_occlusion.
  auto generate_ambient_occlusion(AmbientOcclusionContext context) -> void {
    context.struct_size = sizeof context;
    check(oxc_generate_ambient_occlusion(ctx_, &context, stream_));
  }
  // RendererInstance::apply_pbr (Passes/PBR.cpp:313-534): the lit HDR colour of every pixel into dst_attachment -- B10G11R11 UfloatPack32 (u32
  // per pixel), or R16G16B16A16 Sfloat (u16x4 per pixel) with TransparentBackground in gpu_scene_flags (RendererInstance.cpp:545-546).  It
  // dispatches on HasAtmosphere as PBR.cpp:318 does: with the flag the atmosphere branch (pipeline pbr_apply) from `atmosphere`,
  // directional_light, camera, the context's four sky images and the 32-texel cube; without it the no-atmosphere branch (pbr_apply_no_atmos)
  // with sky_data.  Rules: include/oxcull.h, oxc_apply_pbr_atmosphere and oxc_apply_pbr.
  auto apply_pbr(PBRContext& context, Buffer dst_attachment) -> Buffer {
    if (gpu_scene_flags & OXC_SCENE_HAS_ATMOSPHERE) {
      oxc_pbr_atmosphere_context c = {};
      c.struct_size = sizeof c;
      c.width = context.depth_attachment.width;
      c.height = context.depth_attachment.height;
      c.scene_flags = gpu_scene_flags;
      c.light_count = static_cast<uint32_t>(prepared_frame.lights_buffer.bytes / 64u);
      for (int i = 0; i < 16; i++) c.inv_projection_view[i] = camera.inv_projection_view[i];
      for (int i = 0; i < 3; i++) c.camera_position[i] = camera.position[i], c.sun_dir[i] = directional_light.direction[i];
      c.sun_intensity = directional_light.intensity;
      c.atmosphere = atmosphere;
      c.cube_size = 32;
      c.depth_attachment = context.depth_attachment;
      c.albedo_attachment = context.albedo_attachment;
      c.normal_attachment = context.normal_attachment;
      c.emissive_attachment = context.emissive_attachment;
      c.metallic_roughness_occlusion_attachment = context.metallic_roughness_occlusion_attachment;
      c.ambient_occlusion_attachment = context.ambient_occlusion_attachment;
      c.resolved_shadows_attachment = context.resolved_shadows_attachment;
      c.contact_shadows_attachment = context.contact_shadows_attachment;
      c.lights_buffer = prepared_frame.lights_buffer;
      c.sky_transmittance_lut = context.sky_transmittance_lut_attachment;
      c.sky_view_lut = context.sky_view_lut_attachment;
      c.sky_aerial_perspective_lut = context.sky_aerial_perspective_lut_attachment;
      c.sky_cubemap = context.sky_cubemap_attachment;
      c.final_attachment = dst_attachment;
      check(oxc_apply_pbr_atmosphere(ctx_, &c, stream_));
      return dst_attachment;
    }
    oxc_pbr_context c = {};
    c.struct_size = sizeof c;
    c.width = context.depth_attachment.width;
    c.height = context.depth_attachment.height;
    c.scene_flags = gpu_scene_flags;
    c.light_count = static_cast<uint32_t>(prepared_frame.lights_buffer.bytes / 64u);
    c.sky_has_texture = sky_data.has_texture;
    for (int i = 0; i < 16; i++) c.inv_projection_view[i] = camera.inv_projection_view[i];
    for (int i = 0; i < 3; i++) {
      c.camera_position[i] = camera.position[i];
      c.sun_dir[i] = directional_light.direction[i];
      c.base_ambient_color[i] = 0.03f;  // glm::vec3(0.03f), PBR.cpp:480
      c.sky_ambient_color[i] = sky_data.ambient_color[i];
    }
    for (int i = 0; i < 4; i++) c.sky_solid_color[i] = sky_data.solid_color[i];
    c.sun_intensity = directional_light.intensity;
    c.depth_attachment = context.depth_attachment;
    c.albedo_attachment = context.albedo_attachment;
    c.normal_attachment = context.normal_attachment;
    c.emissive_attachment = context.emissive_attachment;
    c.metallic_roughness_occlusion_attachment = context.metallic_roughness_occlusion_attachment;
    c.ambient_occlusion_attachment = context.ambient_occlusion_attachment;
    c.resolved_shadows_attachment = context.resolved_shadows_attachment;
    c.contact_shadows_attachment = context.contact_shadows_attachment;
    c.lights_buffer = prepared_frame.lights_buffer;
    c.final_attachment = dst_attachment;
    check(oxc_apply_pbr(ctx_, &c, stream_));
    return dst_attachment;
  }
  // The pair the reference builds in its constructor (RendererInstance.cpp:136-251): sky_transmittance_lut, then sky_multiscatter_lut from it.
  // Called once the `atmosphere` record and `hemisphere_directions` are set, and again whenever the record changes.  Rules: include/oxcull.h,
  // oxc_generate_sky_luts.
  auto generate_sky_luts(AtmosphereContext& context) -> void {
    oxc_sky_lut_context c = {};
    c.struct_size = sizeof c;
    c.atmosphere = atmosphere;
    c.hemisphere_directions = hemisphere_directions;
    c.sky_transmittance_lut = context.sky_transmittance_lut_attachment;
    c.sky_multiscatter_lut = context.sky_multiscatter_lut_attachment;
    check(oxc_generate_sky_luts(ctx_, &c, stream_));
  }
  // RendererInstance::draw_atmosphere (Passes/PBR.cpp:9-141) without its sky_ibl pass: sky_view_lut and sky_aerial_perspective_lut from the
  // two LUTs above, directional_light and camera.  Rules: include/oxcull.h, oxc_draw_atmosphere.
  auto draw_atmosphere(AtmosphereContext& context) -> void {
    oxc_atmosphere_context c = {};
    c.struct_size = sizeof c;
    c.atmosphere = atmosphere;
    for (int i = 0; i < 3; i++) c.sun_dir[i] = directional_light.direction[i], c.camera_position[i] = camera.position[i];
    c.sun_intensity = directional_light.intensity;
    for (int i = 0; i < 16; i++) c.camera_inv_projection_view[i] = camera.inv_projection_view[i];
    c.sky_transmittance_lut = context.sky_transmittance_lut_attachment;
    c.sky_multiscatter_lut = context.sky_multiscatter_lut_attachment;
    c.sky_view_lut = context.sky_view_lut_attachment;
    c.sky_aerial_perspective_lut = context.sky_aerial_perspective_lut_attachment;
    check(oxc_draw_atmosphere(ctx_, &c, stream_));
  }
  // The sky_ibl pass of RendererInstance::draw_atmosphere (Passes/PBR.cpp:52-94), after draw_atmosphere: 64 samples of sky_view_lut per texel of
  // the 32 x 32 x 6 cube, blended into the cube's own history.  frame_index is render_context->num_frames; 0.15f is the sun_ambient_strength the
  // engine pushes.  Rules: include/oxcull.h, oxc_generate_sky_ibl.
  auto generate_sky_ibl(AtmosphereContext& context, uint32_t frame_index) -> void {
    oxc_sky_ibl_context c = {};
    c.struct_size = sizeof c;
    c.atmosphere = atmosphere;
    for (int i = 0; i < 3; i++) c.sun_dir[i] = directional_light.direction[i], c.camera_position[i] = camera.position[i];
    c.sun_intensity = directional_light.intensity;
    c.sun_ambient_strength = 0.15f;
    c.frame_index = frame_index;
    c.cube_size = 32;
    c.sky_view_lut = context.sky_view_lut_attachment;
    c.sky_transmittance_lut = context.sky_transmittance_lut_attachment;
    c.sky_cubemap = context.sky_cubemap_attachment;
    check(oxc_generate_sky_ibl(ctx_, &c, stream_));
  }
  // The `fxaa` pass (RendererInstance.cpp:1225-1255), between apply_pbr and apply_eye_adaptation: with HasFXAA in gpu_scene_flags, edge
  // anti-aliasing of context.final_attachment into context.fxaa_attachment, which is then handed on as context.final_attachment (the
  // reference's std::tie swaps the two names); without the flag nothing runs.  Rules: include/oxcull.h, oxc_apply_fxaa.
  auto apply_fxaa(PostProcessContext& context) -> void {
    if (!(gpu_scene_flags & OXC_SCENE_HAS_FXAA)) return;
    oxc_fxaa_context c = {};
    c.struct_size = sizeof c;
    c.width = context.extent.width;
    c.height = context.extent.height;
    c.source_format = (gpu_scene_flags & OXC_SCENE_TRANSPARENT_BACKGROUND) ? 1u : 0u;
    c.final_attachment = context.final_attachment;
    c.fxaa_attachment = context.fxaa_attachment;
    check(oxc_apply_fxaa(ctx_, &c, stream_));
    std::swap(context.final_attachment, context.fxaa_attachment);
  }
  // RendererInstance::apply_eye_adaptation (Passes/PostProcess.cpp:7-77): the luminance histogram of context.final_attachment into
  // histogram_bin_indices_buffer and the adapted luminance and exposure into prepared_frame.exposure_buffer.  time_coeff is computed here
  // with this platform's expf (PostProcess.cpp:63).  Rules: include/oxcull.h, oxc_apply_eye_adaptation.
  auto apply_eye_adaptation(PostProcessContext& context) -> void {
    oxc_eye_adaptation_context c = {};
    c.struct_size = sizeof c;
    c.width = context.extent.width;
    c.height = context.extent.height;
    c.source_format = (gpu_scene_flags & OXC_SCENE_TRANSPARENT_BACKGROUND) ? 1u : 0u;
    c.min_exposure = eye_adaptation.min_exposure;
    c.max_exposure = eye_adaptation.max_exposure;
    c.ev100_bias = eye_adaptation.ev100_bias;
    c.time_coeff = 1.0f - std::exp(-eye_adaptation.adaptation_speed * context.delta_time);
    c.final_attachment = context.final_attachment;
    c.histogram_buffer = histogram_bin_indices_buffer;
    c.exposure_buffer = prepared_frame.exposure_buffer;
    check(oxc_apply_eye_adaptation(ctx_, &c, stream_));
  }
  // RendererInstance::apply_bloom (Passes/PostProcess.cpp:79-203): the prefiltered half-resolution image and its downsample pyramid into
  // bloom_downsampled_attachment (the reference declares it inside the pass; here caller-owned, of bloom_upsampled_attachment's shape), the
  // upsample pyramid into context.bloom_upsampled_attachment.  The exposure is read from prepared_frame.exposure_buffer when gpu_scene_flags
  // has HasEyeAdaptation.  Rules: include/oxcull.h, oxc_apply_bloom.
  auto apply_bloom(PostProcessContext& context, const BloomCVars& cvar, const ImagePyramid& bloom_downsampled_attachment) -> void {
    context.bloom_intensity = cvar.intensity;
    oxc_bloom_context c = {};
    c.struct_size = sizeof c;
    c.width = context.extent.width;
    c.height = context.extent.height;
    c.source_format = (gpu_scene_flags & OXC_SCENE_TRANSPARENT_BACKGROUND) ? 1u : 0u;
    c.scene_flags = gpu_scene_flags;
    c.threshold = cvar.threshold;
    c.soft_threshold = cvar.soft_threshold;
    c.clamp_value = cvar.clamp;
    c.radius = cvar.radius;
    c.final_attachment = context.final_attachment;
    c.exposure_buffer = prepared_frame.exposure_buffer;
    c.bloom_downsampled_attachment = bloom_downsampled_attachment;
    c.bloom_upsampled_attachment = context.bloom_upsampled_attachment;
    check(oxc_apply_bloom(ctx_, &c, stream_));
  }
  // RendererInstance::apply_tonemap (Passes/PostProcess.cpp:205-247): exposure, bloom composite, tone curve, lens effects and the 8-bit store
  // of context.final_attachment into context.dst_attachment, whose format (the swapchain's: 0 R8G8B8A8 Srgb, 1 B8G8R8A8 Srgb; 2 R8G8B8A8 Unorm)
  // the caller names.  Reads post_proces_settings and tonemap_type (the reference's spelling), gpu_scene_flags, context.bloom_intensity as
  // apply_bloom left it, and prepared_frame.exposure_buffer.  Rules: include/oxcull.h, oxc_apply_tonemap.
  auto apply_tonemap(PostProcessContext& context, uint32_t dst_format = 0) -> Buffer {
    oxc_tonemap_context c = {};
    c.struct_size = sizeof c;
    c.width = context.extent.width;
    c.height = context.extent.height;
    c.source_format = (gpu_scene_flags & OXC_SCENE_TRANSPARENT_BACKGROUND) ? 1u : 0u;
    c.output_format = dst_format;
    c.scene_flags = gpu_scene_flags;
    c.tonemap_type = static_cast<uint32_t>(tonemap_type);
    c.exposure = post_proces_settings.exposure;
    c.chromatic_aberration_amount = post_proces_settings.chromatic_aberration_amount;
    c.vignette_amount = post_proces_settings.vignette_amount;
    c.film_grain_scale = post_proces_settings.film_grain_scale;
    c.film_grain_amount = post_proces_settings.film_grain_amount;
    c.film_grain_seed = post_proces_settings.film_grain_seed;
    c.bloom_intensity = context.bloom_intensity;
    c.final_attachment = context.final_attachment;
    c.bloom_upsampled_attachment = context.bloom_upsampled_attachment;
    c.exposure_buffer = prepared_frame.exposure_buffer;
    c.dst_attachment = context.dst_attachment;
    check(oxc_apply_tonemap(ctx_, &c, stream_));
    return context.dst_attachment;
  }
  // The terrain map producers (Scene/Terrain.cpp:406-461, Passes/Terrain.cpp:134-156): the stages of context.stages in the order generate,
  // derive, minmax.  The three free functions below, with the reference's names, each run one.  Rules: include/oxcull.h,
  // oxc_generate_terrain_maps.
  auto generate_terrain_maps(oxc_terrain_maps_context context) -> void {
    context.struct_size = sizeof context;
    check(oxc_generate_terrain_maps(ctx_, &context, stream_));
  }
  // The terrain brush (Passes/Terrain.cpp:35-132): the stages of context.stages in the order trace, apply.  The free function
  // apply_terrain_brush below does what the reference's method does after its params are built.  Rules: include/oxcull.h,
  // oxc_apply_terrain_brush.
  auto apply_terrain_brush(oxc_terrain_brush_context context) -> void {
    context.struct_size = sizeof context;
    check(oxc_apply_terrain_brush(ctx_, &context, stream_));
  }
  // The terrain decode (Passes/Terrain.cpp:279-360): the four G-buffer images at the terrain pixels, after decode_visbuffer on the same
  // attachments.  The free function decode_terrain below has the reference's name and argument shape.  Rules: include/oxcull.h,
  // oxc_decode_terrain.
  auto decode_terrain(oxc_terrain_decode_context context) -> void {
    context.struct_size = sizeof context;
    check(oxc_decode_terrain(ctx_, &context, stream_));
  }
  // RendererInstance::draw_terrain_for_visbuffer (Passes/Terrain.cpp:218-277, pipeline terrain_visbuffer): the visible patches of the terrain
  // cull, tessellated by the stated rules, into the depth|vis image of draw_for_visbuffer.  projection_scale is the engine's resolution.y *
  // 0.5 / tan(radians(fov) * 0.5), evaluated in binary64 and rounded once by terrain_projection_scale.  Rules: include/oxcull.h,
  // oxc_draw_terrain.
  auto draw_terrain_for_visbuffer(oxc_terrain_draw_context context) -> void {
    context.struct_size = sizeof context;
    check(oxc_draw_terrain(ctx_, &context, stream_));
  }
  static auto terrain_projection_scale(double resolution_y, double fov_degrees) -> float {
    return static_cast<float>(resolution_y * 0.5 / std::tan(fov_degrees * 3.14159265358979323846 / 180.0 * 0.5));
  }
  // RendererInstance::apply_debug_view (Passes/Debug.cpp:9-153, pipelines debug_view and rmvsm_debug): the picture of context.debug_view
  // into context.debug_attachment, cleared to black first as the reference's clear_image does; with no mesh instance in the frame the six
  // geometry views return the cleared image (Debug.cpp:36-49), here without a launch on an image the caller cleared.  Rules:
  // include/oxcull.h, oxc_apply_debug_view.
  auto apply_debug_view(DebugContext& context, Extent3D extent) -> Buffer {
    if (prepared_frame.mesh_instance_count == 0 && context.debug_view >= OXC_DEBUG_VIEW_TRIANGLES && context.debug_view <= OXC_DEBUG_VIEW_MESH_LODS)
      return context.debug_attachment;
    oxc_prepared_frame f = {};
    f.mesh_instance_count = prepared_frame.mesh_instance_count;
    f.max_meshlet_instance_count = prepared_frame.max_meshlet_instance_count;
    f.meshes_buffer = prepared_frame.meshes_buffer;
    f.mesh_instances_buffer = prepared_frame.mesh_instances_buffer;
    f.meshlet_instances_buffer = prepared_frame.meshlet_instances_buffer;
    oxc_debug_view_context c = {};
    c.struct_size = sizeof c;
    c.width = extent.width;
    c.height = extent.height;
    c.debug_view = context.debug_view;
    c.clear = 1;
    c.heatmap_scale = context.overdraw_heatmap_scale;
    c.meshlet_instance_count = static_cast<uint32_t>(prepared_frame.meshlet_instances_buffer.bytes / 8u);
    const ShadowResolveContext& v = context.vsm;
    c.page_size = v.page_size, c.page_table_size = v.page_table_size, c.physical_page_table_size = v.physical_page_table_size, c.clipmap_count = v.clipmap_count;
    c.first_clipmap_width = v.first_clipmap_width, c.clipmap_selection_bias = v.clipmap_selection_bias, c.virtual_extent = v.virtual_extent;
    for (int i = 0; i < 16; i++) c.inv_projection_view[i] = v.inv_projection_view[i];
    c.resolution[0] = v.resolution[0], c.resolution[1] = v.resolution[1];
    c.visbuffer_attachment = context.visbuffer_attachment;
    c.depth_attachment = context.depth_attachment;
    c.overdraw_attachment = context.overdraw_attachment;
    c.albedo_attachment = context.albedo_attachment;
    c.normal_attachment = context.normal_attachment;
    c.emissive_attachment = context.emissive_attachment;
    c.metallic_roughness_occlusion_attachment = context.metallic_roughness_occlusion_attachment;
    c.ambient_occlusion_attachment = context.ambient_occlusion_attachment;
    c.vsm_clipmaps_buffer = context.vsm_clipmaps_buffer;
    c.virtual_page_table = context.vsm_page_table_attachment;
    c.debug_attachment = context.debug_attachment;
    check(oxc_apply_debug_view(ctx_, &f, &c, stream_));
    return context.debug_attachment;
  }
  // The editor's mouse_picking stage (ViewportPanel.cpp:1439-1497): the transform index behind context.picking_texel into
  // context.transform_id.  Rules: include/oxcull.h, oxc_pick_transform.
  auto pick_transform(PickingContext& context, Extent3D extent) -> Buffer {
    const oxc_prepared_frame f = record_frame();
    oxc_pick_context c = {};
    c.struct_size = sizeof c;
    c.width = extent.width, c.height = extent.height;
    c.x = context.picking_texel[0], c.y = context.picking_texel[1];
    c.terrain_transform_index = context.terrain_transform_index;
    c.meshlet_instance_count = static_cast<uint32_t>(prepared_frame.meshlet_instances_buffer.bytes / 8u);
    c.visbuffer_attachment = context.visbuffer_attachment;
    c.transform_id = context.transform_id;
    check(oxc_pick_transform(ctx_, &f, &c, stream_));
    return context.transform_id;
  }
  // The editor's highlight_mask_stage and highlight_composite_stage (ViewportPanel.cpp:1166-1345) as the stages of `stages`
  // (OXC_HIGHLIGHT_MASK after the visbuffer is drawn, OXC_HIGHLIGHT_COMPOSITE after apply_tonemap): the outline of the selected transforms
  // over original_result_attachment, an image of `dst_format` as apply_tonemap wrote it, into context.outlined_composite.  Rules:
  // include/oxcull.h, oxc_apply_highlight.
  auto apply_highlight(HighlightContext& context, uint32_t stages, Extent3D extent, Buffer original_result_attachment = {}, uint32_t dst_format = 0) -> Buffer {
    const oxc_prepared_frame f = record_frame();
    oxc_highlight_context c = {};
    c.struct_size = sizeof c;
    c.stages = stages;
    c.width = extent.width, c.height = extent.height;
    c.color_format = dst_format;
    c.terrain_transform_index = context.terrain_transform_index;
    c.meshlet_instance_count = static_cast<uint32_t>(prepared_frame.meshlet_instances_buffer.bytes / 8u);
    c.selected_count = static_cast<uint32_t>(context.transform_indices.bytes / 4u);
    for (int i = 0; i < 4; i++) c.outline_color[i] = context.outline_color[i];
    c.dilate_radius = context.dilate_radius, c.outline_width = context.outline_width, c.occluded_mode = context.occluded_mode;
    c.visbuffer_attachment = context.visbuffer_attachment;
    c.transform_indices = context.transform_indices;
    c.mask_bits = context.silhouette_mask_bits;
    c.mask_attachment = context.silhouette_mask;
    c.depth_attachment = context.depth_attachment;
    c.color_attachment = original_result_attachment;
    c.dst_attachment = context.outlined_composite;
    check(oxc_apply_highlight(ctx_, &f, &c, stream_));
    return context.outlined_composite;
  }
  // The 2D block of the render function (RendererInstance.cpp:1080-1223), between apply_pbr and the FXAA pass: `2d_forward_vis_pass` and
  // `2d_forward_pass` as the stages of `stages` over context's batch, onto depth_attachment and final_attachment (an image of `source_format`
  // as apply_pbr wrote it); the engine's clear of visbuffer_attachment_2d is folded in.  Returns final_attachment.  Rules: include/oxcull.h,
  // oxc_draw_sprites.
  auto draw_sprites(SpriteContext& context, uint32_t stages, Extent3D extent, ImageAttachment depth_attachment, Buffer final_attachment = {}, uint32_t source_format = 0)
      -> Buffer {
    oxc_prepared_frame f = {};
    f.transforms_world_buffer = prepared_frame.transforms_world_buffer;
    oxc_sprite_context c = {};
    c.struct_size = sizeof c;
    c.stages = stages;
    c.width = extent.width, c.height = extent.height;
    c.clear = 1;
    c.source_format = source_format;
    c.first_sprite = context.batch_offset, c.sprite_count = context.batch_count;
    c.material_count = static_cast<uint32_t>(prepared_frame.materials_buffer.bytes / 56u);
    c.transform_count = static_cast<uint32_t>(prepared_frame.transforms_world_buffer.bytes / 64u);
    for (int i = 0; i < 16; i++) c.projection_view[i] = context.projection_view[i];
    c.sprites_buffer = context.sprites_buffer;
    c.materials_buffer = prepared_frame.materials_buffer;
    c.depth_attachment = depth_attachment;
    c.visbuffer_2d = context.visbuffer_attachment_2d;
    c.final_attachment = final_attachment;
    check(oxc_draw_sprites(ctx_, &f, &c, stream_));
    return final_attachment;
  }
  // The editor's mouse_picking_2d stage: texel context.picking_texel of visbuffer_attachment_2d into context.transform_id.
  auto pick_sprite(SpritePickingContext& context, Extent3D extent) -> Buffer {
    oxc_sprite_pick_context c = {};
    c.struct_size = sizeof c;
    c.width = extent.width, c.height = extent.height;
    c.x = context.picking_texel[0], c.y = context.picking_texel[1];
    c.visbuffer_2d = context.visbuffer_attachment_2d;
    c.transform_id = context.transform_id;
    check(oxc_pick_sprite(ctx_, &c, stream_));
    return context.transform_id;
  }
  auto build_meshlet_bounds(oxc_meshlet_bounds_desc desc) -> void {
    desc.struct_size = sizeof desc;
    check(oxc_build_meshlet_bounds(ctx_, &desc, stream_));
  }
  // AssetManager_GLTF.cpp:570-588: the three quantised vertex streams of the mesh blob
  auto quantize_vertex_streams(oxc_vertex_streams_desc desc) -> void {
    desc.struct_size = sizeof desc;
    check(oxc_quantize_vertex_streams(ctx_, &desc, stream_));
  }

  oxc_ctx* native() { return ctx_; }

private:
  // the record buffers the editor's passes resolve a visbuffer texel with
  oxc_prepared_frame record_frame() const {
    oxc_prepared_frame f = {};
    f.mesh_instance_count = prepared_frame.mesh_instance_count;
    f.max_meshlet_instance_count = prepared_frame.max_meshlet_instance_count;
    f.mesh_instances_buffer = prepared_frame.mesh_instances_buffer;
    f.meshlet_instances_buffer = prepared_frame.meshlet_instances_buffer;
    return f;
  }
  void check(oxc_status st) {
    if (st != OXC_OK) throw std::runtime_error(std::string("oxcull: ") + oxc_last_error(ctx_));
  }
  oxc_ctx* ctx_ = nullptr;
  void* stream_ = nullptr;
};

namespace GPU {
using TerrainErosion = oxc_terrain_erosion;    // SceneGPU.hpp:358-372, 80 bytes
using TerrainGenerate = oxc_terrain_generate;  // SceneGPU.hpp:374-384, 120 bytes
using TerrainDerive = oxc_terrain_derive;      // SceneGPU.hpp:386-395, 40 bytes
using TerrainBrushParams = oxc_terrain_brush_params;  // scene.slang:606-621, 96 bytes
using TerrainBrushHit = oxc_terrain_brush_hit;        // scene.slang:601-604
using TerrainRegion = oxc_terrain_region;             // scene.slang:588-591
using TerrainData = oxc_terrain_data;                 // scene.slang:634-647, SceneGPU.hpp:440-453, 76 bytes
struct TerrainMinMax {                         // SceneGPU.hpp:397-400
  uint32_t resolution[2] = {};
  uint32_t patch_count[2] = {};
};
}  // namespace GPU

struct uvec2 {  // stands in for glm::uvec2
  uint32_t x = 0, y = 0;
};

// Scene/Terrain.hpp:22-31 of the reference: the seven images and the region record, here linear buffers in the layouts include/oxcull.h
// states (patch_minmax the RG32F image oxc_cull_terrain takes).  `renderer` is what the reference's passes take from the render graph: the
// instance whose context and stream the three passes below run on.
struct TerrainMaps {
  RendererInstance* renderer = nullptr;
  Buffer heightmap = {};
  Buffer ridgemap = {};
  Buffer normalmap = {};
  Buffer splatmap = {};
  ImageAttachment patch_minmax = {};
  Buffer height_edit = {};
  Buffer splat_edit = {};
  Buffer region = {};  // device memory, 16 bytes of GPU::TerrainRegion; {} for zero origins
};

namespace detail {
inline oxc_terrain_maps_context terrain_context(const TerrainMaps& maps, uint32_t stages, const uint32_t* resolution) {
  if (!maps.renderer) throw std::runtime_error("TerrainMaps::renderer is not set");
  oxc_terrain_maps_context c = {};
  c.stages = stages;
  for (int k = 0; k < 2; k++) c.resolution[k] = c.generate.resolution[k] = c.derive.resolution[k] = resolution[k], c.patch_count[k] = 1;
  c.generate.erosion.detail = 1.0f;  // a stage that does not read the record still passes its limit
  c.region = maps.region;
  c.heightmap = maps.heightmap, c.ridgemap = maps.ridgemap, c.normalmap = maps.normalmap, c.splatmap = maps.splatmap;
  c.height_edit = maps.height_edit, c.splat_edit = maps.splat_edit, c.patch_minmax = maps.patch_minmax;
  return c;
}
}  // namespace detail

// Scene/Terrain.hpp:33-35 of the reference, the same names and argument lists
inline auto terrain_generate_pass(TerrainMaps& maps, const GPU::TerrainGenerate& settings, uvec2 dispatch_texels) -> void {
  oxc_terrain_maps_context c = detail::terrain_context(maps, OXC_TERRAIN_GENERATE, settings.resolution);
  c.generate = settings;
  c.dispatch_texels[0] = dispatch_texels.x, c.dispatch_texels[1] = dispatch_texels.y;
  maps.renderer->generate_terrain_maps(c);
}
inline auto terrain_derive_pass(TerrainMaps& maps, const GPU::TerrainDerive& settings, uvec2 dispatch_texels) -> void {
  oxc_terrain_maps_context c = detail::terrain_context(maps, OXC_TERRAIN_DERIVE, settings.resolution);
  c.derive = settings;
  c.dispatch_texels[0] = dispatch_texels.x, c.dispatch_texels[1] = dispatch_texels.y;
  maps.renderer->generate_terrain_maps(c);
}
inline auto terrain_minmax_pass(TerrainMaps& maps, const GPU::TerrainMinMax& settings, uvec2 dispatch_patches) -> void {
  oxc_terrain_maps_context c = detail::terrain_context(maps, OXC_TERRAIN_MINMAX, settings.resolution);
  c.patch_count[0] = settings.patch_count[0], c.patch_count[1] = settings.patch_count[1];
  c.dispatch_patches[0] = dispatch_patches.x, c.dispatch_patches[1] = dispatch_patches.y;
  maps.renderer->generate_terrain_maps(c);
}

// RendererInstance.hpp's TerrainBrushContext of the reference, with the params the method builds from the Terrain (Passes/Terrain.cpp:42-67)
// and the two settings records it copies from it carried beside the maps.  hit_buffer and maps.region are device memory, 16 bytes each.
struct TerrainBrushContext {
  TerrainMaps maps = {};
  Buffer hit_buffer = {};
  GPU::TerrainBrushParams params = {};
  bool painting = false;
  GPU::TerrainGenerate generate_settings = {};  // terrain.generate_settings, terrain.derive_settings with the fields bake fills
  GPU::TerrainDerive derive_settings = {};
};

// RendererInstance::apply_terrain_brush (Passes/Terrain.cpp:69-156) after the params are built: trace; if painting, apply, then the three
// regional passes with the reference's dispatch sizes.
inline auto apply_terrain_brush(TerrainBrushContext& context) -> void {
  if (!context.maps.renderer) throw std::runtime_error("TerrainMaps::renderer is not set");
  const GPU::TerrainBrushParams& params = context.params;
  oxc_terrain_brush_context c = {};
  c.stages = OXC_TERRAIN_BRUSH_TRACE | (context.painting ? OXC_TERRAIN_BRUSH_APPLY : 0u);
  c.params = params;
  c.heightmap = context.maps.heightmap, c.height_edit = context.maps.height_edit, c.splat_edit = context.maps.splat_edit;
  c.hit = context.hit_buffer, c.region = context.maps.region;
  context.maps.renderer->apply_terrain_brush(c);
  if (!context.painting) return;

  GPU::TerrainGenerate generate_settings = context.generate_settings;
  GPU::TerrainDerive derive_settings = context.derive_settings;
  GPU::TerrainMinMax minmax_settings = {};
  for (int k = 0; k < 2; k++) {
    generate_settings.resolution[k] = derive_settings.resolution[k] = minmax_settings.resolution[k] = params.resolution[k];
    minmax_settings.patch_count[k] = params.patch_count[k];
  }
  const uint32_t derive_texels = 2u * static_cast<uint32_t>(std::ceil(params.radius_texels + 1.0f)) + 1u;
  terrain_generate_pass(context.maps, generate_settings, uvec2{derive_texels, derive_texels});
  terrain_derive_pass(context.maps, derive_settings, uvec2{derive_texels, derive_texels});
  const float patch_texels_x = static_cast<float>(params.resolution[0]) / static_cast<float>(params.patch_count[0]);
  const float patch_texels_y = static_cast<float>(params.resolution[1]) / static_cast<float>(params.patch_count[1]);
  const uint32_t derive_patches = static_cast<uint32_t>(std::ceil(static_cast<float>(derive_texels) / std::min(patch_texels_x, patch_texels_y))) + 1u;
  terrain_minmax_pass(context.maps, minmax_settings, uvec2{derive_patches, derive_patches});
}

// RendererInstance.hpp's TerrainDecodeContext of the reference: its buffers and attachments under the reference's names, with what the
// reference takes from the prepared frame (the camera's inv_projection_view, the materials) and from the terrain buffer carried beside them.
struct TerrainDecodeContext {
  RendererInstance* renderer = nullptr;
  GPU::TerrainData terrain = {};  // terrain_buffer
  float inv_projection_view[16] = {};
  uvec2 map_resolution = {};
  Buffer materials_buffer = {};
  uint32_t material_count = 0;
  Buffer brush_hit_buffer = {};
  Buffer visbuffer_attachment = {};
  oxc_image depth_attachment = {};
  Buffer normalmap_attachment = {};
  Buffer splatmap_attachment = {};
  Buffer albedo_attachment = {};
  Buffer normal_attachment = {};
  Buffer emissive_attachment = {};
  Buffer metallic_roughness_occlusion_attachment = {};
};

// RendererInstance::decode_terrain (Passes/Terrain.cpp:279-360)
inline auto decode_terrain(TerrainDecodeContext& context) -> void {
  if (!context.renderer) throw std::runtime_error("TerrainDecodeContext::renderer is not set");
  oxc_terrain_decode_context c = {};
  c.width = context.depth_attachment.width, c.height = context.depth_attachment.height;
  for (int k = 0; k < 16; k++) c.inv_projection_view[k] = context.inv_projection_view[k];
  c.terrain = context.terrain;
  c.map_resolution[0] = context.map_resolution.x, c.map_resolution[1] = context.map_resolution.y;
  c.material_count = context.material_count;
  c.visbuffer_attachment = context.visbuffer_attachment, c.depth_attachment = context.depth_attachment;
  c.normalmap = context.normalmap_attachment, c.splatmap = context.splatmap_attachment;
  c.materials_buffer = context.materials_buffer, c.brush_hit = context.brush_hit_buffer;
  c.albedo_attachment = context.albedo_attachment, c.normal_attachment = context.normal_attachment;
  c.emissive_attachment = context.emissive_attachment, c.metallic_roughness_occlusion_attachment = context.metallic_roughness_occlusion_attachment;
  context.renderer->decode_terrain(c);
}

}  // namespace ox::amd
