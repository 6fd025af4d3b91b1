// oxcull_abi_terrain.cpp -- the terrain map producers of liboxcull.so's C ABI: oxc_generate_terrain_maps (height, ridge, normal, splat and the
// per-patch min / max), oxc_apply_terrain_brush (the brush ray trace and the strokes into the edit images) and oxc_decode_terrain (the
// G-buffer of the terrain pixels, the consumer of the normal map, the splat map and the hit record) -- and oxc_draw_terrain, the tessellated
// patches into the depth|vis image, with its stats reader.  The terrain cull, the consumer of the min / max, is in oxcull_abi_cull.cpp.
#include "oxcull_host.hpp"

namespace {
constexpr uint32_t kStageAll = OXC_TERRAIN_GENERATE | OXC_TERRAIN_DERIVE | OXC_TERRAIN_MINMAX;

// roundup(dispatch, group) as a thread count, capped at roundup(extent, group): what lies beyond cannot land inside the map without wrapping
uint32_t threads_of(uint32_t dispatch, uint32_t extent, uint32_t group) {
  const uint64_t want = ((uint64_t)dispatch + group - 1u) / group * group;
  return (uint32_t)std::min<uint64_t>(want, (extent + group - 1u) / group * group);
}
}  // namespace

extern "C" {

oxc_status oxc_generate_terrain_maps(oxc_ctx* ctx, const oxc_terrain_maps_context* c, void* hip_stream) {
  if (!ctx) return OXC_INVALID_ARG;
  if (!c || c->struct_size != sizeof(oxc_terrain_maps_context)) return fail(ctx, OXC_INVALID_ARG, "generate_terrain_maps: bad context / struct_size");
  const char* const entry = "generate_terrain_maps";
  const uint32_t stages = c->stages;
  if (stages == 0u || (stages & ~kStageAll)) return bad_arg(ctx, entry, "stages must be a non-empty mask of OXC_TERRAIN_GENERATE | OXC_TERRAIN_DERIVE | OXC_TERRAIN_MINMAX");
  const uint32_t *res = c->resolution, *pc = c->patch_count;
  if (res[0] < 1u || res[0] > 16384u || res[1] < 1u || res[1] > 16384u) return bad_arg(ctx, entry, "resolution: every side must be in 1 .. 16384");
  if (pc[0] < 1u || pc[0] > 4096u || pc[1] < 1u || pc[1] > 4096u) return bad_arg(ctx, entry, "patch_count: every side must be in 1 .. 4096");
  if (c->generate.resolution[0] != res[0] || c->generate.resolution[1] != res[1]) return bad_arg(ctx, entry, "generate.resolution must equal resolution");
  if (c->derive.resolution[0] != res[0] || c->derive.resolution[1] != res[1]) return bad_arg(ctx, entry, "derive.resolution must equal resolution");
  if (c->generate.height_octaves > 16u) return bad_arg(ctx, entry, "generate.height_octaves must be at most 16");
  if (c->generate.erosion.octaves > 16u) return bad_arg(ctx, entry, "generate.erosion.octaves must be at most 16");
  if (!std::isfinite(c->generate.erosion.detail) || !(c->generate.erosion.detail > 0.0f)) return bad_arg(ctx, entry, "generate.erosion.detail must be finite and above 0");

  const uint64_t texels = (uint64_t)res[0] * res[1], patches = (uint64_t)pc[0] * pc[1];
  const oxc_image& mm = c->patch_minmax;
  const bool mm_extent = mm.width == pc[0] && mm.height == pc[1] && mm.levels == 1u && mm.level_offset[0] == 0u;
  const uint32_t G = OXC_TERRAIN_GENERATE, D = OXC_TERRAIN_DERIVE, M = OXC_TERRAIN_MINMAX;
  const MapBuffer buffers[] = {
      {"region", c->region.dptr, c->region.bytes, 16u, 8u, kStageAll, 0u, true},
      {"heightmap", c->heightmap.dptr, c->heightmap.bytes, texels * 2u, 2u, kStageAll, G, false},
      {"ridgemap", c->ridgemap.dptr, c->ridgemap.bytes, texels * 2u, 2u, G | D, G, false},
      {"normalmap", c->normalmap.dptr, c->normalmap.bytes, texels * 4u, 4u, D, D, false},
      {"splatmap", c->splatmap.dptr, c->splatmap.bytes, texels * 4u, 4u, D, D, false},
      {"height_edit", c->height_edit.dptr, c->height_edit.bytes, texels * 4u, 4u, G, 0u, false},
      {"splat_edit", c->splat_edit.dptr, c->splat_edit.bytes, texels * 4u, 4u, D, 0u, false},
      {"patch_minmax", mm.dptr, mm_extent ? patches * 8u : 0u, patches * 8u, 8u, M, M, false, " must be one RG32F level at offset 0 of patch_count's extent"},
  };
  if (const oxc_status st = check_buffers(ctx, entry, buffers, stages)) return st;

  OXC_ENTER(ctx, hip_stream, s);
  TerrainMapsArgs a;
  std::memset(&a, 0, sizeof a);
  a.g = c->generate;
  a.d = c->derive;
  for (int k = 0; k < 2; k++) {
    a.res[k] = res[k];
    a.patches[k] = pc[k];
    a.threads_texels[k] = threads_of(c->dispatch_texels[k], res[k], 16u);
    a.threads_patches[k] = threads_of(c->dispatch_patches[k], pc[k], 8u);
  }
  terrain_maps_constants(a);
  a.region = static_cast<const uint32_t*>(c->region.dptr);
  a.heightmap = static_cast<uint16_t*>(c->heightmap.dptr);
  a.ridgemap = static_cast<uint16_t*>(c->ridgemap.dptr);
  a.normalmap = static_cast<uint32_t*>(c->normalmap.dptr);
  a.splatmap = static_cast<uint32_t*>(c->splatmap.dptr);
  a.height_edit = static_cast<const float*>(c->height_edit.dptr);
  a.splat_edit = static_cast<const uint32_t*>(c->splat_edit.dptr);
  a.patch_minmax = static_cast<float2*>(mm.dptr);
  if (stages & G) launch_terrain_generate(a, s);
  if (stages & D) launch_terrain_derive(a, s);
  if (stages & M) launch_terrain_minmax(a, s);
  OXC_HIP(ctx, hipGetLastError());
  return OXC_OK;
}

oxc_status oxc_apply_terrain_brush(oxc_ctx* ctx, const oxc_terrain_brush_context* c, void* hip_stream) {
  if (!ctx) return OXC_INVALID_ARG;
  if (!c || c->struct_size != sizeof(oxc_terrain_brush_context)) return fail(ctx, OXC_INVALID_ARG, "apply_terrain_brush: bad context / struct_size");
  const char* const entry = "apply_terrain_brush";
  const oxc_terrain_brush_params& p = c->params;
  const uint32_t stages = c->stages;
  if (stages == 0u || (stages & ~(OXC_TERRAIN_BRUSH_TRACE | OXC_TERRAIN_BRUSH_APPLY))) return bad_arg(ctx, entry, "stages must be a non-empty mask of OXC_TERRAIN_BRUSH_TRACE | OXC_TERRAIN_BRUSH_APPLY");
  const uint32_t *res = p.resolution, *pc = p.patch_count;
  if (res[0] < 1u || res[0] > 16384u || res[1] < 1u || res[1] > 16384u) return bad_arg(ctx, entry, "params.resolution: every side must be in 1 .. 16384");
  if (pc[0] < 1u || pc[0] > 4096u || pc[1] < 1u || pc[1] > 4096u) return bad_arg(ctx, entry, "params.patch_count: every side must be in 1 .. 4096");
  if (p.mode > OXC_TERRAIN_BRUSH_PAINT_LAYER) return bad_arg(ctx, entry, "params.mode must be in 0 .. 4");
  if (!std::isfinite(p.radius_texels) || !(p.radius_texels >= 0.0f && p.radius_texels <= 4096.0f)) return bad_arg(ctx, entry, "params.radius_texels must be finite and in 0 .. 4096");
  if (!std::isfinite(p.falloff)) return bad_arg(ctx, entry, "params.falloff must be finite");

  // what the requested stages do, as the buffer table sees it: the trace, the apply of a height mode, the apply of PaintLayer
  const uint32_t T = 1u, H = 2u, P = 4u;
  const uint32_t uses = (stages & OXC_TERRAIN_BRUSH_TRACE ? T : 0u) | (stages & OXC_TERRAIN_BRUSH_APPLY ? (p.mode == OXC_TERRAIN_BRUSH_PAINT_LAYER ? P : H) : 0u);
  const uint64_t texels = (uint64_t)res[0] * res[1];
  const MapBuffer buffers[] = {
      {"heightmap", c->heightmap.dptr, c->heightmap.bytes, texels * 2u, 2u, T | H, 0u, false},
      {"height_edit", c->height_edit.dptr, c->height_edit.bytes, texels * 4u, 4u, H, H, false},
      {"splat_edit", c->splat_edit.dptr, c->splat_edit.bytes, texels * 4u, 4u, P, P, false},
      {"hit", c->hit.dptr, c->hit.bytes, 16u, 8u, T | H | P, T, false},
      {"region", c->region.dptr, c->region.bytes, 16u, 8u, T, T, false},
  };
  if (const oxc_status st = check_buffers(ctx, entry, buffers, uses)) return st;

  OXC_ENTER(ctx, hip_stream, s);
  TerrainBrushArgs a;
  std::memset(&a, 0, sizeof a);
  a.p = p;
  a.groups = (2u * (uint32_t)std::ceil(p.radius_texels) + 1u + 15u) / 16u;  // the reference's dispatch: at most 513
  a.heightmap = static_cast<const uint16_t*>(c->heightmap.dptr);
  a.height_edit = static_cast<float*>(c->height_edit.dptr);
  a.splat_edit = static_cast<uint32_t*>(c->splat_edit.dptr);
  a.hit = static_cast<uint32_t*>(c->hit.dptr);
  a.region = static_cast<uint32_t*>(c->region.dptr);
  if (stages & OXC_TERRAIN_BRUSH_TRACE) launch_terrain_brush_trace(a, s);
  if (stages & OXC_TERRAIN_BRUSH_APPLY) launch_terrain_brush_apply(a, s);
  OXC_HIP(ctx, hipGetLastError());
  return OXC_OK;
}

oxc_status oxc_decode_terrain(oxc_ctx* ctx, const oxc_terrain_decode_context* c, void* hip_stream) {
  if (!ctx) return OXC_INVALID_ARG;
  if (!c || c->struct_size != sizeof(oxc_terrain_decode_context)) return fail(ctx, OXC_INVALID_ARG, "decode_terrain: bad context / struct_size");
  const char* const entry = "decode_terrain";
  const oxc_image& dimg = c->depth_attachment;
  const oxc_terrain_data& T = c->terrain;
  if (c->width == 0u || c->height == 0u) return bad_arg(ctx, entry, "the extent must not be zero");
  if (dimg.width != c->width || dimg.height != c->height) return bad_arg(ctx, entry, "depth_attachment extent differs from (width, height)");
  uint64_t pixels;
  OXC_TRY(pixel_images(ctx, entry, dimg, nullptr, nullptr, pixels));
  const uint32_t* res = c->map_resolution;
  if (res[0] < 1u || res[0] > 16384u || res[1] < 1u || res[1] > 16384u) return bad_arg(ctx, entry, "map_resolution: every side must be in 1 .. 16384");

  const bool ring = T.brush_radius > 0.0f;  // false for a NaN: the record is not read then
  const uint64_t texels = (uint64_t)res[0] * res[1];
  const oxc_buffer &mat = c->materials_buffer, &mro = c->metallic_roughness_occlusion_attachment;
  const MapBuffer buffers[] = {
      {"visbuffer_attachment", c->visbuffer_attachment.dptr, c->visbuffer_attachment.bytes, pixels * 4u, 4u, 1u, 0u, false},
      {"depth_attachment", dimg.dptr, pixels * 4u, pixels * 4u, 4u, 1u, 0u, false},
      {"normalmap", c->normalmap.dptr, c->normalmap.bytes, texels * 4u, 4u, 1u, 0u, false},
      {"splatmap", c->splatmap.dptr, c->splatmap.bytes, texels * 4u, 4u, 1u, 0u, false},
      {"materials_buffer", mat.dptr, mat.bytes, (uint64_t)c->material_count * 56u, 4u, 1u, 0u, c->material_count == 0u, " is smaller than material_count records of 56 bytes"},
      {"brush_hit", c->brush_hit.dptr, c->brush_hit.bytes, 16u, 8u, 1u, 0u, !ring},
      {"albedo_attachment", c->albedo_attachment.dptr, c->albedo_attachment.bytes, pixels * 4u, 4u, 1u, 1u, false},
      {"normal_attachment", c->normal_attachment.dptr, c->normal_attachment.bytes, pixels * 8u, 8u, 1u, 1u, false},
      {"emissive_attachment", c->emissive_attachment.dptr, c->emissive_attachment.bytes, pixels * 4u, 4u, 1u, 1u, false},
      {"metallic_roughness_occlusion_attachment", mro.dptr, mro.bytes, pixels * 4u, 4u, 1u, 1u, false},
  };
  if (const oxc_status st = check_buffers(ctx, entry, buffers, 1u)) return st;

  OXC_ENTER(ctx, hip_stream, s);
  TerrainDecodeArgs a;
  std::memset(&a, 0, sizeof a);
  a.w = c->width, a.h = c->height;
  a.fw = (float)c->width, a.fh = (float)c->height;
  for (int k = 0; k < 16; k++) a.ipv[k] = c->inv_projection_view[k];
  a.t = T;
  a.map_w = res[0], a.map_h = res[1];
  a.material_count = mat.dptr ? c->material_count : 0u;
  a.vis = static_cast<const uint32_t*>(c->visbuffer_attachment.dptr);
  a.depth = static_cast<const float*>(dimg.dptr);
  a.normalmap = static_cast<const uint32_t*>(c->normalmap.dptr);
  a.splatmap = static_cast<const uint32_t*>(c->splatmap.dptr);
  a.materials = static_cast<const uint32_t*>(mat.dptr);
  a.hit = ring ? static_cast<const uint32_t*>(c->brush_hit.dptr) : nullptr;
  a.albedo = static_cast<uint32_t*>(c->albedo_attachment.dptr);
  a.normal = static_cast<uint2*>(c->normal_attachment.dptr);
  a.emissive = static_cast<uint32_t*>(c->emissive_attachment.dptr);
  a.mro = static_cast<uint32_t*>(mro.dptr);
  launch_terrain_decode(a, s);
  OXC_HIP(ctx, hipGetLastError());
  return OXC_OK;
}

oxc_status oxc_draw_terrain(oxc_ctx* ctx, const oxc_terrain_draw_context* c, void* hip_stream) {
  if (!ctx) return OXC_INVALID_ARG;
  if (!c || c->struct_size != sizeof(oxc_terrain_draw_context)) return fail(ctx, OXC_INVALID_ARG, "draw_terrain: bad context / struct_size");
  const char* const entry = "draw_terrain";
  const oxc_terrain_data& T = c->terrain;
  if (c->width < 1u || c->width > 16384u || c->height < 1u || c->height > 16384u) return bad_arg(ctx, entry, "the extent must be 1 .. 16384 a side");
  const uint32_t *res = c->map_resolution, *pc = T.patch_count;
  if (res[0] < 1u || res[0] > 16384u || res[1] < 1u || res[1] > 16384u) return bad_arg(ctx, entry, "map_resolution: every side must be in 1 .. 16384");
  if (pc[0] < 1u || pc[0] > 4096u || pc[1] < 1u || pc[1] > 4096u) return bad_arg(ctx, entry, "terrain.patch_count: every side must be in 1 .. 4096");
  const uint64_t pixels = (uint64_t)c->width * c->height, texels = (uint64_t)res[0] * res[1];
  const oxc_buffer &vp = c->visible_patches_buffer, &cmd = c->draw_cmd_buffer, &vd = c->visdepth_buffer;
  const MapBuffer buffers[] = {
      {"heightmap", c->heightmap.dptr, c->heightmap.bytes, texels * 2u, 2u, 1u, 0u, false},
      {"visible_patches_buffer", vp.dptr, vp.bytes, 4u, 4u, 1u, 0u, false},
      {"draw_cmd_buffer", cmd.dptr, cmd.bytes, 16u, 4u, 1u, 0u, false},
      {"visdepth_buffer", vd.dptr, vd.bytes, pixels * 8u, 8u, 1u, 1u, false},
  };
  if (const oxc_status st = check_buffers(ctx, entry, buffers, 1u)) return st;
  const oxc_image& dep = c->depth_attachment;
  if (dep.dptr && (dep.width != c->width || dep.height != c->height || dep.levels != 1u)) return bad_arg(ctx, entry, "depth_attachment must be one R32F level of the draw's extent");
  if (c->visbuffer_attachment.dptr && c->visbuffer_attachment.bytes < pixels * 4u) return bad_arg(ctx, entry, "visbuffer_attachment smaller than width * height u32");

  OXC_ENTER(ctx, hip_stream, s);
  OXC_TRY(ensure_raster_scratch(ctx, s, "draw_terrain: the first draw of a context allocates the raster scratch; make one un-captured call first"));
  TerrainDrawArgs a;
  std::memset(&a, 0, sizeof a);
  std::memcpy(a.r.pv, c->projection_view, 64);
  a.r.visdepth = static_cast<unsigned long long*>(vd.dptr);
  a.r.width = c->width, a.r.height = c->height;
  bind_raster_scratch(ctx, a.r);
  for (int k = 0; k < 3; k++) a.camera_position[k] = c->camera_position[k];
  a.near_clip = c->near_clip, a.projection_scale = c->projection_scale;
  a.t = T;
  a.map_w = res[0], a.map_h = res[1];
  a.heightmap = static_cast<const uint16_t*>(c->heightmap.dptr);
  a.visible = static_cast<const uint32_t*>(vp.dptr);
  a.visible_capacity = std::min<uint64_t>(vp.bytes / 4u, 1ull << 24);  // no list of distinct patches is longer: what lies beyond is skipped like an entry past the end
  a.draw_cmd = static_cast<const uint32_t*>(cmd.dptr);
  a.stats = a.r.clip_count + kTerrainStatsWord;
  const uint32_t full_grid = ctx->num_cus * 8;
  const uint32_t max_grid = ctx->terrain_draw_grid ? std::min(ctx->terrain_draw_grid, full_grid) : full_grid;  // OXC_TUNE_TERRAIN_DRAW_GRID
  launch_draw_terrain(a, c->clear != 0, ctx->terrain_draw_stats, dep.dptr ? reinterpret_cast<float*>(static_cast<char*>(dep.dptr) + dep.level_offset[0]) : nullptr,
                      static_cast<uint32_t*>(c->visbuffer_attachment.dptr), max_grid, s);
  OXC_HIP(ctx, hipGetLastError());
  return OXC_OK;
}

oxc_status oxc_debug_terrain_draw_stats(oxc_ctx* ctx, uint32_t* host_out8, void* hip_stream) {
  if (!ctx) return OXC_INVALID_ARG;
  if (!host_out8) return fail(ctx, OXC_INVALID_ARG, "debug_terrain_draw_stats: null pointer");
  if (!ctx->raster_scratch) return fail(ctx, OXC_INVALID_ARG, "debug_terrain_draw_stats: no oxc_draw_terrain call on this context yet");
  OXC_ENTER(ctx, hip_stream, s);
  OXC_HIP(ctx, hipMemcpyAsync(host_out8, static_cast<const uint32_t*>(ctx->raster_scratch) + kTerrainStatsWord, 32, hipMemcpyDeviceToHost, s));
  OXC_HIP(ctx, hipStreamSynchronize(s));
  return OXC_OK;
}

}  // extern "C"
