// oxcull_abi_vsm.cpp -- the virtual shadow map entry points of liboxcull.so's C ABI: HPB build, page update, shadow draw, shadow
// resolve, and their stats readers.
#include "oxcull_host.hpp"

// Entries of the shadow draw's big-pair and clip queues (the tile queue holds twice as many): enough for every (triangle, clipmap) pair the
// frame's index buffer can hold, at most 2^24 (1.07 GB of scratch) and at least 4096.  Beyond them overflow passes find the pairs again
// and draw each with a whole wave (k_vsm_draw_clipped<RESCAN>, k_vsm_draw_big_rescan), and a big-pair wave walks the tiles that did not
// fit: slower, same image.  oxc_debug_vsm_draw_stats reports how many went past each queue.
constexpr uint64_t kVsmDrawCapacityMax = 1u << 24, kVsmDrawCapacityMin = 4096;

extern "C" {

oxc_status oxc_generate_hpb(oxc_ctx* ctx, oxc_buffer page_table, const oxc_image_array_u8* h, void* hip_stream) {
  if (!ctx) return OXC_INVALID_ARG;
  if (!h || !h->dptr) return fail(ctx, OXC_INVALID_ARG, "generate_hpb: null hpb_attachment");
  if (h->levels == 0 || h->levels > 13 || h->width == 0 || h->height == 0) return fail(ctx, OXC_INVALID_ARG, "generate_hpb: bad extent / level count");
  const uint64_t pages = (uint64_t)h->width * h->height * h->layers;
  if (pages && (!page_table.dptr || page_table.bytes < pages * 4u)) return fail(ctx, OXC_INVALID_ARG, "generate_hpb: virtual_page_table smaller than width*height*layers u32");
  for (uint32_t k = 0; k < h->levels; k++)
    if (h->level_offset[k] > 0xFFFFFFFFull) return fail(ctx, OXC_INVALID_ARG, "generate_hpb: level offsets must fit 32 bits");
  OXC_ENTER(ctx, hip_stream, s);
  launch_generate_hpb(static_cast<const uint32_t*>(page_table.dptr), static_cast<uint8_t*>(h->dptr), h->width, h->height, h->layers, h->levels, h->level_offset, s);
  OXC_HIP(ctx, hipGetLastError());
  return OXC_OK;
}

oxc_status oxc_update_virtual_shadowmap(oxc_ctx* ctx, const oxc_vsm_update_context* c, void* hip_stream) {
  if (!ctx) return OXC_INVALID_ARG;
  if (!c || c->struct_size != sizeof(oxc_vsm_update_context)) return fail(ctx, OXC_INVALID_ARG, "update_virtual_shadowmap: bad context / struct_size");
  const char* const entry = "update_virtual_shadowmap";
  VsmShape sh;
  OXC_TRY(vsm_shape(ctx, entry, *c, sh));
  const int32_t n = sh.n, ps = sh.ps, phys = sh.phys, layers = sh.layers;
  const uint32_t P = sh.P, phys_count = sh.phys_count;
  const uint64_t entries = sh.entries;
  const oxc_image& dimg = c->depth_attachment;
  if (c->depth_extent[0] < 0 || c->depth_extent[1] < 0 || (uint32_t)c->depth_extent[0] != dimg.width || (uint32_t)c->depth_extent[1] != dimg.height)
    return fail(ctx, OXC_INVALID_ARG, "update_virtual_shadowmap: depth_extent must equal the depth attachment's extent");
  if (dimg.width && dimg.height && (!dimg.dptr || dimg.levels != 1 || dimg.level_offset[0] != 0))
    return fail(ctx, OXC_INVALID_ARG, "update_virtual_shadowmap: depth_attachment must be one R32F level at offset 0");
  OXC_TRY(vsm_tables(ctx, entry, *c, sh));
  OXC_TRY(vsm_dirty_flags(ctx, entry, c->vsm_clipmap_dirty_flags_buffer, sh));
  if (!c->dirty_physical_pages_buffer.dptr || c->dirty_physical_pages_buffer.bytes < std::min<uint64_t>(entries, phys_count) * 8u)
    return fail(ctx, OXC_INVALID_ARG, "update_virtual_shadowmap: dirty_physical_pages_buffer smaller than min(pages, physical pages) u32x2");
  if (!c->clear_cmd_buffer.dptr || c->clear_cmd_buffer.bytes < 12u) return fail(ctx, OXC_INVALID_ARG, "update_virtual_shadowmap: clear_cmd_buffer smaller than a VkDispatchIndirectCommand");
  if (!c->counters_buffer.dptr || c->counters_buffer.bytes < 32u) return fail(ctx, OXC_INVALID_ARG, "update_virtual_shadowmap: counters_buffer smaller than u32[8]");
  const bool invalidate = !c->sun_moved && c->dirty_mesh_instance_count > 0;
  if (invalidate) {
    if (!c->dirty_mesh_instance_indices.dptr || c->dirty_mesh_instance_indices.bytes < (uint64_t)c->dirty_mesh_instance_count * 4u)
      return fail(ctx, OXC_INVALID_ARG, "update_virtual_shadowmap: dirty_mesh_instance_indices smaller than dirty_mesh_instance_count u32");
    if (!c->mesh_instances_buffer.dptr || !c->meshes_buffer.dptr || !c->transforms_world_buffer.dptr || !c->transforms_previous_buffer.dptr)
      return fail(ctx, OXC_INVALID_ARG, "update_virtual_shadowmap: invalidation needs mesh_instances, meshes, transforms_world and transforms_previous");
  }
  const oxc_image_array_u8& h = c->hpb_attachment;
  if (h.dptr) {
    if (h.width != (uint32_t)n || h.height != (uint32_t)n || h.layers != (uint32_t)layers || h.levels == 0 || h.levels > 13)
      return fail(ctx, OXC_INVALID_ARG, "update_virtual_shadowmap: hpb_attachment must be n x n x clipmap_count with 1..13 levels");
    for (uint32_t k = 0; k < h.levels; k++)
      if (h.level_offset[k] > 0xFFFFFFFFull) return fail(ctx, OXC_INVALID_ARG, "update_virtual_shadowmap: hpb level offsets must fit 32 bits");
  }
  const oxc_image& pimg = c->physical_page_image;
  if (pimg.dptr && (pimg.width != (uint32_t)phys || pimg.height != (uint32_t)phys || pimg.levels != 1 || pimg.level_offset[0] != 0 ||
                    (reinterpret_cast<uintptr_t>(pimg.dptr) & 15u)))
    return fail(ctx, OXC_INVALID_ARG, "update_virtual_shadowmap: physical_page_image must be one 16-byte aligned R32F level of physical_page_table_size^2");
  OXC_ENTER(ctx, hip_stream, s);
  const uint64_t want = align_up((uint64_t)phys_count * 4u, 256) + align_up(entries, 256);
  OXC_TRY(grow_scratch(ctx, s, ctx->vsm_scratch, ctx->vsm_scratch_bytes, want, want,
                       "update_virtual_shadowmap: scratch must grow but the stream is being captured; make one un-captured call of this size first",
                       "hipMalloc(vsm scratch)"));
  VsmArgs a = {};
  a.page_table = static_cast<uint32_t*>(c->virtual_page_table.dptr);
  a.clipmaps = static_cast<const float*>(c->vsm_clipmaps_buffer.dptr);
  a.depth = static_cast<const float*>(dimg.dptr);
  a.depth_w = dimg.width;
  a.depth_h = dimg.height;
  a.depth_vec4 = (dimg.width % 4u == 0u && (reinterpret_cast<uintptr_t>(dimg.dptr) & 15u) == 0u) ? 1u : 0u;
  a.n = (uint32_t)n;
  a.layers = (uint32_t)layers;
  a.page_size = (uint32_t)ps;
  a.phys_side = P;
  a.phys_count = phys_count;
  a.sun_moved = c->sun_moved ? 1u : 0u;
  a.invalidate = invalidate ? 1u : 0u;
  a.dirty_ids = static_cast<const uint32_t*>(c->dirty_mesh_instance_indices.dptr);
  a.dirty_count = invalidate ? c->dirty_mesh_instance_count : 0u;
  a.mesh_instance_count = (uint32_t)std::min<uint64_t>(c->mesh_instances_buffer.bytes / sizeof(GpuMeshInstance), 0xFFFFFFFFu);
  a.mesh_count = (uint32_t)std::min<uint64_t>(c->meshes_buffer.bytes / sizeof(GpuMesh), 0xFFFFFFFFu);
  a.transform_count = (uint32_t)std::min<uint64_t>(c->transforms_world_buffer.bytes / 64u, 0xFFFFFFFFu);
  a.transform_previous_count = (uint32_t)std::min<uint64_t>(c->transforms_previous_buffer.bytes / 64u, 0xFFFFFFFFu);
  a.mesh_instances = static_cast<const GpuMeshInstance*>(c->mesh_instances_buffer.dptr);
  a.meshes = static_cast<const GpuMesh*>(c->meshes_buffer.dptr);
  a.transforms = static_cast<const float*>(c->transforms_world_buffer.dptr);
  a.transforms_previous = static_cast<const float*>(c->transforms_previous_buffer.dptr);
  a.dirty_flags = static_cast<uint32_t*>(c->vsm_clipmap_dirty_flags_buffer.dptr);
  a.dirty_coords = static_cast<uint32_t*>(c->dirty_physical_pages_buffer.dptr);
  a.clear_cmd = static_cast<uint32_t*>(c->clear_cmd_buffer.dptr);
  a.counters = static_cast<uint32_t*>(c->counters_buffer.dptr);
  a.physical = static_cast<float*>(pimg.dptr);
  a.physical_size = (uint32_t)phys;
  a.free_list = static_cast<uint32_t*>(ctx->vsm_scratch);
  a.mark = static_cast<uint8_t*>(ctx->vsm_scratch) + align_up((uint64_t)phys_count * 4u, 256);
  for (int k = 0; k < 16; k++) a.inv_pv[k] = c->inv_projection_view[k];
  clipmap_selection_constants(a, *c, sh);
  {
    KernelTimer t(ctx, OXC_K_VSM_UPDATE, s);
    launch_vsm_update(a, ctx->num_cus, static_cast<uint8_t*>(h.dptr), h.levels, h.level_offset, s);
  }
  OXC_HIP(ctx, hipGetLastError());
  return OXC_OK;
}

oxc_status oxc_draw_physical_pages(oxc_ctx* ctx, const oxc_prepared_frame* f, const oxc_vsm_draw_context* c, void* hip_stream) {
  if (!ctx) return OXC_INVALID_ARG;
  if (!f || !c || c->struct_size != sizeof(oxc_vsm_draw_context)) return fail(ctx, OXC_INVALID_ARG, "draw_physical_pages: bad frame / context / struct_size");
  const char* const entry = "draw_physical_pages";
  VsmShape sh;
  OXC_TRY(vsm_shape(ctx, entry, *c, sh));
  const int32_t n = sh.n, ps = sh.ps, phys = sh.phys, layers = sh.layers;
  const uint32_t P = sh.P;
  const uint64_t entries = sh.entries;
  if ((int64_t)n * ps > 16384) return fail(ctx, OXC_INVALID_ARG, "draw_physical_pages: V = page_table_size * page_size must be <= 16384 (the guard band's fixed-point range)");
  if (c->wide_triangle_index > 2u) return fail(ctx, OXC_INVALID_ARG, "draw_physical_pages: wide_triangle_index must be 0, 1 or 2");
  OXC_TRY(vsm_tables(ctx, entry, *c, sh));
  OXC_TRY(vsm_dirty_flags(ctx, entry, c->vsm_clipmap_dirty_flags_buffer, sh));
  if (!c->draw_geometry_cmd_buffer.dptr || c->draw_geometry_cmd_buffer.bytes < 20u)
    return fail(ctx, OXC_INVALID_ARG, "draw_physical_pages: draw_geometry_cmd_buffer must hold a VkDrawIndexedIndirectCommand (run oxc_cull_geometry with the triangle stage first)");
  const oxc_image& img = c->physical_page_image;
  if (!img.dptr || img.width != (uint32_t)phys || img.height != (uint32_t)phys || img.levels != 1 || img.level_offset[0] != 0 ||
      (reinterpret_cast<uintptr_t>(img.dptr) & 15u))
    return fail(ctx, OXC_INVALID_ARG, "draw_physical_pages: physical_page_image must be one 16-byte aligned R32F level of physical_page_table_size^2");
  const bool cmds = c->draw_commands_buffer.dptr != nullptr;
  if (cmds != (c->draw_count_buffer.dptr != nullptr) || cmds != (c->draw_clipmaps_buffer.dptr != nullptr))
    return fail(ctx, OXC_INVALID_ARG, "draw_physical_pages: draw_commands / draw_count / draw_clipmaps buffers must be given together");
  if (cmds && (c->draw_commands_buffer.bytes < (uint64_t)layers * 20u || c->draw_count_buffer.bytes < 4u || c->draw_clipmaps_buffer.bytes < (uint64_t)layers * 4u))
    return fail(ctx, OXC_INVALID_ARG, "draw_physical_pages: draw_commands (clipmap_count x 20 bytes), draw_count (4) or draw_clipmaps (clipmap_count u32) too small");
  if (!f->meshes_buffer.dptr || !f->transforms_world_buffer.dptr || !f->mesh_instances_buffer.dptr || !f->meshlet_instances_buffer.dptr ||
      !f->reordered_indices_buffer.dptr)
    return fail(ctx, OXC_INVALID_ARG, "draw_physical_pages: null PreparedFrame buffer");
  OXC_ENTER(ctx, hip_stream, s);
  OXC_JOIN(ctx, s);  // reads reordered_indices / the draw command
  const uint64_t max_tris = f->reordered_indices_buffer.bytes / (c->wide_triangle_index == 2u ? 24u : 12u);
  // a capacity set with OXC_TUNE_VSM_DRAW_CAPACITY holds; otherwise the queues grow with the frame (not inside a capture: there the
  // current ones are used, and the overflow passes keep the image right)
  uint32_t cap = ctx->vsm_draw_capacity_request
                     ? std::min<uint32_t>(std::max<uint32_t>(ctx->vsm_draw_capacity_request, 64u), 1u << 24)
                     : (uint32_t)std::min(std::max(max_tris * (uint64_t)layers, kVsmDrawCapacityMin), kVsmDrawCapacityMax);
  if (ctx->vsm_draw_scratch && (ctx->vsm_draw_capacity_request || stream_is_capturing(s))) cap = ctx->vsm_draw_capacity;
  cap = std::max(cap, ctx->vsm_draw_capacity);
  const uint32_t wpl = (uint32_t)((uint64_t)n * n / 32u);
  Carve carve{kVsmDrawHeaderBytes};
  const uint64_t o_bitmap = carve((uint64_t)layers * wpl * 4u);
  const uint64_t o_map = carve(entries * 4u);
  const uint64_t o_rows = carve((uint64_t)f->mesh_instance_count * sizeof(DrawRow));
  const uint64_t o_big = carve((uint64_t)cap * sizeof(VsmBig));
  const uint64_t o_clip = carve((uint64_t)cap * 8u);
  const uint64_t o_tile = carve((uint64_t)cap * 2u * 8u);
  OXC_TRY(grow_scratch(ctx, s, ctx->vsm_draw_scratch, ctx->vsm_draw_scratch_bytes, carve.off, carve.off,
                       "draw_physical_pages: scratch must grow but the stream is being captured; make one un-captured call of this shape first",
                       "hipMalloc(vsm draw scratch)"));
  ctx->vsm_draw_capacity = cap;  // (never below the previous calls': the scratch holds the largest queues asked for so far)
  char* const sc = static_cast<char*>(ctx->vsm_draw_scratch);
  VsmDrawArgs a;
  std::memset(&a, 0, sizeof a);
  a.rows = reinterpret_cast<DrawRow*>(sc + o_rows);
  a.mesh_instance_count = f->mesh_instance_count;
  a.meshes = static_cast<const GpuMesh*>(f->meshes_buffer.dptr);
  a.transforms = static_cast<const float*>(f->transforms_world_buffer.dptr);
  a.mesh_instances = static_cast<const GpuMeshInstance*>(f->mesh_instances_buffer.dptr);
  a.meshlet_instances = static_cast<const GpuMeshletInstance*>(f->meshlet_instances_buffer.dptr);
  a.indices = static_cast<const uint32_t*>(f->reordered_indices_buffer.dptr);
  a.draw_cmd = static_cast<const uint32_t*>(c->draw_geometry_cmd_buffer.dptr);
  a.wide = c->wide_triangle_index;
  a.max_triangles = (uint32_t)std::min<uint64_t>(max_tris, 0xFFFFFFFFull);
  a.page_table = static_cast<const uint32_t*>(c->virtual_page_table.dptr);
  a.clipmaps = static_cast<const float*>(c->vsm_clipmaps_buffer.dptr);
  a.dirty_flags = static_cast<const uint32_t*>(c->vsm_clipmap_dirty_flags_buffer.dptr);
  a.n = (uint32_t)n;
  a.layers = (uint32_t)layers;
  a.page_size = (uint32_t)ps;
  a.phys_side = P;
  a.V = (uint32_t)(n * ps);
  a.ps_shift = (ps & (ps - 1)) == 0 ? __builtin_ctz((uint32_t)ps) : -1;
  a.words_per_layer = wpl;
  a.physical = static_cast<float*>(img.dptr);
  a.physical_size = (uint32_t)phys;
  a.out_cmds = static_cast<uint32_t*>(c->draw_commands_buffer.dptr);
  a.out_count = static_cast<uint32_t*>(c->draw_count_buffer.dptr);
  a.out_clipmaps = static_cast<uint32_t*>(c->draw_clipmaps_buffer.dptr);
  a.header = reinterpret_cast<uint32_t*>(sc);
  a.bitmap = reinterpret_cast<uint32_t*>(sc + o_bitmap);
  a.pagemap = reinterpret_cast<uint32_t*>(sc + o_map);
  a.big_list = reinterpret_cast<VsmBig*>(sc + o_big);
  a.big_capacity = cap;
  a.clip_list = reinterpret_cast<uint2*>(sc + o_clip);
  a.clip_capacity = cap;
  a.tile_list = reinterpret_cast<uint2*>(sc + o_tile);
  a.tile_capacity = cap * 2u;
  const uint32_t full_grid = ctx->num_cus * 8;
  launch_vsm_draw(a, ctx->vsm_draw_stats, ctx->vsm_draw_grid ? std::min(ctx->vsm_draw_grid, full_grid) : full_grid, s);  // OXC_TUNE_VSM_DRAW_GRID
  OXC_HIP(ctx, hipGetLastError());
  return OXC_OK;
}

oxc_status oxc_resolve_shadowmap(oxc_ctx* ctx, const oxc_shadow_resolve_context* c, void* hip_stream) {
  if (!ctx) return OXC_INVALID_ARG;
  if (!c || c->struct_size != sizeof(oxc_shadow_resolve_context)) return fail(ctx, OXC_INVALID_ARG, "resolve_shadowmap: bad context / struct_size");
  const char* const entry = "resolve_shadowmap";
  VsmShape sh;
  OXC_TRY(vsm_shape(ctx, entry, *c, sh));
  const int32_t n = sh.n, ps = sh.ps, phys = sh.phys;
  const oxc_image& dimg = c->depth_attachment;
  const oxc_image& oimg = c->resolved_shadows_attachment;
  uint64_t pixels;
  OXC_TRY(pixel_images(ctx, entry, dimg, &oimg, "resolved_shadows_attachment", pixels));
  if (bad_pixel_buffer(c->normal_attachment, pixels, 8u))
    return bad_arg(ctx, entry, "normal_attachment must be 8-byte aligned u16x4 texels of the depth attachment's extent");
  OXC_TRY(vsm_tables(ctx, entry, *c, sh));
  const oxc_image& pimg = c->physical_page_image;
  if (!pimg.dptr || pimg.width != (uint32_t)phys || pimg.height != (uint32_t)phys || pimg.levels != 1 || pimg.level_offset[0] != 0)
    return fail(ctx, OXC_INVALID_ARG, "resolve_shadowmap: physical_page_image must be one R32F level of physical_page_table_size^2");
  OXC_ENTER(ctx, hip_stream, s);
  if (!pixels) return OXC_OK;
  VsmResolveArgs a;
  std::memset(&a, 0, sizeof a);
  OXC_TRY(arm_counters(ctx, entry, "hipMalloc(vsm resolve counters)", ctx->vsm_resolve_stats, 32, s, &a.stats));
  a.depth = static_cast<const float*>(dimg.dptr);
  a.normal = static_cast<const uint32_t*>(c->normal_attachment.dptr);
  a.out = static_cast<float*>(oimg.dptr);
  a.w = dimg.width;
  a.h = dimg.height;
  a.clipmaps = static_cast<const float*>(c->vsm_clipmaps_buffer.dptr);
  a.page_table = static_cast<const uint32_t*>(c->virtual_page_table.dptr);
  a.physical = static_cast<const float*>(pimg.dptr);
  a.n = (uint32_t)n;
  a.layers = (uint32_t)sh.layers;
  a.page_size = (uint32_t)ps;
  a.phys_side = sh.P;
  a.phys_count = sh.phys_count;
  a.physical_size = (uint32_t)phys;
  a.fn = (float)n;
  a.fV = (float)((int64_t)n * ps);
  // per-call constants, binary32 in the Slang's order (include/oxcull.h)
  for (int k = 0; k < 16; k++) a.inv_pv[k] = c->inv_projection_view[k];
  clipmap_selection_constants(a, *c, sh);
  {  // perpendicular_basis(L): t = normalize(cross(axis, L)), bitangent = cross(L, t)
    const float* L = c->directional_light_dir;
    const float ax = std::fabs(L[1]) < 0.999f ? 0.0f : 1.0f, ay = std::fabs(L[1]) < 0.999f ? 1.0f : 0.0f, az = 0.0f;
    const float cx = ay * L[2] - az * L[1], cy = az * L[0] - ax * L[2], cz = ax * L[1] - ay * L[0];
    const float len = std::sqrt((cx * cx + cy * cy) + cz * cz);
    const float t[3] = {cx / len, cy / len, cz / len};
    for (int k = 0; k < 3; k++) a.light[k] = L[k], a.tangent[k] = t[k];
    a.bitangent[0] = L[1] * t[2] - L[2] * t[1];
    a.bitangent[1] = L[2] * t[0] - L[0] * t[2];
    a.bitangent[2] = L[0] * t[1] - L[1] * t[0];
  }
  a.z_length = c->z_length;
  a.inv_z_length = 1.0f / c->z_length;
  for (uint32_t i = 0; i < 40; i++) {  // hammersley2d(i, N) = (f32(i) / f32(N), f32(reversebits(i)) * 2^-32)
    const uint32_t k = i < 16 ? i : i - 16;
    uint32_t rev = 0;
    for (int bit = 0; bit < 32; bit++) rev |= ((k >> bit) & 1u) << (31 - bit);
    a.ham[i][0] = (float)k / (i < 16 ? 16.0f : 24.0f);
    a.ham[i][1] = (float)rev * 0x1p-32f;
  }
  launch_vsm_resolve(a, s);
  OXC_HIP(ctx, hipGetLastError());
  return OXC_OK;
}

oxc_status oxc_debug_vsm_draw_stats(oxc_ctx* ctx, uint32_t* host_out8, void* hip_stream) {
  if (!ctx) return OXC_INVALID_ARG;
  if (!host_out8) return fail(ctx, OXC_INVALID_ARG, "debug_vsm_draw_stats: null pointer");
  if (!ctx->vsm_draw_scratch) return fail(ctx, OXC_INVALID_ARG, "debug_vsm_draw_stats: no oxc_draw_physical_pages call on this context yet");
  OXC_ENTER(ctx, hip_stream, s);
  std::vector<uint32_t> h(kVsmDrawHeaderBytes / 4);
  OXC_HIP(ctx, hipMemcpyAsync(h.data(), ctx->vsm_draw_scratch, kVsmDrawHeaderBytes, hipMemcpyDeviceToHost, s));
  OXC_HIP(ctx, hipStreamSynchronize(s));
  const uint32_t cap = ctx->vsm_draw_capacity;
  auto beyond = [](uint32_t count, uint32_t capacity) { return count > capacity ? count - capacity : 0u; };
  host_out8[0] = h[128];  // pairs kept by the page bitmap (counting kernels only)
  host_out8[1] = h[160];  // fragments written (counting kernels only)
  host_out8[2] = h[32];   // big pairs (pixel box beyond the in-wave path)
  host_out8[3] = beyond(h[32], cap);  // ... of which the big list could not hold
  host_out8[4] = h[64];   // (big pair, drawable page) tiles
  host_out8[5] = beyond(h[64], cap * 2u);
  host_out8[6] = h[96];   // pairs that crossed a clip plane
  host_out8[7] = beyond(h[96], cap);
  return OXC_OK;
}

oxc_status oxc_debug_vsm_resolve_stats(oxc_ctx* ctx, uint32_t* host_out8, void* hip_stream) {
  return read_counters(ctx, "debug_vsm_resolve_stats", "oxc_resolve_shadowmap", &oxc_ctx::vsm_resolve_stats, host_out8, 32, hip_stream);
}

}  // extern "C"
