// oxcull_abi_raster.cpp -- the visbuffer draw of liboxcull.so's C ABI (oxc_draw_visbuffer) and its stats reader.
#include "oxcull_host.hpp"

// Big triangles (and clipped triangle ids) queued per draw; beyond that the producing lane rasterises the triangle itself and an
// overflow pass re-walks the index list for the crossing triangles the id queue could not hold (both slow, both correct).  240 MB of scratch, allocated by the first draw.
// oxc_debug_set_tuning(OXC_TUNE_RASTER_BIG_CAPACITY) before that first draw shrinks it so that the tests can reach the overflow paths with a small scene.
constexpr uint32_t kRasterBigCapacity = 1u << 22;

// The scratch of the draws into the depth|vis image (oxc_draw_visbuffer, oxc_draw_terrain): allocated by whichever runs first on the context
oxc_status ensure_raster_scratch(oxc_ctx* ctx, hipStream_t s, const char* capture_msg) {
  if (ctx->raster_scratch) return OXC_OK;
  if (stream_is_capturing(s)) return fail(ctx, OXC_INVALID_ARG, capture_msg);
  uint32_t cap = kRasterBigCapacity;
  if (ctx->raster_capacity_request) cap = std::min<uint32_t>(std::max<uint32_t>(ctx->raster_capacity_request, kBigSegs * 16), 1u << 24) / kBigSegs * kBigSegs;
  hipError_t e = hipMalloc(&ctx->raster_scratch, (size_t)cap * kTriSetupBytes + kRasterHeaderBytes + (size_t)cap * 4 + (size_t)cap * 2 * 8);
  if (e != hipSuccess) return fail(ctx, OXC_OUT_OF_MEMORY, "hipMalloc(raster scratch)", e);
  ctx->raster_capacity = cap;
  return OXC_OK;
}

// ... and its parts as the kernels see them: header (clip / tile counters, segment counters), big list, clip queue, tile list
void bind_raster_scratch(const oxc_ctx* ctx, DrawArgs& a) {
  char* const rs = static_cast<char*>(ctx->raster_scratch);
  a.clip_count = reinterpret_cast<uint32_t*>(rs);
  a.tile_count = reinterpret_cast<uint32_t*>(rs) + 32;
  a.big_seg_counts = reinterpret_cast<uint32_t*>(rs + 256);
  const uint32_t cap = ctx->raster_capacity;
  a.big_seg_capacity = cap / kBigSegs;
  a.big_list = reinterpret_cast<TriSetup*>(rs + kRasterHeaderBytes);
  a.clip_capacity = cap;  // more clipped triangles than that in one draw: k_draw_clipped<RESCAN> finds them again
  a.clip_list = reinterpret_cast<uint32_t*>(rs + kRasterHeaderBytes + (size_t)cap * kTriSetupBytes);
  a.tile_capacity = cap * 2;
  a.tile_list = reinterpret_cast<uint2*>(rs + kRasterHeaderBytes + (size_t)cap * (kTriSetupBytes + 4));
}

extern "C" {

oxc_status oxc_draw_visbuffer(oxc_ctx* ctx, const oxc_prepared_frame* f, const oxc_draw_context* d, void* hip_stream) {
  if (!ctx) return OXC_INVALID_ARG;
  if (!f || !d || d->struct_size != sizeof(oxc_draw_context)) return fail(ctx, OXC_INVALID_ARG, "draw_visbuffer: bad frame / context / struct_size");
  if (d->width == 0 || d->height == 0 || d->width > 16384 || d->height > 16384) return fail(ctx, OXC_INVALID_ARG, "draw_visbuffer: extent must be 1..16384");
  if (d->wide_triangle_index > 2u) return fail(ctx, OXC_INVALID_ARG, "draw_visbuffer: wide_triangle_index must be 0, 1 or 2");
  const uint64_t n = (uint64_t)d->width * d->height;
  if (!d->visdepth_buffer.dptr || d->visdepth_buffer.bytes < n * 8u) return fail(ctx, OXC_INVALID_ARG, "draw_visbuffer: visdepth_buffer smaller than width*height u64");
  if (!d->draw_geometry_cmd_buffer.dptr) return fail(ctx, OXC_INVALID_ARG, "draw_visbuffer: draw_geometry_cmd_buffer is null (run oxc_cull_geometry with the triangle stage first)");
  if (!f->meshes_buffer.dptr || !f->transforms_world_buffer.dptr || !f->mesh_instances_buffer.dptr || !f->meshlet_instances_buffer.dptr ||
      !f->reordered_indices_buffer.dptr)
    return fail(ctx, OXC_INVALID_ARG, "draw_visbuffer: null PreparedFrame buffer");
  const oxc_image& dep = d->depth_attachment;
  if (dep.dptr && (dep.width != d->width || dep.height != d->height)) return fail(ctx, OXC_INVALID_ARG, "draw_visbuffer: depth_attachment extent differs from the draw extent");
  if (d->visbuffer_attachment.dptr && d->visbuffer_attachment.bytes < n * 4u) return fail(ctx, OXC_INVALID_ARG, "draw_visbuffer: visbuffer_attachment smaller than width*height u32");
  OXC_ENTER(ctx, hip_stream, s);
  OXC_JOIN(ctx, s);  // reads reordered_indices / the draw command
  OXC_TRY(ensure_raster_scratch(ctx, s, "draw_visbuffer: the first call allocates its scratch; make one un-captured call first"));
  OXC_TRY(grow_scratch(ctx, s, ctx->raster_rows, ctx->raster_rows_cap, f->mesh_instance_count, (size_t)f->mesh_instance_count * sizeof(DrawRow),
                       "draw_visbuffer: more mesh instances than any earlier call (scratch would grow); make one un-captured call first", "hipMalloc(raster rows)"));
  DrawArgs a;
  std::memset(&a, 0, sizeof a);
  std::memcpy(a.pv, d->projection_view, 64);
  a.rows = static_cast<DrawRow*>(ctx->raster_rows);
  a.mesh_instance_count = f->mesh_instance_count;
  a.meshes = static_cast<const GpuMesh*>(f->meshes_buffer.dptr);
  a.transforms = static_cast<const float*>(f->transforms_world_buffer.dptr);
  a.mesh_instances = static_cast<const GpuMeshInstance*>(f->mesh_instances_buffer.dptr);
  a.meshlet_instances = static_cast<const GpuMeshletInstance*>(f->meshlet_instances_buffer.dptr);
  a.indices = static_cast<const uint32_t*>(f->reordered_indices_buffer.dptr);
  a.draw_cmd = static_cast<const uint32_t*>(d->draw_geometry_cmd_buffer.dptr);
  a.visdepth = static_cast<unsigned long long*>(d->visdepth_buffer.dptr);
  a.width = d->width;
  a.height = d->height;
  a.wide = d->wide_triangle_index;
  bind_raster_scratch(ctx, a);
  const uint32_t full_grid = ctx->num_cus * 8;
  const uint32_t max_grid = ctx->raster_grid ? std::min(ctx->raster_grid, full_grid) : full_grid;  // OXC_TUNE_RASTER_GRID
  {
    KernelTimer t(ctx, OXC_K_DRAW_VISBUFFER, s);
    launch_draw_visbuffer(a, d->clear != 0, dep.dptr ? reinterpret_cast<float*>(static_cast<char*>(dep.dptr) + dep.level_offset[0]) : nullptr,
                          static_cast<uint32_t*>(d->visbuffer_attachment.dptr), max_grid, s);
  }
  OXC_HIP(ctx, hipGetLastError());
  return OXC_OK;
}

oxc_status oxc_debug_raster_stats(oxc_ctx* ctx, uint32_t* host_out4, void* hip_stream) {
  if (!ctx) return OXC_INVALID_ARG;
  if (!host_out4) return fail(ctx, OXC_INVALID_ARG, "debug_raster_stats: null pointer");
  if (!ctx->raster_scratch) return fail(ctx, OXC_INVALID_ARG, "debug_raster_stats: no oxc_draw_visbuffer call on this context yet");
  OXC_ENTER(ctx, hip_stream, s);
  std::vector<uint32_t> h(kRasterHeaderBytes / 4);
  OXC_HIP(ctx, hipMemcpyAsync(h.data(), ctx->raster_scratch, kRasterHeaderBytes, hipMemcpyDeviceToHost, s));
  OXC_HIP(ctx, hipStreamSynchronize(s));
  const uint32_t seg_cap = ctx->raster_capacity / kBigSegs;
  uint64_t big = 0;
  uint32_t overflowed = 0;
  for (uint32_t k = 0; k < kBigSegs; k++) {
    const uint32_t c = h[64 + k * kBigSegStride];
    big += c;
    overflowed += c > seg_cap ? 1u : 0u;
  }
  host_out4[0] = (uint32_t)std::min<uint64_t>(big, 0xFFFFFFFFull);
  host_out4[1] = h[0];
  host_out4[2] = h[32];
  host_out4[3] = overflowed;
  return OXC_OK;
}

}  // extern "C"
