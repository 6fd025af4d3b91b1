// oxcull_abi.cpp -- host side of liboxcull.so: the C ABI declared in include/oxcull.h.
//
// Mirrors what RendererInstance::generate_hiz / ::cull_geometry do on the host in the reference
// (Oxylus/src/Render/Passes/CullGeometry.cpp): pick the pipeline variant from the context flags,
// hand out freshly initialised counter buffers, and enqueue the passes in order.  Where the
// reference records vuk passes that run at end_frame, this enqueues HIP kernels on the caller's
// stream; nothing here synchronises except scratch growth and oxc_read_counters.
//
// One translation unit per subsystem, all on oxcull_host.hpp (the context, stream ordering, the shared argument rules):
//   oxcull_abi.cpp        the context's life, profiling, tuning and the debug entries that belong to no single subsystem (this file)
//   oxcull_abi_cull.cpp   HiZ build, the cull calls and their bookkeeping, terrain
//   oxcull_abi_raster.cpp the visbuffer draw
//   oxcull_abi_mesh.cpp   meshlet bounds, vertex quantisation, the mesh blob
//   oxcull_abi_vsm.cpp    HPB build, VSM page update, shadow draw, shadow resolve
//   oxcull_abi_pixel.cpp  contact shadows, ambient occlusion, visbuffer decode, PBR
//   oxcull_abi_post.cpp   eye adaptation, bloom, tonemap, FXAA, the sky LUTs
//   oxcull_abi_terrain.cpp the terrain map producers, the terrain brush and the terrain decode
//   oxcull_abi_debug.cpp  the debug views
//   oxcull_abi_editor.cpp the editor's selection path: the transform pick and the selection highlight
//   oxcull_abi_sprites.cpp the 2D pass: the sprite queue's host helpers, the sprite draw and the sprite pick
//   oxcull_abi_comm.cpp   the RCCL exchange
#include <new>

#include "oxcull_host.hpp"

extern "C" {

uint32_t oxc_abi_version(void) { return OXC_ABI_VERSION; }

oxc_status oxc_create(int device, oxc_ctx** out) {
  if (!out) return OXC_INVALID_ARG;
  *out = nullptr;
  oxc_ctx* ctx = new (std::nothrow) oxc_ctx();
  if (!ctx) return OXC_OUT_OF_MEMORY;
  ctx->device = device;
  hipError_t e = hipSetDevice(device);
  if (e != hipSuccess) {
    delete ctx;
    return OXC_HIP_ERROR;
  }
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0)
    ctx->num_cus = (uint32_t)prop.multiProcessorCount;
  e = hipMalloc(reinterpret_cast<void**>(&ctx->slots), (size_t)kSlots * SLOT_U32S * 4 + 256);
  if (e != hipSuccess) {
    delete ctx;
    return OXC_OUT_OF_MEMORY;
  }
  // (hipMemset runs on the NULL stream, which does not order against the non-blocking streams callers pass in: without the synchronisation a
  // fill that starts late -- the first one of a process loads its kernel lazily -- lands on slots the first calls have already written)
  (void)hipMemset(ctx->slots, 0, (size_t)kSlots * SLOT_U32S * 4 + 256);
  (void)hipDeviceSynchronize();
  ctx->sink = ctx->slots + (size_t)kSlots * SLOT_U32S;
  *out = ctx;
  return OXC_OK;
}

void oxc_destroy(oxc_ctx* ctx) {
  if (!ctx) return;
  (void)hipSetDevice(ctx->device);
  (void)hipDeviceSynchronize();
  for (auto& ln : ctx->lane)
    if (ln.arena) (void)hipFree(ln.arena);
  if (ctx->batch_dev) (void)hipFree(ctx->batch_dev);
  if (ctx->mv_arena) (void)hipFree(ctx->mv_arena);
  if (ctx->bounds_scratch) (void)hipFree(ctx->bounds_scratch);
  if (ctx->raster_scratch) (void)hipFree(ctx->raster_scratch);
  if (ctx->raster_rows) (void)hipFree(ctx->raster_rows);
  if (ctx->sprite_scratch) (void)hipFree(ctx->sprite_scratch);
  if (ctx->vsm_scratch) (void)hipFree(ctx->vsm_scratch);
  if (ctx->vsm_draw_scratch) (void)hipFree(ctx->vsm_draw_scratch);
  for (const auto& pc : {ctx->vsm_resolve_stats, ctx->contact_shadows_stats, ctx->ambient_occlusion_stats, ctx->visbuffer_decode_stats, ctx->visbuffer_decode_textured_stats, ctx->pbr_apply_stats, ctx->fxaa_stats})
    if (pc.dev) (void)hipFree(pc.dev);
  if (ctx->comm) (void)oxc_comm_destroy(ctx);
  if (ctx->slots) (void)hipFree(ctx->slots);
  if (ctx->order_event) (void)hipEventDestroy(ctx->order_event);
  if (ctx->fork_event) (void)hipEventDestroy(ctx->fork_event);
  if (ctx->mv_side) (void)hipStreamDestroy(ctx->mv_side);
  if (ctx->mv_fork) (void)hipEventDestroy(ctx->mv_fork);
  if (ctx->mv_join) (void)hipEventDestroy(ctx->mv_join);
  for (auto& tp : ctx->tri)
    if (tp.done) (void)hipEventDestroy(tp.done);
  if (ctx->side) (void)hipStreamDestroy(ctx->side);
  delete ctx;
}

const char* oxc_last_error(const oxc_ctx* ctx) { return ctx ? ctx->last_error.c_str() : "null context"; }

oxc_status oxc_reserve(oxc_ctx* ctx, uint32_t max_mesh_instances, uint32_t max_meshlet_instances) {
  if (!ctx) return OXC_INVALID_ARG;
  OXC_HIP(ctx, hipSetDevice(ctx->device));
  return ensure_capacity(ctx, max_mesh_instances, max_meshlet_instances);  // (synchronises the device when it has to grow)
}

oxc_status oxc_profile_begin(oxc_ctx* ctx) {
  if (!ctx) return OXC_INVALID_ARG;
  ctx->recs.clear();
  ctx->profiling = true;
  return OXC_OK;
}

oxc_status oxc_profile_end(oxc_ctx* ctx, oxc_kernel_times* out) {
  if (!ctx) return OXC_INVALID_ARG;
  if (!out) return fail(ctx, OXC_INVALID_ARG, "profile_end: null out");
  ctx->profiling = false;
  std::memset(out, 0, sizeof *out);
  OXC_HIP(ctx, hipSetDevice(ctx->device));
  OXC_HIP(ctx, hipDeviceSynchronize());
  for (auto& r : ctx->recs) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, r.a, r.b) == hipSuccess && r.id >= 0 && r.id < OXC_K_COUNT) {
      out->total_ms[r.id] += ms;
      out->launches[r.id] += 1;
    }
    (void)hipEventDestroy(r.a);
    (void)hipEventDestroy(r.b);
  }
  ctx->recs.clear();
  // cost of an empty event pair on an idle stream (subtract per launch)
  hipEvent_t a, b;
  OXC_HIP(ctx, hipEventCreate(&a));
  OXC_HIP(ctx, hipEventCreate(&b));
  double acc = 0;
  const int reps = 32;
  for (int i = 0; i < reps; i++) {
    OXC_HIP(ctx, hipEventRecord(a, nullptr));
    OXC_HIP(ctx, hipEventRecord(b, nullptr));
    OXC_HIP(ctx, hipEventSynchronize(b));
    float ms = 0.f;
    OXC_HIP(ctx, hipEventElapsedTime(&ms, a, b));
    acc += ms;
  }
  (void)hipEventDestroy(a);
  (void)hipEventDestroy(b);
  out->empty_pair_ms = acc / reps;
  return OXC_OK;
}

oxc_status oxc_stream_read_probe(oxc_ctx* ctx, const void* dptr, uint64_t bytes, void* hip_stream) {
  if (!ctx) return OXC_INVALID_ARG;
  if (!dptr || (reinterpret_cast<uintptr_t>(dptr) & 15u)) return fail(ctx, OXC_INVALID_ARG, "stream_read_probe: pointer must be 16-byte aligned");
  OXC_HIP(ctx, hipSetDevice(ctx->device));
  launch_stream_read(dptr, bytes, ctx->sink, ctx->num_cus * 8, static_cast<hipStream_t>(hip_stream));
  OXC_HIP(ctx, hipGetLastError());
  return OXC_OK;
}

oxc_status oxc_debug_set_tuning(oxc_ctx* ctx, uint32_t knob, uint32_t value) {
  if (!ctx) return OXC_INVALID_ARG;
  switch (knob) {
    case OXC_TUNE_ASYNC_MTEST_BLOCKS_PER_CU: ctx->async_mtest_per_cu = value; return OXC_OK;
    case OXC_TUNE_ASYNC_TRI_BLOCKS_PER_CU: ctx->async_tri_per_cu = value; return OXC_OK;
    case OXC_TUNE_TRI_BLOCKS_PER_CU:
      if (value == 0) return fail(ctx, OXC_INVALID_ARG, "set_tuning: the triangle grid needs at least one block per CU");
      ctx->tri_blocks_per_cu = value;
      return OXC_OK;
    case OXC_TUNE_MV_EXPAND_ASYNC: ctx->mv_expand_async = value; return OXC_OK;
    case OXC_TUNE_TRI_LOADS:
      if (value > 2u) return fail(ctx, OXC_INVALID_ARG, "set_tuning: OXC_TUNE_TRI_LOADS is 0 (by the scene), 1 (nt) or 2 (plain)");
      ctx->tri_loads = value;
      return OXC_OK;
    case OXC_TUNE_RASTER_BIG_CAPACITY:
      if (ctx->raster_scratch) return fail(ctx, OXC_INVALID_ARG, "set_tuning: the raster scratch is allocated by the first oxc_draw_visbuffer; set its capacity before");
      ctx->raster_capacity_request = value;
      return OXC_OK;
    case OXC_TUNE_VSM_DRAW_STATS: ctx->vsm_draw_stats = value != 0u; return OXC_OK;
    case OXC_TUNE_VSM_RESOLVE_STATS: ctx->vsm_resolve_stats.on = value != 0u; return OXC_OK;
    case OXC_TUNE_CONTACT_SHADOWS_STATS: ctx->contact_shadows_stats.on = value != 0u; return OXC_OK;
    case OXC_TUNE_VISBUFFER_DECODE_STATS: ctx->visbuffer_decode_stats.on = value != 0u; return OXC_OK;
    case OXC_TUNE_VISBUFFER_DECODE_TEXTURED_STATS: ctx->visbuffer_decode_textured_stats.on = value != 0u; return OXC_OK;
    case OXC_TUNE_PBR_APPLY_STATS: ctx->pbr_apply_stats.on = value != 0u; return OXC_OK;
    case OXC_TUNE_FXAA_STATS: ctx->fxaa_stats.on = value != 0u; return OXC_OK;
    case OXC_TUNE_EYE_ADAPTATION_GRID: ctx->eye_adaptation_grid = value; return OXC_OK;
    case OXC_TUNE_RASTER_GRID: ctx->raster_grid = value; return OXC_OK;
    case OXC_TUNE_TERRAIN_DRAW_GRID: ctx->terrain_draw_grid = value; return OXC_OK;
    case OXC_TUNE_TERRAIN_DRAW_STATS: ctx->terrain_draw_stats = value != 0; return OXC_OK;
    case OXC_TUNE_VSM_DRAW_GRID: ctx->vsm_draw_grid = value; return OXC_OK;
    case OXC_TUNE_BOUNDS_GRID: ctx->bounds_grid = value; return OXC_OK;
    case OXC_TUNE_BOUNDS_CHUNK: ctx->bounds_chunk = value; return OXC_OK;
    case OXC_TUNE_BLOOM_TAIL_LEVEL: ctx->bloom_tail_level = value; return OXC_OK;
    case OXC_TUNE_AMBIENT_OCCLUSION_STATS: ctx->ambient_occlusion_stats.on = value != 0u; return OXC_OK;
    case OXC_TUNE_VSM_DRAW_CAPACITY:
      if (ctx->vsm_draw_scratch) return fail(ctx, OXC_INVALID_ARG, "set_tuning: the shadow draw's scratch is allocated by the first oxc_draw_physical_pages; set its capacity before");
      ctx->vsm_draw_capacity_request = value;
      return OXC_OK;
    default: return fail(ctx, OXC_INVALID_ARG, "set_tuning: unknown knob");
  }
}

oxc_status oxc_debug_read_u32(oxc_ctx* ctx, const void* dptr, uint32_t n, uint32_t* host_out, void* hip_stream) {
  if (!ctx) return OXC_INVALID_ARG;
  if (!dptr || !host_out) return fail(ctx, OXC_INVALID_ARG, "debug_read_u32: null pointer");
  OXC_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t s = static_cast<hipStream_t>(hip_stream);
  OXC_HIP(ctx, hipMemcpyAsync(host_out, dptr, (size_t)n * 4u, hipMemcpyDeviceToHost, s));
  OXC_HIP(ctx, hipStreamSynchronize(s));
  return OXC_OK;
}

}  // extern "C"
