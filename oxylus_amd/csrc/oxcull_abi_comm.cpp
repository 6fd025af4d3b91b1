// oxcull_abi_comm.cpp -- the multi-GPU exchange of liboxcull.so: counter packing and RCCL through dlopen (oxc_comm_*, oxc_exchange_counts,
// oxc_broadcast_hiz*).
#include <dlfcn.h>

#include "oxcull_host.hpp"

extern "C" {

// ---- RCCL through dlopen: the exchange entry points are the only users ----
struct OxcRcclId {  // ncclUniqueId: passed BY VALUE to ncclCommInitRank
  char internal[OXC_COMM_UNIQUE_ID_BYTES];
};
namespace {
struct Rccl {
  void* lib = nullptr;
  int (*GetUniqueId)(void*) = nullptr;
  int (*CommInitRank)(void**, int, OxcRcclId, int) = nullptr;
  int (*CommDestroy)(void*) = nullptr;
  int (*AllGather)(const void*, void*, size_t, int, void*, hipStream_t) = nullptr;
  int (*Broadcast)(const void*, void*, size_t, int, int, void*, hipStream_t) = nullptr;
  const char* (*GetErrorString)(int) = nullptr;
};
Rccl* rccl() {
  static Rccl r;
  static bool tried = false;
  if (!tried) {
    tried = true;
    r.lib = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
    if (!r.lib) r.lib = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (r.lib) {
      r.GetUniqueId = reinterpret_cast<decltype(r.GetUniqueId)>(dlsym(r.lib, "ncclGetUniqueId"));
      r.CommInitRank = reinterpret_cast<decltype(r.CommInitRank)>(dlsym(r.lib, "ncclCommInitRank"));
      r.CommDestroy = reinterpret_cast<decltype(r.CommDestroy)>(dlsym(r.lib, "ncclCommDestroy"));
      r.AllGather = reinterpret_cast<decltype(r.AllGather)>(dlsym(r.lib, "ncclAllGather"));
      r.Broadcast = reinterpret_cast<decltype(r.Broadcast)>(dlsym(r.lib, "ncclBroadcast"));
      r.GetErrorString = reinterpret_cast<decltype(r.GetErrorString)>(dlsym(r.lib, "ncclGetErrorString"));
    }
  }
  return (r.lib && r.GetUniqueId && r.CommInitRank && r.CommDestroy && r.AllGather && r.Broadcast) ? &r : nullptr;
}
oxc_status rccl_fail(oxc_ctx* ctx, const char* what, int code) {
  static thread_local std::string msg;
  Rccl* r = rccl();
  msg = std::string(what) + ": " + ((r && r->GetErrorString) ? r->GetErrorString(code) : "RCCL error");
  ctx->last_error = msg;
  return OXC_RCCL_ERROR;
}
constexpr int kNcclUint8 = 1, kNcclUint32 = 3;  // ncclDataType_t values (rccl.h: ncclInt8 0, ncclUint8 1, ncclInt32 2, ncclUint32 3)
}  // namespace

oxc_status oxc_comm_unique_id(oxc_ctx* ctx, void* id128_host_out) {
  if (!ctx) return OXC_INVALID_ARG;
  if (!id128_host_out) return fail(ctx, OXC_INVALID_ARG, "comm_unique_id: null output");
  Rccl* r = rccl();
  if (!r) return fail(ctx, OXC_RCCL_ERROR, "librccl.so could not be loaded (needed only for the multi-GPU exchange)");
  OXC_HIP(ctx, hipSetDevice(ctx->device));
  int rc = r->GetUniqueId(id128_host_out);
  return rc == 0 ? OXC_OK : rccl_fail(ctx, "ncclGetUniqueId", rc);
}

oxc_status oxc_comm_init(oxc_ctx* ctx, const void* id128_host, uint32_t rank, uint32_t world) {
  if (!ctx) return OXC_INVALID_ARG;
  if (!id128_host || world == 0 || rank >= world) return fail(ctx, OXC_INVALID_ARG, "comm_init: null id or rank >= world");
  if (ctx->comm) return fail(ctx, OXC_INVALID_ARG, "comm_init: the context already has a communicator");
  Rccl* r = rccl();
  if (!r) return fail(ctx, OXC_RCCL_ERROR, "librccl.so could not be loaded (needed only for the multi-GPU exchange)");
  OXC_HIP(ctx, hipSetDevice(ctx->device));
  OxcRcclId id;
  std::memcpy(&id, id128_host, sizeof id);
  int rc = r->CommInitRank(&ctx->comm, (int)world, id, (int)rank);
  if (rc != 0) {
    ctx->comm = nullptr;
    return rccl_fail(ctx, "ncclCommInitRank", rc);
  }
  ctx->comm_rank = rank;
  ctx->comm_world = world;
  return OXC_OK;
}

oxc_status oxc_comm_destroy(oxc_ctx* ctx) {
  if (!ctx) return OXC_INVALID_ARG;
  if (ctx->comm) {
    Rccl* r = rccl();
    if (r) (void)r->CommDestroy(ctx->comm);
    ctx->comm = nullptr;
    ctx->comm_world = 0;
  }
  return OXC_OK;
}

oxc_status oxc_pack_counters(oxc_ctx* ctx, const oxc_cull_geometry_context* c, void* counts4_dptr, void* hip_stream) {
  if (!ctx) return OXC_INVALID_ARG;
  if (!c || c->struct_size != sizeof(oxc_cull_geometry_context) || !counts4_dptr) return fail(ctx, OXC_INVALID_ARG, "pack_counters: bad context struct or null output");
  if (!c->visibility_buffer.dptr || !c->cull_triangles_cmd_buffer.dptr || !c->draw_geometry_cmd_buffer.dptr)
    return fail(ctx, OXC_INVALID_ARG, "pack_counters: the context has no counter buffers yet (no cull_geometry call has filled them in)");
  OXC_ENTER(ctx, hip_stream, s);
  OXC_JOIN(ctx, s);
  launch_pack_counters(static_cast<const uint32_t*>(c->visibility_buffer.dptr), static_cast<const uint32_t*>(c->cull_triangles_cmd_buffer.dptr),
                       static_cast<const uint32_t*>(c->draw_geometry_cmd_buffer.dptr), static_cast<uint32_t*>(counts4_dptr), s);
  OXC_HIP(ctx, hipGetLastError());
  return OXC_OK;
}

oxc_status oxc_pack_counters_batch(oxc_ctx* ctx, uint32_t count, const oxc_cull_geometry_context* cs, void* counts4_dptr, void* hip_stream) {
  if (!ctx) return OXC_INVALID_ARG;
  if (!cs || !counts4_dptr || count == 0 || count > kMaxBatch) return fail(ctx, OXC_INVALID_ARG, "pack_counters_batch: 1..16 contexts and an output buffer");
  PackBlob b;
  std::memset(&b, 0, sizeof b);
  b.count = count;
  for (uint32_t e = 0; e < count; e++) {
    if (cs[e].struct_size != sizeof(oxc_cull_geometry_context)) return fail(ctx, OXC_INVALID_ARG, "pack_counters_batch: bad context struct");
    if (!cs[e].visibility_buffer.dptr || !cs[e].cull_triangles_cmd_buffer.dptr || !cs[e].draw_geometry_cmd_buffer.dptr)
      return fail(ctx, OXC_INVALID_ARG, "pack_counters_batch: a context has no counter buffers yet (no cull_geometry call has filled them in)");
    b.vis[e] = static_cast<const uint32_t*>(cs[e].visibility_buffer.dptr);
    b.tri_cmd[e] = static_cast<const uint32_t*>(cs[e].cull_triangles_cmd_buffer.dptr);
    b.draw_cmd[e] = static_cast<const uint32_t*>(cs[e].draw_geometry_cmd_buffer.dptr);
  }
  OXC_ENTER(ctx, hip_stream, s);
  OXC_JOIN(ctx, s);
  launch_pack_counters_batch(b, static_cast<uint32_t*>(counts4_dptr), s);
  OXC_HIP(ctx, hipGetLastError());
  return OXC_OK;
}

oxc_status oxc_exchange_counts(oxc_ctx* ctx, const void* counts4_dptr, void* all_counts_dptr, void* hip_stream) {
  if (!ctx) return OXC_INVALID_ARG;
  if (!ctx->comm) return fail(ctx, OXC_INVALID_ARG, "exchange_counts: oxc_comm_init has not been called");
  if (!counts4_dptr || !all_counts_dptr) return fail(ctx, OXC_INVALID_ARG, "exchange_counts: null buffer");
  OXC_ENTER(ctx, hip_stream, s);
  int rc = rccl()->AllGather(counts4_dptr, all_counts_dptr, 4, kNcclUint32, ctx->comm, s);
  return rc == 0 ? OXC_OK : rccl_fail(ctx, "ncclAllGather", rc);
}

oxc_status oxc_broadcast_hiz(oxc_ctx* ctx, const oxc_image* hiz, uint64_t total_bytes, uint32_t root, void* hip_stream) {
  if (!ctx) return OXC_INVALID_ARG;
  if (!ctx->comm) return fail(ctx, OXC_INVALID_ARG, "broadcast_hiz: oxc_comm_init has not been called");
  if (!hiz || !hiz->dptr || total_bytes == 0 || root >= ctx->comm_world) return fail(ctx, OXC_INVALID_ARG, "broadcast_hiz: null image, zero size or bad root");
  OXC_ENTER(ctx, hip_stream, s);
  int rc = rccl()->Broadcast(hiz->dptr, hiz->dptr, (size_t)total_bytes, kNcclUint8, (int)root, ctx->comm, s);
  return rc == 0 ? OXC_OK : rccl_fail(ctx, "ncclBroadcast", rc);
}

oxc_status oxc_broadcast_hiz_levels(oxc_ctx* ctx, const oxc_image* hiz, uint32_t first_level, uint64_t total_bytes, uint32_t root, void* hip_stream) {
  if (!ctx) return OXC_INVALID_ARG;
  if (!ctx->comm) return fail(ctx, OXC_INVALID_ARG, "broadcast_hiz_levels: oxc_comm_init has not been called");
  if (!hiz || !hiz->dptr || first_level >= hiz->levels || hiz->levels > 13 || root >= ctx->comm_world) return fail(ctx, OXC_INVALID_ARG, "broadcast_hiz_levels: null image, bad level or bad root");
  const uint64_t begin = hiz->level_offset[first_level];
  if (total_bytes <= begin) return fail(ctx, OXC_INVALID_ARG, "broadcast_hiz_levels: total_bytes does not reach first_level");
  OXC_ENTER(ctx, hip_stream, s);
  char* p = static_cast<char*>(hiz->dptr) + begin;
  int rc = rccl()->Broadcast(p, p, (size_t)(total_bytes - begin), kNcclUint8, (int)root, ctx->comm, s);
  return rc == 0 ? OXC_OK : rccl_fail(ctx, "ncclBroadcast", rc);
}

}  // extern "C"
