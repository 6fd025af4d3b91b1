// oxcull_abi_cull.cpp -- the cull path of liboxcull.so's C ABI: the two scratch arenas (each laid out by one function, walked once for
// its size and once to bind its pointers) and the counter-slot ring, the HiZ build, the cull calls -- oxc_cull_geometry and its batched
// form, each a sequence of named steps -- with their async-triangle and share_pass_tests bookkeeping, terrain.
#include "oxcull_host.hpp"

namespace {
constexpr uint32_t kMaxPackedInstances = 1u << 24;  // MESHLET_INSTANCE_ID_BITS, visbuffer.slang:9-10

// The lane arena for M mesh instances, N meshlets and Vw views (use_hpb): every part once, in arena order.  Returns the arena's size; with
// `base` (the allocation) it also binds the lane's pointers (Carve::take).
uint64_t lay_out_lane(oxc_ctx::Lane& L, uint32_t M, uint32_t N, uint32_t Vw, void* base) {
  const uint32_t m_chunks = cdiv(N, 64u), t_chunks = cdiv(N, kTriChunk);  // meshlet counts: per wave step, >= 64 meshlets
  Carve carve{0, static_cast<char*>(base)};
  carve.take(L.cache, (uint64_t)M * sizeof(InstCache));
  carve.take(L.cache_alt, (uint64_t)M * sizeof(InstCache));
  carve.take(L.view_cache, (uint64_t)M * Vw * sizeof(InstCache) + 64);
  carve.take(L.mesh_counts, (uint64_t)M * 4);
  carve.take(L.mesh_offsets, (uint64_t)M * 4);
  carve.take(L.bits, (uint64_t)cdiv(N, 64) * 8);
  carve.take(L.m_chunk_counts, (uint64_t)m_chunks * 4);
  carve.take(L.m_supers, (uint64_t)cdiv(m_chunks, kChunksPerSuper) * 4 * kSuperStride);
  carve.take(L.m_tickets, (uint64_t)kTicketCounters * 4 * kSuperStride);
  carve.take(L.m_supers_late, (uint64_t)cdiv(m_chunks, kChunksPerSuper) * 4 * kSuperStride);
  carve.take(L.m_tickets_late, (uint64_t)kTicketCounters * 4 * kSuperStride);
  carve.take(L.camera_test_bits, (uint64_t)cdiv(N, 64) * 8);
  carve.take(L.step_info, (uint64_t)m_chunks * 8);
  carve.take(L.tri_masks, (uint64_t)N * 16);  // one 64-bit pass mask per visible meshlet (two in wide mode)
  carve.take(L.t_chunk_counts, (uint64_t)t_chunks * 4);
  carve.take(L.t_supers, (uint64_t)cdiv(t_chunks, kChunksPerSuper) * 4 * kSuperStride);
  carve.take(L.t_supers_alt, (uint64_t)cdiv(t_chunks, kChunksPerSuper) * 4 * kSuperStride);
  return carve.off;
}

}  // namespace

// Grows the lane's scratch arena when the call needs more than it holds: device sync + free + malloc (documented in
// include/oxcull.h; oxc_reserve up front avoids it).  Never during stream capture: `s` = the calling stream.
// (Not grow_scratch: what goes with the old arena is forgotten between the sync and the free, and a failed malloc zeroes the capacities.)
oxc_status ensure_capacity(oxc_ctx* ctx, uint32_t mesh_instances, uint32_t meshlets, uint32_t views, uint32_t lane_index, hipStream_t s) {
  oxc_ctx::Lane* L = &ctx->lane[lane_index];
  if (mesh_instances <= L->cap_mesh_instances && meshlets <= L->cap_meshlets && views <= L->cap_views && L->arena) return OXC_OK;
  if (stream_is_capturing(s))
    return fail(ctx, OXC_INVALID_ARG, "scratch memory must grow but the stream is being captured: call oxc_reserve (or one un-captured call of this size) first");
  const uint32_t Vw = std::max(views, L->cap_views);
  const uint32_t M = std::max(std::max(mesh_instances, L->cap_mesh_instances), 1u);
  const uint32_t N = std::max(std::max(meshlets, L->cap_meshlets), 1u);
  const uint64_t bytes = lay_out_lane(*L, M, N, Vw, nullptr);
  OXC_HIP(ctx, hipDeviceSynchronize());  // in-flight work (the side stream's included) may still use the old arena
  for (auto& tp : ctx->tri) tp.valid = false;
  if (lane_index == 0) ctx->shared.valid = false;  // the early call's bits go with the arena
  if (L->arena) OXC_HIP(ctx, hipFree(L->arena));
  L->arena = nullptr;
  hipError_t e = hipMalloc(&L->arena, bytes);
  if (e != hipSuccess) {
    L->cap_mesh_instances = L->cap_meshlets = 0;
    return fail(ctx, OXC_OUT_OF_MEMORY, "hipMalloc(scratch arena)", e);
  }
  L->arena_bytes = lay_out_lane(*L, M, N, Vw, L->arena);
  L->cap_views = Vw;
  L->cap_mesh_instances = M;
  L->cap_meshlets = N;
  return OXC_OK;
}

namespace {

// Per-call slots come from the lower half of the ring, seed slots (oxc_seed_meshlet_instances: they
// must outlive many calls) from the upper half, so a wrapping call ring never lands on a live seed.
uint32_t* next_slot(oxc_ctx* ctx) {
  uint32_t* s = ctx->slots + (size_t)(ctx->slot_cursor % (kSlots / 2)) * SLOT_U32S;
  ctx->slot_cursor++;
  return s;
}
uint32_t* next_seed_slot(oxc_ctx* ctx) {
  uint32_t* s = ctx->slots + (size_t)(kSlots / 2 + ctx->seed_cursor % (kSlots / 2)) * SLOT_U32S;
  ctx->seed_cursor++;
  return s;
}

// Everything oxc_cull_geometry derives from (frame, context) before it touches the device.
struct CallInfo {
  uint32_t stages, M, N, views;
  bool do_meshes, do_meshlets, do_tris, occl, late;
};

oxc_status check_call(oxc_ctx* ctx, const oxc_prepared_frame* f, const oxc_cull_geometry_context* c, CallInfo& ci) {
  if (!f || !c || c->struct_size != sizeof(oxc_cull_geometry_context)) return fail(ctx, OXC_INVALID_ARG, "cull_geometry: bad frame/context struct");
  const uint32_t stages = c->stages ? c->stages : (uint32_t)OXC_STAGE_ALL;
  const uint32_t M = f->mesh_instance_count, N = f->max_meshlet_instance_count;
  const bool do_meshes = c->init_cull_meshes && (stages & OXC_STAGE_MESHES);
  const bool do_meshlets = (stages & OXC_STAGE_MESHLETS) != 0;
  const bool do_tris = (stages & OXC_STAGE_TRIANGLES) != 0;
  if (c->cull_camera.mesh_instance_count != M) return fail(ctx, OXC_INVALID_ARG, "cull_geometry: cull_camera.mesh_instance_count != frame.mesh_instance_count");
  if (M && (!f->meshes_buffer.dptr || !f->transforms_world_buffer.dptr || !f->mesh_instances_buffer.dptr))
    return fail(ctx, OXC_INVALID_ARG, "cull_geometry: meshes/transforms/mesh_instances buffer missing");
  if (f->mesh_instances_buffer.bytes < (uint64_t)M * sizeof(GpuMeshInstance)) return fail(ctx, OXC_INVALID_ARG, "cull_geometry: mesh_instances_buffer too small");
  if (N && (!f->meshlet_instances_buffer.dptr || f->meshlet_instances_buffer.bytes < (uint64_t)N * 8))
    return fail(ctx, OXC_INVALID_ARG, "cull_geometry: meshlet_instances_buffer missing or < 8*N bytes");
  if (do_meshlets && N && (!f->visible_meshlet_instances_indices_buffer.dptr || f->visible_meshlet_instances_indices_buffer.bytes < (uint64_t)N * 4))
    return fail(ctx, OXC_INVALID_ARG, "cull_geometry: visible_meshlet_instances_indices_buffer missing or < 4*N bytes");
  if (do_tris && N) {
    if (c->wide_triangle_index > 2u) return fail(ctx, OXC_INVALID_ARG, "cull_geometry: wide_triangle_index must be 0, 1 or 2");
    const uint64_t tris_per_meshlet = c->wide_triangle_index ? 128u : 64u, index_bytes = c->wide_triangle_index == 2u ? 8u : 4u;
    if (!f->reordered_indices_buffer.dptr || f->reordered_indices_buffer.bytes < (uint64_t)N * tris_per_meshlet * 3 * index_bytes)
      return fail(ctx, OXC_INVALID_ARG, "cull_geometry: reordered_indices_buffer missing or < N*64*3*4 bytes (N*128*3*4 with wide_triangle_index = 1, N*128*3*8 with 2)");
    // (wide_triangle_index = 2, {id, corner} pairs: no id limit below 2^32 -- N is a u32)
    if (c->wide_triangle_index != 2u && N > (c->wide_triangle_index ? kMaxPackedInstances / 2 : kMaxPackedInstances))
      return fail(ctx, OXC_INVALID_ARG, "cull_geometry: too many meshlet instances for the packed index (2^24, visbuffer.slang:9-14; 2^23 with wide_triangle_index = 1; pairs, wide_triangle_index = 2, have no limit)");
  }
  const bool occl = (c->cull_flags & OXC_CULL_TEST_OCCLUSION) != 0;
  const bool late = (c->cull_flags & OXC_CULL_LATE_PASS) != 0;
  if (c->use_hiz && do_meshlets) {
    if (!image_ok(c->hiz_attachment)) return fail(ctx, OXC_INVALID_ARG, "cull_geometry: use_hiz without a hiz_attachment");
    if (occl && N && (!f->meshlet_instance_visibility_mask_buffer.dptr || f->meshlet_instance_visibility_mask_buffer.bytes < (uint64_t)cdiv(N, 32u) * 4u))
      return fail(ctx, OXC_INVALID_ARG, "cull_geometry: visibility mask buffer missing or < ceil(N/32)*4 bytes");
  }
  if (c->small_triangle_cull > 1u) return fail(ctx, OXC_INVALID_ARG, "cull_geometry: small_triangle_cull must be 0 or 1");
  if (c->share_pass_tests > 1u || c->unordered_output > 1u) return fail(ctx, OXC_INVALID_ARG, "cull_geometry: share_pass_tests must be 0 or 1, unordered_output 0 or 1");
  if (c->implicit_meshlet_instances > 1u || c->_reserved1 != 0u) return fail(ctx, OXC_INVALID_ARG, "cull_geometry: implicit_meshlet_instances must be 0 or 1, _reserved1 0");
  if (c->meshlet_instance_runs_buffer.dptr && c->meshlet_instance_runs_buffer.bytes < (uint64_t)M * 8u)
    return fail(ctx, OXC_INVALID_ARG, "cull_geometry: meshlet_instance_runs_buffer < 8 bytes per mesh instance");
  if (c->implicit_meshlet_instances && (!c->meshlet_instance_runs_buffer.dptr || do_tris || !do_meshes))
    return fail(ctx, OXC_INVALID_ARG, "cull_geometry: implicit_meshlet_instances needs meshlet_instance_runs_buffer, cull_meshes in the call and no triangle stage");
  const uint32_t views = c->use_hpb ? c->vsm_clipmap_count : 0u;
  if (c->use_hpb && do_meshlets) {
    if (c->use_hiz) return fail(ctx, OXC_INVALID_ARG, "cull_geometry: use_hiz and use_hpb are exclusive (CullGeometry.cpp:129,199)");
    if (views == 0 || views > 16) return fail(ctx, OXC_INVALID_ARG, "cull_geometry: vsm_clipmap_count must be 1..16");
    if (!c->vsm_clipmaps_buffer.dptr || c->vsm_clipmaps_buffer.bytes < (uint64_t)views * sizeof(oxc_virtual_clipmap) || !c->vsm_clipmap_dirty_flags_buffer.dptr ||
        c->vsm_clipmap_dirty_flags_buffer.bytes < (uint64_t)views * 4u)
      return fail(ctx, OXC_INVALID_ARG, "cull_geometry: use_hpb needs vsm_clipmaps_buffer (76 B per clipmap) / vsm_clipmap_dirty_flags_buffer (4 B per clipmap)");
    const oxc_image_array_u8& h = c->hpb_attachment;
    if (!h.dptr || !h.width || !h.height || h.layers < views || h.levels < 1 || h.levels > 13)
      return fail(ctx, OXC_INVALID_ARG, "cull_geometry: use_hpb without a valid hpb_attachment (layers >= clipmaps, 1..13 levels)");
    for (uint32_t k = 0; k < h.levels; k++) {  // the page test addresses the pyramid with 32-bit byte offsets (test_vsm_page)
      const uint64_t mw = std::max(1u, h.width >> k), mh = std::max(1u, h.height >> k);
      if (h.level_offset[k] + (uint64_t)h.layers * mw * mh > 0xFFFFFFFFull)
        return fail(ctx, OXC_INVALID_ARG, "cull_geometry: hpb_attachment larger than 4 GiB (the reference's is 64 x 64 pages x 10 clipmaps, Shadowmaps.cpp:84-98)");
    }
  }
  if (!c->init_cull_meshes && (!c->visibility_buffer.dptr || !c->cull_meshlets_cmd_buffer.dptr))
    return fail(ctx, OXC_INVALID_ARG, "cull_geometry: init_cull_meshes=false needs the visibility/cull_meshlets_cmd buffers of the sequence");
  ci = {stages, M, N, views, do_meshes, do_meshlets, do_tris, occl, late};
  return OXC_OK;
}

// The counters of the sequence a cull call works on and, where the host knows it (oxc_seed_meshlet_instances), the length of its list (else 0)
struct CullLists {
  uint32_t *vis, *meshlets_cmd;
  uint32_t n_host;
};

// The caller's context is told where a call leaves its triangle-stage and draw commands: in the call's slot
void name_cmd_buffers(oxc_cull_geometry_context* c, uint32_t* slot) {
  c->cull_triangles_cmd_buffer = {slot + SLOT_TRI_CMD, 12};
  c->draw_geometry_cmd_buffer = {slot + SLOT_DRAW_CMD, 20};
}

// With init_cull_meshes the counters are those of `slot`, and the caller's context is told; otherwise that context names them.
CullLists resolve_lists(oxc_ctx* ctx, oxc_cull_geometry_context* c, uint32_t* slot, uint32_t N) {
  CullLists l = {nullptr, nullptr, 0};
  if (c->init_cull_meshes) {
    l.vis = slot + SLOT_VIS;
    l.meshlets_cmd = slot + SLOT_MESHLETS_CMD;
    c->visibility_buffer = {l.vis, 12};
    c->cull_meshlets_cmd_buffer = {l.meshlets_cmd, 12};
    return l;
  }
  l.vis = static_cast<uint32_t*>(c->visibility_buffer.dptr);
  l.meshlets_cmd = static_cast<uint32_t*>(c->cull_meshlets_cmd_buffer.dptr);
  if (l.vis >= ctx->slots && l.vis < ctx->slots + (size_t)kSlots * SLOT_U32S && ((l.vis - ctx->slots) % SLOT_U32S) == SLOT_VIS)
    l.n_host = ctx->seeded_total[(l.vis - ctx->slots) / SLOT_U32S];
  if (l.n_host > N) l.n_host = 0;
  return l;
}

// ---- oxc_cull_geometry in steps ----
// async_triangles: the call's number and what goes with its parity
struct TriSet {
  uint64_t call_no;
  bool async;
  InstCache* rows;
  uint32_t* t_supers;
  oxc_ctx::TriPending* pending;  // the ring entry that will describe this call's triangle stage
};

// share_pass_tests: what plan_shared_tests decided
struct SharePlan {
  uint32_t mode = 0;                            // 1: the early call that publishes its results, 2: the late call that continues it
  bool armed_late = false, arm_late = false;    // a late call whose early call did its prepare work / the early call that does it
  uint32_t* slot = nullptr;                     // the call's counter slot
  uint32_t *m_supers = nullptr, *m_tickets = nullptr, *t_supers = nullptr;  // the accumulators and
  InstCache* rows = nullptr;                    // instance rows the call uses: its own, or (armed late call) those its early call prepared
};

// What the steps of one oxc_cull_geometry call hand to each other
struct CullCall {
  oxc_ctx* ctx;
  const oxc_prepared_frame* f;
  oxc_cull_geometry_context* c;
  hipStream_t s;
  CallInfo ci;
  TriSet tri;
  CullLists lists;
  uint32_t mask_bits;
  bool unord_tris, unord_meshlets;  // unordered_output (include/oxcull.h): which stages append by themselves
  SharePlan share;
  uint32_t *tri_cmd, *draw_cmd;
  uint32_t max_grid, m_chunks, t_chunks, n_supers_tris;
};

// ---- async_triangles bookkeeping (include/oxcull.h).  Calls alternate between two sets of instance rows / triangle-count
// accumulators, so that what this call's prepare kernel writes on `s` is never what a triangle stage still in flight on the
// side stream reads; the set of this call was last used by the call before the previous one.
oxc_status begin_triangle_bookkeeping(CullCall& k) {
  oxc_ctx* ctx = k.ctx;
  oxc_ctx::Lane& L0 = ctx->lane[0];
  TriSet& t = k.tri;
  t.call_no = ctx->call_seq++;
  t.async = k.c->async_triangles != 0 && k.ci.do_tris;
  t.rows = (t.call_no & 1u) ? L0.cache_alt : L0.cache;
  t.t_supers = (t.call_no & 1u) ? L0.t_supers_alt : L0.t_supers;
  t.pending = &ctx->tri[t.call_no % oxc_ctx::kTriRing];
  t.pending->valid = false;  // (the stage of call_no - kTriRing: every call since has waited for it where it mattered, and the side stream is in order)
  if (!t.async || k.ci.do_meshes) {
    // in order on `s`: the triangle stage shares tri_masks / chunk counts with the side stream; cull_meshes rewrites the
    // MeshletInstance records a pending stage reads
    OXC_JOIN(ctx, k.s);
  } else if (t.call_no >= 2) {
    const oxc_ctx::TriPending* old = &ctx->tri[(t.call_no - 2) % oxc_ctx::kTriRing];
    OXC_TRY(wait_triangles(ctx, k.s, [old](const oxc_ctx::TriPending& tp) { return &tp == old; }));
  }
  return OXC_OK;
}

// the meshlet emit of this call overwrites the visible list: wait for the pending stages that still read it -- all but the
// early triangle stage of the same sequence when this is its late call (the late list starts behind the early one)
oxc_status wait_for_visible_list(const CullCall& k) {
  const bool late = k.ci.late;
  const uint32_t* vis_now = k.lists.vis;
  const void* const visible_buf = k.f->visible_meshlet_instances_indices_buffer.dptr;
  return wait_triangles(k.ctx, k.s, [&](const oxc_ctx::TriPending& tp) { return !(late && !tp.late && tp.vis == vis_now && tp.visible == visible_buf); });
}

// ---- share_pass_tests (include/oxcull.h): is this the early call that publishes its frustum + cone results (1), or the late call that
// continues it (2)?  An early call in order on one stream (no async_triangles) also does the late call's prepare work in its own
// prepare kernel -- accumulators, counter slot; the instance rows are the same -- so that a late call that follows it immediately
// launches no prepare kernel at all.
// `slot`: the slot the call has taken already (init_cull_meshes), else null: it is taken here, AFTER the slot an arming early call takes for
// its late call -- which slot a call gets decides which counters a later call reads.
SharePlan plan_shared_tests(const CullCall& k, uint32_t* slot) {
  oxc_ctx* ctx = k.ctx;
  const oxc_prepared_frame* f = k.f;
  const oxc_cull_geometry_context* c = k.c;
  oxc_ctx::Lane& L0 = ctx->lane[0];
  const uint64_t call_no = k.tri.call_no;
  SharePlan p;
  p.slot = slot;
  p.m_supers = L0.m_supers;
  p.m_tickets = L0.m_tickets;
  p.t_supers = k.tri.t_supers;
  p.rows = k.tri.rows;
  if (c->use_hiz && k.ci.occl && c->share_pass_tests && k.ci.do_meshlets && !k.unord_meshlets) {
    oxc_ctx::SharedTests now;
    now.N = k.ci.N;
    now.n_host = k.lists.n_host;
    now.M = k.ci.M;
    now.flags = c->cull_flags & ~(uint32_t)OXC_CULL_LATE_PASS;
    now.mask_bits = k.mask_bits;  // (the early call's "one run of mask bits" is a statement about this many bits)
    now.meshlet_instances = f->meshlet_instances_buffer.dptr;
    now.mask = f->meshlet_instance_visibility_mask_buffer.dptr;
    now.meshes = f->meshes_buffer.dptr;
    now.transforms = f->transforms_world_buffer.dptr;
    now.mesh_instances = f->mesh_instances_buffer.dptr;
    now.vis = k.lists.vis;
    now.camera = c->cull_camera;
    if (!k.ci.late) {
      p.mode = 1u;
      p.arm_late = c->async_triangles == 0;
      now.valid = true;
      if (p.arm_late) {
        now.armed_for_call = call_no + 1;
        now.capture_id = stream_capture_id(k.s);
        now.late_slot = next_slot(ctx);
        now.late_t_supers = (call_no & 1u) ? L0.t_supers : L0.t_supers_alt;  // the other set: this call's triangle stage uses t_supers
        now.rows = p.rows;
      }
      ctx->shared = now;
    } else if (!k.ci.do_meshes && !c->init_cull_meshes && ctx->shared.valid && ctx->shared.same_inputs(now)) {
      p.mode = 2u;
      if (ctx->shared.armed_for_call == call_no && c->async_triangles == 0 && ctx->shared.capture_id == stream_capture_id(k.s)) {
        p.armed_late = true;
        p.slot = ctx->shared.late_slot;
        p.t_supers = ctx->shared.late_t_supers;
        p.rows = ctx->shared.rows;
        p.m_supers = L0.m_supers_late;
        p.m_tickets = L0.m_tickets_late;
      }
      ctx->shared.valid = false;  // the bits are consumed ONCE: a second late call, or a late call of a later frame whose early call did not
                                  // publish, tests for itself (what the host can check of "nothing was written in between" is little enough)
    }
  } else if (c->use_hiz && k.ci.do_meshlets && !k.ci.late) {
    ctx->shared.valid = false;  // an early HiZ call without the flag starts a frame whose late call must not pick up an older frame's bits
  }
  if (!p.armed_late && ctx->shared.armed_for_call <= call_no) ctx->shared.armed_for_call = ~0ull;  // (armed for this call only)
  if (!p.slot) p.slot = next_slot(ctx);
  return p;
}

// --- prepare (+ cull_meshes test): CullGeometry.cpp:69-117
void launch_prepare_and_meshes(const CullCall& k) {
  oxc_ctx* ctx = k.ctx;
  const oxc_prepared_frame* f = k.f;
  const oxc_cull_geometry_context* c = k.c;
  oxc_ctx::Lane& L0 = ctx->lane[0];
  const SharePlan& sh = k.share;
  const uint32_t M = k.ci.M, N = k.ci.N;
  PrepareArgs pa;
  pa.meshes = static_cast<const GpuMesh*>(f->meshes_buffer.dptr);
  pa.transforms = static_cast<const float*>(f->transforms_world_buffer.dptr);
  pa.mesh_instances = static_cast<GpuMeshInstance*>(f->mesh_instances_buffer.dptr);
  pa.cache = sh.rows;
  pa.mesh_counts = L0.mesh_counts;
  pa.slot = sh.slot;
  pa.vis = k.lists.vis;
  pa.meshlets_cmd = k.lists.meshlets_cmd;
  pa.supers_meshlets = sh.m_supers;
  pa.supers_tris = sh.t_supers;
  pa.tickets = sh.m_tickets;
  pa.slot_late = sh.arm_late ? ctx->shared.late_slot : nullptr;
  pa.supers_meshlets_late = sh.arm_late ? L0.m_supers_late : nullptr;
  pa.supers_tris_late = sh.arm_late ? ctx->shared.late_t_supers : nullptr;
  pa.tickets_late = sh.arm_late ? L0.m_tickets_late : nullptr;
  pa.n_supers_meshlets = cdiv(cdiv(std::max(N, 1u), 64u), kChunksPerSuper);
  pa.n_supers_tris = k.n_supers_tris;
  pa.mesh_instance_count = M;
  pa.cull_flags = c->cull_flags;
  pa.do_cull_meshes = k.ci.do_meshes ? 1u : 0u;
  pa.init_vis = c->init_cull_meshes ? 1u : 0u;
  pa.seed_total = 0;
  pa.cam = c->cull_camera;
  pa.clipmaps = static_cast<const oxc_virtual_clipmap*>(c->vsm_clipmaps_buffer.dptr);
  pa.view_cache = L0.view_cache;
  const uint32_t prep_threads = std::max(std::max(M * 8u, pa.n_supers_tris), 1u);  // 8 lanes per mesh instance
  if (!sh.armed_late) {  // (an armed late call: the early call of the frame did all of this)
    KernelTimer t(ctx, OXC_K_PREPARE, k.s);
    launch_prepare(pa, std::min(cdiv(prep_threads, 256), k.max_grid), (c->use_hpb && k.ci.do_meshlets) ? k.ci.views : 0u, k.s);
  }
  if (k.ci.do_meshes) {
    {
      KernelTimer t(ctx, OXC_K_MESHES_SCAN, k.s);
      launch_scan_mesh_counts(L0.mesh_counts, L0.mesh_offsets, M, N, k.lists.vis, k.lists.meshlets_cmd, k.s);
    }
    KernelTimer t(ctx, OXC_K_MESHES_EXPAND, k.s);
    launch_expand(L0.mesh_counts, L0.mesh_offsets, M, N, f->meshlet_instances_buffer.dptr, std::max(std::min(cdiv(M, 4), k.max_grid), 1u), k.s);
  }
}

// The meshlet emit's arguments after a test that left one count per wave step of `count_meshlets` meshlets in the accumulators `supers`
MeshletEmitArgs emit_args(const CullCall& k, uint32_t n_host, uint32_t count_meshlets, uint32_t* supers) {
  MeshletEmitArgs ea;
  ea.n_host = n_host;
  ea.n_cap = k.ci.N;
  ea.count_meshlets = count_meshlets;
  ea.bits = k.ctx->lane[0].bits;
  ea.chunk_counts = k.ctx->lane[0].m_chunk_counts;
  ea.supers = supers;
  ea.vis = k.lists.vis;
  ea.tri_cmd = k.tri_cmd;
  ea.out = static_cast<uint32_t*>(k.f->visible_meshlet_instances_indices_buffer.dptr);
  return ea;
}

// --- meshlet stage against the shadow pages of the VSM clipmaps (use_hpb): CullGeometry.cpp:199-273
oxc_status meshlet_stage_hpb(const CullCall& k) {
  oxc_ctx* ctx = k.ctx;
  const oxc_cull_geometry_context* c = k.c;
  oxc_ctx::Lane& L0 = ctx->lane[0];
  HpbTestArgs ha;
  std::memset(&ha, 0, sizeof ha);
  ha.cache = k.share.rows;
  ha.view_cache = L0.view_cache;
  ha.meshlet_instances = static_cast<const GpuMeshletInstance*>(k.f->meshlet_instances_buffer.dptr);
  ha.vis = k.lists.vis;
  ha.bits = L0.bits;
  ha.chunk_counts = L0.m_chunk_counts;
  ha.supers = L0.m_supers;
  ha.tickets = L0.m_tickets;
  ha.clipmaps = static_cast<const oxc_virtual_clipmap*>(c->vsm_clipmaps_buffer.dptr);
  ha.dirty = static_cast<const uint32_t*>(c->vsm_clipmap_dirty_flags_buffer.dptr);
  ha.clipmap_count = k.ci.views;
  ha.mesh_instance_count = k.ci.M;
  ha.n_cap = k.ci.N;
  const oxc_image_array_u8& h = c->hpb_attachment;
  ha.hpb_data = static_cast<const uint8_t*>(h.dptr);
  ha.hpb_w = h.width;
  ha.hpb_h = h.height;
  ha.hpb_layers = h.layers;
  ha.hpb_levels = h.levels;
  for (uint32_t j = 0; j < h.levels && j < 13; j++) ha.hpb_level_off[j] = (uint32_t)h.level_offset[j];
  std::memcpy(ha.light_dir, c->cull_camera.position, 12);  // camera.position = -light_dir (Shadowmaps.cpp:433-437)
  {
    KernelTimer t(ctx, OXC_K_MESHLETS_TEST, k.s);
    launch_hpb_test(ha, std::min(k.m_chunks, k.max_grid), k.s);
  }
  const MeshletEmitArgs ea = emit_args(k, 0, 64u * kGroupsPerWave, L0.m_supers);  // one count per wave step
  OXC_TRY(wait_for_visible_list(k));
  KernelTimer t(ctx, OXC_K_MESHLETS_EMIT, k.s);
  launch_meshlets_emit(ea, false, false, std::min(cdiv(std::max(k.ci.N, 1u), kMeshletSpan), k.max_grid), k.s);
  return OXC_OK;
}

// --- meshlet stage against the camera, with or without the HiZ pyramid: CullGeometry.cpp:129-335
oxc_status meshlet_stage(const CullCall& k) {
  oxc_ctx* ctx = k.ctx;
  const oxc_prepared_frame* f = k.f;
  const oxc_cull_geometry_context* c = k.c;
  oxc_ctx::Lane& L0 = ctx->lane[0];
  const uint32_t N = k.ci.N;
  const bool occl = k.ci.occl, late = k.ci.late;
  // Two kernels only run side by side when neither fills every wave slot (tools/overlap_probe.py): with async_triangles the
  // persistent kernels of both stages take a share of the CUs' slots instead of all of them.
  const uint32_t mtest_limit = (c->async_triangles && ctx->async_mtest_per_cu) ? ctx->async_mtest_per_cu * ctx->num_cus : 0u;
  MeshletTestArgs ta;
  std::memset(&ta, 0, sizeof ta);
  ta.n_host = k.lists.n_host;
  ta.n_cap = N;
  ta.mask_bits = k.mask_bits;
  ta.cache = k.share.rows;
  ta.meshlet_instances = static_cast<const GpuMeshletInstance*>(f->meshlet_instances_buffer.dptr);
  ta.vis = k.lists.vis;
  ta.mask = static_cast<uint32_t*>(f->meshlet_instance_visibility_mask_buffer.dptr);
  ta.bits = L0.bits;
  ta.chunk_counts = L0.m_chunk_counts;
  ta.supers = k.share.m_supers;
  if (c->use_hiz) {
    ta.tickets = k.share.m_tickets;  // the HiZ variants take their work dynamically (step cost varies 10x)
    const oxc_image& h = c->hiz_attachment;
    ta.hiz_data = static_cast<const float*>(h.dptr);
    ta.hiz_w = h.width;
    ta.hiz_h = h.height;
    ta.hiz_levels = h.levels;
    for (uint32_t j = 0; j < h.levels && j < 13; j++) ta.hiz_level_off[j] = (uint32_t)(h.level_offset[j] / 4);
    // LDS-staged top of the pyramid: the longest suffix of levels that fits kHizLdsTexels floats
    uint32_t first = h.levels, used = 0;
    while (first > 0) {
      const uint64_t n = (uint64_t)std::max(1u, h.width >> (first - 1)) * std::max(1u, h.height >> (first - 1));
      if (used + n > kHizLdsTexels) break;
      used += (uint32_t)n;
      first--;
    }
    ta.hiz_lds_first = first;
    uint32_t off = 0;
    for (uint32_t j = first; j < h.levels; j++) {
      ta.hiz_lds_off[j] = off;
      off += std::max(1u, h.width >> j) * std::max(1u, h.height >> j);
    }
  }
  ta.near_clip = c->cull_camera.near_clip;
  std::memcpy(ta.cam_pos, c->cull_camera.position, 12);
  ta.dbg_occlusion = ctx->dbg_occlusion;  // (oxc_debug_count_occlusion_candidates; null unless a measurement asked for it)
  if (k.share.mode) {  // include/oxcull.h: the late call of a frame reuses the early call's frustum + cone results (plan_shared_tests)
    ta.share = k.share.mode;
    ta.camera_test_bits = L0.camera_test_bits;
    ta.step_info = L0.step_info;
  }
  ctx->last_share_mode = k.share.armed_late ? 3u : ta.share;
  if (k.unord_meshlets) {  // the test kernel appends: it writes the visible list (wait for the stages that still read it) and both counters
    ta.out = static_cast<uint32_t*>(f->visible_meshlet_instances_indices_buffer.dptr);
    ta.count_a = k.tri_cmd;
    OXC_TRY(wait_for_visible_list(k));
    KernelTimer t(ctx, late ? OXC_K_MESHLETS_TEST_LATE : OXC_K_MESHLETS_TEST, k.s);
    launch_meshlets_test(ta, c->use_hiz != 0, occl, late, std::min(k.m_chunks, k.max_grid), ctx->num_cus, mtest_limit, k.s);
    return OXC_OK;
  }
  {
    KernelTimer t(ctx, late ? OXC_K_MESHLETS_TEST_LATE : OXC_K_MESHLETS_TEST, k.s);
    launch_meshlets_test(ta, c->use_hiz != 0, occl, late, std::min(k.m_chunks, k.max_grid), ctx->num_cus, mtest_limit, k.s);
  }
  // one count per wave step: 64 * groups per wave
  const MeshletEmitArgs ea = emit_args(k, k.lists.n_host, c->use_hiz ? 64u * kHizGroupsPerWave : 64u * kPlainGroups, k.share.m_supers);
  OXC_TRY(wait_for_visible_list(k));
  KernelTimer t(ctx, late ? OXC_K_MESHLETS_EMIT_LATE : OXC_K_MESHLETS_EMIT, k.s);
  launch_meshlets_emit(ea, c->use_hiz != 0, late, std::min(cdiv(std::max(N, 1u), kMeshletSpan), k.max_grid), k.s);
  return OXC_OK;
}

// --- triangle stage: CullGeometry.cpp:337-403
oxc_status triangle_stage(const CullCall& k) {
  oxc_ctx* ctx = k.ctx;
  const oxc_prepared_frame* f = k.f;
  const oxc_cull_geometry_context* c = k.c;
  oxc_ctx::Lane& L0 = ctx->lane[0];
  const uint32_t N = k.ci.N;
  const bool async = k.tri.async, late = k.ci.late;
  uint32_t* const t_supers = k.share.t_supers;
  // (the persistent kernels' share of the CUs' wave slots while the two stages run side by side: see meshlet_stage)
  const uint32_t tri_grid_cap = (async && ctx->async_tri_per_cu) ? ctx->async_tri_per_cu * ctx->num_cus : ctx->num_cus * ctx->tri_blocks_per_cu;
  hipStream_t ts = k.s;
  if (async) {  // fork: everything enqueued on `s` so far (this call's meshlet emit, the caller's earlier consumers of the index list) precedes the stage
    if (!ctx->side) OXC_HIP(ctx, hipStreamCreateWithFlags(&ctx->side, hipStreamNonBlocking));
    if (!ctx->fork_event) OXC_HIP(ctx, hipEventCreateWithFlags(&ctx->fork_event, hipEventDisableTiming));
    OXC_HIP(ctx, hipEventRecord(ctx->fork_event, k.s));
    OXC_HIP(ctx, hipStreamWaitEvent(ctx->side, ctx->fork_event, 0));
    ts = ctx->side;
  }
  TriTestArgs tt;
  tt.cache = k.share.rows;
  tt.meshlet_instances = static_cast<const GpuMeshletInstance*>(f->meshlet_instances_buffer.dptr);
  tt.visible = static_cast<const uint32_t*>(f->visible_meshlet_instances_indices_buffer.dptr);
  tt.vis = k.lists.vis;
  tt.tri_cmd = k.tri_cmd;
  tt.tri_masks = L0.tri_masks;
  tt.chunk_counts = L0.t_chunk_counts;
  tt.supers = t_supers;
  tt.resolution[0] = c->cull_camera.resolution[0];
  tt.resolution[1] = c->cull_camera.resolution[1];
  tt.draw_cmd = k.draw_cmd;
  tt.out = static_cast<uint32_t*>(f->reordered_indices_buffer.dptr);
  tt.ticket = t_supers;  // (zeroed by this call's prepare kernel; the fused form has no other use for the accumulators)
  tt.ticket_count = std::max(k.n_supers_tris, 1u);
  // Geometry shared between instances (the engine's case: a few Mesh records, many MeshInstances) is read with plain loads -- the next visible
  // meshlet of another instance finds the lines in L2; unique geometry is streamed once with `nt` loads (oxcull_kernels.hip, OXC_TRI_LOAD_*).
  // "Shared" = at least four mesh instances per Mesh record of the caller's meshes_buffer.
  const uint64_t mesh_records = f->meshes_buffer.bytes / sizeof(GpuMesh);
  const bool cached_loads = ctx->tri_loads == 2u || (ctx->tri_loads == 0u && mesh_records != 0u && (uint64_t)k.ci.M >= 4u * mesh_records);
  ctx->last_tri_loads = (cached_loads && !c->small_triangle_cull) ? 2u : 1u;
  // (a cap set by hand stands; what the default cap is depends on the form of the stage, below)
  const bool default_cap = !(async && ctx->async_tri_per_cu) && ctx->tri_blocks_per_cu == kTriangleBlocksPerCU;
  if (k.unord_tris) {  // one launch: test + expansion per work item (a span of kFusedTriSpan visible meshlets, or a chunk of it)
    KernelTimer t(ctx, late ? OXC_K_TRIANGLES_TEST_LATE : OXC_K_TRIANGLES_TEST, ts);
    // (the default cap is "one resident round": of the instantiation that runs, which the launcher knows; a cap set by hand stands)
    launch_tris_fused(tt, late, c->wide_triangle_index, c->small_triangle_cull != 0, cached_loads, std::min(cdiv(std::max(N, 1u), kFusedTriSpan), tri_grid_cap),
                      default_cap ? ctx->num_cus : 0u, ts);
  } else {
    {
      KernelTimer t(ctx, late ? OXC_K_TRIANGLES_TEST_LATE : OXC_K_TRIANGLES_TEST, ts);
      // (the ordered test kernel walks 64-meshlet chunks with a grid stride: with the default cap it takes four resident rounds of blocks and
      //  lets the dispatcher balance them -- late launch 149.6 -> 140.3 us on the configs[2] frame; a cap set by hand stands)
      launch_tris_test(tt, late, c->wide_triangle_index != 0, c->small_triangle_cull != 0, cached_loads, std::min(k.t_chunks, (default_cap && !c->wide_triangle_index) ? ctx->num_cus * 32u : tri_grid_cap), ts);  // (WIDE, 4 waves per SIMD: 8 per CU measured better than 32)
    }
    TriEmitArgs te;
    te.tri_masks = L0.tri_masks;
    te.visible = tt.visible;
    te.vis = k.lists.vis;
    te.tri_cmd = k.tri_cmd;
    te.chunk_counts = L0.t_chunk_counts;
    te.supers = t_supers;
    te.draw_cmd = k.draw_cmd;
    te.out = static_cast<uint32_t*>(f->reordered_indices_buffer.dptr);
    KernelTimer t(ctx, late ? OXC_K_TRIANGLES_EMIT_LATE : OXC_K_TRIANGLES_EMIT, ts);
    launch_tris_emit(te, late, c->wide_triangle_index, std::min(cdiv(std::max(N, 1u), kTriSpan), tri_grid_cap), ts);
  }
  if (async) {
    oxc_ctx::TriPending& my_tri = *k.tri.pending;
    if (!my_tri.done) OXC_HIP(ctx, hipEventCreateWithFlags(&my_tri.done, hipEventDisableTiming));
    OXC_HIP(ctx, hipEventRecord(my_tri.done, ts));
    my_tri.valid = true;
    my_tri.late = late;
    my_tri.vis = k.lists.vis;
    my_tri.visible = f->visible_meshlet_instances_indices_buffer.dptr;
    my_tri.capture_id = stream_capture_id(k.s);  // (the side stream joined the caller's capture through the fork event)
  }
  return OXC_OK;
}

// ---- oxc_cull_geometry_batch in steps ----
// What the steps of one batched call hand to each other
struct BatchCall {
  oxc_ctx* ctx;
  const oxc_prepared_frame* frames;
  oxc_cull_geometry_context* contexts;
  hipStream_t s;
  uint32_t count;
  CallInfo ci[kMaxBatch] = {};
  BatchCore cores[kMaxBatch] = {};  // every field once; k_prepare_batch rebuilds the seven stage blocks from it on the device (expand_batch_core)
  // plan_batch: one launch per stage serves all elements / they are views of one scene / from one camera position / with implicit_meshlet_instances;
  // batch_meshes_stage: the MeshletInstance expansion runs on the side stream
  bool fusable = false, multiview = false, same_pos = false, implicit_lists = false, mv_expand_async = false;
  uint32_t g_prep = 1, g_expand = 1, g_test = 1, g_emit = 1, g_ttest = 1, g_temit = 1;  // grid.x of each stage: the largest any element asks for
  uint32_t cap = 0, max_grid = 0;
};

// Can the elements share their launches, and in which form?  Enqueues nothing.
oxc_status plan_batch(BatchCall& b) {
  const oxc_prepared_frame* frames = b.frames;
  const oxc_cull_geometry_context* contexts = b.contexts;
  const CallInfo* ci = b.ci;
  const uint32_t count = b.count;
  b.fusable = count > 1 && count <= kMaxBatch;
  for (uint32_t e = 0; b.fusable && e < count; e++) {
    OXC_TRY(check_call(b.ctx, &frames[e], &contexts[e], b.ci[e]));
    const oxc_cull_geometry_context& c = contexts[e];
    b.fusable = !c.use_hiz && !c.use_hpb && !c.wide_triangle_index && !c.small_triangle_cull && !ci[e].late && ci[e].stages == ci[0].stages && ci[e].do_meshes == ci[0].do_meshes &&
                (c.init_cull_meshes != 0) == (contexts[0].init_cull_meshes != 0);
  }
  if (!b.fusable) return OXC_OK;
  // Several VIEWS of one scene (every element runs cull_meshes + cull_meshlets over the same meshes / transforms with its own camera --
  // shadow cascades, BASELINE configs[4]): the meshlet stage then runs once over the scene for all views (k_mv_test) instead of
  // once per view over that view's list.  Same outputs, element by element.
  b.multiview = ci[0].do_meshes && ci[0].do_meshlets && ci[0].M > 0;
  b.same_pos = true;
  for (uint32_t e = 1; b.multiview && e < count; e++) {
    b.multiview = ci[e].M == ci[0].M && frames[e].meshes_buffer.dptr == frames[0].meshes_buffer.dptr &&
                  frames[e].transforms_world_buffer.dptr == frames[0].transforms_world_buffer.dptr && contexts[e].cull_flags == contexts[0].cull_flags;
    b.same_pos = b.same_pos && std::memcmp(contexts[e].cull_camera.position, contexts[0].cull_camera.position, 12) == 0;
  }
  // implicit_meshlet_instances: all elements or none, and only where nothing reads the records -- the multi-view meshlet stage
  uint32_t n_implicit = 0;
  for (uint32_t e = 0; e < count; e++) n_implicit += contexts[e].implicit_meshlet_instances ? 1u : 0u;
  if (n_implicit && (n_implicit != count || !b.multiview || ci[0].do_tris))
    return fail(b.ctx, OXC_INVALID_ARG, "cull_geometry_batch: implicit_meshlet_instances must be set on every element of a multi-view batch (same scene, cull_meshes in every element, no triangle stage)");
  b.implicit_lists = n_implicit != 0;
  return OXC_OK;
}

// The elements one call at a time: a batch that cannot be fused, or whose prepare launch was refused
oxc_status cull_one_by_one(const BatchCall& b) {
  for (uint32_t e = 0; e < b.count; e++) OXC_TRY(oxc_cull_geometry(b.ctx, &b.frames[e], &b.contexts[e], b.s));
  return OXC_OK;
}

// The device copy of the argument blocks, allocated by the context's first batched call
oxc_status ensure_batch_block(oxc_ctx* ctx, hipStream_t s) {
  if (ctx->batch_dev) return OXC_OK;
  if (stream_is_capturing(s))
    return fail(ctx, OXC_INVALID_ARG, "cull_geometry_batch: the first batched call allocates its argument block; make one un-captured call first");
  hipError_t e = hipMalloc(reinterpret_cast<void**>(&ctx->batch_dev), sizeof(BatchElem) * kMaxBatch);
  if (e != hipSuccess) return fail(ctx, OXC_OUT_OF_MEMORY, "hipMalloc(batch argument block)", e);
  OXC_HIP(ctx, hipMemset(ctx->batch_dev, 0, sizeof(BatchElem) * kMaxBatch));  // fields no plain-pipeline block uses stay 0
  // The fill runs on the NULL stream; `s` is usually a non-blocking stream, i.e. NOT ordered behind it.  Round 4 found the race the hard way:
  // in a fresh process the first hipMemset loads its kernel lazily, k_prepare_batch (on `s`) wrote the argument blocks first, the late fill
  // zeroed them and the next kernel dereferenced null -- "memory access fault on address (nil)" in 2 of ~25 bench runs, only on slow boxes.
  OXC_HIP(ctx, hipDeviceSynchronize());
  return OXC_OK;
}

// Element e: its counter slot and lists, its core, and what it asks of the stages' grids
void fill_batch_core(BatchCall& b, uint32_t e) {
  const oxc_prepared_frame* f = &b.frames[e];
  oxc_cull_geometry_context* c = &b.contexts[e];
  oxc_ctx::Lane& L = b.ctx->lane[e];
  const uint32_t M = b.ci[e].M, N = b.ci[e].N, max_grid = b.max_grid;
  uint32_t* slot = next_slot(b.ctx);
  const CullLists lists = resolve_lists(b.ctx, c, slot, N);
  name_cmd_buffers(c, slot);
  const uint32_t m_chunks = cdiv(std::max(N, 1u), kMeshletChunk), t_chunks = cdiv(std::max(N, 1u), kTriChunk);

  BatchCore& k = b.cores[e];
  k.meshes = static_cast<const GpuMesh*>(f->meshes_buffer.dptr);
  k.transforms = static_cast<const float*>(f->transforms_world_buffer.dptr);
  k.mesh_instances = static_cast<GpuMeshInstance*>(f->mesh_instances_buffer.dptr);
  k.meshlet_instances = static_cast<GpuMeshletInstance*>(f->meshlet_instances_buffer.dptr);
  k.visible_out = static_cast<uint32_t*>(f->visible_meshlet_instances_indices_buffer.dptr);
  k.reordered_out = static_cast<uint32_t*>(f->reordered_indices_buffer.dptr);
  k.cache = L.cache;
  k.view_cache = L.view_cache;
  k.mesh_counts = L.mesh_counts;
  k.mesh_offsets = L.mesh_offsets;
  k.bits = L.bits;
  k.m_chunk_counts = L.m_chunk_counts;
  k.m_supers = L.m_supers;
  k.tri_masks = L.tri_masks;
  k.t_chunk_counts = L.t_chunk_counts;
  k.t_supers = L.t_supers;
  k.slot = slot;
  k.vis = lists.vis;
  k.meshlets_cmd = lists.meshlets_cmd;
  k.n_supers_meshlets = cdiv(cdiv(std::max(N, 1u), 64u), kChunksPerSuper);
  k.n_supers_tris = cdiv(t_chunks, kChunksPerSuper);
  k.mesh_instance_count = M;
  k.cull_flags = c->cull_flags;
  k.do_cull_meshes = b.ci[0].do_meshes ? 1u : 0u;
  k.init_vis = c->init_cull_meshes ? 1u : 0u;
  k.n_host = lists.n_host;
  k.n_cap = N;
  k.count_meshlets = 64u * kPlainGroups;
  k.cam = c->cull_camera;
  b.g_prep = std::max(b.g_prep, std::min(cdiv(std::max(std::max(M * 8u, k.n_supers_tris), 1u), 256), max_grid));
  b.g_expand = std::max(b.g_expand, std::max(std::min(cdiv(M, 4), max_grid), 1u));
  b.g_test = std::max(b.g_test, std::min(m_chunks, max_grid));
  b.g_emit = std::max(b.g_emit, std::min(cdiv(std::max(N, 1u), kMeshletSpan), max_grid));
  b.g_ttest = std::max(b.g_ttest, std::min(t_chunks, max_grid));
  b.g_temit = std::max(b.g_temit, std::min(cdiv(std::max(N, 1u), kTriSpan), max_grid));
}

// One launch hands over all element cores: a 4.5 KB kernarg segment.  A runtime that refuses a segment of that
// size fails the launch synchronously (false); nothing has been enqueued then and the elements are culled one by one.
bool launch_batch_prepare(const BatchCall& b) {
  static_assert(kBatchPerPrepare == kMaxBatch, "one prepare launch per batched call");
  BatchBlob blob;
  std::memset(&blob, 0, sizeof blob);
  blob.count = b.count;
  blob.first = 0;
  std::memcpy(blob.core, b.cores, sizeof(BatchCore) * b.count);
  KernelTimer t(b.ctx, OXC_K_PREPARE, b.s);
  launch_prepare_batch(blob, b.ctx->batch_dev, b.g_prep, b.s);
  return hipGetLastError() == hipSuccess;
}

// --- cull_meshes of every element: the scan, then the MeshletInstance expansion -- in order on `s`, or (multi-view, nothing of the call reads the
// records) on the context's lowest-priority side stream, forked from `s` here and joined at the end of the call (multiview_meshlet_stage)
oxc_status batch_meshes_stage(BatchCall& b) {
  oxc_ctx* ctx = b.ctx;
  {
    KernelTimer t(ctx, OXC_K_MESHES_SCAN, b.s);
    launch_scan_batch(ctx->batch_dev, b.count, b.s);
  }
  if (b.implicit_lists) return OXC_OK;  // (implicit: the records have no reader in this call; the runs are written by k_mv_group)
  // Round 5: in the multi-view form nothing of this call reads the MeshletInstance records (k_mv_test walks the instances' bounds), so their
  // expansion -- a pure store stream, 466 MB per 16 views of a 10 M-meshlet scene -- runs on the context's side stream beside the
  // latency-bound set-up launches and the VALU-bound test of the meshlet stage, and is joined at the end of the call (fork / join by
  // events, capturable like async_triangles).  A triangle stage in the call reads the records: in order then.
  const bool on_side = b.mv_expand_async = b.multiview && b.ci[0].do_meshlets && !b.ci[0].do_tris && ctx->mv_expand_async != 0;
  // (Round 6 measured the fork behind the meshlet stage's three set-up launches instead -- they are chains of dependent loads and take 78 us next to
  //  the store stream against 33 us alone -- : 0.2600 against 0.2615 ms per 16 views on one box, 0.2616 against 0.2568 on another; the test and the
  //  emit then share the machine with the whole store stream.  The fork stays here.)
  hipStream_t es = b.s;
  if (on_side) {
    if (!ctx->mv_side) {  // its own stream, at the lowest priority: the store stream yields wave slots to the meshlet stage's launches
      int lo = 0, hi = 0;
      OXC_HIP(ctx, hipDeviceGetStreamPriorityRange(&lo, &hi));
      OXC_HIP(ctx, hipStreamCreateWithPriority(&ctx->mv_side, hipStreamNonBlocking, lo));
    }
    if (!ctx->mv_fork) OXC_HIP(ctx, hipEventCreateWithFlags(&ctx->mv_fork, hipEventDisableTiming));
    if (!ctx->mv_join) OXC_HIP(ctx, hipEventCreateWithFlags(&ctx->mv_join, hipEventDisableTiming));
    OXC_HIP(ctx, hipEventRecord(ctx->mv_fork, b.s));
    OXC_HIP(ctx, hipStreamWaitEvent(ctx->mv_side, ctx->mv_fork, 0));
    es = ctx->mv_side;
  }
  {
    KernelTimer t(ctx, OXC_K_MESHES_EXPAND, es);
    // (beside the meshlet stage the expansion takes mv_expand_async blocks per CU, not every wave slot: the small set-up launches queue behind it otherwise)
    const uint32_t ecap = on_side ? std::max(1u, ctx->num_cus * ctx->mv_expand_async / b.count) : b.cap;
    launch_expand_batch(ctx->batch_dev, b.count, std::min(b.g_expand, ecap), es);
  }
  if (on_side) OXC_HIP(ctx, hipEventRecord(ctx->mv_join, es));
  return OXC_OK;
}

// The multi-view arena for `count` views of Mv mesh instances, view e with at most vchunks_max[e] chunks: view table | groups [M][views] |
// chunks per instance, their prefix [M] | totals | step list | per view: vchunks, vchunk0 [M], ballots [chunks][4], counts, idbase [chunks],
// supers, totals.  Every part once, in arena order; returns the arena's size and, with `base` (the allocation), binds `ma` and the views.
uint64_t lay_out_multiview(MvArgs& ma, MvView* views, uint32_t Mv, uint32_t count, const uint32_t* vchunks_max, void* base) {
  uint64_t steps_max = 0;
  for (uint32_t e = 0; e < count; e++) steps_max += vchunks_max[e];
  Carve carve{0, static_cast<char*>(base)};
  carve.take(ma.dev, sizeof(MvView) * kMaxBatch);
  carve.take(ma.groups, (uint64_t)Mv * count * sizeof(MvGroup));
  carve.take(ma.grp_chunks, (uint64_t)Mv * 4);
  carve.take(ma.inst_step0, (uint64_t)Mv * 4);
  carve.take(ma.step_total, 64);
  carve.take(ma.steps, steps_max * 8);
  for (uint32_t e = 0; e < count; e++) {
    MvView& w = views[e];
    carve.take(w.vchunks, (uint64_t)Mv * 4);
    carve.take(w.vchunk0, (uint64_t)Mv * 4);
    carve.take(w.bits, (uint64_t)vchunks_max[e] * 32);
    carve.take(w.counts, (uint64_t)vchunks_max[e] * 4);
    carve.take(w.idbase, (uint64_t)vchunks_max[e] * 4);
    carve.take(w.supers, (uint64_t)cdiv(vchunks_max[e], kChunksPerSuper) * 4 * kSuperStride);
    carve.take(w.scan_total, 64);
  }
  return carve.off;
}

// --- meshlet stage of the views of one scene: one pass over the scene for all views (plan_batch)
oxc_status multiview_meshlet_stage(const BatchCall& b) {
  oxc_ctx* ctx = b.ctx;
  const uint32_t count = b.count, Mv = b.ci[0].M;
  uint32_t vchunks_max[kMaxBatch];
  uint32_t max_vchunks = 0;
  for (uint32_t e = 0; e < count; e++) {
    vchunks_max[e] = cdiv(std::max(b.ci[e].N, 1u), 256u) + Mv;  // sum over instances of ceil(count / 256) <= N / 256 + M
    max_vchunks = std::max(max_vchunks, vchunks_max[e]);
  }
  MvArgs ma;
  std::memset(&ma, 0, sizeof ma);
  MvBlob blob;
  std::memset(&blob, 0, sizeof blob);
  const uint64_t bytes = lay_out_multiview(ma, blob.v, Mv, count, vchunks_max, nullptr);
  OXC_TRY(grow_scratch(ctx, b.s, ctx->mv_arena, ctx->mv_arena_bytes, bytes, bytes,
                       "cull_geometry_batch: the multi-view scratch must grow but the stream is being captured; make one un-captured call of this size first",
                       "hipMalloc(multi-view scratch)"));
  lay_out_multiview(ma, blob.v, Mv, count, vchunks_max, ctx->mv_arena);
  ma.views = count;
  ma.M = Mv;
  ma.same_pos = b.same_pos ? 1u : 0u;
  ma.tickets = ctx->lane[0].m_tickets;
  for (uint32_t e = 0; e < count; e++) {
    MvView& w = blob.v[e];
    oxc_ctx::Lane& L = ctx->lane[e];
    w.rows = L.cache;
    w.mesh_counts = L.mesh_counts;
    w.mesh_offsets = L.mesh_offsets;
    w.out = static_cast<uint32_t*>(b.frames[e].visible_meshlet_instances_indices_buffer.dptr);
    w.runs = static_cast<uint32_t*>(b.contexts[e].meshlet_instance_runs_buffer.dptr);
    w.tri_cmd = b.cores[e].slot + SLOT_TRI_CMD;
    w.n_cap = b.ci[e].N;
    w.n_supers = cdiv(vchunks_max[e], kChunksPerSuper);
    std::memcpy(w.cam_pos, b.contexts[e].cull_camera.position, 12);
  }
  {
    KernelTimer t(ctx, OXC_K_MULTIVIEW_SETUP, b.s);
    launch_mv_setup(ma, blob, std::max(1u, std::min(cdiv(Mv, 16u), b.max_grid)), b.s);  // 16 lanes per mesh instance
  }
  {
    KernelTimer t(ctx, OXC_K_MESHLETS_TEST, b.s);
    launch_mv_test(ma, ctx->num_cus, b.s);
  }
  {
    KernelTimer t(ctx, OXC_K_MESHLETS_EMIT, b.s);
    launch_mv_emit(ma, max_vchunks, b.max_grid, b.s);
  }
  if (b.mv_expand_async) OXC_HIP(ctx, hipStreamWaitEvent(b.s, ctx->mv_join, 0));  // join: the records are part of what the call leaves behind on `s`
  return OXC_OK;
}

// --- the stages that run per element over its own list, grid.y = element: the meshlet stage (unless the multi-view one ran) and the triangle stage
void plain_batch_stages(const BatchCall& b) {
  oxc_ctx* ctx = b.ctx;
  if (b.ci[0].do_meshlets && !b.multiview) {
    {
      KernelTimer t(ctx, OXC_K_MESHLETS_TEST, b.s);
      // At 64 VGPRs (8 waves/SIMD) the test kernel wants every block it can get: with 16 x 1M meshlets, blocks per element
      // 384 -> 74.6 us, 512 -> 73.7, 768 -> 73.2, 1024 -> 70.7, 2048 -> 70.0 (>= 977 blocks: one 1024-meshlet step per block)
      launch_meshlets_test_batch(ctx->batch_dev, b.count, b.g_test, b.s);
    }
    KernelTimer t(ctx, OXC_K_MESHLETS_EMIT, b.s);
    launch_meshlets_emit_batch(ctx->batch_dev, b.count, std::min(b.g_emit, b.cap), b.s);
  }
  if (b.ci[0].do_tris) {
    {
      KernelTimer t(ctx, OXC_K_TRIANGLES_TEST, b.s);
      launch_tris_test_batch(ctx->batch_dev, b.count, std::min(b.g_ttest, b.cap), b.s);
    }
    KernelTimer t(ctx, OXC_K_TRIANGLES_EMIT, b.s);
    launch_tris_emit_batch(ctx->batch_dev, b.count, std::min(b.g_temit, b.cap), b.s);
  }
}

}  // namespace

extern "C" {

oxc_status oxc_generate_hiz(oxc_ctx* ctx, const oxc_main_geometry_context* c, void* hip_stream) {
  if (!ctx) return OXC_INVALID_ARG;
  if (!c || c->struct_size != sizeof(oxc_main_geometry_context)) return fail(ctx, OXC_INVALID_ARG, "generate_hiz: bad context struct");
  const oxc_image& d = c->depth_attachment;
  const oxc_image& h = c->hiz_attachment;
  if (!d.dptr || !d.width || !d.height) return fail(ctx, OXC_INVALID_ARG, "generate_hiz: depth_attachment missing");
  if (!image_ok(h)) return fail(ctx, OXC_INVALID_ARG, "generate_hiz: hiz_attachment missing or levels not in 1..13");
  if (h.width > 4096 || h.height > 4096) return fail(ctx, OXC_INVALID_ARG, "generate_hiz: hiz extent > 4096 (13 mips) unsupported");
  HizArgs a;
  a.depth = reinterpret_cast<const float*>(static_cast<const char*>(d.dptr) + d.level_offset[0]);
  a.hiz = static_cast<float*>(h.dptr);
  a.dw = d.width;
  a.dh = d.height;
  a.w = h.width;
  a.h = h.height;
  a.levels = std::min(h.levels, 13u);  // CullGeometry.cpp:24
  for (uint32_t k = 0; k < 13; k++) {
    if (k < a.levels && (h.level_offset[k] & 3u)) return fail(ctx, OXC_INVALID_ARG, "generate_hiz: level offset not 4-byte aligned");
    a.level_off[k] = k < a.levels ? (uint32_t)(h.level_offset[k] / 4) : 0u;
  }
  const bool tiled = (a.w % 64 == 0) && (a.h % 64 == 0);
  if (!tiled && (uint64_t)a.w * a.h > 4096) return fail(ctx, OXC_INVALID_ARG, "generate_hiz: extent must be a multiple of 64 or <= 4096 texels");
  if (tiled && (h.level_offset[0] & 15u)) return fail(ctx, OXC_INVALID_ARG, "generate_hiz: mip 0 must be 16-byte aligned");
  if (tiled && a.levels > 1 && (h.level_offset[1] & 7u)) return fail(ctx, OXC_INVALID_ARG, "generate_hiz: mip 1 must be 8-byte aligned");  // (k_hiz_tile stores it as float2)
  OXC_ENTER(ctx, hip_stream, s);
  {
    KernelTimer t(ctx, OXC_K_HIZ, s);
    launch_hiz(a, ctx->num_cus, s);
  }
  OXC_HIP(ctx, hipGetLastError());
  return OXC_OK;
}

oxc_status oxc_seed_meshlet_instances(oxc_ctx* ctx, oxc_cull_geometry_context* c, uint32_t total, void* hip_stream) {
  if (!ctx) return OXC_INVALID_ARG;
  if (!c || c->struct_size != sizeof(oxc_cull_geometry_context)) return fail(ctx, OXC_INVALID_ARG, "seed: bad context struct");
  OXC_ENTER(ctx, hip_stream, s);
  uint32_t* slot = next_seed_slot(ctx);
  ctx->shared.valid = false;  // (share_pass_tests: a new list)
  ctx->seeded_total[(slot - ctx->slots) / SLOT_U32S] = total;
  launch_seed_slot(slot, total, s);
  OXC_HIP(ctx, hipGetLastError());
  c->visibility_buffer = {slot + SLOT_VIS, 12};
  c->cull_meshlets_cmd_buffer = {slot + SLOT_MESHLETS_CMD, 12};
  return OXC_OK;
}

oxc_status oxc_cull_geometry(oxc_ctx* ctx, const oxc_prepared_frame* f, oxc_cull_geometry_context* c, void* hip_stream) {
  if (!ctx) return OXC_INVALID_ARG;
  CullCall k = {};
  k.ctx = ctx;
  k.f = f;
  k.c = c;
  k.s = static_cast<hipStream_t>(hip_stream);
  OXC_TRY(check_call(ctx, f, c, k.ci));
  const uint32_t N = k.ci.N;
  if (c->implicit_meshlet_instances)
    return fail(ctx, OXC_INVALID_ARG, "cull_geometry: implicit_meshlet_instances is accepted by oxc_cull_geometry_batch's multi-view path only (this call's meshlet test reads the records)");
  OXC_HIP(ctx, hipSetDevice(ctx->device));
  OXC_TRY(ensure_capacity(ctx, k.ci.M, N, k.ci.views, 0, k.s));
  OXC_ORDER(ctx, hip_stream);
  ctx->last_share_mode = 0;
  ctx->last_tri_loads = 0;
  if (k.ci.do_meshes) ctx->shared.valid = false;  // (share_pass_tests: the MeshletInstance list is rebuilt; a flagged early call marks its results valid below)
  OXC_TRY(begin_triangle_bookkeeping(k));

  // the sequence's counters and the call's own slot
  uint32_t* slot = c->init_cull_meshes ? next_slot(ctx) : nullptr;  // (otherwise taken by plan_shared_tests: a late call may find its slot prepared)
  k.lists = resolve_lists(ctx, c, slot, N);
  k.mask_bits = (uint32_t)std::min<uint64_t>(f->meshlet_instance_visibility_mask_buffer.bytes / 4u * 32u, 0xFFFFFFFEull);
  k.unord_tris = c->unordered_output != 0u && k.ci.do_tris;
  k.unord_meshlets = k.ci.do_meshlets && !c->use_hpb && !c->use_hiz && c->unordered_output != 0u;  // (the plain meshlet test appends by itself)
  k.share = plan_shared_tests(k, slot);
  k.tri_cmd = k.share.slot + SLOT_TRI_CMD;
  k.draw_cmd = k.share.slot + SLOT_DRAW_CMD;
  name_cmd_buffers(c, k.share.slot);

  k.max_grid = ctx->num_cus * 8;
  k.m_chunks = cdiv(std::max(N, 1u), kMeshletChunk);
  k.t_chunks = cdiv(std::max(N, 1u), kTriChunk);
  k.n_supers_tris = cdiv(k.t_chunks, kChunksPerSuper);
  launch_prepare_and_meshes(k);
  if (k.ci.do_meshlets) OXC_TRY(c->use_hpb ? meshlet_stage_hpb(k) : meshlet_stage(k));
  if (k.ci.do_tris) OXC_TRY(triangle_stage(k));
  OXC_HIP(ctx, hipGetLastError());
  return OXC_OK;
}

oxc_status oxc_join_triangles(oxc_ctx* ctx, void* hip_stream) {
  if (!ctx) return OXC_INVALID_ARG;
  OXC_HIP(ctx, hipSetDevice(ctx->device));
  OXC_ORDER(ctx, hip_stream);  // an ordered call of the context like any other: what it joined stays joined for the calls that follow
  return join_triangles(ctx, static_cast<hipStream_t>(hip_stream));
}

oxc_status oxc_cull_geometry_batch(oxc_ctx* ctx, uint32_t count, const oxc_prepared_frame* frames, oxc_cull_geometry_context* contexts,
                                   void* hip_stream) {
  if (!ctx) return OXC_INVALID_ARG;
  if (count == 0) return OXC_OK;
  if (!frames || !contexts) return fail(ctx, OXC_INVALID_ARG, "cull_geometry_batch: null frames/contexts");
  BatchCall b = {ctx, frames, contexts, static_cast<hipStream_t>(hip_stream), count};
  OXC_TRY(plan_batch(b));
  if (!b.fusable) return cull_one_by_one(b);
  OXC_HIP(ctx, hipSetDevice(ctx->device));
  ctx->shared.valid = false;  // (share_pass_tests: a batch may rebuild any list)
  for (uint32_t e = 0; e < count; e++) OXC_TRY(ensure_capacity(ctx, b.ci[e].M, b.ci[e].N, 0, e, b.s));
  OXC_ORDER(ctx, hip_stream);
  OXC_JOIN(ctx, b.s);  // the batched call uses lane 0's scratch in order on hip_stream
  OXC_TRY(ensure_batch_block(ctx, b.s));
  b.max_grid = ctx->num_cus * 8;
  for (uint32_t e = 0; e < count; e++) fill_batch_core(b, e);
  // grid.y = count; grid.x cap per element for the small stages (the meshlet test kernel takes its full grid: plain_batch_stages)
  b.cap = std::max(b.max_grid / count, ctx->num_cus * 2);
  if (!launch_batch_prepare(b)) return cull_one_by_one(b);
  if (b.ci[0].do_meshes) OXC_TRY(batch_meshes_stage(b));
  if (b.ci[0].do_meshlets && b.multiview) OXC_TRY(multiview_meshlet_stage(b));
  plain_batch_stages(b);
  OXC_HIP(ctx, hipGetLastError());
  return OXC_OK;
}

oxc_status oxc_read_counters(oxc_ctx* ctx, const oxc_cull_geometry_context* c, oxc_counters* out, void* hip_stream) {
  if (!ctx) return OXC_INVALID_ARG;
  if (!c || !out) return fail(ctx, OXC_INVALID_ARG, "read_counters: null argument");
  OXC_ENTER(ctx, hip_stream, s);
  OXC_JOIN(ctx, s);
  uint32_t vis[3] = {0, 0, 0}, mc[3] = {0, 0, 0}, tc[3] = {0, 0, 0}, dc[5] = {0, 0, 0, 0, 0};
  if (c->visibility_buffer.dptr) OXC_HIP(ctx, hipMemcpyAsync(vis, c->visibility_buffer.dptr, 12, hipMemcpyDeviceToHost, s));
  if (c->cull_meshlets_cmd_buffer.dptr) OXC_HIP(ctx, hipMemcpyAsync(mc, c->cull_meshlets_cmd_buffer.dptr, 12, hipMemcpyDeviceToHost, s));
  if (c->cull_triangles_cmd_buffer.dptr) OXC_HIP(ctx, hipMemcpyAsync(tc, c->cull_triangles_cmd_buffer.dptr, 12, hipMemcpyDeviceToHost, s));
  if (c->draw_geometry_cmd_buffer.dptr) OXC_HIP(ctx, hipMemcpyAsync(dc, c->draw_geometry_cmd_buffer.dptr, 20, hipMemcpyDeviceToHost, s));
  OXC_HIP(ctx, hipStreamSynchronize(s));
  out->total_visible_meshlet_instances = vis[0];
  out->early_visible_meshlet_instances = vis[1];
  out->late_visible_meshlet_instances = vis[2];
  out->cull_meshlets_cmd_x = mc[0];
  out->cull_triangles_cmd_x = tc[0];
  out->draw_index_count = dc[0];
  // wide_triangle_index = 2 only: a call that emitted more indices than VkDrawIndexedIndirectCommand.indexCount can count zeroed instanceCount
  // (the command draws nothing); every other path leaves the 1 this library initialises it with
  if (c->draw_geometry_cmd_buffer.dptr && c->wide_triangle_index == 2u && (!c->stages || (c->stages & OXC_STAGE_TRIANGLES)) && dc[1] == 0u)
    return fail(ctx, OXC_INVALID_ARG, "read_counters: the call emitted more than 2^32 - 1 indices (pairs): draw_index_count wrapped, instanceCount was set to 0; cull fewer meshlets per call");
  return OXC_OK;
}

uint32_t oxc_debug_shared_tests_mode(const oxc_ctx* ctx) { return ctx ? ctx->last_share_mode : 0u; }
uint32_t oxc_debug_tri_loads_mode(const oxc_ctx* ctx) { return ctx ? ctx->last_tri_loads : 0u; }

oxc_status oxc_debug_count_occlusion_candidates(oxc_ctx* ctx, void* counters_dptr) {
  if (!ctx) return OXC_INVALID_ARG;
  ctx->dbg_occlusion = static_cast<uint32_t*>(counters_dptr);
  return OXC_OK;
}

oxc_status oxc_cull_terrain(oxc_ctx* ctx, oxc_terrain_context* c, void* hip_stream) {
  if (!ctx) return OXC_INVALID_ARG;
  if (!c || c->struct_size != sizeof(oxc_terrain_context)) return fail(ctx, OXC_INVALID_ARG, "cull_terrain: bad context / struct_size");
  const uint64_t total64 = (uint64_t)c->patch_count[0] * c->patch_count[1];
  if (c->patch_count[0] == 0 || c->patch_count[1] == 0 || total64 > (1u << 24)) return fail(ctx, OXC_INVALID_ARG, "cull_terrain: patch_count must be 1..2^24 patches");
  const uint32_t total = (uint32_t)total64;
  const oxc_image& mm = c->patch_minmax_attachment;
  if (!mm.dptr || mm.width != c->patch_count[0] || mm.height != c->patch_count[1]) return fail(ctx, OXC_INVALID_ARG, "cull_terrain: patch_minmax_attachment must be patch_count.x x patch_count.y RG32F");
  if (!c->visible_patches_buffer.dptr || c->visible_patches_buffer.bytes < (uint64_t)total * 4u) return fail(ctx, OXC_INVALID_ARG, "cull_terrain: visible_patches_buffer smaller than patch_total u32");
  if (!c->patch_visibility_mask_buffer.dptr || c->patch_visibility_mask_buffer.bytes < (uint64_t)cdiv(total, 32u) * 4u)
    return fail(ctx, OXC_INVALID_ARG, "cull_terrain: patch_visibility_mask_buffer smaller than ceil(patch_total / 32) words");
  const bool needs_hiz = (c->cull_flags & (OXC_CULL_TEST_OCCLUSION | OXC_CULL_LATE_PASS)) != 0u;
  const oxc_image& h = c->hiz_attachment;
  if (needs_hiz && (!h.dptr || h.levels == 0 || h.levels > 13 || h.width == 0 || h.height == 0)) return fail(ctx, OXC_INVALID_ARG, "cull_terrain: TestOcclusion / LatePass need hiz_attachment");
  OXC_HIP(ctx, hipSetDevice(ctx->device));
  const hipStream_t s = static_cast<hipStream_t>(hip_stream);
  // the two-kernel form borrows the meshlet stage's ballot / count scratch (one ballot per 64, one count per 1024 patches)
  // emit_bits is indexed [block * 16 + wave]: 16 ballots per STARTED block of 1024 patches, so the request is rounded up to whole blocks
  // (lane.bits holds ceil(n / 64) ballots for a request of n)
  if (total > 1024u) OXC_TRY(ensure_capacity(ctx, 0, cdiv(total, 1024u) * 1024u, 0, 0, s));
  OXC_ORDER(ctx, hip_stream);
  uint32_t* slot = next_slot(ctx);
  TerrainArgs a;
  std::memset(&a, 0, sizeof a);
  std::memcpy(a.pv, c->cull_camera.projection_view, 64);
  a.near_clip = c->cull_camera.near_clip;
  a.cull_flags = c->cull_flags;
  a.world_min[0] = c->world_min[0];
  a.world_min[1] = c->world_min[1];
  a.world_size[0] = c->world_size[0];
  a.world_size[1] = c->world_size[1];
  a.pcx = c->patch_count[0];
  a.pcy = c->patch_count[1];
  a.base_height = c->base_height;
  a.height_scale = c->height_scale;
  a.patch_minmax = reinterpret_cast<const float2*>(static_cast<const char*>(mm.dptr) + mm.level_offset[0]);
  if (needs_hiz) {
    a.hiz_data = static_cast<const float*>(h.dptr);
    a.hiz_w = h.width;
    a.hiz_h = h.height;
    a.hiz_levels = h.levels;
    for (uint32_t k = 0; k < h.levels; k++) a.hiz_level_off[k] = (uint32_t)(h.level_offset[k] / 4);
  }
  a.mask = static_cast<uint32_t*>(c->patch_visibility_mask_buffer.dptr);
  a.visible = static_cast<uint32_t*>(c->visible_patches_buffer.dptr);
  a.draw_cmd = slot + SLOT_DRAW_CMD;
  a.emit_bits = ctx->lane[0].bits;
  a.block_counts = ctx->lane[0].m_chunk_counts;
  c->cull_camera.mesh_instance_count = total;  // Terrain.cpp:171
  c->draw_cmd_buffer = {a.draw_cmd, 16};
  launch_cull_terrain(a, s);
  OXC_HIP(ctx, hipGetLastError());
  return OXC_OK;
}

}  // extern "C"
