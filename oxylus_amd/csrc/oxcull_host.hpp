// oxcull_host.hpp -- what the host translation units of liboxcull.so (oxcull_abi*.cpp) share: the context, error and stream-ordering
// helpers, and the argument rules more than one pass applies.  Private to them; not installed.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "oxcull.h"
#include "oxcull_debug.h"
#include "oxcull_kernels.hpp"
#include "oxcull_types.hpp"

using namespace oxc;

#pragma GCC visibility push(hidden)  // nothing in here is part of the library's ABI

constexpr uint32_t kSlots = 8192;  // counter-slot ring (1 MiB): a slot is reused kSlots / 2 calls (or seeds) later -- include/oxcull.h states that lifetime

inline uint32_t cdiv(uint32_t a, uint32_t b) { return (a + b - 1) / b; }
// (Sizing persistent grids to the exact SGPR-limited residency and balancing chunks per block was tried:
// no gain for the plain kernel, 183 -> 219 us for the HiZ variant; oversubscribed grids schedule better.)
inline uint64_t align_up(uint64_t v, uint64_t a) { return (v + a - 1) / a * a; }

// Lays out one scratch allocation: each call returns the offset of the next part, 256-byte aligned; `off` ends as the size of the whole.
// take() states a part once for both uses of a layout: a layout function walked without `base` gives the size, and walked again with the
// allocation as `base` it binds every field to its part.
struct Carve {
  uint64_t off = 0;
  char* base = nullptr;
  uint64_t operator()(uint64_t bytes) {
    const uint64_t o = off;
    off = align_up(off + bytes, 256);
    return o;
  }
  template <class T>
  void take(T*& field, uint64_t bytes) {
    const uint64_t o = (*this)(bytes);
    if (base) field = reinterpret_cast<T*>(base + o);
  }
};

#pragma GCC visibility pop
struct oxc_ctx {
  int device = 0;
  uint32_t num_cus = 256;
  std::string last_error;
  // scratch: one lane per batch element (lane 0 serves the single-frame entry points)
  struct Lane {
    void* arena = nullptr;
    uint64_t arena_bytes = 0;
    uint32_t cap_mesh_instances = 0, cap_meshlets = 0;
    InstCache* cache = nullptr;
    InstCache* cache_alt = nullptr;   // second set of rows: calls alternate, so that a triangle stage still in flight on the side stream keeps the rows of ITS call
    InstCache* view_cache = nullptr;  // [views][M] rows for use_hpb
    uint32_t cap_views = 0;
    uint32_t* mesh_counts = nullptr;
    uint32_t* mesh_offsets = nullptr;
    uint64_t* bits = nullptr;
    uint32_t* m_chunk_counts = nullptr;
    uint32_t* m_supers = nullptr;
    uint32_t* m_tickets = nullptr;
    uint32_t* m_supers_late = nullptr;   // share_pass_tests: the accumulators of the late call, zeroed by the early call's prepare kernel
    uint32_t* m_tickets_late = nullptr;
    uint64_t* camera_test_bits = nullptr;  // share_pass_tests: the early call's "passed frustum and cone" ballots ...
    uint2* step_info = nullptr;        // ... and each wave step's run of mask bits, for the late call of the same frame
    uint64_t* tri_masks = nullptr;
    uint32_t* t_chunk_counts = nullptr;
    uint32_t* t_supers = nullptr;
    uint32_t* t_supers_alt = nullptr;  // alternates with t_supers like the cache rows (prepare zeroes the next call's accumulators on the caller's stream)
  };
  Lane lane[kMaxBatch];
  BatchElem* batch_dev = nullptr;  // device copy of the argument blocks of the current batched call (kMaxBatch elements)
  void* mv_arena = nullptr;        // multi-view meshlet stage (batched views of one scene): view table, groups, step list, per-view chunk arrays
  uint64_t mv_arena_bytes = 0;
  // oxc_build_meshlet_bounds: per-meshlet {min xyz, max xyz} for all meshlets, then per chunk of kBoundsChunk
  // meshlets the compacted triangle normals (768 B each) and their counts
  float* bounds_scratch = nullptr;
  uint32_t bounds_scratch_cap = 0;
  uint32_t bounds_grid = 0;   // OXC_TUNE_BOUNDS_GRID: cap of every grid-stride launch of the bounds producer and the stream quantiser in blocks, 0 = uncapped
  uint32_t bounds_chunk = 0;  // OXC_TUNE_BOUNDS_CHUNK: meshlets per gather/cone launch pair, 0 = kBoundsChunk; the scratch layout does not follow it
  void* raster_scratch = nullptr;  // oxc_draw_visbuffer: list of large triangles + its counter
  uint32_t raster_capacity = 0;    // entries of the big / clip lists (the tile list has twice as many)
  uint32_t raster_capacity_request = 0;  // oxc_debug_set_tuning(OXC_TUNE_RASTER_BIG_CAPACITY): used by the first draw instead of the default
  uint32_t raster_grid = 0;              // OXC_TUNE_RASTER_GRID: cap of every launch of the draw in blocks, 0 = uncapped
  uint32_t terrain_draw_grid = 0;        // OXC_TUNE_TERRAIN_DRAW_GRID: the same for oxc_draw_terrain
  bool terrain_draw_stats = false;       // OXC_TUNE_TERRAIN_DRAW_STATS: counting kernels (the fragment counter)
  void* raster_rows = nullptr;     // oxc_draw_visbuffer: one DrawRow per mesh instance
  uint32_t raster_rows_cap = 0;
  void* sprite_scratch = nullptr;  // oxc_draw_sprites: records, boxes, the clipped sprites' side array, bin counts and bin lists
  uint64_t sprite_scratch_bytes = 0;
  void* vsm_scratch = nullptr;     // oxc_update_virtual_shadowmap: free page list (u32 per physical page), then the per-page mark map (a byte per entry)
  uint64_t vsm_scratch_bytes = 0;
  void* vsm_draw_scratch = nullptr;  // oxc_draw_physical_pages: header, drawable-page bitmaps and maps, rows, big-pair / clip / tile queues
  uint64_t vsm_draw_scratch_bytes = 0;
  uint32_t vsm_draw_capacity = 0;          // entries of the big-pair and clip queues of that scratch (the tile queue holds 4x as many)
  uint32_t vsm_draw_capacity_request = 0;  // oxc_debug_set_tuning(OXC_TUNE_VSM_DRAW_CAPACITY): used by the first shadow draw
  uint32_t vsm_draw_grid = 0;              // OXC_TUNE_VSM_DRAW_GRID: cap of every launch of the shadow draw in blocks, 0 = uncapped
  bool vsm_draw_stats = false;             // oxc_debug_set_tuning(OXC_TUNE_VSM_DRAW_STATS): counting kernels
  // The counters a pass's counting instantiation adds to: switched by oxc_debug_set_tuning, allocated by the first counting call
  // (arm_counters), read by the pass's oxc_debug_*_stats (read_counters).
  struct PassCounters {
    uint32_t* dev = nullptr;
    bool on = false;
  };
  PassCounters vsm_resolve_stats;        // OXC_TUNE_VSM_RESOLVE_STATS: u32[8]
  PassCounters contact_shadows_stats;    // OXC_TUNE_CONTACT_SHADOWS_STATS: u32[12]
  PassCounters ambient_occlusion_stats;  // OXC_TUNE_AMBIENT_OCCLUSION_STATS: u32[15] (16 allocated)
  PassCounters visbuffer_decode_stats;   // OXC_TUNE_VISBUFFER_DECODE_STATS: u32[4]
  PassCounters visbuffer_decode_textured_stats;  // OXC_TUNE_VISBUFFER_DECODE_TEXTURED_STATS: u32[13] (16 allocated)
  PassCounters pbr_apply_stats;          // OXC_TUNE_PBR_APPLY_STATS: u32[9]
  PassCounters fxaa_stats;               // OXC_TUNE_FXAA_STATS: u32[4]
  uint32_t eye_adaptation_grid = 0;      // OXC_TUNE_EYE_ADAPTATION_GRID: cap of the histogram kernel's grid in blocks, 0 = uncapped
  uint32_t bloom_tail_level = 0;         // OXC_TUNE_BLOOM_TAIL_LEVEL: the first level of oxc_apply_bloom's tail kernel, 0 = the library's choice
  void* comm = nullptr;           // ncclComm_t (oxc_comm_init)
  uint32_t comm_rank = 0, comm_world = 0;
  // counter slots
  uint32_t* slots = nullptr;
  uint32_t slot_cursor = 0;
  uint32_t seed_cursor = 0;
  uint32_t* sink = nullptr;
  std::vector<uint32_t> seeded_total = std::vector<uint32_t>(kSlots, 0u);  // per counter slot: list length given to oxc_seed_meshlet_instances (0: unknown)
  // The context owns ONE set of scratch buffers, so its calls are ordered: a call on another stream than the previous
  // call's first waits for that call on the device (order_stream).
  hipStream_t last_stream = nullptr;
  bool has_last_stream = false;
  hipEvent_t order_event = nullptr;
  // async_triangles: the triangle stage of a call runs on `side`, forked from the caller's stream after the meshlet emit.
  // tri[k % kTriRing] describes the stage of lane-0 call number k (call_seq) while it may still be in flight.
  hipStream_t side = nullptr;
  hipEvent_t fork_event = nullptr;
  hipStream_t mv_side = nullptr;
  hipEvent_t mv_fork = nullptr, mv_join = nullptr;  // multi-view batch: the MeshletInstance expansion on `side` beside the meshlet stage
  uint32_t tri_loads = 0;                            // OXC_TUNE_TRI_LOADS: 0 = by the scene (shared geometry -> plain loads), 1 = always `nt`, 2 = always plain
  uint32_t mv_expand_async = 4;                      // blocks per CU the side-stream expansion takes; oxc_debug_set_tuning(OXC_TUNE_MV_EXPAND_ASYNC, 0): in order on the caller's stream (A/B aid)
  struct TriPending {
    hipEvent_t done = nullptr;
    bool valid = false;
    bool late = false;
    const uint32_t* vis = nullptr;  // the sequence's visibility counters (the late list starts at vis[1])
    const void* visible = nullptr;  // visible_meshlet_instances_indices_buffer it reads
    unsigned long long capture_id = 0;  // the HIP-graph capture `done` was recorded in (0: none).  An event recorded outside a capture cannot be
                                        // waited for inside one and the reverse (hipErrorStreamCaptureIsolation): wait_triangles only waits within
                                        // the same capture
  };
  static constexpr uint32_t kTriRing = 4;
  TriPending tri[kTriRing];
  // share_pass_tests: what the last flagged early HiZ call tested, i.e. what lane[0].camera_test_bits / step_info describe
  struct SharedTests {
    bool valid = false;
    uint32_t N = 0, n_host = 0, M = 0, flags = 0, mask_bits = 0;
    const void *meshlet_instances = nullptr, *mask = nullptr, *meshes = nullptr, *transforms = nullptr, *mesh_instances = nullptr, *vis = nullptr;
    oxc_cull_camera camera = {};
    // the early call also did the late call's prepare work (PrepareArgs::slot_late): valid for lane-0 call number `armed_for_call` only
    uint64_t armed_for_call = ~0ull;
    unsigned long long capture_id = 0;  // the capture the arming early call was part of (0: none): an armed late call must be part of the same
                                        // one -- replayed alone, nobody would zero its accumulators again
    uint32_t* late_slot = nullptr;
    uint32_t* late_t_supers = nullptr;
    InstCache* rows = nullptr;
    bool same_inputs(const SharedTests& o) const {
      return N == o.N && n_host == o.n_host && M == o.M && flags == o.flags && mask_bits == o.mask_bits && meshlet_instances == o.meshlet_instances && mask == o.mask && meshes == o.meshes &&
             transforms == o.transforms && mesh_instances == o.mesh_instances && vis == o.vis && std::memcmp(&camera, &o.camera, sizeof camera) == 0;
    }
  };
  SharedTests shared;
  uint32_t last_share_mode = 0;  // oxc_debug_shared_tests_mode
  uint32_t last_tri_loads = 0;   // oxc_debug_tri_loads_mode: 0 = the last call ran no triangle stage, 1 = nt loads, 2 = plain loads
  uint64_t call_seq = 0;  // lane-0 oxc_cull_geometry calls so far: parity selects cache / t_supers
  // resident blocks per CU of the persistent kernels while the two stages share the machine (0 = no limit); oxc_debug_set_tuning
  // overrides the defaults (tuning aid of tools/kbench.py)
  uint32_t async_mtest_per_cu = kAsyncMeshletBlocksPerCU, async_tri_per_cu = kAsyncTriangleBlocksPerCU;
  uint32_t tri_blocks_per_cu = kTriangleBlocksPerCU;  // grid cap of the triangle kernels (blocks walk their chunks with a grid stride)
  uint32_t* dbg_occlusion = nullptr;  // oxc_debug_count_occlusion_candidates: 256 strided counters the counting instantiations of the HiZ meshlet tests add to
  // profiling (oxc_profile_begin/end)
  bool profiling = false;
  struct Rec {
    int id;
    hipEvent_t a, b;
  };
  std::vector<Rec> recs;
};
#pragma GCC visibility push(hidden)

inline oxc_status fail(oxc_ctx* ctx, oxc_status st, const char* what, hipError_t e = hipSuccess) {
  if (ctx) {
    ctx->last_error = what;
    if (e != hipSuccess) {
      ctx->last_error += ": ";
      ctx->last_error += hipGetErrorString(e);
    }
  }
  return st;
}

#define OXC_ORDER(ctx, stream)                                            \
  do {                                                                    \
    oxc_status _o = order_stream(ctx, static_cast<hipStream_t>(stream)); \
    if (_o != OXC_OK) return _o;                                          \
  } while (0)

#define OXC_HIP(ctx, expr)                                        \
  do {                                                            \
    hipError_t _e = (expr);                                       \
    if (_e != hipSuccess) return fail(ctx, OXC_HIP_ERROR, #expr, _e); \
  } while (0)

#define OXC_TRY(expr)                 \
  do {                                \
    oxc_status _t = (expr);           \
    if (_t != OXC_OK) return _t;      \
  } while (0)

// How an ordered entry point begins its device work, once its arguments are checked: on the context's device, behind the context's
// previous call (order_stream), with `s` naming the caller's stream.
#define OXC_ENTER(ctx, hip_stream, s)         \
  OXC_HIP(ctx, hipSetDevice(ctx->device));    \
  OXC_ORDER(ctx, hip_stream);                 \
  const hipStream_t s = static_cast<hipStream_t>(hip_stream)

// 0 when `s` is not being captured, else the id of the capture it belongs to
inline unsigned long long stream_capture_id(hipStream_t s) {
  hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
  unsigned long long id = 0;
  if (hipStreamGetCaptureInfo(s, &st, &id) != hipSuccess) {
    (void)hipGetLastError();
    return 0;
  }
  return st == hipStreamCaptureStatusNone ? 0ull : (id ? id : ~0ull);
}

inline bool stream_is_capturing(hipStream_t s) {
  hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(s, &st) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  return st != hipStreamCaptureStatusNone;
}

// Device-side ordering of a context's calls across streams (see oxc_ctx::last_stream).  Not across a capture boundary: an event
// recorded outside a capture cannot be waited for inside it (and the reverse), so when `s` is being captured the wait for a
// previous call on ANOTHER stream is skipped -- include/oxcull.h asks the caller to have that stream's work complete (or inside the
// same capture through the caller's own events) before the capture begins.
inline oxc_status order_stream(oxc_ctx* ctx, hipStream_t s) {
  // (a previous stream that is itself being captured: recording on it would add a node to THAT capture and the wait below would pull `s`
  // into it -- the two are not ordered here either; same promise of the caller as above)
  if (ctx->has_last_stream && ctx->last_stream != s && !stream_is_capturing(s) && !stream_is_capturing(ctx->last_stream)) {
    if (!ctx->order_event) OXC_HIP(ctx, hipEventCreateWithFlags(&ctx->order_event, hipEventDisableTiming));
    // (the previous stream may have been destroyed by its owner since -- its work is complete then, nothing to wait for: the record
    // fails, and the error is dropped)
    if (hipEventRecord(ctx->order_event, ctx->last_stream) == hipSuccess)
      OXC_HIP(ctx, hipStreamWaitEvent(s, ctx->order_event, 0));
    else
      (void)hipGetLastError();
  }
  ctx->last_stream = s;
  ctx->has_last_stream = true;
  return OXC_OK;
}

// The scratch the draws into the depth|vis image share (oxcull_abi_raster.cpp): allocated by the first of them, never inside a capture
// (`capture_msg`); bind_raster_scratch points the kernels' argument struct at its parts.
oxc_status ensure_raster_scratch(oxc_ctx* ctx, hipStream_t s, const char* capture_msg);
void bind_raster_scratch(const oxc_ctx* ctx, DrawArgs& a);

// Grows the lane's scratch arena when the call needs more than it holds (oxcull_abi_cull.cpp; oxc_reserve calls it too)
oxc_status ensure_capacity(oxc_ctx* ctx, uint32_t mesh_instances, uint32_t meshlets, uint32_t views = 0, uint32_t lane_index = 0, hipStream_t s = nullptr);

// ---- async_triangles: what is in flight on the context's own stream ----
// Makes `s` wait for every pending triangle stage for which `needed` says so.
// Only within one capture (or outside any): a stage recorded outside a capture cannot be waited for inside it -- include/oxcull.h asks the
// caller to have joined before the capture begins -- and a stage recorded INSIDE a capture that has ended is ordered by the graph itself at
// every replay (the capture could not end before oxc_join_triangles), so from un-captured calls it is simply forgotten.
// retire: the caller is an ordered call of the context on `s` (OXC_ORDER ran): everything the context does later is behind this wait, so
// the entry need not be waited for again.
template <class Pred>
oxc_status wait_triangles(oxc_ctx* ctx, hipStream_t s, Pred needed, bool retire = false) {
  const unsigned long long cid = stream_capture_id(s);
  for (auto& tp : ctx->tri) {
    if (!tp.valid) continue;
    if (tp.capture_id != cid) {
      // An entry of another capture is forgotten by an un-captured call only once that capture has ENDED (the graph orders the stage at
      // every replay).  While it is still open -- the side stream joined it through the fork event and stays in capture mode until the
      // stage is joined -- the entry must survive an un-captured call made in between: the oxc_join_triangles inside the capture still
      // has to find it (round-4 advisor finding).
      if (cid == 0 && !(ctx->side && stream_capture_id(ctx->side) == tp.capture_id)) tp.valid = false;
      continue;
    }
    if (!needed(tp)) continue;
    OXC_HIP(ctx, hipStreamWaitEvent(s, tp.done, 0));
    if (retire) tp.valid = false;
  }
  return OXC_OK;
}
inline oxc_status join_triangles(oxc_ctx* ctx, hipStream_t s) {
  return wait_triangles(ctx, s, [](const oxc_ctx::TriPending&) { return true; }, true);
}
#define OXC_JOIN(ctx, stream) OXC_TRY(join_triangles(ctx, static_cast<hipStream_t>(stream)))

// Brackets one kernel launch with events while profiling is on.
struct KernelTimer {
  oxc_ctx* ctx;
  hipStream_t s;
  oxc_ctx::Rec r;
  bool on;
  KernelTimer(oxc_ctx* c, int id, hipStream_t st) : ctx(c), s(st), on(c->profiling) {
    if (!on) return;
    r.id = id;
    if (hipEventCreate(&r.a) != hipSuccess || hipEventCreate(&r.b) != hipSuccess) {
      on = false;
      return;
    }
    (void)hipEventRecord(r.a, s);
  }
  ~KernelTimer() {
    if (!on) return;
    (void)hipEventRecord(r.b, s);
    ctx->recs.push_back(r);
  }
};

inline bool image_ok(const oxc_image& im) { return im.dptr && im.width && im.height && im.levels >= 1 && im.levels <= 13; }

// ---- the rules the VSM entry points (page update, shadow draw, shadow resolve) and the per-pixel passes (shadow resolve, contact
// shadows, ambient occlusion) share.  `entry` is the entry point's name as oxc_last_error prefixes it.

// OXC_INVALID_ARG with the message "<entry>: <what><more><rest>"
inline oxc_status bad_arg(oxc_ctx* ctx, const char* entry, const char* what, const char* more = "", const char* rest = "") {
  std::string m;
  for (const char* part : {entry, ": ", what, more, rest}) m += part;
  return fail(ctx, OXC_INVALID_ARG, m.c_str());
}

struct VsmShape {
  int32_t n, ps, phys, layers;  // page_table_size, page_size, physical_page_table_size, clipmap_count
  uint32_t P, phys_count;       // physical pages per side, in all
  uint64_t entries;             // page-table entries of all clipmaps
};

// The shape rule, from the four fields every VSM context carries under the same names.
template <class Context>
oxc_status vsm_shape(oxc_ctx* ctx, const char* entry, const Context& c, VsmShape& sh) {
  const int32_t n = c.page_table_size, ps = c.page_size, phys = c.physical_page_table_size, layers = c.clipmap_count;
  if (layers < 1 || layers > 16) return bad_arg(ctx, entry, "clipmap_count must be 1..16");
  if (n < 8 || n > 256 || n % 8) return bad_arg(ctx, entry, "page_table_size must be a multiple of 8 in [8, 256]");
  if (ps < 16 || ps % 16 || phys < ps || phys % ps) return bad_arg(ctx, entry, "page_size must be a multiple of 16 and divide physical_page_table_size");
  const uint32_t P = (uint32_t)(phys / ps);
  if ((uint64_t)P * P > 65536u) return bad_arg(ctx, entry, "more than 65536 physical pages (16 address bits)");
  sh = {n, ps, phys, layers, P, P * P, (uint64_t)layers * n * n};
  return OXC_OK;
}

// virtual_page_table and vsm_clipmaps_buffer hold the shape's entries and records
template <class Context>
oxc_status vsm_tables(oxc_ctx* ctx, const char* entry, const Context& c, const VsmShape& sh) {
  if (!c.virtual_page_table.dptr || c.virtual_page_table.bytes < sh.entries * 4u) return bad_arg(ctx, entry, "virtual_page_table smaller than clipmap_count * n * n u32");
  if (!c.vsm_clipmaps_buffer.dptr || c.vsm_clipmaps_buffer.bytes < (uint64_t)sh.layers * sizeof(oxc_virtual_clipmap))
    return bad_arg(ctx, entry, "vsm_clipmaps_buffer smaller than clipmap_count records");
  return OXC_OK;
}

inline oxc_status vsm_dirty_flags(oxc_ctx* ctx, const char* entry, const oxc_buffer& flags, const VsmShape& sh) {
  if (!flags.dptr || flags.bytes < (uint64_t)sh.layers * 4u) return bad_arg(ctx, entry, "vsm_clipmap_dirty_flags_buffer smaller than clipmap_count u32");
  return OXC_OK;
}

// The clipmap index without log2 (include/oxcull.h, mark visible pages): k < *always has (double)k - (double)bias < 0 and always counts;
// k >= *always counts when r > thr[k], the largest binary32 <= exp2(k - bias) -- (double)r > T <=> r > that value, r being a binary32.
inline void vsm_level_thresholds(int layers, float bias, uint32_t* always, float* thr) {
  *always = 0;
  for (int k = 0; k + 1 < layers; k++) {
    const double dk = (double)k - (double)bias;
    if (dk < 0.0) {
      *always = (uint32_t)(k + 1);
      thr[k] = 0.0f;
      continue;
    }
    const double T = std::exp2(dk);
    float f = (float)T;
    if ((double)f > T) f = std::nextafter(f, -INFINITY);
    thr[k] = f;
  }
}

// The per-call constants by which a pixel selects its clipmap, binary32 in the Slang's order (include/oxcull.h).  One function for the
// page update's VsmArgs and the resolve's VsmResolveArgs: the two kernels must select the same clipmap for the same pixel.
template <class Args, class Context>
void clipmap_selection_constants(Args& a, const Context& c, const VsmShape& sh) {
  a.off_x = (1.0f / c.resolution[0]) * 0.5f;
  a.off_y = (1.0f / c.resolution[1]) * 0.5f;
  const float scale_ratio = (float)(sh.n - 1) / (float)sh.n;  // get_first_clipmap_texel_length, rmvsm.slang:148-155
  const float effective_width = c.first_clipmap_width * scale_ratio;
  a.texel_len = (effective_width * 2.0f) / c.virtual_extent;
  vsm_level_thresholds(sh.layers, c.clipmap_selection_bias, &a.lvl_always, a.lvl_thr);
}

// The image contract of a per-pixel pass: an extent of at most 65536, the depth one R32F level at offset 0 and, where the pass writes an
// R32F image (`out`, the field `out_name`), that image of the depth's extent.  An empty image is valid: the pass is a no-op then.
inline oxc_status pixel_images(oxc_ctx* ctx, const char* entry, const oxc_image& depth, const oxc_image* out, const char* out_name, uint64_t& pixels) {
  pixels = (uint64_t)depth.width * depth.height;
  if (depth.width > 65536u || depth.height > 65536u) return bad_arg(ctx, entry, "depth extent beyond 65536");
  if (pixels && (!depth.dptr || depth.levels != 1 || depth.level_offset[0] != 0)) return bad_arg(ctx, entry, "depth_attachment must be one R32F level at offset 0");
  if (out && (out->width != depth.width || out->height != depth.height || (pixels && (!out->dptr || out->levels != 1 || out->level_offset[0] != 0))))
    return bad_arg(ctx, entry, out_name, " must be one R32F level of the depth attachment's extent");
  return OXC_OK;
}

// not a buffer of one `texel`-byte texel per pixel, aligned to its texel
inline bool bad_pixel_buffer(const oxc_buffer& b, uint64_t pixels, uint64_t texel) {
  return pixels && (!b.dptr || b.bytes < pixels * texel || (reinterpret_cast<uintptr_t>(b.dptr) & (texel - 1u)));
}

struct ByteSpan {
  uintptr_t lo, hi;  // [lo, hi)
  bool overlaps(const ByteSpan& o) const { return lo < o.hi && o.lo < hi; }
};

// ---- the checks the sky passes (oxc_generate_sky_luts, oxc_draw_atmosphere, oxc_generate_sky_ibl) and oxc_apply_pbr_atmosphere share, each
// applied in the order of its header block's limits
struct SkyBuffer {
  const oxc_buffer& b;
  uint64_t bytes;
  const char* name;
  bool output;
};
inline bool bad_lut_side(const uint32_t* size) { return size[0] < 2u || size[0] > 4096u || size[1] < 2u || size[1] > 4096u; }
inline uint64_t lut_bytes(const uint32_t* size) { return (uint64_t)size[0] * size[1] * 8u; }
// every side of the aerial LUT in 1 .. 4096 and at most 2^26 texels
inline oxc_status check_aerial_size(oxc_ctx* ctx, const char* entry, const uint32_t* ap, uint64_t& texels) {
  if (ap[0] < 1u || ap[0] > 4096u || ap[1] < 1u || ap[1] > 4096u || ap[2] < 1u || ap[2] > 4096u)
    return bad_arg(ctx, entry, "aerial_perspective_lut_size: every side must be in 1 .. 4096");
  texels = (uint64_t)ap[0] * ap[1] * ap[2];
  if (texels > (1ull << 26)) return bad_arg(ctx, entry, "aerial_perspective_lut_size: more than 2^26 texels");
  return OXC_OK;
}
inline oxc_status check_radii(oxc_ctx* ctx, const char* entry, const oxc_atmosphere& A) {
  if (!std::isfinite(A.planet_radius) || !std::isfinite(A.atmos_radius)) return bad_arg(ctx, entry, "planet_radius and atmos_radius must be finite");
  if (!(A.planet_radius > 0.0f)) return bad_arg(ctx, entry, "planet_radius must be above 0");
  if (!(A.atmos_radius > A.planet_radius)) return bad_arg(ctx, entry, "atmos_radius must be above planet_radius");
  return OXC_OK;
}
// every buffer, in the order given: non-null, then aligned to 8 bytes, then large enough; then no output shares a byte with another buffer
inline oxc_status check_sky_buffers(oxc_ctx* ctx, const char* entry, std::initializer_list<SkyBuffer> buffers) {
  for (const SkyBuffer& s : buffers) {
    if (!s.b.dptr) return bad_arg(ctx, entry, s.name, " must not be null");
    if (reinterpret_cast<uintptr_t>(s.b.dptr) & 7u) return bad_arg(ctx, entry, s.name, " must be aligned to 8 bytes");
    if (s.b.bytes < s.bytes) return bad_arg(ctx, entry, s.name, " is smaller than its extent");
  }
  for (const SkyBuffer& s : buffers) {
    if (!s.output) continue;
    const uintptr_t lo = reinterpret_cast<uintptr_t>(s.b.dptr);
    for (const SkyBuffer& o : buffers) {
      const uintptr_t olo = reinterpret_cast<uintptr_t>(o.b.dptr);
      if (&o != &s && ByteSpan{lo, lo + (uintptr_t)s.bytes}.overlaps({olo, olo + (uintptr_t)o.bytes})) return bad_arg(ctx, entry, s.name, " must not overlap ", o.name);
    }
  }
  return OXC_OK;
}

// ---- the buffer table of the terrain calls and the debug views.  One buffer of the call, as the limits see it: which stages (or views)
// touch it, which write it, its texel (= alignment) and the bytes its extent asks
struct MapBuffer {
  const char* name;
  const void* dptr;
  uint64_t have, need;
  uint32_t align, touched_by, written_by;
  bool may_be_null;
  const char* too_small = " is smaller than its extent";
};

// The buffer limits those calls share, over the buffers `stages` touches: in the table's order non-null, aligned, large enough; then no
// written buffer sharing a byte with another touched one.  The message of the first broken rule, or OXC_OK.
template <size_t N>
inline oxc_status check_buffers(oxc_ctx* ctx, const char* entry, const MapBuffer (&buffers)[N], uint32_t stages) {
  for (const MapBuffer& b : buffers) {
    if (!(b.touched_by & stages)) continue;
    if (!b.dptr) {
      if (b.may_be_null) continue;
      return bad_arg(ctx, entry, b.name, " must not be null");
    }
    if (reinterpret_cast<uintptr_t>(b.dptr) & (b.align - 1u)) return bad_arg(ctx, entry, b.name, " must be aligned to its texel");
    if (b.have < b.need) return bad_arg(ctx, entry, b.name, b.too_small);
  }
  for (const MapBuffer& w : buffers) {
    if (!(w.written_by & stages)) continue;
    const uintptr_t lo = reinterpret_cast<uintptr_t>(w.dptr);
    for (const MapBuffer& o : buffers) {
      if (&o == &w || !(o.touched_by & stages) || !o.dptr) continue;
      const uintptr_t olo = reinterpret_cast<uintptr_t>(o.dptr);
      if (ByteSpan{lo, lo + (uintptr_t)w.need}.overlaps({olo, olo + (uintptr_t)o.need})) return bad_arg(ctx, entry, w.name, " must not overlap ", o.name);
    }
  }
  return OXC_OK;
}

// The counting instantiation's counters for this call, zeroed on `s`: `bytes` of them, allocated by the first counting call (never inside
// a capture).  nullptr while the pass is not counting.
inline oxc_status arm_counters(oxc_ctx* ctx, const char* entry, const char* malloc_label, oxc_ctx::PassCounters& pc, size_t bytes, hipStream_t s, uint32_t** out) {
  if (!pc.on) return OXC_OK;
  if (!pc.dev) {
    if (stream_is_capturing(s)) return bad_arg(ctx, entry, "the counters are allocated by the first counting call; make one outside the capture");
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&pc.dev), bytes);
    if (e != hipSuccess) return fail(ctx, OXC_OUT_OF_MEMORY, malloc_label, e);
  }
  OXC_HIP(ctx, hipMemsetAsync(pc.dev, 0, bytes, s));
  *out = pc.dev;
  return OXC_OK;
}

// oxc_debug_<pass>_stats: `bytes` of the counters of the last counting call of `pass` to the host; synchronises
inline oxc_status read_counters(oxc_ctx* ctx, const char* entry, const char* pass, oxc_ctx::PassCounters oxc_ctx::*which, uint32_t* host_out, size_t bytes, void* hip_stream) {
  if (!ctx) return OXC_INVALID_ARG;
  if (!host_out) return bad_arg(ctx, entry, "null pointer");
  const uint32_t* dev = (ctx->*which).dev;
  if (!dev) return bad_arg(ctx, entry, "no counting ", pass, " call on this context yet");
  OXC_ENTER(ctx, hip_stream, s);
  OXC_HIP(ctx, hipMemcpyAsync(host_out, dev, bytes, hipMemcpyDeviceToHost, s));
  OXC_HIP(ctx, hipStreamSynchronize(s));
  return OXC_OK;
}

// Grows one scratch buffer of the context to `bytes` when the call wants more (`want`, in the unit `have` is kept in) than it holds:
// device sync + free + malloc, never during stream capture (`capture_msg`).  On failure the buffer is gone and `have` is 0.
template <class T, class N>
oxc_status grow_scratch(oxc_ctx* ctx, hipStream_t s, T*& ptr, N& have, N want, size_t bytes, const char* capture_msg, const char* malloc_label) {
  if (want <= have) return OXC_OK;
  if (stream_is_capturing(s)) return fail(ctx, OXC_INVALID_ARG, capture_msg);
  OXC_HIP(ctx, hipDeviceSynchronize());  // in-flight work may still use the old scratch
  if (ptr) OXC_HIP(ctx, hipFree(ptr));
  ptr = nullptr;
  have = 0;
  hipError_t e = hipMalloc(reinterpret_cast<void**>(&ptr), bytes);
  if (e != hipSuccess) return fail(ctx, OXC_OUT_OF_MEMORY, malloc_label, e);
  have = want;
  return OXC_OK;
}

#pragma GCC visibility pop
